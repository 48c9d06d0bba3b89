#!/usr/bin/env python3
"""Rates of the spectral peaks (emspec_peaks_device, emspec_batch_peaks) at the bench shape (64 streams x
2^22 samples, N = 4096, hop 256), one process, warm-up then medians / event means:
  1. the standalone kernel on the dB array of the whole batch at k = 1, 8 and 32 (HIP events, 20 launches after 3), as ms, GB/s
     of the 4 B per cell it reads and columns/s; beside it the time reduction's kernel (reduce.hip.inc, dB only, f = 64), which
     reads the same 4 B per cell - as the difference of emspec_batch_device's dB time at factor 64 and at factor 1, the only way
     the library exposes it;
  2. emspec_batch_peaks, k = 8, page-locked buffers, FAST and EXACT, beside emspec_batch index out and dB out, with the copy in
     timed alone.
   python tools/peaks_rate.py [--out profiles/peaks_rate.txt] [--streams 64]      (needs an MI355X)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
import numpy as np
import torch

import emspec
from bench import synth_device

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--streams", type=int, default=64)
args = ap.parse_args()
lib = emspec.load()
S, L, n, hop, R, MIN_DB = args.streams, 1 << 22, 4096, 256, 1024, -60.0
dev = torch.device("cuda", 0)
Cn = emspec.num_columns(L, n, hop)
hip = C.CDLL("libamdhip64.so")
lines, res = [], {"streams": S, "columns": S * Cn, "library": emspec.build_info()}


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(fn, steps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e-3


def wall(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(max(t) - min(t))


say(f"# {res['library']}; {S} streams x 2^22 samples, N = {n}, hop {hop}: {S * Cn} columns of {R} rows, {S * Cn * R * 4 / 1e9:.2f} GB of dB")
x = synth_device(S, L, 0, dev)
pin = emspec.PinnedArray((S, L), np.float32)
pin.array[...] = x.cpu().numpy()

# 1. the standalone kernel, and the time reduction's kernel on the same dB
with emspec.Engine() as e:
    db = torch.empty((S, Cn, R), dtype=torch.float32, device=dev)
    e.batch_device(x, n, hop, True, db=db)
    torch.cuda.synchronize()
    cells = S * Cn * R
    for k in (1, 8, 32):
        out = torch.empty((S, Cn, k, 2), dtype=torch.float32, device=dev)
        dt = events(lambda: e.peaks_device(db, k, MIN_DB, out=out))
        e.device_status()
        used = float((out[..., 0] >= 0).float().mean().item())
        res[f"kernel_k{k}_ms"] = dt * 1e3
        res[f"kernel_k{k}_GBps"] = cells * 4 / dt / 1e9
        say(f"emspec_peaks_device k={k:<2d} min_db {MIN_DB:.0f}: {dt * 1e3:.3f} ms = {cells * 4 / dt / 1e9:.0f} GB/s of dB read, {S * Cn / dt:.3e} columns/s "
            f"({used * 100:.0f} % of the slots used)")
        del out
    t1 = events(lambda: e.batch_device(x, n, hop, True, db=db), steps=10)
    e.set_time_reduce(64)
    rdb = torch.empty((S, -(-Cn // 64), R), dtype=torch.float32, device=dev)
    t64 = events(lambda: e.batch_device(x, n, hop, True, db=rdb), steps=10)
    e.set_time_reduce(1)
    add = t64 - t1
    res["reduce_f64_db_ms"] = add * 1e3
    say(f"reduce_columns_kernel dB only f=64 on the same cells: {add * 1e3:.3f} ms = {cells * 4 / add / 1e9 if add > 0 else float('inf'):.0f} GB/s "
        f"(emspec_batch_device dB at factor 64, {t64 * 1e3:.2f} ms, minus factor 1, {t1 * 1e3:.2f} ms: a difference of two event means)")
    del db, rdb

# 2. the host entries, page-locked buffers
pk = emspec.PinnedArray((S, Cn, 8, 2), np.float32)
pix = emspec.PinnedArray((S, Cn, R), np.uint8)
d_in = torch.empty(pin.array.nbytes, dtype=torch.uint8, device=dev)
t_in, _ = wall(lambda: hip.hipMemcpy(C.c_void_p(d_in.data_ptr()), C.c_void_p(pin.array.ctypes.data), C.c_size_t(pin.array.nbytes), 1))
del d_in
say(f"copy in alone ({pin.array.nbytes / 1e9:.2f} GB, page-locked): {t_in * 1e3:.1f} ms = {S * Cn / t_in:.3e} columns/s")
for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
    with emspec.Engine(mode=mode) as e:
        def run_peaks():
            assert lib.emspec_batch_peaks(e._h, C.c_void_p(pin.array.ctypes.data), S, L, n, hop, 1, 8, MIN_DB, C.c_void_p(pk.array.ctypes.data)) == 0
        dt, spread = wall(run_peaks)
        res[f"{name}_host_peaks_columns_per_s"] = S * Cn / dt
        say(f"emspec_batch_peaks {name:5s} k=8, pinned: {S * Cn / dt:.3e} columns/s ({dt * 1e3:.1f} ms, spread {spread * 1e3:.1f} ms; {pk.array.nbytes / 1e6:.0f} MB out)")
        o = emspec.Out(None, None, C.c_void_p(pix.array.ctypes.data))

        def run_idx():
            assert lib.emspec_batch(e._h, C.c_void_p(pin.array.ctypes.data), S, L, n, hop, 1, C.byref(o)) == 0
        dt, spread = wall(run_idx)
        res[f"{name}_host_index_columns_per_s"] = S * Cn / dt
        say(f"emspec_batch       {name:5s} index out, pinned: {S * Cn / dt:.3e} columns/s ({dt * 1e3:.1f} ms, spread {spread * 1e3:.1f} ms; {pix.array.nbytes / 1e6:.0f} MB out)")
pix.close()
pdb = emspec.PinnedArray((S, Cn, R), np.float32)
with emspec.Engine() as e:
    o = emspec.Out(C.c_void_p(pdb.array.ctypes.data), None, None)

    def run_db():
        assert lib.emspec_batch(e._h, C.c_void_p(pin.array.ctypes.data), S, L, n, hop, 1, C.byref(o)) == 0
    dt, spread = wall(run_db, reps=3)
    res["FAST_host_db_columns_per_s"] = S * Cn / dt
    say(f"emspec_batch       FAST  dB out, pinned: {S * Cn / dt:.3e} columns/s ({dt * 1e3:.1f} ms, spread {spread * 1e3:.1f} ms; {pdb.array.nbytes / 1e6:.0f} MB out)")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
