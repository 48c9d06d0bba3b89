#!/usr/bin/env python3
"""Rates of the batch entries with the time reduction (emspec_set_time_reduce) at the bench shape
(64 streams x 2^22 samples, N = 4096, hop 256), both arithmetic modes, factor 1 / 4 / 64:
  1. emspec_batch_device, index only and dB + index (HIP events, 20 steps after warm-up), and what the reduction pass adds
     over factor 1 as GB/s of the full-rate bytes it reads (1 B per cell, 5 B with dB);
  2. emspec_batch, uint8 index out, page-locked buffers, with each stage timed alone (copy in, kernels, copy out);
  3. emspec_batch_pcm_packed, S16 stereo -> L R M S from 16 sources, the same way.
   python tools/overview_rate.py [--lib path/to/libemspec.so] [--out profiles/overview_rate.txt]      (needs an MI355X)
--lib times another build of the library (the parent commit's, which has no time reduction: factor 1 only); run the two
alternately on one box, as tools/ab_kernel.py does, to compare factor 1 with the parent."""
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
ap.add_argument("--lib")
ap.add_argument("--out")
ap.add_argument("--streams", type=int, default=64)
args = ap.parse_args()
if args.lib:
    emspec.LIB_PATH = os.path.abspath(args.lib)
lib = emspec.load()
HAS = hasattr(lib, "emspec_set_time_reduce")
FACTORS = (1, 4, 64) if HAS else (1,)
S, L, n, hop, R = args.streams, 1 << 22, 4096, 256, 1024
dev = torch.device("cuda", 0)
Cn = emspec.num_columns(L, n, hop)
hip = C.CDLL("libamdhip64.so")
lines, res = [], {"streams": S, "columns": S * Cn, "library": emspec.build_info()}


def say(s):
    print(s, flush=True)
    lines.append(s)


def cr(f):
    return -(-Cn // f)


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


say(f"# {res['library']}; {S} streams x 2^22 samples, N = {n}, hop {hop}: {S * Cn} full-rate columns")
x = synth_device(S, L, 0, dev)
pin = emspec.PinnedArray((S, L), np.float32)
pin.array[...] = x.cpu().numpy()
pix = emspec.PinnedArray((S, Cn, R), np.uint8)

for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
    with emspec.Engine(mode=mode) as e:
        base = {}
        for f in FACTORS:
            if HAS:
                e.set_time_reduce(f)
            idx = torch.empty((S, cr(f), R), dtype=torch.uint8, device=dev)
            db = torch.empty((S, cr(f), R), dtype=torch.float32, device=dev)
            for what, kw, bpc in (("index", {"index": idx}, 1), ("dB + index", {"db": db, "index": idx}, 5)):
                dt = events(lambda: e.batch_device(x, n, hop, True, **kw))
                e.device_status()
                key = f"{name}_device_{what.replace(' + ', '_')}_f{f}"
                res[key + "_columns_per_s"] = S * Cn / dt
                extra = ""
                if f == 1:
                    base[what] = dt
                else:
                    add = dt - base[what]
                    gbs = S * Cn * R * bpc / add / 1e9 if add > 0 else float("inf")
                    res[key + "_reduce_GBps"] = gbs
                    extra = f"; + {add * 1e3:.2f} ms over factor 1 = {gbs:.0f} GB/s of the {bpc} B per full-rate cell the reduction reads (parity dump: 2,600 GB/s)"
                say(f"emspec_batch_device {name:5s} f={f:<2d} {what:10s}: {S * Cn / dt:.3e} columns/s ({dt * 1e3:.2f} ms){extra}")
            del idx, db
        for f in FACTORS:
            if HAS:
                e.set_time_reduce(f)
            out_bytes = S * cr(f) * R
            o = emspec.Out(None, None, C.c_void_p(pix.array.ctypes.data))

            def run_idx():
                assert lib.emspec_batch(e._h, C.c_void_p(pin.array.ctypes.data), S, L, n, hop, 1, C.byref(o)) == 0
            dt, spread = wall(run_idx)
            res[f"{name}_host_index_f{f}_columns_per_s"] = S * Cn / dt
            d_in = torch.empty(pin.array.nbytes, dtype=torch.uint8, device=dev)
            t_in, _ = wall(lambda: hip.hipMemcpy(C.c_void_p(d_in.data_ptr()), C.c_void_p(pin.array.ctypes.data), C.c_size_t(pin.array.nbytes), 1))
            d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
            t_out, _ = wall(lambda: hip.hipMemcpy(C.c_void_p(pix.array.ctypes.data), C.c_void_p(d_out.data_ptr()), C.c_size_t(out_bytes), 2))
            idx = d_out.view(S, cr(f), R)
            t_k = events(lambda: e.batch_device(x, n, hop, True, index=idx), steps=10)
            del d_in, d_out, idx
            say(f"emspec_batch        {name:5s} f={f:<2d} index out, pinned: {S * Cn / dt:.3e} full-rate columns/s ({dt * 1e3:.1f} ms, spread {spread * 1e3:.1f} ms); "
                f"alone: copy in {t_in * 1e3:.1f} ms, kernels {t_k * 1e3:.1f} ms, copy out {t_out * 1e3:.2f} ms ({out_bytes / 1e6:.0f} MB)")
        # S16 stereo -> L R M S, 16 sources = 64 streams
        src_n = max(S // 4, 1)
        fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
        raw = emspec.PinnedArray((src_n, L * 2), np.int16)
        raw.array[...] = np.clip(pin.array[:2 * src_n].reshape(src_n, 2, L).transpose(0, 2, 1).reshape(src_n, -1) * 20000.0, -32768, 32767).astype(np.int16)
        wire = pix.array.reshape(-1)
        offs = np.zeros(src_n * 4 + 1, np.int64)
        for f in FACTORS:
            if HAS:
                e.set_time_reduce(f)

            def run_pcm():
                assert lib.emspec_batch_pcm_packed(e._h, C.c_void_p(raw.array.ctypes.data), C.byref(fmt), src_n, L, n, hop, 1,
                                                   C.c_void_p(wire.ctypes.data), C.c_int64(wire.size), offs.ctypes.data_as(C.c_void_p)) == 0
            dt, spread = wall(run_pcm)
            res[f"{name}_pcm_packed_f{f}_columns_per_s"] = src_n * 4 * Cn / dt
            d_in = torch.empty(raw.array.nbytes, dtype=torch.uint8, device=dev)
            t_in, _ = wall(lambda: hip.hipMemcpy(C.c_void_p(d_in.data_ptr()), C.c_void_p(raw.array.ctypes.data), C.c_size_t(raw.array.nbytes), 1))
            del d_in
            say(f"emspec_batch_pcm_packed {name:5s} f={f:<2d} S16 stereo -> L R M S: {src_n * 4 * Cn / dt:.3e} full-rate columns/s ({dt * 1e3:.1f} ms, spread "
                f"{spread * 1e3:.1f} ms; copy in alone {t_in * 1e3:.1f} ms; {offs[-1] / 1e6:.1f} MB of images out)")
        raw.close()
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
