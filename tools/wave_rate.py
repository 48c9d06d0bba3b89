#!/usr/bin/env python3
"""Rates of the waveform envelope (emspec_wave_device, emspec_set_wave_out), one GPU call, every number
after a warm-up:
  1. the kernel (HIP events, 20 launches after 3) on the bench shape (64 streams x 2^22 samples, N = 4096, hop 256) at factor 1,
     64 and 65536 and on ONE stream of 2^25 samples at factor 65536, as ms and GB/s of the samples it reads; in the same run the
     peaks kernel at k = 1 and the time reduction's kernel (dB only, f = 64), both on the dB of the same batch (4 B per cell) -
     re-measured here, not quoted.  A shape below half of the peaks kernel's bytes/s is flagged.
  2. the host entries with the envelope set against cleared, the two alternating call by call in one process:
     emspec_batch_pcm_packed (S16 stereo -> L R M S, 16 sources) and emspec_batch index out, FAST and EXACT, page-locked buffers.
  3. the same entries, envelope cleared, against another build of the library (--parent: the parent commit's libemspec.so), child
     processes alternating this, parent, this, ... as tools/ab_kernel.py does.  The margin is the spread of the parent's own
     repeats (the medians of its rounds); a difference beyond it is a defect in the row's "off" path.
   python tools/wave_rate.py [--parent path/to/parent/libemspec.so] [--out profiles/wave_rate.txt] [--rounds 3]   (needs an MI355X)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
import numpy as np
import torch

import emspec

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--parent")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--child", help="(internal) the library a child process times the host entries of")
ap.add_argument("--data", help="(internal) directory with the child's input")
args = ap.parse_args()
S, L, n, hop, R, MIN_DB = args.streams, 1 << 22, 4096, 256, 1024, -60.0
Cn = (L - n) // hop + 1   # (emspec_num_columns; not asked of the library here: a child picks its library first)


def child():
    """Times emspec_batch_pcm_packed and emspec_batch index out of ONE library, FAST and EXACT: envelope cleared and - where the
    library has it - set, alternating call by call.  Prints one JSON line of wall times in seconds."""
    assert not emspec._libs, "a library was loaded before the child chose its own"
    emspec.LIB_PATH = os.path.abspath(args.child)
    lib = emspec.load()
    has = hasattr(lib, "emspec_set_wave_out")
    f32 = np.fromfile(os.path.join(args.data, "pcm.f32"), np.float32).reshape(S, L)
    pins = []

    def pinned(shape, dtype, fill=None):
        p = emspec.PinnedArray(shape, dtype)
        if fill is not None:
            p.array[...] = fill
        pins.append(p)
        return p.array

    s16 = np.round(np.clip(f32, -1, 1) * 32767).astype(np.int16)
    st = np.empty((S // 4, L, 2), np.int16)
    st[:, :, 0], st[:, :, 1] = s16[0::4], s16[1::4]
    stereo = pinned((S // 4, 2 * L), np.int16, st.reshape(S // 4, 2 * L))
    src = pinned((S, L), np.float32, f32)
    del st, s16, f32
    lrms = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
    wire = pinned((S * emspec.wire_bound(Cn, R),), np.uint8)
    index = pinned((S, Cn, R), np.uint8)
    wave = pinned((S, Cn, 2), np.float32)
    offs = np.zeros(S + 1, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    res = {"library": emspec.build_info(), "has_wave": has}
    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            h = e._h
            out = emspec.Out(None, None, index.ctypes.data)
            entries = {"pcm_packed": lambda: e._chk(lib.emspec_batch_pcm_packed(h, p(stereo), C.byref(lrms), S // 4, L, n, hop, 1, p(wire),
                                                                                 C.c_int64(wire.size), p(offs))),
                       "index": lambda: e._chk(lib.emspec_batch(h, p(src), S, L, n, hop, 1, C.byref(out)))}
            for key, fn in entries.items():
                t = {"cleared": [], "set": []}
                for i in range(2 + args.calls):
                    for state in ("cleared", "set") if has else ("cleared",):
                        if has:
                            e._chk(lib.emspec_set_wave_out(h, p(wave) if state == "set" else None, wave.size // 2))
                        t0 = time.perf_counter()
                        fn()
                        if i >= 2:
                            t[state].append(time.perf_counter() - t0)
                if has:
                    e._chk(lib.emspec_set_wave_out(h, None, 0))
                res[f"{name}_{key}"] = t
    print(json.dumps(res))
    for q in pins:
        q.close()


if args.child:
    child()
    sys.exit(0)

from bench import synth_device

lib = emspec.load()
dev = torch.device("cuda", 0)
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


say(f"# {res['library']}; {S} streams x 2^22 samples, N = {n}, hop {hop}: {S * Cn} columns; {S * Cn * hop * 4 / 1e9:.2f} GB of samples under them")
x = synth_device(S, L, 0, dev)

# 1. the kernels
say("# 1. kernels: HIP events, 20 launches after 3; bytes = what the kernel reads (samples for the envelope, dB cells for the two others)")
with emspec.Engine() as e:
    db = torch.empty((S, Cn, R), dtype=torch.float32, device=dev)
    e.batch_device(x, n, hop, True, db=db)
    torch.cuda.synchronize()
    cells = S * Cn * R
    pk = torch.empty((S, Cn, 1, 2), dtype=torch.float32, device=dev)
    t_pk = events(lambda: e.peaks_device(db, 1, MIN_DB, out=pk))
    res["peaks_k1_GBps"] = cells * 4 / t_pk / 1e9
    say(f"peaks_kernel k=1 on the batch's dB (re-measured): {t_pk * 1e3:.3f} ms = {res['peaks_k1_GBps']:.0f} GB/s of dB read")
    t1 = events(lambda: e.batch_device(x, n, hop, True, db=db), steps=10)
    e.set_time_reduce(64)
    rdb = torch.empty((S, -(-Cn // 64), R), dtype=torch.float32, device=dev)
    t64 = events(lambda: e.batch_device(x, n, hop, True, db=rdb), steps=10)
    e.set_time_reduce(1)
    add = t64 - t1
    res["reduce_f64_db_GBps"] = cells * 4 / add / 1e9 if add > 0 else float("inf")
    say(f"reduce_columns_kernel dB only f=64 on the same cells (re-measured): {add * 1e3:.3f} ms = {res['reduce_f64_db_GBps']:.0f} GB/s "
        f"(emspec_batch_device dB at factor 64, {t64 * 1e3:.2f} ms, minus factor 1, {t1 * 1e3:.2f} ms: a difference of two event means)")
    res["column_kernels_ms"] = t1 * 1e3
    del db, rdb, pk
    one = synth_device(1, 1 << 25, 0, dev)
    shapes = [(x, 1), (x, 64), (x, 65536), (one, 65536)]
    for src, f in shapes:
        s_, l_ = src.shape
        c_ = emspec.num_columns(l_, n, hop)
        out = torch.empty((s_, emspec.reduced_columns(c_, f), 2), dtype=torch.float32, device=dev)
        dt = events(lambda: e.wave_device(src, n, hop, f, out=out))
        e.device_status()
        gbps = s_ * c_ * hop * 4 / dt / 1e9
        key = f"wave_S{s_}_f{f}"
        res[key + "_ms"], res[key + "_GBps"] = dt * 1e3, gbps
        flag = "" if gbps >= 0.5 * res["peaks_k1_GBps"] else "   << below half of the peaks kernel's bytes/s: see the note at the end"
        say(f"emspec_wave_device {s_:2d} x 2^{l_.bit_length() - 1} samples, factor {f:<5d} (windows of {min(f, c_) * hop} samples, "
            f"{'one team of lanes per window' if min(f, c_) * hop <= 16384 else 'pieces of 65536 samples over workgroups, keys by integer atomics'}): "
            f"{dt * 1e3:.3f} ms = {gbps:.0f} GB/s of samples read = {dt / t1 * 100:.1f} % of the column kernels' {t1 * 1e3:.2f} ms{flag}")
        del out
    del one

# 2. + 3. the host entries, in child processes (one library each), this build and the parent alternating
tmp = tempfile.mkdtemp(prefix="wave_rate_")
x.cpu().numpy().tofile(os.path.join(tmp, "pcm.f32"))
del x
torch.cuda.empty_cache()
here = emspec.LIB_PATH
order = [here, args.parent] * args.rounds if args.parent else [here] * args.rounds
runs = {here: [], args.parent: []}
for path in order:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--data", tmp, "--calls", str(args.calls), "--streams", str(S)],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        say(f"child for {path} failed ({r.returncode}): {r.stderr[-500:]}")
        break
    runs[path].append(json.loads(r.stdout.strip().splitlines()[-1]))
os.remove(os.path.join(tmp, "pcm.f32"))
os.rmdir(tmp)
med = statistics.median
say(f"# 2. host entries, envelope set against cleared: alternating call by call, {args.calls} calls each after 2, {len(runs[here])} processes; page-locked buffers; "
    f"median over all calls; columns/s = {S * Cn} columns / median")
say(f"# 3. the same entries cleared against the parent's library ({runs[args.parent][0]['library'] if args.parent and runs[args.parent] else 'not given'}): "
    "processes alternating; margin = max - min of the medians of the parent's own rounds")
for name in ("FAST", "EXACT"):
    for key, label in (("pcm_packed", "emspec_batch_pcm_packed S16 stereo L R M S"), ("index", "emspec_batch index out")):
        k = f"{name}_{key}"
        if not runs[here]:
            break
        cl = [t for r in runs[here] for t in r[k]["cleared"]]
        st = [t for r in runs[here] for t in r[k]["set"]]
        res[k + "_cleared_ms"], res[k + "_set_ms"] = med(cl) * 1e3, med(st) * 1e3
        say(f"{name:5s} {label:44s} cleared {med(cl) * 1e3:7.2f} ms ({S * Cn / med(cl):.3e} columns/s)  set {med(st) * 1e3:7.2f} ms ({S * Cn / med(st):.3e} columns/s)  "
            f"set - cleared {(med(st) - med(cl)) * 1e3:+6.2f} ms = {(med(st) / med(cl) - 1) * 100:+5.1f} %")
        if args.parent and runs[args.parent]:
            assert all(r["library"] != res["library"] for r in runs[args.parent]), "the parent's library is this build"
            pr = [med(r[k]["cleared"]) for r in runs[args.parent]]
            mine = [med(r[k]["cleared"]) for r in runs[here]]
            margin, diff = max(pr) - min(pr), med(mine) - med(pr)
            res[k + "_parent_ms"], res[k + "_margin_ms"] = med(pr) * 1e3, margin * 1e3
            say(f"{'':5s} {'':44s} parent  {med(pr) * 1e3:7.2f} ms (its rounds: {', '.join(f'{v * 1e3:.2f}' for v in pr)}; margin {margin * 1e3:.2f} ms)  "
                f"this build cleared, rounds: {', '.join(f'{v * 1e3:.2f}' for v in mine)}  cleared - parent {diff * 1e3:+6.2f} ms: "
                f"{'within the margin' if abs(diff) <= margin else ('FASTER than the parent beyond the margin' if diff < 0 else 'SLOWER than the parent beyond the margin')}")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
