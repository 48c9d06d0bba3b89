#!/usr/bin/env python3
"""What the live history (emspec_set_live_history / emspec_history_view) costs, on the GPU box.

  history_rate.py live [--lib path/to/libemspec.so] [--history W] [--calls 800] [--streams 64]
      per-call host time of the live entry points, 64 streams x one hop per call, N = 4096 / hop 256, every buffer page-locked,
      out = dB, block form (emspec_push_samples_multi) and per-frame form (emspec_columns), both arithmetic modes: median
      microseconds per call (the first tenth dropped).  --lib times another build of the library (the parent commit's, which has
      no history: run the two alternately on one box, as tools/ab_kernel.py does); --history W sets a history of W columns.
  history_rate.py view [--streams 64] [--groups 2000] [--factors 1,4,64] [--wide-streams 16]
      the view kernel through emspec_history_view_device, HIP events: streams x groups x 1,024 rows at each factor, for
      dB + index and for RGBA only: ms per view and (bytes read + bytes written) / time; one group of all W columns per stream
      (the split-group path); and beside them the time-reduction kernel on the same cell count (emspec_batch_device at the
      same factor against factor 1, as tools/overview_rate.py measures it).  A factor whose ring (streams x groups x factor
      columns of 4 KB) would pass 12 GB is measured with --wide-streams streams instead, and says so.
Prints one line per figure."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
import numpy as np  # noqa: E402

import emspec  # noqa: E402
from emspec import synth  # noqa: E402

N, HOP, R = 4096, 256, 1024


def live(args):
    S, calls = args.streams, args.calls
    pcm = synth.streams(min(S, 8), N + HOP * (calls + 4))
    pcm = np.ascontiguousarray(np.tile(pcm, ((S + 7) // 8, 1))[:S])
    for mode, mname in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        for form in ("samples", "frames"):
            with emspec.Engine(mode=mode) as e:
                if args.history:
                    e.set_live_history(args.history)
                keep = [emspec.PinnedArray((S, N if form == "frames" else HOP), np.float32),
                        emspec.PinnedArray((S, R) if form == "frames" else (S, 1, R), np.float32)]
                fin, db = keep[0].array, keep[1].array
                ts = np.empty(calls)
                if form == "samples":
                    e.push_samples_multi(pcm[:, :N - HOP].copy(), N, HOP, True, want_db=False, db=None)   # prime: no frame yet
                for i in range(calls):
                    fin[:] = pcm[:, i * HOP:i * HOP + N] if form == "frames" else pcm[:, N - HOP + i * HOP:N + i * HOP]
                    t0 = time.perf_counter()
                    if form == "frames":
                        e.columns(fin, HOP, True, db=db)
                    else:
                        e.push_samples_multi(fin, N, HOP, True, db=db)
                    ts[i] = time.perf_counter() - t0
                ts = ts[calls // 10:]
                held = e.live_history(0) if args.history else None
                print(f"{args.tag:8s} {mname:5s} S={S} {form:7s} pinned out=db history={args.history:<5d} median {np.median(ts) * 1e6:6.1f} us  "
                      f"p90 {np.percentile(ts, 90) * 1e6:6.1f} us" + (f"  (held {held})" if held else ""), flush=True)
                for p in keep:
                    p.close()


def events(fn, steps=20, warm=3):
    import torch
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


def fill(e, S, columns):
    """Emit `columns` columns on each of S streams: the same block of one launch's frames over and over, no output."""
    per = 32 if S > 32 else 64
    block = synth.streams(min(S, 8), per * HOP)
    block = np.ascontiguousarray(np.tile(block, ((S + 7) // 8, 1))[:S])
    e.push_samples_multi(np.ascontiguousarray(np.tile(block, (1, 1))[:, :N - HOP]), N, HOP, True, want_db=False)
    D = emspec.latency_columns(N, HOP, True)
    done = 0
    while done < columns:
        _, _, counts, _ = e.push_samples_multi(block, N, HOP, True, want_db=False)
        done = e.live_history(0)[0]
    return done, D


def view(args):
    import torch
    dev = torch.device("cuda", 0)
    factors = [int(f) for f in args.factors.split(",")]
    G = args.groups
    for f in factors:
        S = args.streams
        if S * G * f * R * 4 > 12e9:
            S = args.wide_streams
        Wn = G * f
        with emspec.Engine() as e:
            e.set_live_history(Wn)
            t0 = time.perf_counter()
            end, _ = fill(e, S, Wn)
            first = end - Wn
            db = torch.empty((S, G, R), dtype=torch.float32, device=dev)
            idx = torch.empty((S, G, R), dtype=torch.uint8, device=dev)
            rgba = torch.empty((S, G, R, 4), dtype=torch.uint8, device=dev)
            print(f"# ring {S} streams x {Wn} columns = {S * Wn * R * 4 / 1e9:.2f} GB, filled in {time.perf_counter() - t0:.1f} s", flush=True)
            cells = S * G * R
            for what, kw, wbytes in (("dB + index", dict(db=db, index=idx), 5), ("RGBA only", dict(rgba=rgba), 4)):
                dt = events(lambda: e.history_view_device(first, f, G, streams=S, **kw))
                moved = cells * f * 4 + cells * wbytes
                print(f"view  S={S:2d} groups={G} f={f:<3d} {what:10s}: {dt * 1e3:7.3f} ms  {moved / dt / 1e9:6.0f} GB/s "
                      f"({cells * f * 4 / 1e9:.2f} GB read, {cells * wbytes / 1e9:.2f} GB written)", flush=True)
            if f == factors[0]:
                # one group of all W columns per stream: the split-group path
                d1 = torch.empty((S, 1, R), dtype=torch.float32, device=dev)
                i1 = torch.empty((S, 1, R), dtype=torch.uint8, device=dev)
                dt = events(lambda: e.history_view_device(first, 65536 if Wn > 65536 else Wn, 1, streams=S, db=d1, index=i1))
                cols = min(Wn, 65536)
                print(f"view  S={S:2d} groups=1 f={cols} (one group of the ring, cut over waves) dB + index: {dt * 1e3:7.3f} ms  "
                      f"{S * cols * R * 4 / dt / 1e9:6.0f} GB/s read", flush=True)
            del db, idx, rgba
    # the time-reduction kernel on the same cell count: emspec_batch_device, factor f against factor 1 (tools/overview_rate.py)
    from bench import synth_device
    S, L = 64, 1 << 22
    Cn = emspec.num_columns(L, N, HOP)
    x = synth_device(S, L, 0, dev)
    with emspec.Engine() as e:
        base = None
        for f in [1] + [f for f in factors if f > 1]:
            e.set_time_reduce(f)
            cr = -(-Cn // f)
            db = torch.empty((S, cr, R), dtype=torch.float32, device=dev)
            idx = torch.empty((S, cr, R), dtype=torch.uint8, device=dev)
            dt = events(lambda: e.batch_device(x, N, HOP, True, db=db, index=idx))
            if f == 1:
                base = dt
                print(f"batch S=64 x {Cn} columns f=1   dB + index: {dt * 1e3:7.3f} ms", flush=True)
            else:
                add = dt - base
                print(f"batch S=64 x {Cn} columns f={f:<3d} dB + index: {dt * 1e3:7.3f} ms; + {add * 1e3:.3f} ms over factor 1 = "
                      f"{S * Cn * R * 5 / add / 1e9:.0f} GB/s of the 5 B per full-rate cell the reduction reads", flush=True)
            del db, idx


ap = argparse.ArgumentParser()
sub = ap.add_subparsers(dest="cmd", required=True)
a = sub.add_parser("live")
a.add_argument("--lib")
a.add_argument("--history", type=int, default=0)
a.add_argument("--calls", type=int, default=800)
a.add_argument("--streams", type=int, default=64)
a.add_argument("--tag", default="this")
b = sub.add_parser("view")
b.add_argument("--streams", type=int, default=64)
b.add_argument("--groups", type=int, default=2000)
b.add_argument("--factors", default="1,4,64")
b.add_argument("--wide-streams", type=int, default=16)
args = ap.parse_args()
if getattr(args, "lib", None):
    emspec.LIB_PATH = os.path.abspath(args.lib)
live(args) if args.cmd == "live" else view(args)
