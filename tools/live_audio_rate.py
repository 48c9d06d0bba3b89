#!/usr/bin/env python3
"""What the live audio history (emspec_set_live_audio / emspec_audio_view / emspec_audio_batch) costs, on
the GPU box.

  live_audio_rate.py live [--lib path/to/libemspec.so] [--audio W] [--calls 800] [--streams 64] [--tag NAME]
      per-call host time of the live entry points, 64 streams x one hop per call, N = 4096 / hop 256, every buffer page-locked,
      out = dB, FAST, block form (emspec_push_samples_multi) and per-frame form (emspec_columns): median microseconds per call
      (the first tenth dropped), and beside them one tiny torch kernel launch + synchronise timed the same way in the same
      run.  --lib times another build of the library (the parent commit's, which has no audio history: run the two alternately
      on one box, as tools/ab_kernel.py does); --audio W sets an audio history of W samples.
  live_audio_rate.py view [--streams 64] [--samples 512000]
      the view kernel through emspec_audio_view_device, HIP events: streams x samples from a ring of W = 2^19, from a ring
      slot and to a destination on 16-byte boundaries, and from a slot and to a destination that are odd multiples of 4 bytes
      (first sample and destination moved by one sample: source and destination still agree modulo 16 bytes), and with the
      destination alone moved (they disagree: the word-by-word path); beside them a device-to-device hipMemcpyAsync of the same
      byte count, timed in the same run.  ms per call and (bytes read + bytes written) / time.
  live_audio_rate.py batch [--streams 64] [--samples 512000]
      emspec_audio_batch_device over the same range at N = 4096 and N = 1024 (hop 256), beside emspec_batch_device over a
      linear copy of the same samples: the difference is the view's time.
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

N, HOP, R, W19 = 4096, 256, 1024, 1 << 19


def live(args):
    import torch
    S, calls = args.streams, args.calls
    pcm = synth.streams(min(S, 8), N + HOP * (calls + 4))
    pcm = np.ascontiguousarray(np.tile(pcm, ((S + 7) // 8, 1))[:S])
    for form in ("samples", "frames"):
        with emspec.Engine(mode=emspec.MODE_FAST) as e:
            if args.audio:
                e.set_live_audio(args.audio)
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
            held = e.live_audio(0) if args.audio else None
            print(f"{args.tag:8s} FAST  S={S} {form:7s} pinned out=db audio={args.audio:<7d} median {np.median(ts) * 1e6:6.1f} us  "
                  f"p90 {np.percentile(ts, 90) * 1e6:6.1f} us" + (f"  (held {held})" if held else ""), flush=True)
            for p in keep:
                p.close()
    x = torch.zeros(64, device="cuda")
    ts = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        x.add_(1.0)
        torch.cuda.synchronize()
        ts[i] = time.perf_counter() - t0
    ts = ts[calls // 10:]
    print(f"{args.tag:8s} one tiny torch kernel launch + synchronise: median {np.median(ts) * 1e6:6.1f} us  p90 {np.percentile(ts, 90) * 1e6:6.1f} us", flush=True)


def fill(e, S, total):
    """A session of S streams with `total` samples stored (block form, 16,384 samples per call)."""
    import torch
    base = synth.streams(8, 16384)
    block = np.ascontiguousarray(np.tile(base, ((S + 7) // 8, 1))[:S])
    fed = 0
    while fed < total:
        e.push_samples_multi(block, N, HOP, True, want_db=False)
        fed += block.shape[1]
    torch.cuda.synchronize()
    return e.live_audio(0)


def events(fn, steps=20, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(steps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def view(args):
    import torch
    S, count = args.streams, args.samples
    with emspec.Engine(mode=emspec.MODE_FAST) as e:
        e.set_live_audio(W19)
        end, first = fill(e, S, W19 + 16384)
        a = (first + 3) // 4 * 4
        a += (4 - a % W19 % 4) % 4            # a ring slot on a 16-byte boundary
        assert a % W19 % 4 == 0 and a + count + 1 <= end
        dst = torch.empty((S * count + 4,), dtype=torch.float32, device="cuda")
        src = torch.empty((S * count,), dtype=torch.float32, device="cuda")
        nbytes = S * count * 4
        rows = [("aligned slot and destination", a, 0), ("slot and destination odd multiples of 4 bytes", a + 1, 1),
                ("destination alone moved by 4 bytes (word by word)", a, 1)]
        for name, va, off in rows:
            ms = events(lambda: e.audio_view_device(va, count, dst[off:]))
            print(f"view  S={S} x {count} samples, {name}: {ms:7.3f} ms  {2 * nbytes / ms / 1e9:7.2f} TB/s  (slot {va % W19}, wraps: {va % W19 + count > W19})", flush=True)
        ms = events(lambda: dst[:S * count].copy_(src))
        print(f"copy  hipMemcpyAsync device to device, {nbytes} bytes: {ms:7.3f} ms  {2 * nbytes / ms / 1e9:7.2f} TB/s", flush=True)


def batch(args):
    import torch
    S, count = args.streams, args.samples
    with emspec.Engine(mode=emspec.MODE_FAST) as e:
        e.set_live_audio(W19)
        end, first = fill(e, S, W19 + 16384)
        a = (first + HOP - 1) // HOP * HOP
        assert a + count <= end
        lin = torch.empty((S, count), dtype=torch.float32, device="cuda")
        e.audio_view_device(a, count, lin)
        for n in (4096, 1024):
            C = emspec.num_columns(count, n, HOP)
            db = torch.empty((S, C, R), dtype=torch.float32, device="cuda")
            ms_a = events(lambda: e.audio_batch_device(a, count, n, HOP, True, db=db), steps=10)
            ms_b = events(lambda: e.batch_device(lin, n, HOP, True, db=db), steps=10)
            print(f"batch S={S} x {count} samples N={n} hop={HOP}: {C} columns  audio_batch_device {ms_a:7.3f} ms  batch_device over a linear copy "
                  f"{ms_b:7.3f} ms  difference {ms_a - ms_b:+7.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["live", "view", "batch"])
    ap.add_argument("--lib")
    ap.add_argument("--audio", type=int, default=0)
    ap.add_argument("--calls", type=int, default=800)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--samples", type=int, default=512000)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if args.lib:
        emspec.LIB_PATH = args.lib
        args.tag = args.tag or "parent"
    args.tag = args.tag or "this"
    {"live": live, "view": view, "batch": batch}[args.what](args)


if __name__ == "__main__":
    main()
