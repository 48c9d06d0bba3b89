#!/usr/bin/env python3
"""The live one-hop call, float push against PCM push, in the same run (profiles/live_pcm_rate.txt): 64 streams, N = 4096,
hop 256, one hop of new samples per call, page-locked blocks and outputs (dB out).  Float: emspec_push_samples_multi on 64
float32 streams.  PCM: emspec_push_samples_pcm on 16 stereo int16 sources x (L, R, M, S) = 64 streams.  The PCM form adds one
kernel launch (the decode) without a synchronisation of its own and its frame kernels read the new samples from device
memory instead of page-locked host memory; what one launch + wait costs on the same box is tools/ubench/launch_sync.hip.

    python tools/live_pcm_rate.py [--calls 3000] > profiles/live_pcm_rate.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "em-spec_amd"))
import emspec  # noqa: E402


def run(e, call, calls, prime):
    for _ in range(prime):
        call()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return statistics.median(ts), ts[len(ts) // 10], ts[len(ts) * 9 // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3000)
    a = ap.parse_args()
    S, n, hop, views = 64, 4096, 256, 4
    print(f"# {emspec.build_info()}")
    print(f"# {S} streams, N = {n}, hop {hop}: one hop per call, dB out, page-locked block and output; median [10 % .. 90 %] of {a.calls} calls "
          f"after {n // hop + 40} priming calls; three rounds each, alternating")
    rng = np.random.default_rng(1)
    fblk = emspec.PinnedArray((S, hop), np.float32)
    fblk.array[...] = rng.uniform(-0.5, 0.5, size=(S, hop)).astype(np.float32)
    pblk = emspec.PinnedArray((S // views, hop * 2), np.int16)
    pblk.array[...] = rng.integers(-16000, 16000, size=(S // views, hop * 2)).astype(np.int16)
    fmt = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            out = emspec.PinnedArray((S, 1, e.rows), np.float32)
            cnt, first = np.zeros(S, np.int64), np.zeros(S, np.int64)
            p = lambda arr: C.c_void_p(arr.ctypes.data)
            lib, h, R = e._lib, e._h, e.rows

            def push_float():
                e._chk(lib.emspec_push_samples_multi(h, p(fblk.array), S, hop, hop, n, hop, 1, p(out.array), None, R, 1, p(cnt), p(first)))

            def push_pcm():
                e._chk(lib.emspec_push_samples_pcm(h, p(pblk.array), C.byref(fmt), S // views, hop, hop * 4, n, hop, 1, p(out.array), None, R, 1,
                                                   p(cnt), p(first)))

            res = {"float": [], "pcm": []}
            for _ in range(3):
                for key, fn in (("float", push_float), ("pcm", push_pcm)):
                    e.reset()
                    res[key].append(run(e, fn, a.calls, n // hop + 40))
            for key, label in (("float", "emspec_push_samples_multi, 64 float32 streams"), ("pcm", "emspec_push_samples_pcm, 16 stereo s16 sources x L R M S")):
                meds = [r[0] for r in res[key]]
                print(f"{name:5s} {label:58s} median {statistics.median(meds) * 1e6:7.2f} us/call  rounds " +
                      " ".join(f"{m * 1e6:.2f} [{lo * 1e6:.2f} .. {hi * 1e6:.2f}]" for m, lo, hi in res[key]) +
                      f"  spread of the rounds' medians {(max(meds) - min(meds)) * 1e6:.2f} us")
            d = statistics.median([r[0] for r in res["pcm"]]) - statistics.median([r[0] for r in res["float"]])
            print(f"{name:5s} PCM - float = {d * 1e6:+.2f} us/call")
            out.close()
    fblk.close()
    pblk.close()


if __name__ == "__main__":
    main()
