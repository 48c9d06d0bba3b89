#!/usr/bin/env python3
"""Per-call host time of the live multi-resolution call (emspec_push_samples_multires) against what a renderer had to do
before it existed, on one box in one job.  Shape: 64 streams, one hop per call, sample-block form, page-locked buffers,
16384 / 4096 / hop 256, split at 250 Hz, out = dB, FAST and EXACT.  Wall clock around the C call, median and p90 of the
calls after the first tenth (warm-up: ring priming, allocations).

   python tools/live_multires_rate.py --parent /path/to/libemspec.so-built-from-the-parent-commit [--calls 2200] [--rounds 3]

Measured, one child process per build and variant (the binding loads the library named by emspec.LIB_PATH), rounds alternated:
  (a) + (b)  PARENT build: a single-resolution live session at n_low on one engine and at n_high on a second, one call each per hop
  (m)        this build: the multi-resolution session, one call per hop           required: median (m) < median (a) + median (b)
  single     the existing live call, 64 x 4096 / 256, on this build against the parent build: at most 1.03 x the parent's median
For the record: (m) as a share of one hop's 5.33 ms.  Figures are the median over the rounds of each round's median / p90.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "em-spec_amd", "libemspec.so")

CHILD = r'''
import os, sys, time
sys.path[:0] = [os.path.join(%(root)r, "em-spec_amd")]
import numpy as np
import emspec
emspec.LIB_PATH = %(lib)r
from emspec import synth
kind, exact, calls = %(kind)r, %(exact)d, %(calls)d
S, n_low, n_high, hop, R = 64, 16384, 4096, 256, 1024
mode = emspec.MODE_EXACT if exact else emspec.MODE_FAST
L = n_low + hop * (calls + 4)
pcm = synth.streams(8, L)
pcm = np.ascontiguousarray(np.tile(pcm, (S // 8, 1)))
keep = []
def pinned(shape, dt):
    p = emspec.PinnedArray(shape, dt)
    keep.append(p)
    return p.array
sin = pinned((S, hop), np.float32)
first = n_low - hop                  # samples every session has seen before the timed calls: the next hop completes a frame
ts = np.empty((calls, 2))
if kind == "pair":
    ea, eb = emspec.Engine(mode=mode), emspec.Engine(mode=mode)
    dba, dbb = pinned((S, 1, R), np.float32), pinned((S, 1, R), np.float32)
    ea.push_samples_multi(pcm[:, :first].copy(), n_low, hop, True, want_db=False)
    eb.push_samples_multi(pcm[:, first - (n_high - hop):first].copy(), n_high, hop, True, want_db=False)
    for i in range(calls):
        sin[:] = pcm[:, first + i * hop:first + (i + 1) * hop]
        t0 = time.perf_counter()
        ea.push_samples_multi(sin, n_low, hop, True, db=dba)
        t1 = time.perf_counter()
        eb.push_samples_multi(sin, n_high, hop, True, db=dbb)
        ts[i] = (t1 - t0, time.perf_counter() - t1)
    ea.close(); eb.close()
elif kind == "multires":
    e = emspec.Engine(mode=mode)
    split = e.split_row_for_hz(250.0)
    db = pinned((S, 1, R), np.float32)
    e.push_samples_multires(pcm[:, :first].copy(), n_low, n_high, hop, split, True, want_db=False)
    for i in range(calls):
        sin[:] = pcm[:, first + i * hop:first + (i + 1) * hop]
        t0 = time.perf_counter()
        e.push_samples_multires(sin, n_low, n_high, hop, split, True, db=db)
        ts[i] = (time.perf_counter() - t0, 0.0)
    e.close()
else:                                # "single": the existing live call at 4096 / 256
    e = emspec.Engine(mode=mode)
    db = pinned((S, 1, R), np.float32)
    e.push_samples_multi(pcm[:, :n_high - hop].copy(), n_high, hop, True, want_db=False)
    for i in range(calls):
        sin[:] = pcm[:, n_high - hop + i * hop:n_high + i * hop]
        t0 = time.perf_counter()
        e.push_samples_multi(sin, n_high, hop, True, db=db)
        ts[i] = (time.perf_counter() - t0, 0.0)
    e.close()
ts = ts[calls // 10:] * 1e6
print("RESULT", " ".join(f"{v:.2f}" for v in (np.median(ts[:, 0]), np.percentile(ts[:, 0], 90), np.median(ts[:, 1]), np.percentile(ts[:, 1], 90))))
for p in keep:
    p.close()
'''


def child(lib, kind, exact, calls):
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, lib=os.path.abspath(lib), kind=kind, exact=exact, calls=calls)],
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit(f"{kind} on {lib} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1]
    return [float(v) for v in line.split()[1:]]


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libemspec.so built from the parent commit")
    ap.add_argument("--calls", type=int, default=2200, help="calls per run; the first tenth is warm-up")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert a.calls - a.calls // 10 >= 1980
    ok = True
    for exact, mname in ((0, "FAST"), (1, "EXACT")):
        runs = {"pair": [], "multires": [], "single_parent": [], "single_here": []}
        for r in range(a.rounds):
            runs["pair"].append(child(a.parent, "pair", exact, a.calls))
            runs["multires"].append(child(HERE, "multires", exact, a.calls))
            runs["single_parent"].append(child(a.parent, "single", exact, a.calls))
            runs["single_here"].append(child(HERE, "single", exact, a.calls))
        col = lambda k, i: med([x[i] for x in runs[k]])
        am, ap90, bm, bp90 = (col("pair", i) for i in range(4))
        mm, mp90 = col("multires", 0), col("multires", 1)
        sp, sp90, sh, sh90 = col("single_parent", 0), col("single_parent", 1), col("single_here", 0), col("single_here", 1)
        print(f"{mname:5s} S=64 16384/4096/256 samples pinned out=db, {a.calls - a.calls // 10} timed calls x {a.rounds} rounds")
        print(f"  (a) parent build, live session at 16384 : median {am:7.1f} us  p90 {ap90:7.1f} us")
        print(f"  (b) parent build, live session at  4096 : median {bm:7.1f} us  p90 {bp90:7.1f} us")
        print(f"  (m) this build, multi-resolution session: median {mm:7.1f} us  p90 {mp90:7.1f} us   = {100 * mm / (256 / 48000 * 1e6):.2f} % of one hop (5.33 ms)")
        good = mm < am + bm
        print(f"  required (m) < (a) + (b): {mm:.1f} < {am + bm:.1f} : {'holds' if good else 'DOES NOT HOLD'}")
        ratio = sh / sp
        print(f"  single 64 x 4096/256: parent build median {sp:7.1f} us p90 {sp90:7.1f} us | this build median {sh:7.1f} us p90 {sh90:7.1f} us"
              f" | ratio {ratio:.3f} (at most 1.03): {'holds' if ratio <= 1.03 else 'DOES NOT HOLD'}", flush=True)
        ok = ok and good and ratio <= 1.03
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
