#!/usr/bin/env python3
"""Per-call host time of the live multi-band call (emspec_push_samples_multiband) against what a renderer had to do before it
existed, and of the calls it must leave unchanged, on one box in one job.  64 streams, one hop per call, sample-block form,
page-locked buffers, out = dB, FAST and EXACT.  Wall clock around the C call, median and p90 of the calls after the first tenth
(warm-up: ring priming, allocations).  Ladder B: 16384 / 4096 / 1024 at hop 256, splits at 250 Hz and 2 kHz.

   python tools/live_multiband_rate.py --parent /path/to/libemspec.so-built-from-the-parent-commit [--calls 2200] [--rounds 3]

Measured, one child process per build and variant (the binding loads the library named by emspec.LIB_PATH), rounds alternated:
  (a) (b) (c)  PARENT build: a single-resolution live session at 16384, 4096 and 1024 on three engines, one call each per hop
  (m)          this build: the multi-band session, one call per hop            required: median (m) < median (a) + (b) + (c)
  (u)          the existing calls - single 64 x 4096 / 256 and two-band 16384 / 4096 - on this build against the parent build:
               at most 1.03 x the parent's median
  (k)          K = 2 (16384, 4096) through the multi-band entry against push_samples_multires of this build: at most 1.03
  (f)          the diagnostic build, ladder B, blocks of 8 hops per call: one live_finalize_bands_kernel against K
               live_finalize_kernel launches (EMSPEC_LIVE_FINALIZE_PER_BAND=1); the bands kernel stays if its median is not above
               the K-launch form's by more than the spread (max - min) of that form's rounds
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
if %(lib)r:
    emspec.LIB_PATH = %(lib)r
from emspec import synth
kind, exact, calls, diag = %(kind)r, %(exact)d, %(calls)d, %(diag)d
S, N, hop, R = 64, (16384, 4096, 1024), 256, 1024
per = 8 if kind == "bands8" else 1            # hops per call
mode = emspec.MODE_EXACT if exact else emspec.MODE_FAST
WRAP = 64                           # the timed calls walk over WRAP blocks of samples again and again: the time is not the signal's
L = N[0] + hop * per * (WRAP + 4)
pcm = synth.streams(8, L)
pcm = np.ascontiguousarray(np.tile(pcm, (S // 8, 1)))
keep = []
def pinned(shape, dt):
    p = emspec.PinnedArray(shape, dt)
    keep.append(p)
    return p.array
blk = hop * per
sin = pinned((S, blk), np.float32)
first = N[0] - hop                  # samples every session has seen before the timed calls: the next hop completes a frame
ts = np.empty((calls, 3))
ts[:] = 0.0
def engine():
    return emspec.Engine(mode=mode, diag=True) if diag else emspec.Engine(mode=mode)
def timed(prime, call):
    prime()
    for i in range(calls):
        sin[:] = pcm[:, first + (i %% WRAP) * blk:first + (i %% WRAP + 1) * blk]
        t0 = time.perf_counter()
        call()
        ts[i, 0] = time.perf_counter() - t0
if kind == "triple":
    es = [engine() for _ in N]
    dbs = [pinned((S, 1, R), np.float32) for _ in N]
    for e, n in zip(es, N):
        e.push_samples_multi(pcm[:, first - (n - hop):first].copy(), n, hop, True, want_db=False)
    for i in range(calls):
        sin[:] = pcm[:, first + (i %% WRAP) * hop:first + (i %% WRAP + 1) * hop]
        for k, (e, n, db) in enumerate(zip(es, N, dbs)):
            t0 = time.perf_counter()
            e.push_samples_multi(sin, n, hop, True, db=db)
            ts[i, k] = time.perf_counter() - t0
    for e in es:
        e.close()
else:
    e = engine()
    db = pinned((S, per, R), np.float32)
    split = tuple(e.split_row_for_hz(f) for f in (250.0, 2000.0))
    if kind in ("bands", "bands8"):
        timed(lambda: e.push_samples_multiband(pcm[:, :first].copy(), N, split, hop, True, want_db=False),
              lambda: e.push_samples_multiband(sin, N, split, hop, True, db=db))
    elif kind == "k2":
        timed(lambda: e.push_samples_multiband(pcm[:, :first].copy(), N[:2], split[:1], hop, True, want_db=False),
              lambda: e.push_samples_multiband(sin, N[:2], split[:1], hop, True, db=db))
    elif kind == "multires":
        timed(lambda: e.push_samples_multires(pcm[:, :first].copy(), N[0], N[1], hop, split[0], True, want_db=False),
              lambda: e.push_samples_multires(sin, N[0], N[1], hop, split[0], True, db=db))
    else:                                # "single": the existing live call at 4096 / 256
        timed(lambda: e.push_samples_multi(pcm[:, first - (N[1] - hop):first].copy(), N[1], hop, True, want_db=False),
              lambda: e.push_samples_multi(sin, N[1], hop, True, db=db))
    e.close()
ts = ts[calls // 10:] * 1e6
print("RESULT", " ".join(f"{np.median(ts[:, k]):.2f} {np.percentile(ts[:, k], 90):.2f}" for k in range(3)))
for p in keep:
    p.close()
'''


def child(lib, kind, exact, calls, diag=False, env=None):
    code = CHILD % dict(root=ROOT, lib=os.path.abspath(lib) if lib else "", kind=kind, exact=exact, calls=calls, diag=int(diag))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
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
        names = ("triple", "bands", "single_parent", "single_here", "multires_parent", "multires_here", "k2", "fin_bands", "fin_per_band")
        runs = {k: [] for k in names}
        for r in range(a.rounds):
            runs["triple"].append(child(a.parent, "triple", exact, a.calls))
            runs["bands"].append(child(HERE, "bands", exact, a.calls))
            runs["single_parent"].append(child(a.parent, "single", exact, a.calls))
            runs["single_here"].append(child(HERE, "single", exact, a.calls))
            runs["multires_parent"].append(child(a.parent, "multires", exact, a.calls))
            runs["multires_here"].append(child(HERE, "multires", exact, a.calls))
            runs["k2"].append(child(HERE, "k2", exact, a.calls))
            runs["fin_bands"].append(child("", "bands8", exact, a.calls, diag=True))
            runs["fin_per_band"].append(child("", "bands8", exact, a.calls, diag=True, env={"EMSPEC_LIVE_FINALIZE_PER_BAND": "1"}))
        col = lambda k, i: med([x[i] for x in runs[k]])
        timed = a.calls - a.calls // 10
        print(f"{mname:5s} S=64 16384/4096/1024 hop 256, samples pinned, out=db, {timed} timed calls x {a.rounds} rounds")
        parts = [col("triple", 2 * k) for k in range(3)]
        for tag, n, k in (("a", 16384, 0), ("b", 4096, 1), ("c", 1024, 2)):
            print(f"  ({tag}) parent build, live session at {n:5d} : median {parts[k]:7.1f} us  p90 {col('triple', 2 * k + 1):7.1f} us")
        mm = col("bands", 0)
        print(f"  (m) this build, multi-band session      : median {mm:7.1f} us  p90 {col('bands', 1):7.1f} us   = {100 * mm / (256 / 48000 * 1e6):.2f} % of one hop (5.33 ms)")
        good = mm < sum(parts)
        print(f"  required (m) < (a) + (b) + (c): {mm:.1f} < {sum(parts):.1f} : {'holds' if good else 'DOES NOT HOLD'}")
        ok = ok and good
        for what, p, h in (("single 64 x 4096/256", "single_parent", "single_here"), ("two-band 64 x 16384/4096/256", "multires_parent", "multires_here")):
            ratio = col(h, 0) / col(p, 0)
            print(f"  (u) {what}: parent build median {col(p, 0):7.1f} us p90 {col(p, 1):7.1f} us | this build median {col(h, 0):7.1f} us p90 {col(h, 1):7.1f} us"
                  f" | ratio {ratio:.3f} (at most 1.03): {'holds' if ratio <= 1.03 else 'DOES NOT HOLD'}")
            ok = ok and ratio <= 1.03
        ratio = col("k2", 0) / col("multires_here", 0)
        print(f"  (k) K = 2 through the multi-band entry: median {col('k2', 0):7.1f} us p90 {col('k2', 1):7.1f} us | push_samples_multires of this build"
              f" {col('multires_here', 0):7.1f} us | ratio {ratio:.3f} (at most 1.03): {'holds' if ratio <= 1.03 else 'DOES NOT HOLD'}")
        ok = ok and ratio <= 1.03
        fb, fk = col("fin_bands", 0), col("fin_per_band", 0)
        each = [x[0] for x in runs["fin_per_band"]]
        spread = max(each) - min(each)
        keep = fb <= fk + spread
        print(f"  (f) diagnostic build, 8 hops per call: one bands kernel median {fb:7.1f} us p90 {col('fin_bands', 1):7.1f} us | K finalize launches median"
              f" {fk:7.1f} us p90 {col('fin_per_band', 1):7.1f} us (rounds {' '.join(f'{v:.1f}' for v in each)}: spread {spread:.1f} us)"
              f" : the bands kernel {'stays' if keep else 'IS SLOWER BY MORE THAN THE SPREAD'}", flush=True)
        ok = ok and keep
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
