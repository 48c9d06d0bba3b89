#!/usr/bin/env python3
"""Per-call host time of the live multi-stream entry points (emspec_columns / emspec_push_samples_multi) on the GPU box:
S streams x one hop per call, N = 4096 / hop 256 (BASELINE configs[2] in its live form).  Prints one line per variant:
median / p90 microseconds per call and columns/s.  usage: live_rate.py [S] [calls] [filter,filter,...] [overlay,overlay,...]
(filters: every token must appear in the variant's label, e.g. FAST,samples,pinned,out=db; an empty string: no filter)
overlays: which overlay settings each variant runs with, in turn - none (the default), peaks (emspec_set_live_peaks, k = 8,
min_db = -60), wave (emspec_set_live_wave), both, audio (emspec_set_live_audio, W = 2^19 samples per stream), level
(emspec_set_live_level), cross (emspec_set_live_cross, views = 2, a = 0, b = 1), meters (envelope + level + cross), all (meters +
peaks).  Their arrays are page-locked or pageable as the other buffers are.
EMSPEC_LIB=path times another build of the library (the parent commit's, which has no overlays: `none` only) in the same
session, as tools/ab_kernel.py does; EMSPEC_MULTIRES=1 times the 16384 / 4096 multi-resolution session (split row 512) instead."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "em-spec_amd"),):
    sys.path.insert(0, p)
import emspec  # noqa: E402
from emspec import synth  # noqa: E402

if os.environ.get("EMSPEC_LIB"):
    emspec.LIB_PATH = os.environ["EMSPEC_LIB"]


def timed(fn, calls):
    ts = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn(i)
        ts[i] = time.perf_counter() - t0
    return ts[calls // 10:]          # the first tenth warms up (ring priming, allocations)


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 600
    only = sys.argv[3].split(",") if len(sys.argv) > 3 else []
    overlays = sys.argv[4].split(",") if len(sys.argv) > 4 else ["none"]
    multires = os.environ.get("EMSPEC_MULTIRES") == "1"
    n, hop, R = (16384, 256, 1024) if multires else (4096, 256, 1024)
    n_high, split = (4096, 512) if multires else (0, 0)
    L = n + hop * (calls + 4)
    pcm = synth.streams(min(S, 8), L)
    pcm = np.ascontiguousarray(np.tile(pcm, ((S + 7) // 8, 1))[:S])
    for mode, mname in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        for pinned in (True, False):
            for form in ("samples", "frames"):
                for outs, overlay in [(o, v) for o in (("db",), ("rgba",), ("db", "rgba")) for v in overlays]:
                    label = f"{mname:5s} S={S:3d} {form:7s} {'pinned' if pinned else 'pageable':8s} out={'+'.join(outs):7s} "
                    if not all(tok in label + " " for tok in only if tok):
                        continue
                    label += f"overlay={overlay:6s} " + ("multires " if multires else "")
                    with emspec.Engine(mode=mode) as e:
                        keep = []
                        def buf(shape, dt):
                            if pinned:
                                p = emspec.PinnedArray(shape, dt)
                                keep.append(p)
                                return p.array
                            return np.empty(shape, dt)
                        if overlay in ("peaks", "both", "all"):
                            e.set_live_peaks(8, -60.0, buf((S * 8 * 2,), np.float32))
                        if overlay in ("wave", "both", "meters", "all"):
                            e.set_live_wave(buf((S * 2,), np.float32))
                        if overlay in ("level", "meters", "all"):
                            e.set_live_level(buf((S,), emspec.LEVEL_DTYPE))
                        if overlay in ("cross", "meters", "all"):
                            e.set_live_cross(2, 0, 1, buf((S // 2,), emspec.CROSS_DTYPE))
                        if overlay == "audio":
                            e.set_live_audio(1 << 19)
                        if form == "frames":
                            fin = buf((S, n), np.float32)
                            db = buf((S, R), np.float32) if "db" in outs else None
                            rgba = buf((S, R, 4), np.uint8) if "rgba" in outs else None
                            def call(i):
                                fin[:] = pcm[:, i * hop:i * hop + n]
                            def run(i):
                                if multires:
                                    e.columns_multires(fin, n_high, hop, split, True, want_db=db is not None, want_rgba=rgba is not None, db=db, rgba=rgba)
                                else:
                                    e.columns(fin, hop, True, want_db=db is not None, want_rgba=rgba is not None, db=db, rgba=rgba)
                            # the copy into the frame block is the caller's (the renderer owns its frames): not timed
                            def step(i):
                                call(i)
                            ts = np.empty(calls)
                            for i in range(calls):
                                step(i)
                                t0 = time.perf_counter()
                                run(i)
                                ts[i] = time.perf_counter() - t0
                            ts = ts[calls // 10:]
                        else:
                            sin = buf((S, hop), np.float32)
                            db = buf((S, 1, R), np.float32) if "db" in outs else None
                            rgba = buf((S, 1, R, 4), np.uint8) if "rgba" in outs else None
                            if multires:
                                e.push_samples_multires(pcm[:, :n - hop].copy(), n, n_high, hop, split, True, want_db=False)
                            else:
                                e.push_samples_multi(pcm[:, :n - hop].copy(), n, hop, True, want_db=False)   # prime: no frame yet
                            ts = np.empty(calls)
                            for i in range(calls):
                                sin[:] = pcm[:, n - hop + i * hop:n + i * hop]
                                t0 = time.perf_counter()
                                if multires:
                                    e.push_samples_multires(sin, n, n_high, hop, split, True, want_db=db is not None, want_rgba=rgba is not None, db=db, rgba=rgba)
                                else:
                                    e.push_samples_multi(sin, n, hop, True, want_db=db is not None, want_rgba=rgba is not None, db=db, rgba=rgba)
                                ts[i] = time.perf_counter() - t0
                            ts = ts[calls // 10:]
                        med, p90 = np.median(ts) * 1e6, np.percentile(ts, 90) * 1e6
                        print(f"{label}"
                              f"median {med:7.1f} us  p90 {p90:7.1f} us  -> {S / (med * 1e-6):.3e} columns/s", flush=True)
                        for p in keep:
                            p.close()


if __name__ == "__main__":
    main()
