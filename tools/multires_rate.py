#!/usr/bin/env python3
"""Rate of the multi-resolution batch (emspec_batch_multires_device) on 64 streams x 2^22 samples, n_low 16384 /
n_high 4096, hop 256, split at 250 Hz on the default axis (row 368), palette index out, FAST and EXACT; beside it each band alone
as a single-resolution emspec_batch_device on an engine whose rows and custom edges are exactly that band's slice of the table
("slice"), and - since a custom table selects the binary-search row lookup (and in FAST mode takes the N = 16384 band off its fused
kernel's fast plan) while the band plans keep the log axis's hinted lookup - on an engine whose own log axis spans the band
("log": fmin / fmax = the band's end edges, the band plan's kernels; its table may differ from the slice in the last bit).
HIP events around each call after two warm-up calls; median of the timed calls.  The multires call should cost at most
1.10 x (low band + high band): the rest is the composition and the orchestration.
   python tools/multires_rate.py [--calls K] [--out FILE]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
import torch  # noqa: E402  (before libemspec: one HIP runtime)
import numpy as np  # noqa: E402
import emspec  # noqa: E402
from emspec import synth  # noqa: E402

S, L, NL, NH, HOP, SPLIT_HZ = 64, 1 << 22, 16384, 4096, 256, 250.0


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return sorted(ts)[len(ts) // 2]


def main():
    calls = arg("--calls", 5)
    out_path = arg("--out", "")
    pcm = torch.from_numpy(synth.streams(S, L)).cuda()
    Cm = emspec.multires_columns(L, NL, NH, HOP)
    d = emspec.multires_shift(NL, NH, HOP)
    Ch = emspec.num_columns(L, NH, HOP)
    lines = [f"multires rate: {S} streams x 2^22 samples, n_low {NL} / n_high {NH}, hop {HOP}, split at {SPLIT_HZ:g} Hz on the "
             f"default axis, palette index out; median of {calls} calls (HIP events, 2 warm-up)",
             f"  {torch.cuda.get_device_name(0)}, {emspec.build_info()}"]
    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            split = e.split_row_for_hz(SPLIT_HZ)
            edges = e.row_edges_hz()
            R = e.rows
            idx = torch.empty((S, Cm, R), dtype=torch.uint8, device="cuda")
            t_m = timed(lambda: e.batch_multires_device(pcm, NL, NH, HOP, split, True, index=idx), calls)
            e.device_status()
        del idx
        lines.append(f"{name:5s} multires {t_m * 1e3:8.2f} ms = {S * Cm / t_m:.3e} columns/s  (low band {NL}: rows 0..{split}, "
                     f"{Cm} columns; high band {NH}: rows {split}..{R}, {Ch} columns, shift {d})")
        print(lines[-1], flush=True)
        for axis in ("slice", "log"):
            band = {}
            for key, n, r0, r1, cols in (("low", NL, 0, split, Cm), ("high", NH, split, R, Ch)):
                kw = {} if axis == "slice" else {"fmin_hz": float(edges[r0]), "fmax_hz": float(edges[r1])}
                with emspec.Engine(mode=mode, rows=r1 - r0, **kw) as b:
                    if axis == "slice":
                        b.set_row_edges_hz(edges[r0:r1 + 1])
                    out = torch.empty((S, cols, r1 - r0), dtype=torch.uint8, device="cuda")
                    band[key] = timed(lambda: b.batch_device(pcm, n, HOP, True, index=out), calls)
                    b.device_status()
                del out
            torch.cuda.empty_cache()
            s = band["low"] + band["high"]
            lines.append(f"      bands alone, {axis:5s} axis: low {band['low'] * 1e3:8.2f} ms + high {band['high'] * 1e3:8.2f} ms = "
                         f"{s * 1e3:8.2f} ms  |  multires / (low + high) = {t_m / s:.3f} (bound 1.10)")
            print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:2]))


if __name__ == "__main__":
    main()
