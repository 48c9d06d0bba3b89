#!/usr/bin/env python3
"""Rate of the multi-band batch (emspec_batch_multiband_device) on 64 streams x 2^22 samples, FFT sizes 16384 /
4096 / 1024, hop 256, splits at 250 Hz and 2 kHz on the default axis (rows 368 and 668), palette index out, FAST and EXACT.

The whole call against the three bands run alone: each band as a single-resolution emspec_batch_device on an engine whose own
log axis spans the band (fmin / fmax = the band's end edges, the band plan's kernels; as the "log" lines of
tools/multires_rate.py).  The call should cost at most 1.10 x the sum: the rest is the composition and the orchestration.
(The two-band lines of profiles/multiband_rate.txt came from a second leg of this tool, the two-band shape through
emspec_batch_multires_device and emspec_batch_multiband_device while the two had a run function and a composition kernel each;
they are one code now, and tools/two_band_batch_rate.py times the two-band batch against another build instead.)

HIP events around each call after two warm-up calls; median of the timed calls.
   python tools/multiband_rate.py [--calls K] [--out FILE]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]

S, L, SIZES, HOP, SPLIT_HZ = 64, 1 << 22, (16384, 4096, 1024), 256, (250.0, 2000.0)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, calls, torch):
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
    out_path = arg("--out", "")
    import torch  # (before libemspec: one HIP runtime)
    import emspec
    from emspec import synth
    calls = arg("--calls", 5)
    pcm = torch.from_numpy(synth.streams(S, L)).cuda()
    Cm = emspec.multiband_columns(L, SIZES, HOP)
    shifts = emspec.multiband_shifts(SIZES, HOP)
    lines = [f"multiband rate: {S} streams x 2^22 samples, FFT sizes {' / '.join(map(str, SIZES))}, hop {HOP}, splits at "
             f"{' and '.join(f'{hz:g}' for hz in SPLIT_HZ)} Hz on the default axis, palette index out; median of {calls} calls (HIP events, 2 warm-up)",
             f"  {torch.cuda.get_device_name(0)}, {emspec.build_info()}"]
    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            split = tuple(e.split_row_for_hz(hz) for hz in SPLIT_HZ)
            edges = e.row_edges_hz()
            R = e.rows
            idx = torch.empty((S, Cm, R), dtype=torch.uint8, device="cuda")
            t_m = timed(lambda: e.batch_multiband_device(pcm, SIZES, split, HOP, True, index=idx), calls, torch)
            e.device_status()
        del idx
        cuts = [0, *split, R]
        lines.append(f"{name:5s} multiband {t_m * 1e3:8.2f} ms = {S * Cm / t_m:.3e} columns/s  (" +
                     "; ".join(f"band {k}: {n}, rows {cuts[k]}..{cuts[k + 1]}, shift {shifts[k]}" for k, n in enumerate(SIZES)) + f"; {Cm} columns)")
        print(lines[-1], flush=True)
        alone = []
        for k, n in enumerate(SIZES):
            r0, r1 = cuts[k], cuts[k + 1]
            with emspec.Engine(mode=mode, rows=r1 - r0, fmin_hz=float(edges[r0]), fmax_hz=float(edges[r1])) as b:
                out = torch.empty((S, Cm + 2 * shifts[k], r1 - r0), dtype=torch.uint8, device="cuda")
                alone.append(timed(lambda: b.batch_device(pcm, n, HOP, True, index=out), calls, torch))
                b.device_status()
            del out
        torch.cuda.empty_cache()
        s = sum(alone)
        lines.append("      bands alone, log axis: " + " + ".join(f"{t * 1e3:8.2f} ms" for t in alone) +
                     f" = {s * 1e3:8.2f} ms  |  multiband / sum = {t_m / s:.3f} (bound 1.10)")
        print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
