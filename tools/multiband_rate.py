#!/usr/bin/env python3
"""Rate of the multi-band batch (emspec_batch_multiband_device) on 64 streams x 2^22 samples, FFT sizes 16384 /
4096 / 1024, hop 256, splits at 250 Hz and 2 kHz on the default axis (rows 368 and 668), palette index out, FAST and EXACT.

1. The whole call against the three bands run alone: each band as a single-resolution emspec_batch_device on an engine whose own
   log axis spans the band (fmin / fmax = the band's end edges, the band plan's kernels; as the "log" lines of
   tools/multires_rate.py).  The call should cost at most 1.10 x the sum: the rest is the composition and the orchestration.
2. The new composition kernel at two bands against multires_compose_kernel: the two-band shape 16384 / 4096 through
   emspec_batch_multires_device and through emspec_batch_multiband_device, alternating, in the same run - the band kernels are the
   same, only the composition differs, and both compositions move the same bytes.  Whole calls by HIP events here; the kernels'
   own durations come from a kernel trace of `--compose N` (N alternating pairs of calls and nothing else), summarised by
   `--trace FILE` from the trace's CSV.  The new kernel may be slower by at most the spread of the old kernel's takes plus 3 %.

HIP events around each call after two warm-up calls; median of the timed calls.
   python tools/multiband_rate.py [--calls K] [--out FILE]
   python tools/multiband_rate.py --compose N              (under a kernel trace)
   python tools/multiband_rate.py --trace KERNEL_TRACE.csv [--out FILE]   (appends to FILE)"""
import csv
import os
import statistics
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
    return sorted(ts)[len(ts) // 2], ts


def trace_summary(path):
    """Per-kernel durations of the two composition kernels from a kernel trace CSV (columns Kernel_Name, Start_Timestamp,
    End_Timestamp in ns): median, spread of the takes, and the new kernel's median against the old one's."""
    takes = {"multires_compose_kernel": [], "multiband_compose_kernel": []}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in takes:
                if k in row["Kernel_Name"]:
                    takes[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    lines = [f"composition kernels at two bands (16384 / 4096, hop {HOP}, {S} streams x 2^22 samples, index out), kernel trace:"]
    med = {}
    for k, v in takes.items():
        if not v:
            lines.append(f"  {k}: not in the trace")
            continue
        v = v[len(v) // 5:]   # (the first takes of a process: code-object load, cold caches)
        med[k] = statistics.median(v)
        lines.append(f"  {k:26s} {len(v):3d} takes: median {med[k]:9.1f} us, min {min(v):9.1f}, max {max(v):9.1f}, "
                     f"spread (max - min) / median {100 * (max(v) - min(v)) / med[k]:.1f} %")
    if len(med) == 2:
        old, new = med["multires_compose_kernel"], med["multiband_compose_kernel"]
        v = takes["multires_compose_kernel"][len(takes["multires_compose_kernel"]) // 5:]
        allowed = 100 * (max(v) - min(v)) / old + 3.0
        lines.append(f"  new / old = {new / old:.3f} ({100 * (new / old - 1):+.1f} %; allowed: the old kernel's spread + 3 % = +{allowed:.1f} %): "
                     f"{'within' if 100 * (new / old - 1) <= allowed else 'SLOWER than'} the bound")
    return lines


def main():
    out_path = arg("--out", "")
    if "--trace" in sys.argv:
        lines = trace_summary(arg("--trace", ""))
        print("\n".join(lines))
        if out_path:
            with open(out_path, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    import torch  # (before libemspec: one HIP runtime)
    import emspec
    from emspec import synth
    calls = arg("--calls", 5)
    pcm = torch.from_numpy(synth.streams(S, L)).cuda()
    two = SIZES[:2]
    if "--compose" in sys.argv:   # alternating pairs of two-band calls and nothing else: for a kernel trace
        with emspec.Engine() as e:
            split = e.split_row_for_hz(SPLIT_HZ[0])
            idx = torch.empty((S, emspec.multiband_columns(L, two, HOP), e.rows), dtype=torch.uint8, device="cuda")
            for _ in range(arg("--compose", 10)):
                e.batch_multires_device(pcm, two[0], two[1], HOP, split, True, index=idx)
                e.batch_multiband_device(pcm, two, (split,), HOP, True, index=idx)
            torch.cuda.synchronize()
            e.device_status()
        return
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
            t_m, _ = timed(lambda: e.batch_multiband_device(pcm, SIZES, split, HOP, True, index=idx), calls, torch)
            # the two-band shape through the old and the new entry, alternating takes
            t_old, t_new = [], []
            for _ in range(calls):
                t_old.append(timed(lambda: e.batch_multires_device(pcm, two[0], two[1], HOP, split[0], True, index=idx), 1, torch)[0])
                t_new.append(timed(lambda: e.batch_multiband_device(pcm, two, split[:1], HOP, True, index=idx), 1, torch)[0])
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
                alone.append(timed(lambda: b.batch_device(pcm, n, HOP, True, index=out), calls, torch)[0])
                b.device_status()
            del out
        torch.cuda.empty_cache()
        s = sum(alone)
        lines.append("      bands alone, log axis: " + " + ".join(f"{t * 1e3:8.2f} ms" for t in alone) +
                     f" = {s * 1e3:8.2f} ms  |  multiband / sum = {t_m / s:.3f} (bound 1.10)")
        print(lines[-1], flush=True)
        mo, mn = statistics.median(t_old), statistics.median(t_new)
        lines.append(f"      two bands {two[0]} / {two[1]}, whole calls, {calls} alternating takes: emspec_batch_multires_device {mo * 1e3:8.2f} ms "
                     f"(min {min(t_old) * 1e3:.2f}, max {max(t_old) * 1e3:.2f}), emspec_batch_multiband_device {mn * 1e3:8.2f} ms "
                     f"(min {min(t_new) * 1e3:.2f}, max {max(t_new) * 1e3:.2f}): new / old = {mn / mo:.3f}")
        print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
