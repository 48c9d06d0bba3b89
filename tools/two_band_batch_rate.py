#!/usr/bin/env python3
"""Rate of the two-band batch (emspec_batch_multires_device) of this build against a library built from another
commit - made when the two-band batch became the K = 2 case of the multi-band batch (§3.13), whose run function and composition
kernel it now uses.  One child process per build and take (the binding loads the library named by emspec.LIB_PATH), builds alternated;
the test signal (two seconds of numpy per stream) is made once and handed on through .npy files under `--tmp DIR`.

1. Whole calls: tools/multires_rate.py (64 streams x 2^22 samples, 16384 / 4096, hop 256, index out, FAST and EXACT) on both builds,
   `--rounds` alternating runs each, median of the runs' medians: this build at most 1.03 x the other.
2. A small call, where the host side of the entry weighs most: 4 streams x 2^17 samples, 8192 / 2048, hop 128, index out, FAST and
   EXACT; `--rounds` alternating runs of `--calls` calls per build (HIP events around each call), median over all calls: at most
   1.03 x the other build - or its own run-to-run spread (max - min of the runs' medians, over their median) where that is larger.
3. The composition kernel: `--twelve LIB` makes 12 two-band device calls at the shape of 1. and nothing else, for a kernel trace of
   each build; `--traces OTHER.csv HERE.csv` compares the composition kernels' own durations (columns Kernel_Name, Start_Timestamp,
   End_Timestamp in ns).  This build's kernel may be slower by at most the spread of the other kernel's takes plus 3 %.

   python tools/two_band_batch_rate.py --parent OTHER_LIBEMSPEC_SO [--rounds 3] [--calls 100] [--tmp DIR] [--out FILE]
   python tools/two_band_batch_rate.py --twelve LIBEMSPEC_SO [--tmp DIR]        (under a kernel trace)
   python tools/two_band_batch_rate.py --traces OTHER.csv HERE.csv [--out FILE]   (appends to FILE)"""
import csv
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
HERE = os.path.join(ROOT, "em-spec_amd", "libemspec.so")
BIG = (64, 1 << 22, 16384, 4096, 256)     # streams, samples, n_low, n_high, hop: the shape of tools/multires_rate.py
SMALL = (4, 1 << 17, 8192, 2048, 128)


def arg(name, default, k=1):
    return type(default)(sys.argv[sys.argv.index(name) + k]) if name in sys.argv else default


def child(lib, what, tmp, *args):
    print(f"... {what} on {lib}", file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, what, tmp, *map(str, args)], capture_output=True, text=True)
    if r.returncode:
        print(f"child {what} on {lib} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
        sys.exit(2)
    return json.loads(r.stdout.strip().splitlines()[-1])


def share_streams(synth, tmp):
    """synth.streams(S, L) of this process through DIR/streams_S_L.npy, made by the first process that asks."""
    import numpy as np
    make = synth.streams

    def streams(S, L):
        path = os.path.join(tmp, f"streams_{S}_{L}.npy")
        if not os.path.exists(path):
            np.save(path, make(S, L))
        return np.load(path)
    synth.streams = streams


def run_child(lib, what, tmp, args):
    import torch  # (before libemspec: one HIP runtime)
    import emspec
    from emspec import synth
    emspec.LIB_PATH = lib
    if tmp:
        share_streams(synth, tmp)
    if what == "whole":   # tools/multires_rate.py as it stands, on this library
        import contextlib
        import io
        import runpy
        sys.argv = ["multires_rate.py", "--calls", args[0]]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            runpy.run_path(os.path.join(ROOT, "tools", "multires_rate.py"), run_name="__main__")
        ms = {m.group(1): float(m.group(2)) for m in re.finditer(r"^(FAST|EXACT)\s+multires\s+([0-9.]+) ms", buf.getvalue(), re.M)}
        print(json.dumps({"ms": ms, "build": emspec.build_info()}))
        return
    S, L, n_low, n_high, hop = BIG if what == "twelve" else SMALL
    pcm = torch.from_numpy(synth.streams(S, L)).cuda()
    out = {"build": emspec.build_info()}
    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            split = e.split_row_for_hz(250.0)
            idx = torch.empty((S, emspec.multires_columns(L, n_low, n_high, hop), e.rows), dtype=torch.uint8, device="cuda")
            call = lambda: e.batch_multires_device(pcm, n_low, n_high, hop, split, True, index=idx)  # noqa: E731
            if what == "twelve":
                for _ in range(12):
                    call()
                torch.cuda.synchronize()
                e.device_status()
                break
            calls = int(args[0])
            for _ in range(max(calls // 10, 2)):
                call()
            torch.cuda.synchronize()
            ts = []
            for _ in range(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            e.device_status()
            out[name] = ts
    print(json.dumps(out))


def kernel_takes(path):
    """{name: durations in us} of the composition kernels in a trace - whatever each build calls its own."""
    takes = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\w+_compose_kernel", r["Kernel_Name"])
            if m:
                takes.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {k: v[len(v) // 5:] for k, v in takes.items()}   # (the first takes of a process: code-object load, cold caches)


def traces(other_csv, here_csv):
    S, L, n_low, n_high, hop = BIG
    lines = [f"composition kernel of the two-band device call ({n_low} / {n_high}, hop {hop}, {S} streams x 2^22 samples, index out, FAST), "
             "one kernel trace of 12 calls per build:"]
    got = {}
    for tag, path in (("other", other_csv), ("this", here_csv)):
        for k, v in kernel_takes(path).items():
            got[tag] = v
            lines.append(f"  {tag:5s} build, {k:26s} {len(v):3d} takes: median {statistics.median(v):9.1f} us, min {min(v):9.1f}, max {max(v):9.1f}, "
                         f"spread (max - min) / median {100 * (max(v) - min(v)) / statistics.median(v):.1f} %")
    old, new = statistics.median(got["other"]), statistics.median(got["this"])
    allowed = 100 * (max(got["other"]) - min(got["other"])) / old + 3.0
    lines.append(f"  this / other = {new / old:.3f} ({100 * (new / old - 1):+.1f} %; allowed: the other kernel's spread + 3 % = +{allowed:.1f} %): "
                 f"{'within' if 100 * (new / old - 1) <= allowed else 'SLOWER than'} the bound")
    return lines


def main():
    out_path = arg("--out", "")
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        return run_child(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3], sys.argv[i + 4:])
    if "--twelve" in sys.argv:
        return run_child(os.path.abspath(arg("--twelve", "")), "twelve", arg("--tmp", ""), [])
    if "--traces" in sys.argv:
        lines = traces(arg("--traces", ""), arg("--traces", "", 2))
        print("\n".join(lines))
        if out_path:
            with open(out_path, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    other, rounds, calls = os.path.abspath(arg("--parent", "")), arg("--rounds", 3), arg("--calls", 100)
    whole, small = {"other": [], "this": []}, {"other": [], "this": []}
    with tempfile.TemporaryDirectory() as own:
        tmp = arg("--tmp", own)
        for _ in range(rounds):
            for tag, lib in (("other", other), ("this", HERE)):
                whole[tag].append(child(lib, "whole", tmp, 5))
                small[tag].append(child(lib, "small", tmp, calls))
    lines = [f"two-band batch, this build ({whole['this'][0]['build']}) against another ({whole['other'][0]['build']}); {rounds} alternating runs per build",
             "whole calls (tools/multires_rate.py: 64 streams x 2^22 samples, 16384 / 4096, hop 256, index out; each run the median of 5 calls):"]
    ok = True
    for mode in ("FAST", "EXACT"):
        o, h = [w["ms"][mode] for w in whole["other"]], [w["ms"][mode] for w in whole["this"]]
        ratio = statistics.median(h) / statistics.median(o)
        ok = ok and ratio <= 1.03
        lines.append(f"  {mode:5s} other build {' '.join(f'{v:7.2f}' for v in o)} ms, median {statistics.median(o):7.2f} | this build "
                     f"{' '.join(f'{v:7.2f}' for v in h)} ms, median {statistics.median(h):7.2f} | this / other = {ratio:.3f} (at most 1.03): "
                     f"{'holds' if ratio <= 1.03 else 'DOES NOT HOLD'}")
    S, L, n_low, n_high, hop = SMALL
    lines.append(f"small call ({S} streams x 2^17 samples, {n_low} / {n_high}, hop {hop}, index out; {calls} calls per run, HIP events around each):")
    for mode in ("FAST", "EXACT"):
        runs_o, runs_h = [statistics.median(w[mode]) for w in small["other"]], [statistics.median(w[mode]) for w in small["this"]]
        mo = statistics.median([t for w in small["other"] for t in w[mode]])
        mh = statistics.median([t for w in small["this"] for t in w[mode]])
        spread = (max(runs_o) - min(runs_o)) / statistics.median(runs_o)
        margin = max(0.03, spread)
        ok = ok and mh / mo <= 1 + margin
        lines.append(f"  {mode:5s} other build: medians of the runs {' '.join(f'{v:7.1f}' for v in runs_o)} us (run-to-run spread {100 * spread:.1f} %), of all "
                     f"{rounds * calls} calls {mo:7.1f} us | this build: {' '.join(f'{v:7.1f}' for v in runs_h)} us, of all calls {mh:7.1f} us | this / other = "
                     f"{mh / mo:.3f} (at most {1 + margin:.3f}): {'holds' if mh / mo <= 1 + margin else 'DOES NOT HOLD'}")
    lines.append("every bar holds" if ok else "A BAR IS MISSED")
    print("\n".join(lines))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
