#!/usr/bin/env python3
"""Rates of the window walk (window.hip.inc: the envelope, the level meters; emspec_wave_device, emspec_level_device,
emspec_cross_device, emspec_set_level_out, emspec_set_cross_out), one GPU call, every number
after a warm-up:
  1. the kernels (HIP events, 20 launches after 3) on the bench shape (64 streams x 2^22 samples, N = 4096, hop 256) at factor 1,
     64 and 65536: the envelope's kernel, the level kernel and the cross kernel (16 pairs of 4 views, channels 0 and 1) on the
     same samples in the same process, as ms and GB/s of the samples each reads, and the level and cross kernels' time over the
     envelope's; a process per round, with --parent alternating this build, parent, this, ... under the margin rule of 3.
  2. the host entries with the settings on against cleared, alternating call by call in one process: emspec_batch index out with
     emspec_set_level_out, and emspec_batch_pcm_packed (S16 stereo -> L R M S, 16 sources) with emspec_set_level_out and with
     both settings; FAST and EXACT, page-locked buffers.
  3. the same entries, settings cleared and on, and the live block call (emspec_columns, 64 streams, dB out) against another build
     of the library (--parent: the parent commit's libemspec.so), child processes alternating this, parent, this, ...  The margin
     is the spread of the parent's own repeats (the medians of its rounds): a time lies inside it when this build's median is at
     most the parent's median plus that spread.
   python tools/level_rate.py [--parent path/to/parent/libemspec.so] [--out profiles/window_rate.txt] [--rounds 3]   (needs an MI355X)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
import numpy as np
import torch

import emspec

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--parent")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--child", help="(internal) the library a child process times the host entries of")
ap.add_argument("--kernels", action="store_true", help="(internal) the child times the kernels instead")
ap.add_argument("--data", help="(internal) directory with the child's input")
args = ap.parse_args()
S, L, n, hop, R = args.streams, 1 << 22, 4096, 256, 1024
Cn = (L - n) // hop + 1   # (emspec_num_columns; not asked of the library here: a child picks its library first)
STATES = ("cleared", "level", "both")


def child():
    """Times emspec_batch_pcm_packed, emspec_batch index out and the live block call of ONE library: settings cleared and - where
    the library has them - set, alternating call by call.  Prints one JSON line of wall times in seconds."""
    assert not emspec._libs, "a library was loaded before the child chose its own"
    emspec.LIB_PATH = os.path.abspath(args.child)
    lib = emspec.load()
    has = hasattr(lib, "emspec_set_level_out")
    f32 = np.fromfile(os.path.join(args.data, "pcm.f32"), np.float32).reshape(S, L)
    pins = []

    def pinned(shape, dtype, fill=None):
        p = emspec.PinnedArray(shape, dtype)
        if fill is not None:
            p.array[...] = fill
        pins.append(p)
        return p.array

    s16 = np.round(np.clip(f32, -1, 1) * 32767).astype(np.int16)
    st = np.empty((S // 4, L, 2), np.int16)
    st[:, :, 0], st[:, :, 1] = s16[0::4], s16[1::4]
    stereo = pinned((S // 4, 2 * L), np.int16, st.reshape(S // 4, 2 * L))
    src = pinned((S, L), np.float32, f32)
    frames = pinned((S, n), np.float32, f32[:, :n])
    del st, s16, f32
    lrms = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
    wire = pinned((S * emspec.wire_bound(Cn, R),), np.uint8)
    index = pinned((S, Cn, R), np.uint8)
    level = pinned((S * Cn * 24,), np.uint8)
    cross = pinned((S // 4 * Cn * 16,), np.uint8)
    ldb = pinned((S, R), np.float32)
    offs = np.zeros(S + 1, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    res = {"library": emspec.build_info(), "has_level": has}

    def settings(e, state, pcm):
        if has:
            e._chk(lib.emspec_set_level_out(e._h, p(level) if state != "cleared" else None, S * Cn))
            e._chk(lib.emspec_set_cross_out(e._h, 0, 1, p(cross) if state == "both" and pcm else None, S // 4 * Cn))

    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            h = e._h
            out = emspec.Out(None, None, index.ctypes.data)
            entries = {"pcm_packed": lambda: e._chk(lib.emspec_batch_pcm_packed(h, p(stereo), C.byref(lrms), S // 4, L, n, hop, 1, p(wire),
                                                                                 C.c_int64(wire.size), p(offs))),
                       "index": lambda: e._chk(lib.emspec_batch(h, p(src), S, L, n, hop, 1, C.byref(out)))}
            for key, fn in entries.items():
                states = [s for s in STATES if has or s == "cleared"]
                if key == "index":
                    states = [s for s in states if s != "both"]      # (cross records are of PCM sources)
                t = {s: [] for s in states}
                for i in range(2 + args.calls):
                    for state in states:
                        settings(e, state, key == "pcm_packed")
                        t0 = time.perf_counter()
                        fn()
                        if i >= 2:
                            t[state].append(time.perf_counter() - t0)
                settings(e, "cleared", False)
                res[f"{name}_{key}"] = t
            if mode == emspec.MODE_FAST:
                ts = []
                for i in range(330):
                    t0 = time.perf_counter()
                    e.columns(frames, hop, True, want_db=True, want_rgba=False, db=ldb)
                    if i >= 30:
                        ts.append(time.perf_counter() - t0)
                res["FAST_live"] = {"cleared": ts}
    print(json.dumps(res))
    for q in pins:
        q.close()


def events(fn, steps=20, warm=3):
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


FACTORS = (1, 64, 65536)


def kernels_child():
    """Times the three kernels of ONE library at the three factors.  Prints one JSON line of seconds per launch."""
    assert not emspec._libs, "a library was loaded before the child chose its own"
    emspec.LIB_PATH = os.path.abspath(args.child)
    emspec.load()
    from bench import synth_device
    dev = torch.device("cuda", 0)
    x = synth_device(S, L, 0, dev)
    res = {"library": emspec.build_info()}
    with emspec.Engine() as e:
        for f in FACTORS:
            Cr = emspec.reduced_columns(Cn, f)
            wv = torch.empty((S, Cr, 2), dtype=torch.float32, device=dev)
            lv = torch.empty((S, Cr, 24), dtype=torch.uint8, device=dev)
            cr = torch.empty((S // 4, Cr, 16), dtype=torch.uint8, device=dev)
            res[f"wave_f{f}"] = events(lambda: e.wave_device(x, n, hop, f, out=wv))
            res[f"level_f{f}"] = events(lambda: e.level_device(x, n, hop, f, out=lv))
            res[f"cross_f{f}"] = events(lambda: e.cross_device(x, 4, 0, 1, n, hop, f, out=cr))
            e.device_status()
    print(json.dumps(res))


if args.child:
    kernels_child() if args.kernels else child()
    sys.exit(0)

from bench import synth_device

lib = emspec.load()
dev = torch.device("cuda", 0)
lines, res = [], {"streams": S, "columns": S * Cn, "library": emspec.build_info()}
here = emspec.LIB_PATH
order = [here, args.parent] * args.rounds if args.parent else [here] * args.rounds
med = statistics.median


def children(extra):
    """A child process per entry of `order` -> {library path: [its JSON lines]}"""
    runs = {here: [], args.parent: []}
    for path in order:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--calls", str(args.calls), "--streams", str(S)] + extra,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:   # (nothing more is started on the GPU behind a failure)
            sys.exit(f"child for {path} failed ({r.returncode}): {r.stderr[-500:]}")
        runs[path].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"  ({len(runs[path])} of {args.rounds}: {os.path.relpath(path, ROOT)})", file=sys.stderr, flush=True)
    return runs


def against_parent(mine, pr):
    """The margin rule: `mine` and `pr` are the rounds' values of this build and of the parent -> (text, inside the margin)"""
    lo, hi, diff = min(pr), max(pr), med(mine) - med(pr)
    ok = diff <= hi - lo
    verdict = ("every round inside the parent's range" if all(lo <= v <= hi for v in mine) else "within the margin of the medians" if abs(diff) <= hi - lo
               else "FASTER than the parent beyond its spread" if diff < 0 else "SLOWER than the parent beyond its spread")
    return (f"parent's rounds {', '.join(f'{v * 1e3:.4f}' for v in pr)} ms (median {med(pr) * 1e3:.4f}, margin {(hi - lo) * 1e3:.4f});  this build's rounds "
            f"{', '.join(f'{v * 1e3:.4f}' for v in mine)} ms;  median - median {diff * 1e3:+.4f} ms: {verdict}"), ok


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f"# {res['library']}; {S} streams x 2^22 samples, N = {n}, hop {hop}: {S * Cn} columns; {S * Cn * hop * 4 / 1e9:.2f} GB of samples under them")

# 1. the kernels, in child processes (one library each)
say(f"# 1. kernels: HIP events, 20 launches after 3, a process per round, {args.rounds} rounds, the median of the rounds; bytes = the samples a kernel "
    "reads (the cross kernel reads 2 of every 4 streams)")
runs = children(["--kernels"])
gb = S * Cn * hop * 4 / 1e9
for f in FACTORS:
    if not runs[here]:
        break
    how = "one team of lanes per window" if min(f, Cn) * hop <= 16384 else "pieces of 65536 samples over workgroups, integer atomics"
    say(f"factor {f:<5d} (windows of {min(f, Cn) * hop} samples, {how}):")
    t_w = med([r[f"wave_f{f}"] for r in runs[here]])
    for key, label, share in (("wave", "envelope", 1), ("level", "level", 1), ("cross", "cross", 2)):
        mine = [r[f"{key}_f{f}"] for r in runs[here]]
        t = med(mine)
        res[f"f{f}_{key}_ms"] = t * 1e3
        say(f"    {label + ' kernel':16s}{t * 1e3:7.3f} ms = {gb / share / t:5.0f} GB/s of samples read" + (f" = {t / t_w:.2f} x the envelope's time" if key != "wave" else ""))
        if args.parent and runs[args.parent]:
            text, ok = against_parent(mine, [r[f"{key}_f{f}"] for r in runs[args.parent]])
            res[f"f{f}_{key}_inside"] = ok
            say(f"{'':20s}{text}")

# 2. + 3. the host entries, in child processes (one library each), this build and the parent alternating
tmp = tempfile.mkdtemp(prefix="level_rate_")
synth_device(S, L, 0, dev).cpu().numpy().tofile(os.path.join(tmp, "pcm.f32"))
torch.cuda.empty_cache()
runs = children(["--data", tmp])
os.remove(os.path.join(tmp, "pcm.f32"))
os.rmdir(tmp)
say(f"# 2. host entries, settings on against cleared: alternating call by call, {args.calls} calls each after 2, {len(runs[here])} processes; page-locked "
    f"buffers; median over all calls; columns/s = {S * Cn} columns / median")
say(f"# 3. the same entries, cleared and set, and the live block call against the parent's library "
    f"({runs[args.parent][0]['library'] if args.parent and runs[args.parent] else 'not given'}): processes alternating; margin = max - min of the "
    "medians of the parent's own rounds")
rows = [(f"{name}_{key}", f"{name:5s} {label}") for name in ("FAST", "EXACT")
        for key, label in (("pcm_packed", "emspec_batch_pcm_packed S16 stereo L R M S"), ("index", "emspec_batch index out"))]
rows.append(("FAST_live", "FAST  emspec_columns 64 streams, dB out (per call)"))
for k, label in rows:
    if not runs[here]:
        break
    cl = [t for r in runs[here] for t in r[k]["cleared"]]
    line = f"{label:52s} cleared {med(cl) * 1e3:8.3f} ms"
    res[k + "_cleared_ms"] = med(cl) * 1e3
    for state in ("level", "both"):
        st = [t for r in runs[here] for t in r[k].get(state, [])]
        if st:
            res[f"{k}_{state}_ms"] = med(st) * 1e3
            line += f"  {state} {med(st) * 1e3:8.3f} ms ({(med(st) - med(cl)) * 1e3:+6.2f} ms = {(med(st) / med(cl) - 1) * 100:+5.1f} %)"
    say(line)
    if args.parent and runs[args.parent]:
        assert all(r["library"] != res["library"] for r in runs[args.parent]), "the parent's library is this build"
        for state in STATES:   # (a parent without the settings has the cleared state only)
            pr = [med(r[k][state]) for r in runs[args.parent] if r[k].get(state)]
            mine = [med(r[k][state]) for r in runs[here] if r[k].get(state)]
            if pr and mine:
                text, ok = against_parent(mine, pr)
                res[f"{k}_{state}_parent_ms"], res[f"{k}_{state}_inside"] = med(pr) * 1e3, ok
                say(f"{'':8s}{state:8s}{text}")
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
