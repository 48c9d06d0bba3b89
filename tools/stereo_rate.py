#!/usr/bin/env python3
"""Rates of the stereo image (emspec_stereo_device, emspec_batch_pcm_stereo, emspec_history_view_stereo),
one process on one box, warm-up then medians of repeats:
  compose  the compose kernel on the bench shape's dB (32 pairs = 64 streams x 2^22 samples, N = 4096, hop 256: 16,369 columns of
           1,024 rows per stream), index + pan out, RGBA out, all four outputs; HIP events, 20 launches after 3, five repeats:
           median ms, the spread of the repeats, bytes moved and TB/s.  Beside it in the same run, on the same cells: the peaks
           kernel at k = 1 (emspec_peaks_device) and the time reduction's kernel (dB only, f = 64: the difference of
           emspec_batch_device's dB time at factor 64 and at factor 1, the only way the library exposes it), and a device copy of
           the array (torch: 4 B read + 4 B written per cell).
  host     emspec_batch_pcm_stereo (index + pan, and RGBA) beside emspec_batch_pcm_packed and emspec_batch_pcm index out, 32 stereo
           S16 sources x 2^22 frames decoded to left / right, page-locked buffers, FAST and EXACT, with the copy in timed alone.
  view     the stereo history view at 32 pairs x 2,000 groups x 1,024 rows, f = 1 and 4, index + pan and RGBA, beside the mono
           view of the same 64 streams (index, RGBA): HIP events.
  unchanged --lib PARENT.so [--rounds 3]
           the paths this feature must not slow down, this build against another build of the library (the parent commit's, built
           from a clean export of its sources), alternating, a fresh process each: emspec_batch index out and
           emspec_batch_pcm_packed from page-locked buffers (median of 5 calls), the live block call with nothing set (64 streams x
           one hop, median of 600 calls) and the mono history view (64 streams x 2,000 groups, f = 4, RGBA; HIP events).
   python tools/stereo_rate.py [compose] [host] [view] [unchanged --lib PATH] [--out profiles/stereo_rate.txt]   (needs an MI355X)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
import numpy as np
import torch

import emspec
from bench import synth_device
from emspec import synth

ap = argparse.ArgumentParser()
ap.add_argument("parts", nargs="*", default=["compose", "host", "view"])
ap.add_argument("--out")
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--lib", help="unchanged: the other build of the library")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--child", help=argparse.SUPPRESS)       # (unchanged: one process per library and round)
args = ap.parse_args()
if args.child:
    emspec.LIB_PATH = os.path.abspath(args.child)
lib = emspec.load()
PAIRS, L, N, HOP, R = args.pairs, 1 << 22, 4096, 256, 1024
S = 2 * PAIRS
dev = torch.device("cuda", 0)
Cn = emspec.num_columns(L, N, HOP)
hip = C.CDLL("libamdhip64.so")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


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


def repeats(fn, n=5, **kw):
    t = [events(fn, **kw) for _ in range(n)]
    return float(np.median(t)), float(max(t) - min(t))


def wall(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(max(t) - min(t))


def compose():
    x = synth_device(S, L, 0, dev)
    with emspec.Engine() as e:
        db = torch.empty((S, Cn, R), dtype=torch.float32, device=dev)
        e.batch_device(x, N, HOP, True, db=db)
        torch.cuda.synchronize()
        cells, pcells = S * Cn * R, PAIRS * Cn * R
        say(f"1. compose kernel: {PAIRS} pairs x {Cn} columns x {R} rows = {pcells / 1e6:.0f} M pair cells, {cells * 4 / 1e9:.2f} GB of dB read")
        lv = torch.empty((PAIRS, Cn, R), dtype=torch.float32, device=dev)
        ix = torch.empty((PAIRS, Cn, R), dtype=torch.uint8, device=dev)
        pn = torch.empty((PAIRS, Cn, R), dtype=torch.uint8, device=dev)
        rg = torch.empty((PAIRS, Cn, R, 4), dtype=torch.uint8, device=dev)
        for what, kw, wbytes in (("index + pan", dict(index=ix, pan=pn), 2), ("RGBA", dict(rgba=rg), 4),
                                 ("level + index + pan + RGBA", dict(level=lv, index=ix, pan=pn, rgba=rg), 10)):
            dt, spread = repeats(lambda: e.stereo_device(db, 2, 0, 1, want=(), **kw))
            moved = cells * 4 + pcells * wbytes
            say(f"   emspec_stereo_device {what:27s}: {dt * 1e3:7.3f} ms (spread {spread * 1e3:.3f})  {moved / 1e9:.2f} GB moved  {moved / dt / 1e12:.2f} TB/s")
        pan = np.bincount(pn[0, :2000].cpu().numpy().ravel(), minlength=33)
        say(f"   (balance bytes of the first 2,000 columns of pair 0: {int((pan > 0).sum())} of 33 values occur, {pan[16] / pan.sum() * 100:.0f} % centre)")
        del lv, ix, pn, rg
        out = torch.empty((S, Cn, 1, 2), dtype=torch.float32, device=dev)
        dt, spread = repeats(lambda: e.peaks_device(db, 1, -60.0, out=out))
        say(f"   emspec_peaks_device k=1 on the same cells        : {dt * 1e3:7.3f} ms (spread {spread * 1e3:.3f})  {cells * 4 / 1e9:.2f} GB read     {cells * 4 / dt / 1e12:.2f} TB/s")
        del out
        cp = torch.empty_like(db)
        dt, spread = repeats(lambda: cp.copy_(db))
        say(f"   device copy of the array (torch)                  : {dt * 1e3:7.3f} ms (spread {spread * 1e3:.3f})  {cells * 8 / 1e9:.2f} GB moved  {cells * 8 / dt / 1e12:.2f} TB/s")
        del cp
        t1, s1 = repeats(lambda: e.batch_device(x, N, HOP, True, db=db), n=3, steps=6, warm=2)
        e.set_time_reduce(64)
        rdb = torch.empty((S, -(-Cn // 64), R), dtype=torch.float32, device=dev)
        t64, s64 = repeats(lambda: e.batch_device(x, N, HOP, True, db=rdb), n=3, steps=6, warm=2)
        e.set_time_reduce(1)
        add = t64 - t1
        say(f"   reduce_columns_kernel dB only, f = 64             : {add * 1e3:7.3f} ms = {cells * 4 / add / 1e12 if add > 0 else float('inf'):.2f} TB/s of the dB it reads "
            f"(emspec_batch_device dB at factor 64, {t64 * 1e3:.2f} ms (spread {s64 * 1e3:.2f}), minus factor 1, {t1 * 1e3:.2f} ms (spread {s1 * 1e3:.2f}))")


def host():
    x = synth_device(S, L, 0, dev)
    raw_t = (torch.stack([x[0::2], x[1::2]], dim=-1).reshape(PAIRS, -1) * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
    pin = emspec.PinnedArray((PAIRS, 2 * L), np.int16)
    pin.array[...] = raw_t.cpu().numpy()
    del x, raw_t
    fmt = emspec.PcmFormat.make("s16", 2, views=["left", "right"])
    pix = emspec.PinnedArray((PAIRS, Cn, R), np.uint8)
    ppn = emspec.PinnedArray((PAIRS, Cn, R), np.uint8)
    prg = emspec.PinnedArray((PAIRS, Cn, R, 4), np.uint8)
    pall = emspec.PinnedArray((S, Cn, R), np.uint8)
    wire = emspec.PinnedArray((S * emspec.wire_bound(Cn, R),), np.uint8)
    say(f"2. host entries: {PAIRS} stereo S16 sources x 2^22 frames ({pin.array.nbytes / 1e6:.0f} MB in) -> {S} streams x {Cn} columns, page-locked buffers; median of 5 calls")
    d_in = torch.empty(pin.array.nbytes, dtype=torch.uint8, device=dev)
    t_in, sp = wall(lambda: hip.hipMemcpy(C.c_void_p(d_in.data_ptr()), C.c_void_p(pin.array.ctypes.data), C.c_size_t(pin.array.nbytes), 1))
    del d_in
    say(f"   copy in alone                                 : {t_in * 1e3:7.1f} ms (spread {sp * 1e3:.1f})  {S * Cn / t_in:.3e} columns/s")
    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            runs = (("emspec_batch_pcm_stereo index + pan", lambda: e.batch_pcm_stereo(pin.array, fmt, N, HOP, True, 0, 1, want=(), index=pix.array, pan=ppn.array),
                     pix.array.nbytes + ppn.array.nbytes),
                    ("emspec_batch_pcm_stereo RGBA", lambda: e.batch_pcm_stereo(pin.array, fmt, N, HOP, True, 0, 1, want=(), rgba=prg.array), prg.array.nbytes),
                    ("emspec_batch_pcm_packed", lambda: e.batch_pcm_packed(pin.array, fmt, N, HOP, True, wire=wire.array), 0),
                    ("emspec_batch_pcm index out", lambda: lib.emspec_batch_pcm(e._h, C.c_void_p(pin.array.ctypes.data), C.byref(fmt), PAIRS, L, N, HOP, 1,
                                                                               C.byref(emspec.Out(None, None, C.c_void_p(pall.array.ctypes.data)))), pall.array.nbytes))
            for what, fn, out_bytes in runs:
                dt, sp = wall(fn)
                say(f"   {name:5s} {what:36s}: {dt * 1e3:7.1f} ms (spread {sp * 1e3:.1f})  {S * Cn / dt:.3e} columns/s" + (f"  {out_bytes / 1e6:.0f} MB out" if out_bytes else ""))
    for p in (pin, pix, ppn, prg, pall, wire):
        p.close()


def fill(e, streams, columns):
    """Emit `columns` columns on each stream: the same block of one launch's frames over and over, no output."""
    per = 32 if streams > 32 else 64
    block = synth.streams(min(streams, 8), per * HOP)
    block = np.ascontiguousarray(np.tile(block, ((streams + 7) // 8, 1))[:streams])
    e.push_samples_multi(np.ascontiguousarray(block[:, :N - HOP]), N, HOP, True, want_db=False)
    done = 0
    while done < columns:
        e.push_samples_multi(block, N, HOP, True, want_db=False)
        done = e.live_history(0)[0]
    return done


def view():
    G = 2000
    say(f"3. history views: {PAIRS} pairs ({S} streams) x {G} groups x {R} rows; HIP events, 20 views after 3, median of 5 repeats")
    for f in (1, 4):
        Wn = G * f
        with emspec.Engine() as e:
            e.set_live_history(Wn)
            end = fill(e, S, Wn)
            first = end - Wn
            pcells, cells = PAIRS * G * R, S * G * R
            ix = torch.empty((PAIRS, G, R), dtype=torch.uint8, device=dev)
            pn = torch.empty((PAIRS, G, R), dtype=torch.uint8, device=dev)
            rg = torch.empty((PAIRS, G, R, 4), dtype=torch.uint8, device=dev)
            mi = torch.empty((S, G, R), dtype=torch.uint8, device=dev)
            mr = torch.empty((S, G, R, 4), dtype=torch.uint8, device=dev)
            for what, fn, wbytes in (("stereo view index + pan", lambda: e.history_view_stereo_device(first, f, G, 2, 0, 1, want=(), index=ix, pan=pn), pcells * 2),
                                     ("stereo view RGBA", lambda: e.history_view_stereo_device(first, f, G, 2, 0, 1, want=(), rgba=rg), pcells * 4),
                                     ("mono view of the 64 streams, index", lambda: e.history_view_device(first, f, G, index=mi), cells),
                                     ("mono view of the 64 streams, RGBA", lambda: e.history_view_device(first, f, G, rgba=mr), cells * 4)):
                dt, sp = repeats(fn)
                moved = cells * f * 4 + wbytes
                say(f"   f={f}  {what:36s}: {dt * 1e3:7.3f} ms (spread {sp * 1e3:.3f})  {moved / 1e9:.2f} GB moved  {moved / dt / 1e12:.2f} TB/s")
            del ix, pn, rg, mi, mr


def unchanged_child():
    """The four figures of one library, as a JSON line."""
    res = {}
    x = synth_device(S, L, 0, dev)
    pin = emspec.PinnedArray((S, L), np.float32)
    pin.array[...] = x.cpu().numpy()
    raw_t = (torch.stack([x[0::2], x[1::2]], dim=-1).reshape(PAIRS, -1) * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
    praw = emspec.PinnedArray((PAIRS, 2 * L), np.int16)
    praw.array[...] = raw_t.cpu().numpy()
    del x, raw_t
    fmt = emspec.PcmFormat.make("s16", 2, views=["left", "right"])
    pix = emspec.PinnedArray((S, Cn, R), np.uint8)
    wire = emspec.PinnedArray((S * emspec.wire_bound(Cn, R),), np.uint8)
    with emspec.Engine() as e:
        o = emspec.Out(None, None, C.c_void_p(pix.array.ctypes.data))
        res["batch_index_ms"] = wall(lambda: lib.emspec_batch(e._h, C.c_void_p(pin.array.ctypes.data), S, L, N, HOP, 1, C.byref(o)))[0] * 1e3
        res["pcm_packed_ms"] = wall(lambda: e.batch_pcm_packed(praw.array, fmt, N, HOP, True, wire=wire.array))[0] * 1e3
    for p in (pin, praw, pix, wire):
        p.close()
    calls = 600
    pcm = synth.streams(8, N + HOP * (calls + 4))
    pcm = np.ascontiguousarray(np.tile(pcm, (S // 8 + 1, 1))[:S])
    with emspec.Engine() as e:
        keep = [emspec.PinnedArray((S, HOP), np.float32), emspec.PinnedArray((S, 1, R), np.float32)]
        fin, db = keep[0].array, keep[1].array
        e.push_samples_multi(pcm[:, :N - HOP].copy(), N, HOP, True, want_db=False, db=None)
        ts = np.empty(calls)
        for i in range(calls):
            fin[:] = pcm[:, N - HOP + i * HOP:N + i * HOP]
            t0 = time.perf_counter()
            e.push_samples_multi(fin, N, HOP, True, db=db)
            ts[i] = time.perf_counter() - t0
        res["live_block_us"] = float(np.median(ts[calls // 10:])) * 1e6
        for p in keep:
            p.close()
    G, f = 2000, 4
    with emspec.Engine() as e:
        e.set_live_history(G * f)
        end = fill(e, S, G * f)
        mr = torch.empty((S, G, R, 4), dtype=torch.uint8, device=dev)
        res["mono_view_ms"] = repeats(lambda: e.history_view_device(end - G * f, f, G, rgba=mr))[0] * 1e3
    print(json.dumps(res))


def unchanged():
    if not args.lib:
        sys.exit("unchanged needs --lib PATH (the parent commit's libemspec.so)")
    say(f"4. unchanged paths, this build against {os.path.basename(os.path.dirname(os.path.abspath(args.lib))) or 'the other'} build, {args.rounds} alternating rounds, a process each")
    names = (("batch_index_ms", "emspec_batch index out, pinned (ms)"), ("pcm_packed_ms", "emspec_batch_pcm_packed S16 stereo -> L R (ms)"),
             ("live_block_us", "live block call, nothing set (us per call)"), ("mono_view_ms", "mono history view 64 x 2,000 x 1,024, f = 4, RGBA (ms)"))
    got = {"parent": [], "this": []}
    for r in range(args.rounds):
        for who, path in (("parent", args.lib), ("this", emspec.LIB_PATH)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--pairs", str(PAIRS)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(out.stderr[-2000:])
            got[who].append(json.loads(out.stdout.strip().splitlines()[-1]))
    for key, label in names:
        fmt_ = "%.1f" if key == "live_block_us" else "%.3f"
        say(f"   {label:56s}: parent " + "  ".join(fmt_ % g[key] for g in got["parent"]) + "   this build " + "  ".join(fmt_ % g[key] for g in got["this"]))


if args.child:
    unchanged_child()
    sys.exit(0)
say(f"# {emspec.build_info()}; tools/stereo_rate.py {' '.join(args.parts)}")
for part in args.parts:
    {"compose": compose, "host": host, "view": view, "unchanged": unchanged}[part]()
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
