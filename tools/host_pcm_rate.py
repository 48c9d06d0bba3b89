#!/usr/bin/env python3
"""Rates of the PCM host entries against the float entry measured IN THE SAME RUN (profiles/host_pcm_rate.txt).
Bench shape: 64 streams x 2^22 samples, N = 4096, hop 256, reassign on; page-locked buffers; one process, one GPU;
median of >= 7 calls after 2 warm-ups, FAST and EXACT.  Cases: emspec_batch_packed float32 (the yardstick, 4 input bytes per
stream-sample), emspec_batch_pcm_packed F32 mono (4), S16 mono (2), S16 stereo -> L R M S from 16 sources (1), and
emspec_batch_pcm palette index out from S16 mono (2; D2H-bound).
Beside every call's wall time the tool times its three stages BY THEMSELVES, in the same process on the same data: the
copy in (the case's input bytes, page-locked host -> device), the compute stream's work on device-resident data (decode
kernel for the PCM cases + emspec_batch_device + one emspec_wire_pack per stream for the packed cases), and the copy out
(the bytes the call really returned: the wire images' total, or the index columns).  The pipeline overlaps the three, so
a call cannot be faster than the longest of them; which one that is, is the call's bound.

    python tools/host_pcm_rate.py [--calls 7] [--streams 64] [--log2-samples 22] > profiles/host_pcm_rate.txt
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
from emspec import synth  # noqa: E402


def timed(fn, calls):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def stage_times(e, torch, calls, S, L, n, hop, Cn, in_bytes, out_bytes, raw_dev, fmt, sources, packed, bufs):
    """(H2D, compute, D2H) medians in seconds, each stage alone."""
    pin, dev, pcm_dev, idx_dev, wire_dev = bufs

    def h2d():
        dev[:in_bytes].copy_(pin[:in_bytes], non_blocking=True)
        torch.cuda.synchronize()

    def d2h():
        pin[:out_bytes].copy_(dev[:out_bytes], non_blocking=True)
        torch.cuda.synchronize()

    def compute():
        if fmt is not None:
            e.pcm_decode_device(raw_dev, fmt, sources, L, out=pcm_dev)
        e.batch_device(pcm_dev, n, hop, True, index=idx_dev)
        if packed:
            for s_ in range(S):
                e.wire_pack(idx_dev[s_], wire_dev, want_size=False)
        torch.cuda.synchronize()

    return timed(h2d, calls)[0], timed(compute, calls)[0], timed(d2h, calls)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--log2-samples", type=int, default=22)
    a = ap.parse_args()
    S, L, n, hop = a.streams, 1 << a.log2_samples, 4096, 256
    assert S % 4 == 0
    Cn = emspec.num_columns(L, n, hop)
    print(f"# {emspec.build_info()}")
    print(f"# {S} streams x 2^{a.log2_samples} samples, N = {n}, hop {hop}, reassign on; pinned buffers; median of {a.calls} calls after 2 warm-ups")
    print("# columns/s = streams x columns / median; spread = max - min of the calls")
    print("# stages alone [ms]: copy in of the case's input bytes | decode + kernels (+ pack) on resident data | copy out of the bytes returned")
    import torch
    pcm = synth.streams(S, L)
    pins = []

    def pinned(arr):
        p = emspec.PinnedArray(arr.shape, arr.dtype)
        p.array[...] = arr
        pins.append(p)
        return p.array

    f32 = pinned(pcm)
    s16 = pinned(np.round(np.clip(pcm, -1, 1) * 32767).astype(np.int16))
    # 16 stereo sources whose L R M S views are 64 streams
    st = np.empty((S // 4, L, 2), np.int16)
    st[:, :, 0] = s16[0::4]
    st[:, :, 1] = s16[1::4]
    stereo = pinned(st.reshape(S // 4, 2 * L))
    del st, pcm
    tpin = torch.empty(S * L * 4, dtype=torch.uint8).pin_memory()
    tdev = torch.empty(S * L * 4, dtype=torch.uint8, device="cuda")
    pcm_dev = torch.from_numpy(f32).cuda()
    raw_f32, raw_s16, raw_st = pcm_dev.clone().view(torch.uint8), torch.from_numpy(s16).cuda(), torch.from_numpy(stereo).cuda()
    mono_f32 = emspec.PcmFormat.make("f32", 1, views=["mono"])
    mono_s16 = emspec.PcmFormat.make("s16", 1, views=["mono"])
    lrms = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
    for mode, name in ((emspec.MODE_FAST, "FAST"), (emspec.MODE_EXACT, "EXACT")):
        with emspec.Engine(mode=mode) as e:
            wire = emspec.PinnedArray((S * emspec.wire_bound(Cn, e.rows),), np.uint8)
            index = emspec.PinnedArray((S, Cn, e.rows), np.uint8)
            offs = np.zeros(S + 1, np.int64)
            p = lambda arr: C.c_void_p(arr.ctypes.data)
            lib, h = e._lib, e._h

            def packed_float():
                e._chk(lib.emspec_batch_packed(h, p(f32), S, L, n, hop, 1, p(wire.array), C.c_int64(wire.array.size), p(offs)))

            def packed_pcm(src, fmt, sources):
                return lambda: e._chk(lib.emspec_batch_pcm_packed(h, p(src), C.byref(fmt), sources, L, n, hop, 1, p(wire.array),
                                                                  C.c_int64(wire.array.size), p(offs)))

            def index_pcm():
                out = emspec.Out(None, None, index.array.ctypes.data)
                e._chk(lib.emspec_batch_pcm(h, p(s16), C.byref(mono_s16), S, L, n, hop, 1, C.byref(out)))

            def index_float():
                out = emspec.Out(None, None, index.array.ctypes.data)
                e._chk(lib.emspec_batch(h, p(f32), S, L, n, hop, 1, C.byref(out)))

            # (label, input bytes per stream-sample, call, raw frames on the device, format, sources, packed)
            cases = [("emspec_batch_packed float32 (yardstick)", 4, packed_float, None, None, S, True),
                     ("emspec_batch_pcm_packed F32 mono, 1 view", 4, packed_pcm(f32, mono_f32, S), raw_f32, mono_f32, S, True),
                     ("emspec_batch_pcm_packed S16 mono, 1 view", 2, packed_pcm(s16, mono_s16, S), raw_s16, mono_s16, S, True),
                     (f"emspec_batch_pcm_packed S16 stereo, L R M S ({S // 4} sources)", 1, packed_pcm(stereo, lrms, S // 4), raw_st, lrms, S // 4, True),
                     ("emspec_batch index out, float32 (yardstick)", 4, index_float, None, None, S, False),
                     ("emspec_batch_pcm index out, S16 mono", 2, index_pcm, raw_s16, mono_s16, S, False)]
            idx_dev = torch.empty((S, Cn, e.rows), dtype=torch.uint8, device="cuda")
            wire_dev = torch.empty(emspec.wire_bound(Cn, e.rows), dtype=torch.uint8, device="cuda")
            base = None
            for label, bps, fn, raw_dev, fmt, sources, is_packed in cases:
                med, lo, hi = timed(fn, a.calls)
                if "yardstick" in label:
                    base = med
                out_bytes = int(offs[S]) if is_packed else S * Cn * e.rows
                t_in, t_k, t_out = stage_times(e, torch, a.calls, S, L, n, hop, Cn, S * L * bps, out_bytes, raw_dev, fmt, sources, is_packed,
                                               (tpin, tdev, pcm_dev, idx_dev, wire_dev))
                bound = max((t_in, "copy in"), (t_k, "compute"), (t_out, "copy out"))[1]
                print(f"{name:5s} {label:62s} in {bps} B/stream-sample  median {med * 1e3:8.2f} ms  spread {(hi - lo) * 1e3:6.2f} ms  "
                      f"{S * Cn / med:9.3e} columns/s  x{base / med:5.2f} of its yardstick  stages alone {t_in * 1e3:6.2f} | {t_k * 1e3:6.2f} | "
                      f"{t_out * 1e3:6.2f} ms ({S * L * bps / t_in / 1e9:4.1f} GB/s in, {out_bytes / t_out / 1e9:4.1f} GB/s out)  longest: {bound}")
            del idx_dev, wire_dev
            wire.close()
            index.close()
    for q in pins:
        q.close()


if __name__ == "__main__":
    main()
