#!/usr/bin/env python3
"""CPU model of the two data-dependent LDS accesses of the headline kernel's per-bin stage (fused4096_pp_kernel, N = 4096,
hop 256, 1024 rows): the row lookup's reads of the edge table, in both forms, and the first round of the ring accumulate
(exchange + store).  It answers where SQ_LDS_BANK_CONFLICT comes from, without a GPU.

  input    F frames of the bench's synthetic stream (emspec.synth.streams), past its onset
  k-hat    three-window reassignment in numpy (float64): Hann, time-weighted Hann, derivative of Hann
  lanes    thread t of a frame's 512 owns bin group bg = ((t & 63) << 3) | (t >> 6), bins 4 bg .. 4 bg + 3 (fused_pp.hip.inc);
           wave w = t >> 6, one instruction per bin slot e = 0 .. 3 and wave
  LDS      a 64-lane instruction is served as two groups of 32 lanes; 32 banks of 4 bytes; lanes of a group that read the same
           dword are served together (broadcast), so a group costs max over banks of the DISTINCT dwords in that bank
  table    two-edge form: eb[r0] and eb[r0 + 1], r0 = clamp(int(h), 0, R - 1)   (two dwords per bin)
           nearest-edge form: eb[m], m = clamp(int(h + 1/2), 0, R)              (one dword per bin; emspec_row_hint.h)
  ring     cell = slot * R + row, slot = (frame + dcol) mod 18; a thread merges neighbouring bins that share a cell first; gated
           bins are masked off; exchange and store each touch the cell once (first round only: a lane that loses the cell to
           another lane of its wave retries, and those rounds come on top; the model counts the same-wave collisions)

Prints array cycles per wave and frame beside the conflict-free cost, and the extra cycles per two-frame iteration of a
workgroup (16 wave-frames).  usage: tools/lds_conflict_model.py [frames, default 400]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "em-spec_amd")]
from emspec import synth

N, HOP, R, D, SLOTS, BANKS = 4096, 256, 1024, 8, 18, 32
FS, FMIN, FMAX, FLOOR = 48000.0, 20.0, 24000.0, 1e-12
F = int(sys.argv[1]) if len(sys.argv) > 1 else 400


def cycles(addr, mask):
    """LDS-array cycles of one 64-lane dword access: per 32-lane group, the largest number of distinct dwords in one bank."""
    tot = 0
    for g in (slice(0, 32), slice(32, 64)):
        a = np.unique(addr[g][mask[g]])
        if a.size:
            tot += int(np.bincount(a % BANKS, minlength=BANKS).max())
    return tot


def main():
    x = synth.streams(1, N + HOP * (F - 1) + 48000)[0][24000:].astype(np.float64)
    n = np.arange(N)
    h = 0.5 - 0.5 * np.cos(2 * np.pi * n / N)
    th = (n - N / 2) * h
    dh = np.pi / N * np.sin(2 * np.pi * n / N)
    edges = (FMIN * (FMAX / FMIN) ** (np.arange(R + 1) / R) * N / FS).astype(np.float32).astype(np.float64)
    l2e0 = np.log2(edges[0])
    rscale = R / (np.log2(edges[-1]) - l2e0)
    t = np.arange(512)
    bg = ((t & 63) << 3) | (t >> 6)
    everyone = np.ones(64, bool)
    two = one = ring = ring_free = 0
    ring_instr = same_wave = 0
    for j in range(F):
        fr = x[j * HOP:j * HOP + N]
        Xh, Xt, Xd = np.fft.rfft(fr * h), np.fft.rfft(fr * th), np.fft.rfft(fr * dh)
        den = np.abs(Xh) ** 2 + 1e-300
        tshift = np.real(Xt * np.conj(Xh)) / den
        kh = np.arange(N // 2 + 1) - np.imag(Xd * np.conj(Xh)) / den * N / (2 * np.pi)
        cf = np.floor(tshift / HOP + 0.5)
        ok = (den / (N * N / 16.0) >= FLOOR) & (np.abs(cf) <= D) & (kh >= edges[0]) & (kh < edges[-1])
        hint = (np.log2(np.maximum(kh, 1e-9)) - l2e0) * rscale
        r0 = np.clip(hint.astype(np.int64), 0, R - 1)
        m = np.clip((hint + 0.5).astype(np.int64), 0, R)
        row = np.clip(np.searchsorted(edges, kh, side="right") - 1, 0, R - 1)
        cell = ((j + cf.astype(np.int64)) % SLOTS) * R + row
        for w in range(8):
            g = bg[np.arange(64) + 64 * w]
            cells = np.stack([cell[4 * g + e] for e in range(4)])
            oks = np.stack([ok[4 * g + e] for e in range(4)])
            for e in range(3):      # a thread merges a bin into its next one when both land in the same cell
                oks[e] &= ~(oks[e] & oks[e + 1] & (cells[e] == cells[e + 1]))
            for e in range(4):
                k = 4 * g + e
                two += cycles(r0[k], everyone) + cycles(r0[k] + 1, everyone)
                one += cycles(m[k], everyone)
                if oks[e].any():
                    ring += 2 * cycles(cells[e], oks[e])
                    ring_free += 2 * (int(oks[e][:32].any()) + int(oks[e][32:].any()))
                    ring_instr += 1
                    same_wave += int(np.unique(cells[e][oks[e]], return_counts=True)[1].max()) - 1
    wf = F * 8
    free = 4 * 2 * 2        # 4 bin slots x 2 dwords x 2 groups: one cycle per group and dword
    print(f"model: {F} frames of the bench stream, N = {N}, hop {HOP}, {R} rows; {wf} wave-frames")
    print("access                                   array cycles per wave and frame   conflict-free   extra per two-frame iteration")
    print(f"edge table, two-edge form (2 dwords/bin)   {two / wf:8.1f}                          {free:4d}            {(two / wf - free) * 16:6.0f}")
    print(f"edge table, nearest-edge form (1 dword)    {one / wf:8.1f}                          {free // 2:4d}            {(one / wf - free // 2) * 16:6.0f}")
    print(f"ring exchange + store, first round         {ring / wf:8.1f}                       <= {free:4d}            {(ring - ring_free) / wf * 16:6.0f}")
    print(f"ring accumulate instructions per wave and frame {ring_instr / wf:.2f} of 4; same-wave collisions (extra rounds) per wave and frame {same_wave / wf:.2f}")
    print(f"table form change: {(one - two) / wf:+.1f} array cycles per wave and frame, {(one - two) / wf * 16:+.0f} per two-frame iteration, "
          f"{(one - two) / wf * 8:+.0f} per column")


if __name__ == "__main__":
    main()
