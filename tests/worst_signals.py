"""Worst-case inputs of a scatter (plain numpy; shared by tests/test_worst_signals_cpu.py and tests/test_gpu_worst_signals.py).

Every parity test and fuzz tool feeds the kernels emspec.synth.streams: sinusoids + a chirp + noise + a click, whose energy is
spread over the image.  The inputs below pile it up instead: a stationary tone sends its main lobe and skirts of up to 2D + 1
frames into ONE cell, an impulse puts every bin of n / hop frames into one column, a 30 Hz tone lives in the lowest rows
only (the EXACT kernels keep those in an L2 scratch behind device-scope atomics), a level of 30 crosses the EXACT mode's upper
power gate.  conditions() measures on the CPU bit model what each signal is meant to provoke, so that a GPU pass cannot be vacuous
(tests/test_worst_signals_cpu.py asserts it for every shape of the GPU matrix).

Deterministic: no RNG beyond emspec.synth.uniform (through synth.stream)."""
import numpy as np

import oracle as O
from emspec import synth

KINDS = ("tone_centre", "tone_between", "tone_low", "impulses", "dc_nyquist", "loud", "chirp_reach", "step", "poisoned")
# the signals every shape of the GPU matrix runs (all nine run on the two shapes every mode serves with a kernel of its own)
CORE_KINDS = ("tone_centre", "tone_low", "impulses", "loud", "chirp_reach")


def length(n, hop, frames):
    return n + hop * (frames - 1)


def signal(kind, n, hop, frames, fs=48000.0):
    """float32 [L], L = n + hop (frames - 1)."""
    L = length(n, hop, frames)
    t = np.arange(L, dtype=np.float64)
    if kind == "tone_centre":            # 1/64 bin off the centre of bin n/8: one bin carries the energy, k-hat is about an integer,
        # and the skirts (about 50 bins a side above the power floor) all reassign into that bin's cell.  (Exactly ON the centre the
        # Hann spectrum has three non-zero bins and a cell receives three: no contention at all.)
        x = 0.9 * np.sin(2 * np.pi * (n // 8 + 1.0 / 64.0) * t / n)
    elif kind == "tone_between":         # half way between two bins: the worst leakage, two equal main bins
        x = 0.9 * np.sin(2 * np.pi * (n // 8 + 0.5) * t / n)
    elif kind == "tone_low":             # only the lowest rows carry energy; the skirts straddle the power floor
        x = 0.9 * np.sin(2 * np.pi * 30.0 * t / fs)
    elif kind == "impulses":             # all bins of n / hop frames into one column; the end impulses reassign out of the image
        x = np.zeros(L)
        x[1000::n + 37] = 1.0
        x[0] = 1.0                       # (the Hann window is 0 here and ~(pi / n)^2 at L - 1: below the power floor at every n ...
        x[L - 1] = 1.0
        # ... so one hop in from either end as well, where only the first / last frame holds them: to column 1 - D < 0 and to
        # column C - 2 + D >= C.  Amplitude 1000: a frame that also holds an impulse of the train reassigns most bins to the stronger
        # of the two after the window's weight, here sin^2(pi hop / n) >= 2.4e-3)
        x[hop] = 1000.0
        x[L - 1 - hop] = 1000.0
    elif kind == "dc_nyquist":           # energy exactly at k = 0 and k = n/2: both are dropped by the axis
        x = 0.5 + 0.4 * np.cos(np.pi * t)
    elif kind == "loud":                 # far outside [-1, 1]: bins above the EXACT mode's upper power gate (amplitude > 22.6)
        x = 30.0 * np.sin(2 * np.pi * 440.0 * t / fs) + 5.0 * np.sign(np.sin(2 * np.pi * 97.0 * t / fs))
    elif kind == "chirp_reach":          # 50 Hz -> 20 kHz over 2n samples, repeated: time offsets out to +-D and past it
        T = 2 * n
        tt = np.mod(t, T)
        x = 0.8 * np.sin(2 * np.pi * (50.0 * tt + 0.5 * ((20000.0 - 50.0) / T) * tt * tt) / fs)
    elif kind == "step":
        x = np.where(t < L // 2, 0.0, 0.8)
    elif kind == "poisoned":             # a NaN and an Inf: every bin of the frames that hold one is dropped
        x = synth.stream(0, L, fs).astype(np.float64)
        x[L // 3] = np.nan
        x[(2 * L) // 3] = np.inf
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def frames_for(n, hop):
    """3 (2D + 2) frames: every column ring (2D + 1 or 2D + 2 slots) wraps at least twice; 12 where that would be hundreds."""
    D = -(-n // (2 * hop))
    return 12 if D > 64 else 3 * (2 * D + 2)


def conditions(kind, cfg, x):
    """What the EXACT bit model does with x (one stream) at cfg: the counts that give each signal its point."""
    x = np.ascontiguousarray(x, np.float32)
    n, hop, R = cfg.n, cfg.hop, cfg.rows
    frames = O.num_columns(x.size, n, hop)
    log2n = n.bit_length() - 1
    qscale = 2.0 ** (52 - (2 * log2n - 4))
    pmax = 2.0 ** 61 / qscale
    pfloor = float(np.float32(cfg.power_floor)) * (n / 4.0) ** 2
    D = -(-n // (2 * hop)) if cfg.reassign else 0
    pw, col, row, q = O.frames_exact(cfg, x, 0, frames)
    _, _, _, hist = O.batch_exact(cfg, x[None], want=("hist",))
    with np.errstate(invalid="ignore"):
        above = pw > pmax
        passed = (pw >= pfloor) & (pw <= pmax)
        near_pass = (pw >= pfloor) & (pw < 2.0 * pfloor)
        near_fail = (pw < pfloor) & (pw > 0.5 * pfloor)
    acc = row >= 0
    # the reach gate |cf| > D: a bin that passed the power gates, was not accumulated, yet reassigns onto the axis - recomputed
    # here from the float64 three-window method (the bit model does not export cf; eo_frames_f64's t-hat is absolute)
    _, that, _, _, _ = O.frames_f64(cfg, x, 0, frames)
    with np.errstate(invalid="ignore"):
        ts = that - (np.arange(frames, dtype=np.float64)[:, None] * hop + n // 2)
        cf = np.floor(ts / hop + 0.5)
        reach = passed & ~acc & (np.abs(cf) > D)
    outside = acc & ((col < 0) | (col >= frames))
    inside = acc & ~outside
    per_cell = np.zeros((frames, R), np.int64)
    np.add.at(per_cell, (col[inside], row[inside]), 1)
    return {
        "kind": kind, "n": n, "hop": hop, "rows": R, "frames": frames,
        "above_pmax": int(above.sum()),
        "frames_above_pmax_with_accumulated": int(np.sum(above.any(axis=1) & acc.any(axis=1))),
        "accumulated": int(acc.sum()),
        "floor_pass_3db": int(near_pass.sum()), "floor_fail_3db": int(near_fail.sum()),
        "reach_dropped": int(reach.sum()),
        "outside_image": int(outside.sum()),
        "max_bins_per_cell": int(per_cell.max()),
        "hist_min": int(hist.min()), "hist_max": int(hist.max()),
    }


# ---- the matrix of tests/test_gpu_worst_signals.py: (n, hop, rows, signals) ----
FAST_SHAPES = [
    (4096, 256, 1024, KINDS),          # fused_pp
    (1024, 256, 1024, KINDS),          # fused_small
    (4096, 512, 1024, CORE_KINDS),     # fused
    (2048, 128, 1024, CORE_KINDS),     # fused_small
    (2048, 300, 1024, CORE_KINDS),     # fused_small, a hop that is no power of two
    (8192, 512, 1024, CORE_KINDS),     # fused_n8192
    (16384, 512, 1024, CORE_KINDS),    # fused_n16384
    (16384, 256, 1024, CORE_KINDS),    # 65 ring slots: the generic records path
    (4096, 256, 2048, CORE_KINDS),     # more rows than the ring holds: records + tile scatter
]
EXACT_SHAPES = [
    (4096, 256, 1024, KINDS),          # exact_fused_lr (low rows in the L2 scratch)
    (2048, 128, 1024, KINDS),
    (1024, 256, 1024, KINDS),
    (16384, 512, 1024, CORE_KINDS),    # records + walking scatter
    (8192, 512, 1024, CORE_KINDS),
    (4096, 128, 1024, CORE_KINDS),
    (4096, 256, 2048, CORE_KINDS),     # records + tile scatter
]


def shapes():
    """Every (n, hop, rows) of the matrix with the union of the signals it runs."""
    out = {}
    for n, hop, rows, kinds in FAST_SHAPES + EXACT_SHAPES:
        cur = out.setdefault((n, hop, rows), [])
        cur.extend(k for k in kinds if k not in cur)
    return out
