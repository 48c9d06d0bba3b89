"""numpy restatement of the waveform envelope (include/emspec.h: emspec_wave_device, emspec_wave_host,
emspec_set_wave_out), and the cases and signals the envelope tests share.

A stream of L samples, FFT size n, hop, factor f: C = num_columns(L, n, hop), Cr = ceil(C / f), off = n // 2 - hop // 2.  Pair g
covers the samples

    W(g) = [ g f hop + off,  min((g + 1) f, C) hop + off )

    key(u) = ~u if u & 0x80000000 else u | 0x80000000        u: a sample's 32 bits; the total order of the floats, -0.0 < +0.0
    lo = the sample of W(g) with the smallest key, hi = the one with the largest, each with its own bits
    NaN samples are skipped; a window without a sample that is not NaN gives (+inf, -inf)

Everything is done on integer views: no float comparison takes part, and every comparison of results is of uint32 views.  Lives
under tests/ (like peaks_ref.py); the product never imports it."""
import numpy as np

F = np.float32
U = np.uint32
SIGN = U(0x80000000)


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def num_columns(L, n, hop):
    return 0 if L < n else (L - n) // hop + 1


def offset(n, hop):
    return n // 2 - hop // 2


def window(g, C, n, hop, f):
    """[first, last + 1) of W(g)"""
    return g * f * hop + offset(n, hop), min((g + 1) * f, C) * hop + offset(n, hop)


def keys(u):
    u = np.asarray(u, U)
    return np.where(u & SIGN, ~u, u | SIGN).astype(U)


def unkeys(k):
    k = np.asarray(k, U)
    return np.where(k & SIGN, k & ~SIGN, ~k).astype(U)


def is_nan_bits(u):
    return (np.asarray(u, U) & U(0x7FFFFFFF)) > U(0x7F800000)


def envelope(pcm, n, hop, f=1):
    """pcm float32 [S, L] -> float32 [S, Cr, 2] of (lo, hi): what the three entry points deliver."""
    x = np.ascontiguousarray(pcm, F)
    if x.ndim == 1:
        x = x[None]
    S, L = x.shape
    C = num_columns(L, n, hop)
    Cr = (C + f - 1) // f
    out = np.empty((S, Cr, 2), F)
    if C == 0 or S == 0:
        return out
    off = offset(n, hop)
    u = x.view(U)[:, off:off + C * hop]
    nan = is_nan_bits(u)
    k = keys(u)
    starts = np.arange(Cr, dtype=np.int64) * (f * hop)
    kmin = np.minimum.reduceat(np.where(nan, U(0xFFFFFFFF), k), starts, axis=1)
    kmax = np.maximum.reduceat(np.where(nan, U(0), k), starts, axis=1)
    some = np.add.reduceat((~nan).astype(np.int64), starts, axis=1) > 0
    o = out.view(U)
    o[:, :, 0] = np.where(some, unkeys(kmin), bits(F(np.inf)))
    o[:, :, 1] = np.where(some, unkeys(kmax), bits(F(-np.inf)))
    return out


def regroup(w1, f):
    """The f = 1 envelope [S, C, 2] -> the envelope at factor f by key-min / key-max over groups of f pairs (a group of empty
    windows (+inf, -inf) stays one: +inf is the largest key, -inf the smallest)."""
    w1 = np.ascontiguousarray(w1, F)
    S, C, _ = w1.shape
    starts = np.arange((C + f - 1) // f, dtype=np.int64) * f
    k = keys(w1.view(U))
    out = np.empty((S, len(starts), 2), F)
    o = out.view(U)
    o[:, :, 0] = unkeys(np.minimum.reduceat(k[:, :, 0], starts, axis=1))
    o[:, :, 1] = unkeys(np.maximum.reduceat(k[:, :, 1], starts, axis=1))
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


def _columns(n, hop, L):
    return num_columns(L, n, hop)


# (n, hop, L, f): S = 3 streams each, an odd L wherever the table of the issue allows
_SHAPES = [
    (256, 1, 300, (1, 7)),
    (256, 3, 256, (1,)),
    (1024, 255, 1024 + 255 * 9 + 100, (1, 4)),
    (1024, 256, 2 ** 15 + 1, (1, 3, _columns(1024, 256, 2 ** 15 + 1), 65536)),
    (4096, 256, 3 * 4096 + 77, (1, 2, 5)),
    (4096, 257, 4096 + 257 * 20, (1, 3)),
    (4096, 4096, 5 * 4096 + 1, (1, 2)),
    (16384, 512, 16384 + 512 * 40 + 1, (1, 16)),
]
CASES = [(n, hop, L, f) for n, hop, L, fs in _SHAPES for f in fs]
S_CASES = 3


def signal(S, L, n, hop, f, seed=0, finite=False):
    """Seeded normal noise [S, L] with what the envelope can get wrong planted, as far as the case has windows for it:
    stream 0: a value larger than all others on the sample just before and just after several window boundaries (the last
              sample of one window, the first of the next: each must show in its own window's hi only), a smaller-than-all
              on a window's first and on a window's last sample, and +-1e30 on the samples just outside the first and last window;
    stream 1: a window of NaN only, a window of -0.0 and +0.0 only (lo = -0.0, hi = +0.0 by their bits), -inf and +inf;
    stream 2: a NaN as a window's first and as another's last sample, denormals of both signs as a window's extremes.
    finite: no NaN and no infinity is planted (the signal also goes through the spectrogram kernels), the noise is scaled to
    +-0.1 and the boundary values to +-1: what the zeros, the denormals and the boundaries test stays."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * hop + f + L % 1000)
    x = rng.standard_normal((S, L)).astype(F)
    big = F(1.0)
    if finite:
        x = (np.clip(x, -4, 4) * F(0.025)).astype(F)
        big = F(1.0 / 4096)
    xu = x.view(U)
    C = num_columns(L, n, hop)
    Cr = (C + f - 1) // f
    if C == 0:
        return x
    off = offset(n, hop)
    w = lambda g: window(g % Cr, C, n, hop, f)
    if off > 0:
        x[0, off - 1] = F(1e30) if not finite else F(0.99)
    if off + C * hop < L:
        x[0, off + C * hop] = F(-1e30) if not finite else F(-0.99)
    for i, g in enumerate(sorted({1 % Cr, Cr // 2, Cr - 1})):
        a, b = w(g)
        if g > 0:
            x[0, a - 1] = F(1000 + i) * big     # just before the boundary: window g - 1's
        x[0, a] = F(2000 + i) * big            # just after: window g's first sample
    a, b = w(Cr // 3)
    x[0, b - 1] = F(-3000) * big               # a window's last sample
    if S > 1:
        a, b = w(1)
        if not finite:
            x[1, a:b] = F(np.nan)
            xu[1, a:b:2] = U(0xFFC00001)                   # (a negative NaN with a payload among them)
        if Cr > 2:
            a, b = w(2)
            x[1, a:b] = F(0.0)
            x[1, a + 1:b:2] = F(-0.0)                       # (a window of one sample holds +0.0 only)
        if Cr > 3 and not finite:
            a, b = w(3)
            x[1, a] = F(np.inf)
            x[1, b - 1] = F(-np.inf)
    if S > 2:
        if not finite:
            a, b = w(0)
            x[2, a] = F(np.nan)
            a, b = w(Cr - 1)
            x[2, b - 1] = F(np.nan)
        if Cr > 2:
            a, b = w(Cr // 2)
            xu[2, a:b] = U(1) + (np.arange(b - a, dtype=U) % U(5))          # denormals 1 .. 5 ulp
            xu[2, a + (b - a) // 2] = U(0x80000007)                         # a negative one: the window's lo
    return x


def case_signal(case, seed=0):
    n, hop, L, f = case
    return signal(S_CASES, L, n, hop, f, seed)
