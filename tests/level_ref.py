"""Python-integer restatement of the level meters (include/emspec.h: emspec_level_*, emspec_cross_*,
emspec_set_level_out, emspec_set_cross_out), exact and unbounded, from uint32 views of the samples.

The windows are the envelope's (wave_ref.window).  A sample with bits u gives an integer k in units of 2^-24:

    NaN: k = 0, counted in `odd`;  otherwise k = x 2^24 rounded to nearest, ties to even, saturated to +-(2^31 - 1); a saturated
    sample (|x| >= 128, +-inf) is counted in `odd` too

evaluated here from the bits alone, in integers: exponent e, mantissa M = m | 2^23 (e > 0): x 2^24 = M 2^(e - 126).

    level record  (sq_lo, sq_hi, peak, odd):  q = k^2;  sq_lo = sum q & 0xffffffff,  sq_hi = sum q >> 32,  peak = max |k|
    cross record  (lo, hi):                   p = k_A k_B;  lo = sum p & 0xffffffff (two's complement),  hi = sum p >> 32 (floor)

level_of / cross_of sum in Python integers; the array forms sum the same limbs in int64, which holds them exactly (at most 2^30
limbs below 2^32 per window), and tests/test_level_cpu.py compares the two.  Lives under tests/ (like
wave_ref.py, whose cases and signals it shares without changing them); the product never imports it."""
import numpy as np

import wave_ref as W
from wave_ref import CASES, S_CASES, case_signal, num_columns, offset, signal, window  # noqa: F401  (shared with the tests)

U = np.uint32
LEVEL = np.dtype([("sq_lo", np.uint64), ("sq_hi", np.uint64), ("peak", np.uint32), ("odd", np.uint32)])
CROSS = np.dtype([("lo", np.uint64), ("hi", np.int64)])
KMAX = 2 ** 31 - 1
assert LEVEL.itemsize == 24 and CROSS.itemsize == 16


def quantise(u):
    """bits -> (k, odd) in Python integers"""
    u = int(u)
    neg, e, m = u >> 31, (u >> 23) & 0xFF, u & 0x7FFFFF
    if e == 255 and m:
        return 0, 1
    if e >= 134:                                   # |x| >= 128, the infinities
        return (-KMAX if neg else KMAX), 1
    if e == 0:                                     # zeros and denormals: below 2^-126
        return 0, 0
    M, sh = m | 0x800000, e - 126                  # x 2^24 = M 2^sh
    if sh >= 0:
        k = M << sh
    else:
        r = -sh
        q, rem, half = M >> r, M & ((1 << r) - 1), 1 << (r - 1)
        k = q + (1 if rem > half or (rem == half and q & 1) else 0)
    return (-k if neg else k), 0


def quantise_all(u):
    """uint32 array -> (int64 array of k, bool array of odd), the same definition vectorised (checked against quantise)"""
    u = np.asarray(u, U).astype(np.int64)
    neg, e, m = (u >> 31) != 0, (u >> 23) & 0xFF, u & 0x7FFFFF
    M = m | 0x800000
    sh = e - 126
    up = M << np.clip(sh, 0, 7)
    r = np.clip(-sh, 1, 25)
    q, rem, half = M >> r, M & ((np.int64(1) << r) - 1), np.int64(1) << (r - 1)
    dn = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    k = np.where(sh >= 0, up, np.where(-sh > 25, 0, dn))
    k = np.where(e == 0, 0, k)
    nan = (e == 255) & (m != 0)
    sat = (e >= 134) & ~nan
    k = np.where(sat, KMAX, np.where(nan, 0, k))
    return np.where(neg, -k, k), nan | sat


def level_of(u):
    """one window's bits -> (sq_lo, sq_hi, peak, odd) as Python integers"""
    k, odd = quantise_all(u)
    ks = [int(v) for v in k]
    return (sum((v * v) & 0xFFFFFFFF for v in ks), sum((v * v) >> 32 for v in ks), max([abs(v) for v in ks], default=0), int(odd.sum()))


def cross_of(ua, ub):
    """two streams' bits of one window -> (lo, hi) as Python integers (>> floors: the arithmetic shift)"""
    ka, _ = quantise_all(ua)
    kb, _ = quantise_all(ub)
    ps = [int(a) * int(b) for a, b in zip(ka, kb)]
    return sum(p & 0xFFFFFFFF for p in ps), sum(p >> 32 for p in ps)


def _starts(L, n, hop, f):
    """the windows tile [off, off + C hop): (C, Cr, off, each window's first sample relative to off)"""
    C = num_columns(L, n, hop)
    Cr = (C + f - 1) // f
    return C, Cr, offset(n, hop), np.arange(Cr, dtype=np.int64) * (f * hop)


def levels(pcm, n, hop, f=1):
    """pcm float32 [S, L] -> LEVEL [S, Cr]: what emspec_level_host / _device and emspec_set_level_out deliver.  (int64 sums of
    at most 2^30 limbs below 2^32: exact; level_of is the same in Python integers.)"""
    x = W.bits(pcm)
    if x.ndim == 1:
        x = x[None]
    S, L = x.shape
    C, Cr, off, starts = _starts(L, n, hop, f)
    out = np.zeros((S, Cr), LEVEL)
    if S == 0 or C == 0:
        return out
    k, odd = quantise_all(x[:, off:off + C * hop])
    a = np.abs(k)
    q = a * a                                                  # < 2^62: exact in int64
    out["sq_lo"] = np.add.reduceat(q & 0xFFFFFFFF, starts, axis=1)
    out["sq_hi"] = np.add.reduceat(q >> 32, starts, axis=1)
    out["peak"] = np.maximum.reduceat(a, starts, axis=1)
    out["odd"] = np.add.reduceat(odd.astype(np.int64), starts, axis=1)
    return out


def crosses(pcm, views, a, b, n, hop, f=1):
    """pcm float32 [pairs * views, L] -> CROSS [pairs, Cr]: pair p is streams p views + a and p views + b"""
    x = W.bits(pcm)
    SV, L = x.shape
    assert SV % views == 0 and 0 <= a < views and 0 <= b < views
    C, Cr, off, starts = _starts(L, n, hop, f)
    out = np.zeros((SV // views, Cr), CROSS)
    if SV == 0 or C == 0:
        return out
    ka, _ = quantise_all(x[a::views, off:off + C * hop])
    kb, _ = quantise_all(x[b::views, off:off + C * hop])
    pr = ka * kb                                               # |p| < 2^62
    out["lo"] = np.add.reduceat(pr & 0xFFFFFFFF, starts, axis=1)
    out["hi"] = np.add.reduceat(pr >> 32, starts, axis=1)       # (numpy's >> on int64 is arithmetic)
    return out


def regroup(records, f):
    """The f = 1 records [S, C] -> the records at factor f: field-wise sums over groups of f, the peak by maximum."""
    records = np.ascontiguousarray(records)
    S, C = records.shape
    starts = np.arange((C + f - 1) // f, dtype=np.int64) * f
    out = np.zeros((S, len(starts)), records.dtype)
    for name in records.dtype.names:
        op = np.maximum if name == "peak" else np.add
        out[name] = op.reduceat(records[name], starts, axis=1)
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def sum_sq(rec):
    return (int(rec["sq_hi"]) << 32) + int(rec["sq_lo"])


def sum_ab(rec):
    return (int(rec["hi"]) << 32) + int(rec["lo"])
