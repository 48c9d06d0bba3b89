"""Other sample rates and log axes, for every column kernel (plain numpy; shared by tests/test_axis_cases_cpu.py and
tests/test_gpu_axes.py).

emspec_create takes any sample_rate > 0 and any 0 < fmin < fmax <= sample_rate / 2; the kernels see the axis only through the edge
tables and the plan's scalars, and make assumptions about both.  The axes below put each of them to the test:

  cd      44.1 kHz, 20 Hz .. 22.05 kHz   the top edge is exactly N / 2 at another rate
  tel     8 kHz, 30 Hz .. 4 kHz          fmin * (fmax / fmin) * N / fs rounds an ulp above N / 2: the table clamps it
  wide32  32 kHz, 55 Hz .. 16 kHz        (emspec_tables.h: edges_bin64), and no route of either mode accumulates the Nyquist bin
  band96  96 kHz, 20 Hz .. 20 kHz        most bins lie above the axis
  hi192   192 kHz, 10 Hz .. 96 kHz       e0 far below one bin: the rows below bin 1
  zoom    48 kHz, 2 kHz .. 4 kHz         one octave: rows much narrower than a bin, bins off both ends of the axis

A case is (axis name, n, hop, rows), reassignment on.  Every shape of FAST_SHAPES / EXACT_SHAPES runs at 1024 rows on every axis,
one shape per kernel at 68 rows, and one records case per mode at 4092 rows; `zoom` only at n >= 4096 and up to 1024 rows (at
n = 1024, and at 4092 rows, only 4 % of its cells are non-zero on the oracle: the octave holds too few bins).  The route of a case is what tests/golden/kernel_plans.json records for it, never what this module says: the FAST
route does not depend on the axis, the EXACT route does (the low-share rule of emspec_kernel_plan.h sends `tel` and `zoom` at
4096 / 256 to the parked kernel and `tel`, `wide32` and `zoom` at 2048 / 128 to the records path).

The signal is row_grid_cases' (half of emspec.synth.streams plus Gaussian noise) plus 0.2 cos(pi t), added in float64 before the
one rounding to float32: the Nyquist bin carries power far above the floor, so a route that accumulated it would show.

The row hint of the FAST kernels (emspec_tables.h: hint_rows_ok) is restated as hint_value(): NARROW_HINTED are axes just inside
its bound for one n each, NARROW_SEARCHED axes past it (the narrow axes of a numpy model of the lookup that gave wrong rows)."""
import math

import numpy as np

import row_grid_cases as G
from emspec import synth

AXES = {
    "cd": (44100.0, 20.0, 22050.0),
    "tel": (8000.0, 30.0, 4000.0),
    "wide32": (32000.0, 55.0, 16000.0),
    "band96": (96000.0, 20.0, 20000.0),
    "hi192": (192000.0, 10.0, 96000.0),
    "zoom": (48000.0, 2000.0, 4000.0),
}
TOP_ABOVE_NYQUIST = ("tel", "wide32")      # the unclamped binary64 top edge exceeds N / 2
TOP_AT_NYQUIST = ("cd", "hi192")           # ... equals it
NYQUIST = 0.2
STREAMS = G.STREAMS

# one (n, hop) per column kernel at 1024 rows (fused_small twice: a hop that is no power of two, and N = 1024)
FAST_SHAPES = [("fused_pp", 4096, 256), ("fused_small", 4096, 300), ("fused_small", 1024, 256), ("fused_8192", 8192, 512),
               ("fused_16384", 16384, 512), ("records_f32", 8192, 256)]
EXACT_SHAPES = [(4096, 256), (2048, 128), (1024, 256), (8192, 512), (16384, 512)]
FAST_SHAPES_68 = [(4096, 256), (4096, 300), (8192, 512), (16384, 512), (8192, 256)]
EXACT_SHAPES_68 = [(4096, 256), (8192, 512)]
RECORDS_4092 = (4096, 256)
assert all((n, hop) in G.FAST_SHAPES[k] for k, n, hop in FAST_SHAPES)
assert all((n, hop, G.LOG) in [s for v in G.EXACT_SHAPES.values() for s in v] for n, hop in EXACT_SHAPES)


def _on(axis, n, rows=1024):
    """`zoom` has 171 bins at n = 4096 and 43 at n = 1024: they cannot fill a tenth of 4092 rows, or of 1024 rows at n = 1024."""
    return axis != "zoom" or (n >= 4096 and rows <= 1024)


FAST_CASES = [(a, n, hop, 1024) for a in AXES for _, n, hop in FAST_SHAPES if _on(a, n)] + \
             [(a, n, hop, 68) for a in AXES for n, hop in FAST_SHAPES_68] + [(a, *RECORDS_4092, 4092) for a in AXES if _on(a, RECORDS_4092[0], 4092)]
EXACT_CASES = [(a, n, hop, 1024) for a in AXES for n, hop in EXACT_SHAPES if _on(a, n)] + \
              [(a, n, hop, 68) for a in AXES for n, hop in EXACT_SHAPES_68] + [(a, *RECORDS_4092, 4092) for a in AXES if _on(a, RECORDS_4092[0], 4092)]
# one case per kernel whose RGBA is compared too
EXACT_RGBA = {("cd", 4096, 256, 1024), ("tel", 4096, 256, 1024), ("tel", 2048, 128, 1024)}
# EXACT streaming against the batch bytes: the parked kernel and the no-parking kernel beside exact_frames_kernel
STREAMING = [("tel", 4096, 256, 1024), ("tel", 1024, 256, 1024)]
DUMP_FRAMES = 6

# (axis, n, hop, rows) -> (seed, noise) where a case needs another draw to meet the input conditions
SIGNAL_OVERRIDES = {}

# the row-lookup probe: rows of the six axes, and the narrow axes at 4096 rows
PROBE_ROWS = (64, 1024, 4096)
PROBE_SIZES = (1024, 4096, 16384)
HINT_BOUND = 2097152.0     # 2^23 / 4
# n -> an axis within 1 % of the bound for that n, on the hinted side (4096 rows)
NARROW_HINTED = {1024: (48000.0, 21750.0, 24000.0), 4096: (48000.0, 21280.0, 24000.0), 16384: (48000.0, 20820.0, 24000.0)}
NARROW_ROWS = 4096
# past the bound: (axis, rows); the float32 edges still increase strictly, so emspec_create takes them
NARROW_SEARCHED = [((48000.0, 23900.0, 24000.0), 4096), ((48000.0, 23980.0, 24000.0), 1024), ((48000.0, 23500.0, 24000.0), 1024)]
# whole columns at N = 4096, hop 256 on narrow axes: (axis, rows, the share of non-zero cells the oracle's image must reach).  Past
# the bound a fused kernel's 1024 rows span at most 0.043 octaves, 61 bins: the 43 bins of this axis fill 4 % of its cells at best
NARROW_COLUMNS = {"searched": (NARROW_SEARCHED[2][0], 1024, 0.02), "hinted": (NARROW_HINTED[4096], 1024, 0.10)}


def kw(axis):
    """The engine's / the oracle's configuration fields of an axis (by name or as a triple)."""
    sr, lo, hi = AXES[axis] if isinstance(axis, str) else axis
    return dict(sample_rate=sr, fmin_hz=lo, fmax_hz=hi)


def columns(n, hop):
    return G.columns(n, hop, 1)


def length(n, hop):
    return G.length(n, hop, 1)


def signal(S, L, seed=G.SEED, noise=G.NOISE, nyquist=NYQUIST):
    """float32 [S][L]: row_grid_cases.signal's terms plus nyquist * cos(pi t), summed in float64 and rounded once."""
    x = 0.5 * synth.streams(S, L).astype(np.float64)
    for s in range(S):
        x[s] += noise * G._gauss((int(seed) + s) * 7919 + 13, L)
    x += nyquist * (1.0 - 2.0 * (np.arange(L) & 1))      # cos(pi t), exactly
    return x.astype(np.float32)


_signals = {}


def case_signal(axis, n, hop, rows):
    """The input of a case (read-only, shared)."""
    seed, noise = SIGNAL_OVERRIDES.get((axis, n, hop, rows), (G.SEED, G.NOISE))
    key = (length(n, hop), seed, noise)
    if key not in _signals:
        x = signal(STREAMS, *key)
        x.setflags(write=False)
        _signals[key] = x
    return _signals[key]


def fast_plan(axis, n, hop, rows):
    """The fixture's record of a FAST case: the route does not look at the axis."""
    return G.fast_plan(n, hop, rows, 1)


def exact_plan(axis, n, hop, rows):
    sr, lo, hi = AXES[axis]
    return G._one("exact", dict(n=n, hop=hop, reassign=1, rows=rows, row0=0, axis_rows=rows, axis=0, parked=0, records=0,
                                sample_rate=sr, fmin=lo, fmax=hi))


def raw_top_edge(axis, n):
    """The top edge before the clamp, by the table's own operations in binary64: fmin * (fmax / fmin) * n / fs."""
    sr, lo, hi = (float(np.float32(v)) for v in AXES[axis])
    return lo * (hi / lo) * float(n) / sr


def hint_value(e0, eR, rows):
    """emspec_tables.h: hint_rows_ok holds iff this is <= HINT_BOUND (libm's log2 here: not for values on the bound)."""
    l0, lR = math.log2(e0), math.log2(eR)
    return 8.0 * (rows / (lR - l0)) * max(1.0, abs(l0), abs(lR)) + 2.0 * rows


def lookup_model(eb, kh, ulps=0):
    """numpy float32 model of HintLookup::row_signed_log on the float32 table eb: log2 correctly rounded and moved by `ulps`
    float32 neighbours, every operation rounded to float32; the row, -1 below the table and rows at or above it."""
    f = np.float32
    eb, kh = np.asarray(eb, f), np.asarray(kh, f)
    R = eb.size - 1
    l2 = np.log2(kh.astype(np.float64)).astype(f)
    for _ in range(abs(ulps)):
        l2 = np.nextafter(l2, f(np.inf if ulps > 0 else -np.inf))
    l2e0 = f(math.log2(float(eb[0])))
    rscale = f(R) / (f(math.log2(float(eb[R]))) - l2e0)
    r0 = np.clip(((l2 - l2e0) * rscale).astype(np.int64), 0, R - 1)
    lo, hi = eb[r0], eb[r0 + 1]
    return r0 + (kh >= hi) - (kh < lo)


def probe_values(eb):
    """Every edge, its float32 neighbours at 1 and 2 ulp, and the row midpoints."""
    f = np.float32
    vals = [eb]
    up, dn = eb.copy(), eb.copy()
    for _ in range(2):
        up, dn = np.nextafter(up, f(np.inf)), np.nextafter(dn, f(-np.inf))
        vals += [up, dn]
    vals.append((0.5 * (eb[:-1].astype(np.float64) + eb[1:])).astype(f))
    return np.ascontiguousarray(np.concatenate(vals), f)


def bisect_rows(eb, kh):
    """-1 below the table, rows at or above it."""
    return np.searchsorted(eb, kh, side="right").astype(np.int64) - 1
