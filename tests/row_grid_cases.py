"""Row counts that are no power of two, for every column kernel (plain numpy; shared by tests/test_row_grid_cases_cpu.py and
tests/test_gpu_row_grids.py).

emspec_create takes any rows % 4 == 0 in 64 .. 4096, and every fused kernel carries arithmetic in the row count R that a power of
two cannot exercise: fused_small's finalize divides by R / 4 with a multiply and a shift, the other kernels finalize with
t < (R >> 2) and so end in a partial wave, the LDS carve-ups place their tables behind SLOTS * R cells, the EXACT row split rounds
to multiples of 8 and of 32, the records scatter sizes its tile from R.  The lists below put each kernel of
tests/golden/kernel_plans.json on

  SWEEP = 68, 100, 516, 1000, 1020 rows: 17 (odd), 25, 129 (one past two waves), 250 and 255 (one under the ring gate) quads; 68, 100,
          516 and 1020 are 4 mod 8, 100 and 1000 break % 16 and % 32;
  the rows on both sides of every row threshold the fixture records (the launches with the fullest LDS, and the smallest low-row
          split, rl = 4);
  2052 and 4092 rows, above the ring gate, on the records paths.

A case is (n, hop, rows, reassign) in FAST mode and (n, hop, rows, axis) in EXACT mode (reassignment on), with the axes of
tests/cdriver/kernel_plan_driver.cpp: 0 the configured log axis, 1 linear edges, 2 warped edges (low_end_boost 0.5).  The route of
a case is what the fixture records for it, never what this module says.

The signal is half of emspec.synth.streams plus seeded Gaussian noise of standard deviation 0.1: the plain synthetic streams leave
95 % of a 1020-row image gated to palette index 0, where a lost quad would compare equal.  tests/test_row_grid_cases_cpu.py asserts
on the oracle's image of every case that the last quad of every column, and at least 85 % of all row quads, are non-zero."""
import json
import os

import numpy as np

from emspec import synth

SWEEP = (68, 100, 516, 1000, 1020)
ABOVE_GATE = (2052, 4092)
STREAMS = 2
SEED, NOISE = 2024, 0.1
# (n, hop, rows) -> (seed, noise) where a shape needs another draw to meet the input conditions (none does)
SIGNAL_OVERRIDES = {}
LOG, LINEAR, WARPED = 0, 1, 2
WARPED_ARGS = (20.0, 24000.0, 0.5, 1.0)     # fmin, fmax, low_end_boost, freq_scale of the driver's axis 2

# the shapes by the kernel that serves them at 1024 rows
FAST_SHAPES = {
    "fused_pp": [(4096, 256), (4096, 512), (4096, 1024)],
    "fused_small": [(4096, 300), (2048, 128), (1024, 256), (1024, 100)],
    "fused_8192": [(8192, 512), (8192, 1024)],
    "fused_16384": [(16384, 512)],
    "records_f32": [(8192, 256), (512, 64)],
}
EXACT_SHAPES = {
    "exact_lr": [(4096, 256, LOG), (4096, 300, LOG), (2048, 128, LOG), (1024, 256, LOG)],
    "exact_parked": [(4096, 256, WARPED)],
    "exact_records": [(8192, 512, LOG), (16384, 512, LOG)],
}

FAST_SWEEP = [(n, hop, rows, 1) for shapes in FAST_SHAPES.values() for n, hop in shapes for rows in SWEEP] + \
             [(n, hop, 1000, 0) for shapes in FAST_SHAPES.values() for n, hop in shapes]
FAST_ABOVE_GATE = [(n, hop, rows, 1) for n, hop in ((4096, 256), (16384, 512)) for rows in ABOVE_GATE]
# both sides of a row threshold, four rows apart: the ring fits / the records path
FAST_BRIMS = [((4096, 200, 932, 1), (4096, 200, 936, 1)), ((2048, 60, 568, 1), (2048, 60, 572, 1)),
              ((1024, 40, 664, 1), (1024, 40, 668, 1)), ((16384, 256, 516, 1), (16384, 256, 520, 1))]
# one case per kernel whose RGBA is compared too
FAST_RGBA = {(4096, 256, 1020, 1), (4096, 300, 1020, 1), (8192, 512, 1020, 1), (16384, 512, 1020, 1), (8192, 256, 1020, 1)}

EXACT_SWEEP = [(n, hop, rows, axis) for shapes in EXACT_SHAPES.values() for n, hop, axis in shapes for rows in SWEEP]
EXACT_ABOVE_GATE = [(4096, 256, rows, LOG) for rows in ABOVE_GATE]
# neighbours that differ in route or in the low-row split rl: the whole ring in LDS / rl = 4 / rl = 16 on the log axis; rl = 36 / 40
# on the warped axis, where 632 rows on the linear axis leave the no-parking kernel for the parked one (the low-share rule); the
# parked kernel / the records path; and a point the fixture names (rl = 64 at N = 2048)
EXACT_BRIMS = [((4096, 256, 600, LOG), (4096, 256, 604, LOG)), ((4096, 256, 604, LOG), (4096, 256, 608, LOG)),
               ((4096, 256, 628, WARPED), (4096, 256, 632, WARPED)), ((4096, 256, 632, WARPED), (4096, 256, 632, LINEAR)),
               ((4096, 255, 940, WARPED), (4096, 255, 944, WARPED))]
EXACT_POINTS = [(2048, 128, 600, LOG)]

# short forced segments (EMSPEC_SEGLEN of the diagnostic build) at the smallest and the largest sweep row: the finalize's [c0, c1)
# test and the ring restart at an odd R.  EXACT: (n, hop, rows, axis, parked) - parked: EMSPEC_EXACT_PARKED=1
SEGLEN = 33
FAST_FORCED = [(n, hop, rows, 1) for k, shapes in FAST_SHAPES.items() if k != "records_f32" for n, hop in shapes for rows in (68, 1020)]
EXACT_FORCED = [(n, hop, rows, LOG, 0) for n, hop in ((4096, 256), (2048, 128), (1024, 256)) for rows in (68, 1020)] + \
               [(4096, 256, rows, WARPED, 1) for rows in (68, 1020)]


def _unique(cases):
    return list(dict.fromkeys(cases))


FAST_CASES = _unique(FAST_SWEEP + FAST_ABOVE_GATE + [c for pair in FAST_BRIMS for c in pair])
EXACT_CASES = _unique(EXACT_SWEEP + EXACT_ABOVE_GATE + [c for pair in EXACT_BRIMS for c in pair] + EXACT_POINTS)


def latency(n, hop, reassign):
    """emspec_tables.h: latency."""
    return (n + 2 * hop - 1) // (2 * hop) if reassign else 0


def columns(n, hop, reassign=1):
    """Past the reach on both sides, and past one forced segment."""
    return max(41, 2 * latency(n, hop, reassign) + 9)


def length(n, hop, reassign=1):
    return n + (columns(n, hop, reassign) - 1) * hop + 3


def _gauss(seed, count):
    """Box-Muller on emspec.synth's counter-based uniforms: no dependence on numpy's generators."""
    u = synth.uniform(seed, 2 * count)
    return np.sqrt(-2.0 * np.log(np.maximum(u[0::2], 1e-300))) * np.cos(2 * np.pi * u[1::2])


def signal(S, L, seed=SEED, noise=NOISE):
    """float32 [S][L]: 0.5 * synth.streams(S, L) + N(0, noise^2), stream s drawn from seed + s."""
    x = 0.5 * synth.streams(S, L).astype(np.float64)
    for s in range(S):
        x[s] += noise * _gauss((int(seed) + s) * 7919 + 13, L)
    return x.astype(np.float32)


_signals = {}


def case_signal(n, hop, rows, reassign=1):
    """The input of a case (read-only, shared: a prefix-free draw per length, seed and level)."""
    seed, noise = SIGNAL_OVERRIDES.get((n, hop, rows), (SEED, NOISE))
    key = (length(n, hop, reassign), seed, noise)
    if key not in _signals:
        x = signal(STREAMS, key[0], seed, noise)
        x.setflags(write=False)
        _signals[key] = x
    return _signals[key]


def edges_hz(axis, rows):
    """The driver's axis as rows + 1 float32 edges in Hz, None for the configured log axis."""
    if axis == LOG:
        return None
    if axis == LINEAR:
        r = np.arange(rows + 1, dtype=np.float32)
        return (np.float32(20.0) + np.float32(24000.0 - 20.0) * r / np.float32(rows)).astype(np.float32)
    import emspec
    return emspec.warped_edges_hz(rows, *WARPED_ARGS)


_plans = None


def plans():
    global _plans
    if _plans is None:
        _plans = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_plans.json")))
    return _plans


def _one(kind, case):
    hit = [w for w in plans() if w["kind"] == kind and w["case"] == case]
    assert len(hit) == 1, (kind, case, len(hit))
    return hit[0]


def fast_plan(n, hop, rows, reassign):
    """The fixture's record of a FAST case (the product build's switches)."""
    return _one("fast", dict(n=n, hop=hop, rows=rows, reassign=reassign, no_fused=0, variant=0))


def exact_plan(n, hop, rows, axis, parked=0):
    return _one("exact", dict(n=n, hop=hop, reassign=1, rows=rows, row0=0, axis_rows=rows, axis=axis, parked=parked, records=0))
