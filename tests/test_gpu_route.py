"""GPU: one tiny batch per kernel route and per side of a route boundary (em-spec_amd/csrc/emspec_kernel_plan.h).  For each shape
Engine.fused() is the route recorded in tests/golden/kernel_plans.json - the fixture the CPU test pins the header to - and the
columns equal the oracle by the comparison the suite uses for the mode: FAST the bounds of tests/test_gpu_sizes.py (|dB error|
< 8.7e-4, palette index within one step, at most max(8, cells / 1000) cells off by one), EXACT dB bits and index byte-equal to the
binary64 bit model.  S = 2 streams of n + 24 hop samples: 25 columns."""
import json
import os

import numpy as np
import pytest

import emspec
import oracle as O
from emspec import synth

pytestmark = pytest.mark.gpu

PLANS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kernel_plans.json")))
WARPED = (20.0, 24000.0, 0.5, 1.0)   # the driver's axis 2: low_end_boost 0.5, past the no-parking kernel's 6 % of low bins


def _recorded(kind, **case):
    hit = [w for w in PLANS if w["kind"] == kind and all(w["case"][k] == v for k, v in case.items())]
    assert len(hit) >= 1, (kind, case)
    return hit[0]["route"]


# n, hop, rows, reassign, the route the fixture must name (so that the list keeps covering every route and both sides)
FAST = [(4096, 256, 1024, 1, "fused_pp"), (4096, 256, 1024, 0, "fused_pp"),
        (4096, 228, 1024, 1, "fused_small"), (4096, 227, 1024, 1, "records_f32"),         # the ring stops fitting: 22 slots
        (2048, 512, 64, 1, "fused_small"), (8192, 512, 1024, 1, "fused_8192"),
        (16384, 512, 1024, 1, "fused_16384"), (16384, 511, 1024, 1, "records_f32"),       # the register park: D = 16 / 17
        (4096, 512, 1028, 1, "records_f32"), (4096, 512, 4096, 1, "records_f32")]         # the rows gate
# ... and axis: 0 the configured log axis, 2 the warped one
EXACT = [(4096, 256, 1024, 0, "exact_lr"), (4096, 256, 64, 0, "exact_lr"), (2048, 256, 1024, 0, "exact_lr"),
         (4096, 256, 1024, 2, "exact_parked"), (4096, 255, 1024, 2, "exact_records"),    # the parked ring stops fitting: D = 8 / 9
         (4096, 256, 4096, 0, "exact_records"), (8192, 512, 1024, 0, "exact_records")]


def test_the_lists_cover_every_route():
    assert {c[4] for c in FAST} == {"fused_pp", "fused_small", "fused_8192", "fused_16384", "records_f32"}
    assert {c[4] for c in EXACT} == {"exact_lr", "exact_parked", "exact_records"}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n,hop,rows,reassign,route", FAST)
def test_fast_route_and_columns(engine, n, hop, rows, reassign, route):
    assert _recorded("fast", n=n, hop=hop, rows=rows, reassign=reassign, no_fused=0, variant=0) == route
    pcm = synth.streams(2, n + 24 * hop)
    e = engine if rows == engine.rows else emspec.Engine(rows=rows)
    try:
        assert bool(e.fused(n, hop, bool(reassign))) == (route != "records_f32")
        out = e.batch(pcm, n, hop, bool(reassign), want=("db", "index"))
        e.device_status()
    finally:
        if e is not engine:
            e.close()
    odb, _, oidx = O.batch_f32(O.make_cfg(n, hop, bool(reassign), rows=rows), pcm, want=("db", "index"))
    assert out["db"].shape == odb.shape == (2, 25, rows)
    worst = float(np.max(np.abs(out["db"] - odb)))
    d = np.abs(out["index"].astype(int) - oidx.astype(int))
    print(f"MEASURED {route} {n}/{hop} rows {rows}: worst |dB error| {worst:.2e}, cells off by one {int(np.count_nonzero(d))} of {d.size}")
    assert worst < 8.7e-4, worst
    assert d.max() <= 1 and int(np.count_nonzero(d)) <= max(8, d.size // 1000)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n,hop,rows,axis,route", EXACT)
def test_exact_route_and_columns(engine, n, hop, rows, axis, route):
    assert _recorded("exact", n=n, hop=hop, rows=rows, reassign=1, row0=0, axis_rows=rows, axis=axis, parked=0, records=0) == route
    pcm = synth.streams(2, n + 24 * hop)
    edges = emspec.warped_edges_hz(rows, *WARPED) if axis else None
    with emspec.Engine(mode=emspec.MODE_EXACT, rows=rows) as x:
        if axis:
            x.set_row_edges_hz(edges)
        assert bool(x.fused(n, hop, True)) == (route != "exact_records")
        out = x.batch(pcm, n, hop, True, want=("db", "index"))
        x.device_status()
    O.set_custom_edges_hz(edges)
    try:
        odb, _, oidx, _ = O.batch_exact(O.make_cfg(n, hop, True, rows=rows), pcm, want=("db", "index"))
    finally:
        O.set_custom_edges_hz(None)
    assert out["db"].shape == odb.shape == (2, 25, rows)
    assert np.array_equal(out["db"].view(np.uint32), odb.view(np.uint32)), "dB bits differ from the bit model"
    assert np.array_equal(out["index"], oidx), "index differs from the bit model"
