"""CPU: the cases of tests/row_grid_cases.py are pinned and cannot pass vacuously.

 - every case has a record in tests/golden/kernel_plans.json, the lists name every route of their mode, and the two sides of every
   brim differ in route or in the low-row split as the fixture records them;
 - the oracle's image of every case's input has its last row quad non-zero in every column and at least 85 % of all row quads
   non-zero somewhere - conditions on the input, measured on the reference alone, so that a kernel that drops or misplaces a quad
   cannot compare equal on the GPU;
 - the division by a multiply and a shift in fused_small.hip.inc's finalize, restated and checked exhaustively."""
import numpy as np
import pytest

import oracle as O
import row_grid_cases as G

FAST_ROUTES = {"fused_pp", "fused_small", "fused_8192", "fused_16384", "records_f32"}
EXACT_ROUTES = {"exact_lr", "exact_parked", "exact_records"}


def test_every_case_is_recorded_and_the_lists_name_every_route():
    assert {G.fast_plan(*c)["route"] for c in G.FAST_CASES} == FAST_ROUTES
    assert {G.exact_plan(*c)["route"] for c in G.EXACT_CASES} == EXACT_ROUTES
    # a shape is served by its own kernel at every sweep row; the warped axis goes to the parked kernel only once the ring needs
    # a row split (the no-parking kernel takes any axis while its whole ring fits)
    for route, shapes in G.FAST_SHAPES.items():
        for n, hop in shapes:
            assert {G.fast_plan(n, hop, rows, 1)["route"] for rows in G.SWEEP} == {route}, (n, hop)
            assert G.fast_plan(n, hop, 1000, 0)["route"] == route
    for route, shapes in G.EXACT_SHAPES.items():
        for n, hop, axis in shapes:
            got = {rows: G.exact_plan(n, hop, rows, axis) for rows in G.SWEEP}
            if route == "exact_parked":
                assert [got[r]["route"] for r in G.SWEEP] == ["exact_lr"] * 3 + ["exact_parked"] * 2
            else:
                assert {w["route"] for w in got.values()} == {route}, (n, hop)
            if route == "exact_lr":     # the whole ring in LDS at the small rows, a row split of rh % 8 == 0 at the large ones
                assert [got[r]["rl"] > 0 for r in G.SWEEP] == [False, False, False, True, True]
                assert all(w["rh"] % 8 == 0 and w["rl"] % 4 == 0 for w in got.values() if w["rl"])
    assert all(G.fast_plan(*c)["route"] == "records_f32" for c in G.FAST_ABOVE_GATE)
    assert all(G.exact_plan(*c)["route"] == "exact_records" for c in G.EXACT_ABOVE_GATE)
    assert set(G.FAST_RGBA) <= set(G.FAST_CASES) and {G.fast_plan(*c)["route"] for c in G.FAST_RGBA} == FAST_ROUTES
    # the forced-segment cases: every fused kernel, at the smallest and the largest sweep row
    assert {G.fast_plan(*c)["route"] for c in G.FAST_FORCED} == FAST_ROUTES - {"records_f32"}
    assert {G.exact_plan(*c)["route"] for c in G.EXACT_FORCED} == {"exact_lr", "exact_parked"}
    assert all(G.exact_plan(*c)["route"] == "exact_parked" for c in G.EXACT_FORCED if c[4])
    assert {c[2] for c in G.FAST_FORCED} == {c[2] for c in G.EXACT_FORCED} == {68, 1020}


def test_each_brim_pair_differs_as_recorded():
    for lo, hi in G.FAST_BRIMS:
        a, b = G.fast_plan(*lo), G.fast_plan(*hi)
        assert hi[2] == lo[2] + 4 and a["route"] != "records_f32" and b["route"] == "records_f32", (lo, hi)
        assert a["lds"] <= 160 * 1024
    x = {c: G.exact_plan(*c) for pair in G.EXACT_BRIMS for c in pair}
    x.update({c: G.exact_plan(*c) for c in G.EXACT_POINTS})
    assert all((x[lo]["route"], x[lo]["rl"]) != (x[hi]["route"], x[hi]["rl"]) for lo, hi in G.EXACT_BRIMS)
    assert [(x[4096, 256, r, G.LOG]["route"], x[4096, 256, r, G.LOG]["rl"]) for r in (600, 604, 608)] == \
        [("exact_lr", 0), ("exact_lr", 4), ("exact_lr", 16)]
    assert [(x[4096, 256, r, G.WARPED]["route"], x[4096, 256, r, G.WARPED]["rl"]) for r in (628, 632)] == [("exact_lr", 36), ("exact_lr", 40)]
    assert x[4096, 256, 632, G.LINEAR]["route"] == "exact_parked"
    assert x[4096, 255, 940, G.WARPED]["route"] == "exact_parked" and x[4096, 255, 944, G.WARPED]["route"] == "exact_records"
    assert (x[2048, 128, 600, G.LOG]["route"], x[2048, 128, 600, G.LOG]["rl"]) == ("exact_lr", 64)
    # the fullest launches these kernels can ask for
    assert G.fast_plan(4096, 200, 932, 1)["lds"] == 163824 and x[4096, 255, 940, G.WARPED]["lds"] == 163600 and 163824 <= 160 * 1024


def _check_input(index, label, reachable=None):
    """reachable: the row quads that can receive anything at all (None: every one)."""
    S, C, R = index.shape
    quads = (index.reshape(S, C, R // 4, 4) != 0).any(axis=3)
    hit = quads.any(axis=(0, 1))
    if reachable is None:
        reachable = np.ones(R // 4, bool)
    assert reachable[-1] and not hit[~reachable].any()
    last, share = float(quads[:, :, -1].mean()), float(hit[reachable].mean())
    print(f"CONDITIONS {label}: last quad non-zero in {100 * last:.1f} % of columns, {100 * share:.1f} % of "
          f"{int(reachable.sum())} reachable row quads non-zero ({100 * float(hit.mean()):.1f} % of all {R // 4})")
    assert last == 1.0, label
    assert share >= 0.85, label


def _quads_a_bin_centre_lies_in(cfg):
    """Without reassignment bin k lands in the row that holds k itself: the row quads that hold a bin of 1 .. n / 2 - 1."""
    _, eb = O.tables(cfg)
    row = np.searchsorted(eb, np.arange(1, cfg.n // 2, dtype=np.float32), side="right") - 1
    out = np.zeros(cfg.rows // 4, bool)
    out[row[(row >= 0) & (row < cfg.rows)] // 4] = True
    return out


@pytest.mark.parametrize("n,hop,rows,reassign", G.FAST_CASES)
def test_fast_input_reaches_every_quad(n, hop, rows, reassign):
    """With reassignment off a bin lands in the row of its own centre, and at 1000 rows the low rows are narrower than a bin: 20 %
    (N = 8192) to 58 % (N = 512) of the row quads hold no bin and are empty for every input.  There the 85 % is asked of the quads
    that hold a bin, and the others must be empty."""
    pcm = G.case_signal(n, hop, rows, reassign)
    assert pcm.dtype == np.float32 and pcm.shape == (G.STREAMS, n + (G.columns(n, hop, reassign) - 1) * hop + 3)
    cfg = O.make_cfg(n, hop, bool(reassign), rows=rows)
    _, _, idx = O.batch_f32(cfg, pcm, want=("index",))
    assert idx.shape == (G.STREAMS, G.columns(n, hop, reassign), rows)
    _check_input(idx, f"FAST {n}/{hop} rows {rows} reassign {reassign}", None if reassign else _quads_a_bin_centre_lies_in(cfg))


@pytest.mark.parametrize("n,hop,rows,axis", G.EXACT_CASES)
def test_exact_input_reaches_every_quad(n, hop, rows, axis):
    pcm = G.case_signal(n, hop, rows)
    assert float(np.max(np.abs(pcm))) <= 4.0          # the EXACT mode's input range
    O.set_custom_edges_hz(G.edges_hz(axis, rows))
    try:
        _, _, idx, _ = O.batch_exact(O.make_cfg(n, hop, True, rows=rows), pcm, want=("index",))
    finally:
        O.set_custom_edges_hz(None)
    _check_input(idx, f"EXACT {n}/{hop} rows {rows} axis {axis}")


def test_signal_is_seeded_float32_noise_on_half_the_synthetic_streams():
    from emspec import synth
    x = G.signal(2, 6000, 7)
    assert x.dtype == np.float32 and x.shape == (2, 6000) and np.array_equal(x, G.signal(2, 6000, 7))
    assert not np.array_equal(x, G.signal(2, 6000, 8))
    noise = x.astype(np.float64) - 0.5 * synth.streams(2, 6000)
    assert abs(float(noise.std()) - 0.1) < 0.005 and abs(float(noise.mean())) < 0.005
    assert abs(np.corrcoef(noise[0], noise[1])[0, 1]) < 0.05
    assert np.array_equal(G.signal(2, 6000, 7, noise=0.0), (0.5 * synth.streams(2, 6000).astype(np.float64)).astype(np.float32))


def test_magic_division_of_the_small_ring_finalize_is_exact():
    """fused_small.hip.inc finalizes up to four columns in one pass: quad q of the pass belongs to column q / qpc, qpc = R / 4,
    taken as __umul24(q, ceil(2^20 / qpc)) >> 20.  For every qpc the launcher can pass (rows 64 .. 1024) and every q of a pass
    the quotient is the integer division's, both factors are below 2^24 and the product fits 32 bits."""
    for qpc in range(16, 257):
        magic = -(-(1 << 20) // qpc)
        q = np.arange(4 * qpc, dtype=np.uint64)
        prod = q * np.uint64(magic)
        assert magic < 1 << 24 and int(q[-1]) < 1 << 24 and int(prod.max()) < 1 << 32, qpc
        assert np.array_equal(prod >> np.uint64(20), q // np.uint64(qpc)), qpc
