"""CPU: every signal of tests/worst_signals.py provokes what it is meant to, at every shape of the GPU matrix
(tests/test_gpu_worst_signals.py), measured on the EXACT bit model - so that a GPU pass cannot be vacuous - and stays inside
the contract of the 64-bit cell sum (sums are taken modulo 2^64; a cell that receives more than 2^63 units
is outside the guarantee)."""
import numpy as np
import pytest

import oracle as O
import worst_signals as WS

CASES = [(n, hop, rows, kind) for (n, hop, rows), kinds in WS.shapes().items() for kind in kinds]


@pytest.mark.parametrize("n,hop,rows,kind", CASES)
def test_signal_meets_its_condition(n, hop, rows, kind):
    cfg = O.make_cfg(n, hop, True, rows=rows)
    c = WS.conditions(kind, cfg, WS.signal(kind, n, hop, WS.frames_for(n, hop)))
    print("CONDITIONS", c)
    # the contract of the cell sum: no signal of the matrix wraps it
    assert c["hist_min"] >= 0 and c["hist_max"] < 2 ** 63
    if kind == "loud":          # bins above the upper power gate, in frames that also accumulate bins
        assert c["above_pmax"] >= 1 and c["frames_above_pmax_with_accumulated"] >= 1
    elif kind == "tone_low":    # bins on both sides of the power floor, within 3 dB
        assert c["floor_pass_3db"] >= 1 and c["floor_fail_3db"] >= 1
    elif kind == "chirp_reach":
        assert c["reach_dropped"] >= 1
    elif kind == "impulses":
        assert c["outside_image"] >= 1
    elif kind == "tone_centre":  # one cell receives at least as many bins as frames overlap one column
        assert c["max_bins_per_cell"] >= n // hop
    elif kind == "dc_nyquist":   # (k = 0 and k = n/2 lie off the axis: nothing lands)
        assert c["accumulated"] == 0
    elif kind == "poisoned":
        assert c["accumulated"] > 0


def test_signals_are_float32_of_the_stated_length_and_deterministic():
    for kind in WS.KINDS:
        x = WS.signal(kind, 1024, 256, 18)
        assert x.dtype == np.float32 and x.shape == (1024 + 256 * 17,)
        assert np.array_equal(x, WS.signal(kind, 1024, 256, 18), equal_nan=True)
    p = WS.signal("poisoned", 1024, 256, 18)
    assert np.isnan(p[p.size // 3]) and np.isposinf(p[(2 * p.size) // 3]) and np.isfinite(np.delete(p, [p.size // 3, (2 * p.size) // 3])).all()


@pytest.mark.parametrize("n,hop,frames", [(4096, 256, 24), (16384, 512, 8)])
def test_the_cell_sum_wraps_for_a_click_of_16000(n, hop, frames):
    """The corner OUTSIDE the contract, stated on the model alone: one click of amplitude 16,000 in a silent float stream puts
    n / hop frames x ~n / 2 bins of up to 2^61 units each into one column; the sums pass 2^63 and, taken modulo 2^64 and read as
    int64, come out negative.  Nothing is asserted about the GPU here."""
    x = np.zeros(n + hop * (frames - 1), np.float32)
    x[n // 2 + 3 * hop + 7] = 16000.0
    _, _, _, hist = O.batch_exact(O.make_cfg(n, hop, True), x[None], want=("hist",))
    assert hist.min() < 0


def test_recorded_conditions_are_current():
    """tests/golden/worst_signal_conditions.json records conditions() for every (shape, signal) of the matrix (the numbers quoted
    with the change that introduced the matrix): re-measured here on the two cheapest shapes, and complete for all."""
    import json
    import os
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "worst_signal_conditions.json")))
    by = {(r["n"], r["hop"], r["rows"], r["kind"]): r for r in rec}
    assert set(by) == set(CASES)
    for n, hop, rows in ((1024, 256, 1024), (2048, 300, 1024)):
        for kind in WS.shapes()[(n, hop, rows)]:
            c = WS.conditions(kind, O.make_cfg(n, hop, True, rows=rows), WS.signal(kind, n, hop, WS.frames_for(n, hop)))
            assert c == by[(n, hop, rows, kind)], (c, by[(n, hop, rows, kind)])
