"""CPU: what the GPU tests of the live history (tests/test_gpu_live_history.py) take for granted.

Their colour case compares the view's palette index with post_ref.cell_index_f32 of dB + shift and excuses the cells
post_ref.index_borderline names - those within 2^-14 of a step, where a float32 evaluation may land on either side - up to a
share of 1e-3.  With continuous dB about 2 x 2^-14 = 1.2e-4 of the cells are borderline, and the cap is 8 times that.  Here the
reference alone - the CPU bit models' columns of the same test signal, under the same maps and factors - must stay under the
cap, so that the cap excuses rounding and never a wrong law."""
import numpy as np
import pytest

import emspec
import history_ref as H
import oracle as O
import overview_ref as V
import post_ref as P

N, HOP, S, R, FRAMES = 1024, 256, 3, 64, 27
CAP = 1e-3


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_borderline_share_of_the_colour_case_is_under_the_cap(exact):
    pcm = H.signal(S, N + HOP * (FRAMES - 1))
    cfg = O.make_cfg(N, HOP, True, rows=R)
    db = (O.batch_exact(cfg, pcm, want=("db",)) if exact else O.batch_f32(cfg, pcm, want=("db",)))[0]
    assert db.shape == (S, FRAMES, R)
    assert np.ptp(db) > 60.0                                  # loud, quiet and silent columns: the law is exercised
    d = O.DEFAULTS
    border = cells = 0
    for law in (H.VIEW_MAP, (d["db_top"], d["db_range"], d["gate_db"], 0.0)):
        for f in (1, 3, FRAMES):
            shifted = (V.reduce_db(db, f) + np.float32(law[3])).astype(np.float32)
            border += int(np.count_nonzero(P.index_borderline(shifted, *law[:3])))
            cells += shifted.size
            assert len(np.unique(P.cell_index_f32(shifted, *law[:3]))) > 8
    print("borderline", border, "of", cells)
    assert border <= CAP * cells, (border, cells)


def test_the_test_map_differs_from_the_configuration_in_every_field():
    cfg = emspec.default_config()
    assert all(a != b for a, b in zip(H.VIEW_MAP, (cfg.db_top, cfg.db_range, cfg.gate_db, 0.0)))
    lut = H.colour_map()
    assert lut.shape == (256, 4) and len({tuple(x) for x in lut}) == 256
