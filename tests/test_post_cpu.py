"""The display post-process law on the CPU: tests/post_ref.py's bound is valid - every correct float32
evaluation of the law lies within it of the binary64 reference - and it has teeth: a warm-up of 128 columns, other AGC
constants, another gain clamp and a chunk that restarts from y = 0 all leave it.  Both gain clamps are reached by
construction.  The GPU tests (tests/test_gpu_post.py) compare the kernels with the same reference under the same bound.
"""
import numpy as np
import pytest

import oracle as O
import post_ref as P

N, HOP, C, S = 1024, 256, 2600, 2
SETTINGS = [(0.95, 1.0), (0.95, 0.0), (0.0, 1.0), (0.6, 0.8)]
TOP_DEFAULT, TOP_LOW = 0.0, -60.0          # the engine's default db_top; one at which the -40 dB clamp can be reached


@pytest.fixture(scope="module")
def raw():
    pcm = P.signals(S, N + HOP * (C - 1), HOP)
    db, _, _ = O.batch_f32(O.make_cfg(N, HOP, True), pcm, want=("db",))
    db.setflags(write=False)
    return db


_refs = {}


def _reference(raw, sm, agc, top):
    key = (sm, agc, top)
    if key not in _refs:
        _refs[key] = P.reference(raw, sm, agc, top)
    return _refs[key]


def _ratio(got, raw, sm, agc, top):
    y, _ = _reference(raw, sm, agc, top)
    return float(np.max(np.abs(got.astype(np.float64) - y))) / P.bound(sm, agc, np.max(np.abs(y)))


def test_signals_are_what_the_docstring_says():
    a, b = P.signals(5, 97 * 256 * 5 + 11), P.signals(5, 97 * 256 * 2)
    assert a.dtype == np.float32 and np.array_equal(a[:, :b.shape[1]], b)          # a prefix, whatever the length
    assert np.max(np.abs(a)) <= 1.0
    seg = 97 * 256
    for s in range(5):
        peaks = [float(np.max(np.abs(a[s, k * seg:(k + 1) * seg]))) for k in range(5)]
        want = [P.LEVELS[(k + s) % 4] / (1.0 + 0.13 * (s // 4)) for k in range(5)]
        for got, lv in zip(peaks, want):
            assert (got == 0.0) if lv == 0.0 else (0.6 * lv < got <= lv)
    assert len({a[s].tobytes() for s in range(5)}) == 5


def test_the_reference_magnitude_covers_what_gets_rounded(raw):
    """bound() wants M above every magnitude that is rounded; the tests hand it max |reference y|.  On these signals that is
    within 1 % of the largest of |raw| and |raw + g| (a loud column's empty cells sit at the -200 dB floor plus a gain of about
    a dB), and every dB value is negative, so |m - p| <= M where the derivation allows 2 M: 52 u M where it charges 54."""
    for sm, agc in SETTINGS:
        for top in (TOP_DEFAULT, TOP_LOW):
            y, g = _reference(raw, sm, agc, top)
            x = raw.astype(np.float64) + g[:, :, None]
            assert np.max(np.abs(y)) >= 0.99 * max(np.max(np.abs(x)), float(np.max(np.abs(raw))))
    assert raw.max() < 0.0


@pytest.mark.parametrize("top", [TOP_DEFAULT, TOP_LOW])
@pytest.mark.parametrize("sm,agc", SETTINGS)
def test_correct_float32_evaluations_lie_within_the_bound(raw, sm, agc, top):
    for fused in (False, True):
        r = _ratio(P.model_f32(raw, sm, agc, top, fused=fused), raw, sm, agc, top)
        print(f"model_f32 fused={fused} sm={sm} agc={agc} db_top={top}: max error / bound = {r:.3f}")
        assert r <= 1.0
    cfg = O.make_cfg(N, HOP, True, db_top=top)
    r = _ratio(O.postprocess(raw, sm, agc, cfg)[0], raw, sm, agc, top)
    print(f"oracle.postprocess sm={sm} agc={agc} db_top={top}: max error / bound = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("name,sm,agc,top,kw", [
    ("warm-up of 128 columns", 0.95, 1.0, TOP_DEFAULT, dict(warm=128)),
    ("warm-up of 128 columns, no AGC", 0.95, 0.0, TOP_DEFAULT, dict(warm=128)),
    ("falling constant 0.025", 0.95, 1.0, TOP_DEFAULT, dict(down=0.025)),
    ("rising constant 0.2", 0.95, 1.0, TOP_DEFAULT, dict(up=0.2)),
    ("gain clamp 39, upper side", 0.95, 1.0, TOP_DEFAULT, dict(gmax=39)),
    ("gain clamp 39, lower side", 0.6, 0.8, TOP_LOW, dict(gmax=39)),
    ("chunk restarts from y = 0", 0.95, 1.0, TOP_DEFAULT, dict(chunk_start="zero")),
])
def test_the_bound_has_teeth(raw, name, sm, agc, top, kw):
    r = _ratio(P.model_f32(raw, sm, agc, top, **kw), raw, sm, agc, top)
    print(f"{name}: max error / bound = {r:.1f}")
    assert r > 1.0


def test_the_chunk_arithmetic_of_the_model_matters_only_through_the_warm_up(raw):
    """One chunk over everything (no restart at all) and the kernel's 1024 / 512 agree to far below the bound at 0.95: the
    figure POST_WARM = 512 rests on."""
    whole = P.model_f32(raw, 0.95, 1.0, TOP_DEFAULT, chunk=1 << 30)
    cut = P.model_f32(raw, 0.95, 1.0, TOP_DEFAULT)
    y, _ = _reference(raw, 0.95, 1.0, TOP_DEFAULT)
    assert np.max(np.abs(whole.astype(np.float64) - cut)) <= 0.01 * P.bound(0.95, 1.0, np.max(np.abs(y)))


def test_both_gain_clamps_are_reached(raw):
    p = P.level(raw)
    for agc in (1.0, 0.8):
        # +40 at the default db_top, on the silent stretch: the level has fallen towards the -200 dB floor
        _, g = _reference(raw, 0.6 if agc == 0.8 else 0.95, agc, TOP_DEFAULT)
        silent = raw.max(axis=2) < -199.0
        at = (g == 40.0) & silent
        assert at.any(axis=1).all()                                   # in every stream
        unclamped = float(np.float32(agc)) * (TOP_DEFAULT - p[at])
        assert np.all(unclamped > 40.0) and unclamped.max() > 100.0      # the unclamped value is beyond the clamp, by far
        assert not (g == -40.0).any()                                 # the other side cannot be reached at this db_top
        # -40 at db_top = -60, on the loud stretch
        _, g = _reference(raw, 0.6 if agc == 0.8 else 0.95, agc, TOP_LOW)
        loud = raw.max(axis=2) > -10.0
        at = (g == -40.0) & loud
        assert at.any(axis=1).all()
        unclamped = float(np.float32(agc)) * (TOP_LOW - p[at])
        assert np.all(unclamped < -40.0) and unclamped.min() < -45.0
        assert (g == 40.0).any()                                      # and +40 is reached there as well
    # both already in the first column (the GPU cases of 1, 2, 3 and 5 columns rely on it): stream 0 starts loud, stream 1 silent
    assert _reference(raw, 0.95, 1.0, TOP_LOW)[1][0, 0] == -40.0 and _reference(raw, 0.95, 1.0, TOP_DEFAULT)[1][1, 0] == 40.0
    assert _reference(raw, 0.6, 0.8, TOP_LOW)[1][0, 0] == -40.0 and _reference(raw, 0.6, 0.8, TOP_DEFAULT)[1][1, 0] == 40.0


def test_few_cells_sit_on_a_palette_step(raw):
    """The GPU index test lets the index differ by one where v 255 + 0.5 is within 2^-14 of an integer: on the reference's own
    dB such cells stay under 0.1 % of all cells."""
    for sm, agc in SETTINGS:
        for top in (TOP_DEFAULT, TOP_LOW):
            y, _ = _reference(raw, sm, agc, top)
            share = float(np.mean(P.index_borderline(y, top)))
            print(f"sm={sm} agc={agc} db_top={top}: cells on a palette step {share:.2e}")
            assert share < 1e-3


def test_index_restatement_equals_the_oracle_colour_stage(raw):
    cfg = O.make_cfg(N, HOP, True)
    out, idx, _ = O.postprocess(raw[:, :300], 0.6, 0.8, cfg)
    assert np.array_equal(P.cell_index_f32(out, TOP_DEFAULT), idx)


def test_per_column_settings_restate_the_scalar_ones(raw):
    y, g = P.reference(raw[:, :400], 0.6, 0.8, TOP_DEFAULT)
    y2, g2 = P.reference(raw[:, :400], np.full(400, 0.6), np.full(400, 0.8), TOP_DEFAULT)
    assert np.array_equal(y, y2) and np.array_equal(g, g2)
