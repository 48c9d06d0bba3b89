"""CPU: the cases of tests/axis_cases.py are pinned and cannot pass vacuously on the GPU.

 - every case has a record in tests/golden/kernel_plans.json; the FAST matrix names every route of its mode, and the EXACT matrix
   reaches exact_lr, exact_parked and exact_records by the axis alone (no switch of the diagnostic build);
 - which specification holds at the top of the axis: the row edges end at min(e[R], N / 2) (emspec_tables.h: edges_bin64; the bit
   models state the same).  On `tel` and `wide32` the unclamped edge exceeds N / 2 at every N of the matrix, so the clamp decides
   there; with it the Nyquist bin of every frame - far above the power floor on this signal - has row -1 in both bit models, and
   the top row of the image does not change when the bin's power does;
 - the oracle's image of every case's input has at least 10 % of its cells non-zero and its top row quad non-zero in at least
   95 % of the columns (`zoom`: 50 %), so a kernel that drops or misplaces the rows at the top of the axis cannot compare equal."""
import ctypes as C

import numpy as np
import pytest

import axis_cases as A
import oracle as O
import row_grid_cases as G

FAST_ROUTES = {"fused_pp", "fused_small", "fused_8192", "fused_16384", "records_f32"}
EXACT_ROUTES = {"exact_lr", "exact_parked", "exact_records"}
SIZES = sorted({n for _, n, _, _ in A.FAST_CASES + A.EXACT_CASES})


def _cfg(axis, n, hop, rows):
    return O.make_cfg(n, hop, True, rows=rows, **A.kw(axis))


def test_every_case_is_recorded_and_the_matrix_reaches_every_route():
    assert {A.fast_plan(*c)["route"] for c in A.FAST_CASES} == FAST_ROUTES
    assert {A.exact_plan(*c)["route"] for c in A.EXACT_CASES} == EXACT_ROUTES
    for a in A.AXES:
        for kernel, n, hop in A.FAST_SHAPES:
            assert A.fast_plan(a, n, hop, 1024)["route"] == kernel
        assert {A.fast_plan(a, n, hop, 68)["route"] for n, hop in A.FAST_SHAPES_68} == FAST_ROUTES
        if a != "zoom":
            assert (a, *A.RECORDS_4092, 4092) in A.FAST_CASES and A.fast_plan(a, *A.RECORDS_4092, 4092)["route"] == "records_f32"
            assert (a, *A.RECORDS_4092, 4092) in A.EXACT_CASES and A.exact_plan(a, *A.RECORDS_4092, 4092)["route"] == "exact_records"
        assert [A.exact_plan(a, n, hop, 68)["route"] for n, hop in A.EXACT_SHAPES_68] == ["exact_lr", "exact_records"]
    # the EXACT route follows the axis (the low-share rule): what the header answers for the defect's axis and for the octave
    route = {c: A.exact_plan(*c)["route"] for c in A.EXACT_CASES}
    assert [route["tel", n, hop, 1024] for n, hop in A.EXACT_SHAPES] == \
        ["exact_parked", "exact_records", "exact_lr", "exact_records", "exact_records"]
    assert [route["cd", n, hop, 1024] for n, hop in A.EXACT_SHAPES] == ["exact_lr"] * 3 + ["exact_records"] * 2
    assert route["zoom", 4096, 256, 1024] == "exact_parked" and route["wide32", 4096, 256, 1024] == "exact_lr"
    assert all(A.exact_plan(*c)["rl"] > 0 for c in A.EXACT_CASES if route[c] == "exact_lr" and c[3] == 1024)
    assert {A.exact_plan(*c)["route"] for c in A.EXACT_RGBA} == EXACT_ROUTES and A.EXACT_RGBA <= set(A.EXACT_CASES)
    assert [route[c] for c in A.STREAMING] == ["exact_parked", "exact_lr"]
    assert all(n >= 4096 and rows <= 1024 for a, n, _, rows in A.FAST_CASES + A.EXACT_CASES if a == "zoom")
    assert len(set(A.FAST_CASES)) == len(A.FAST_CASES) and len(set(A.EXACT_CASES)) == len(A.EXACT_CASES)


def test_the_axis_ends_at_nyquist_by_construction():
    """The specification that holds: e[R] = min(e[R], N / 2), in binary64 and so in float32."""
    assert SIZES == [1024, 2048, 4096, 8192, 16384]
    for n in SIZES:
        for a in A.TOP_ABOVE_NYQUIST:
            assert A.raw_top_edge(a, n) > n / 2, (a, n)                  # the clamp decides
        for a in A.TOP_AT_NYQUIST:
            assert A.raw_top_edge(a, n) == n / 2, (a, n)
        for a in A.TOP_ABOVE_NYQUIST + A.TOP_AT_NYQUIST:
            for rows in (68, 1024, 4092):
                cfg = _cfg(a, n, 256, rows)
                e64, e32 = O.edges64(cfg), O.tables(cfg)[1]
                assert e64[-1] == n / 2 and e32[-1] == np.float32(n / 2) and np.all(np.diff(e64) > 0) and np.all(np.diff(e32) > 0)
    # below the top the table is the unclamped formula's (the clamp touches one entry)
    cfg = _cfg("tel", 4096, 256, 1024)
    lo, hi = float(np.float32(30.0)), float(np.float32(4000.0))
    O.lib().eo_spec_pow.restype = C.c_double
    O.lib().eo_spec_pow.argtypes = [C.c_double, C.c_double]
    want = [lo * O.lib().eo_spec_pow(hi / lo, r / 1024) * 4096.0 / 8000.0 for r in range(1024)]
    assert np.array_equal(O.edges64(cfg)[:-1], np.array(want))


@pytest.mark.parametrize("axis", A.TOP_ABOVE_NYQUIST)
@pytest.mark.parametrize("n,hop", A.EXACT_SHAPES)
def test_the_nyquist_bin_reaches_no_row_in_either_bit_model(axis, n, hop):
    """Bin N / 2 of every frame: power far above the floor, row -1 (its k-hat is exactly N / 2 in the models' arithmetic).  Before
    the clamp frames_exact gave row R - 1 on these two axes, and the one-kernel EXACT routes, which never visit the bin, differed
    from it."""
    pcm = A.case_signal(axis, n, hop, 1024)
    cfg = _cfg(axis, n, hop, 1024)
    pfloor = 1e-14 * (n / 4.0) ** 2
    pw, col, row, q = O.frames_exact(cfg, pcm[0], 0, A.DUMP_FRAMES)
    assert np.all(pw[:, n // 2] > 1e6 * pfloor) and np.all(row[:, n // 2] == -1) and np.all(q[:, n // 2] == 0)
    pw32, _, row32 = O.frames_f32(cfg, pcm[0], 0, A.DUMP_FRAMES)
    assert np.all(pw32[:, n // 2] > 1e6 * pfloor) and np.all(row32[:, n // 2] == -1)
    # the bins below it do land on the top rows: the top of the image is not empty because everything was dropped
    assert np.any(row[:, :n // 2] == 1023)


def test_the_top_row_does_not_follow_the_nyquist_bin_s_power():
    """`tel` at 4096 / 256: a frame's only bin with k-hat = N / 2 exactly is the Nyquist bin.  Its rows are the same whether the
    signal carries 0.2 cos(pi t) or not only if no route accumulates it; the component's skirt (bins N / 2 - 2, N / 2 - 1) does
    change the top rows, so the two images differ there - what is asserted is the dump's row of the bin itself, in both."""
    n, hop = 4096, 256
    cfg = _cfg("tel", n, hop, 1024)
    L = A.length(n, hop)
    for nyq in (A.NYQUIST, 0.0):
        x = A.signal(1, L, nyquist=nyq)[0]
        pw, col, row, q = O.frames_exact(cfg, x, 0, 3)
        assert np.all(row[:, n // 2] == -1) and np.all(q[:, n // 2] == 0)
    with_, without = (O.batch_exact(cfg, A.signal(1, L, nyquist=v), want=("index",))[2] for v in (A.NYQUIST, 0.0))
    assert not np.array_equal(with_[..., -4:], without[..., -4:])      # the input does reach the top quad


def _conditions(index, label, axis):
    S, C, R = index.shape
    cells = float(np.mean(index != 0))
    top = float((index[:, :, -4:] != 0).any(axis=2).mean())
    print(f"CONDITIONS {label}: {100 * cells:.1f} % of the cells non-zero, top row quad non-zero in {100 * top:.1f} % of the columns")
    assert cells >= 0.10, label
    assert top >= (0.50 if axis == "zoom" else 0.95), label


@pytest.mark.parametrize("axis,n,hop,rows", A.FAST_CASES)
def test_fast_input_fills_the_image_and_its_top(axis, n, hop, rows):
    pcm = A.case_signal(axis, n, hop, rows)
    assert pcm.dtype == np.float32 and pcm.shape == (A.STREAMS, n + (A.columns(n, hop) - 1) * hop + 3)
    _, _, idx = O.batch_f32(_cfg(axis, n, hop, rows), pcm, want=("index",))
    assert idx.shape == (A.STREAMS, A.columns(n, hop), rows)
    _conditions(idx, f"FAST {axis} {n}/{hop} rows {rows}", axis)


@pytest.mark.parametrize("axis,n,hop,rows", A.EXACT_CASES)
def test_exact_input_fills_the_image_and_its_top(axis, n, hop, rows):
    pcm = A.case_signal(axis, n, hop, rows)
    assert float(np.max(np.abs(pcm))) <= 4.0          # the EXACT mode's input range
    _, _, idx, _ = O.batch_exact(_cfg(axis, n, hop, rows), pcm, want=("index",))
    _conditions(idx, f"EXACT {axis} {n}/{hop} rows {rows}", axis)


def test_signal_is_the_row_grid_signal_plus_a_nyquist_cosine():
    x = A.signal(2, 6000)
    assert x.dtype == np.float32 and np.array_equal(x, A.signal(2, 6000))
    assert np.array_equal(A.signal(2, 6000, nyquist=0.0), G.signal(2, 6000))
    d = x.astype(np.float64) - G.signal(2, 6000)
    t = np.arange(6000)
    assert np.max(np.abs(d - A.NYQUIST * np.cos(np.pi * t))) < 1e-7
