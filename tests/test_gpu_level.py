"""GPU: the level meters (include/emspec.h: emspec_level_device, emspec_cross_device,
emspec_set_level_out, emspec_set_cross_out).  The device entries and the entries of the host pipeline against tests/level_ref.py,
byte for byte in both arithmetic modes (a record is a function of the samples' bits); the long-window split with its integer
atomics; the images of a call with the settings on are those of the same call with them cleared; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import emspec
import level_ref as LR
import pcm_ref as PR
from emspec import synth
from window_cases import DEVICE_CASES, IDS, PATHS, PRECEDENCE, SPLIT_CASES, _team

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32


@pytest.fixture(scope="module")
def fast():
    with emspec.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def exact():
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        yield e


def _to_dev(x):
    """numpy [S, L] -> a CUDA tensor 4 bytes into an allocation"""
    S, L = x.shape
    buf = torch.empty(S * L + 1, dtype=torch.float32, device="cuda")
    src = buf[1:].view(S, L)
    src.copy_(torch.from_numpy(x))
    assert src.data_ptr() % 16 == 4
    return src


def _records(e, call, rows, Cr, dtype):
    """Runs call(out) on a poisoned uint8 output 8 bytes into an allocation, with a sentinel of 8 bytes on either side that must
    stay -> numpy [rows, Cr] of dtype."""
    size = dtype.itemsize
    obuf = torch.full((rows * Cr * size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    out = obuf[8:8 + rows * Cr * size].view(rows, Cr, size)
    assert out.data_ptr() % 16 == 8
    call(out)
    torch.cuda.synchronize()
    e.device_status()
    got = obuf.cpu().numpy()
    assert np.all(got[:8] == 0xA5) and np.all(got[-8:] == 0xA5), "records were written outside [rows][Cr]"
    return got[8:-8].view(dtype).reshape(rows, Cr)


def _dev_level(e, x, n, hop, f):
    Cr = LR.levels(x[:1, :], n, hop, f).shape[1]
    src = _to_dev(x)
    return _records(e, lambda out: e.level_device(src, n, hop, f, out=out), x.shape[0], Cr, emspec.LEVEL_DTYPE)


def _dev_cross(e, x, views, a, b, n, hop, f):
    Cr = LR.levels(x[:1, :], n, hop, f).shape[1]
    src = _to_dev(x)
    return _records(e, lambda out: e.cross_device(src, views, a, b, n, hop, f, out=out), x.shape[0] // views, Cr, emspec.CROSS_DTYPE)


# ---- 1. the device entry on the cases shared with the envelope's suite (tests/window_cases.py): every team size from one lane
# (hop 1) to 64 (hop = n = 4096), and the split
def test_cases_cover_every_path():
    assert {_team(*c) for c in DEVICE_CASES} == PATHS == {1, 2, 4, 8, 16, 32, 64, "split"}
    assert _team(256, 1, 300, 1) == 1 and _team(4096, 4096, 5 * 4096 + 1, 1) == 64


@pytest.mark.parametrize("case", DEVICE_CASES, **IDS)
def test_level_device_is_the_reference(fast, case):
    n, hop, L, f = case
    x = LR.case_signal(case)
    assert LR.same(_dev_level(fast, x, n, hop, f), LR.levels(x, n, hop, f))


# ---- 2. long windows: pieces over workgroups, combined with 64-bit integer atomics into a zeroed record
@pytest.mark.parametrize("case", SPLIT_CASES, **IDS)
def test_split_path(fast, case):
    n, hop, L, f = case
    x = LR.case_signal(case, seed=2)
    want = LR.levels(x, n, hop, f)
    assert _team(*case) == "split" and (f == 65536 or (want.shape[1] == 3 and 2560 < 16384 < 65536 < 300 * 256))
    assert LR.same(_dev_level(fast, x, n, hop, f), want)
    assert LR.same(_dev_cross(fast, x, 3, 0, 2, n, hop, f), LR.crosses(x, 3, 0, 2, n, hop, f))


def test_exact_engine_with_a_time_reduction_gives_the_same_bytes(exact):
    case = (4096, 257, 4096 + 257 * 20, 3)
    assert case in LR.CASES
    x = LR.case_signal(case)
    exact.set_time_reduce(5)     # the engine's time reduction plays no part: the factor is the call's own
    try:
        assert LR.same(_dev_level(exact, x, *case[:2], case[3]), LR.levels(x, *case[:2], case[3]))
    finally:
        exact.set_time_reduce(1)


# ---- 3. the cross entry
@pytest.mark.parametrize("case", [(256, 1, 300, 7), (1024, 255, 1024 + 255 * 9 + 100, 1), (4096, 256, 3 * 4096 + 77, 2),
                                  (1024, 256, 2 ** 15 + 1, 65536)], **IDS)
def test_cross_device(fast, case):
    n, hop, L, f = case
    x = LR.signal(8, L, n, hop, f, seed=9)                     # two pairs of four views; L odd: the two streams' alignments differ
    assert LR.same(_dev_cross(fast, x, 4, 0, 1, n, hop, f), LR.crosses(x, 4, 0, 1, n, hop, f))
    # a == b: the cross limbs reproduce the level's sums
    self = _dev_cross(fast, x, 4, 2, 2, n, hop, f)
    lv = LR.levels(x[2::4], n, hop, f)
    assert LR.same(self, LR.crosses(x, 4, 2, 2, n, hop, f))
    assert np.array_equal(self["lo"], lv["sq_lo"]) and np.array_equal(self["hi"].astype(np.uint64), lv["sq_hi"])
    # views 1: every stream its own pair
    assert LR.same(_dev_cross(fast, x, 1, 0, 0, n, hop, f), LR.crosses(x, 1, 0, 0, n, hop, f))


# ---- 4. the host pipeline, on the diagnostic library with the unit count forced so that units are crossed
@pytest.fixture(scope="module", params=[False, True], ids=["fast", "exact"])
def pipe(request):
    with emspec.Engine(mode=emspec.MODE_EXACT if request.param else emspec.MODE_FAST, diag=True, rows=256) as e:
        yield e, request.param


def _with_and_without(e, is_exact, run, S, Cr, pairs=0, ab=None):
    """run() -> dict of arrays.  Once with the settings on (poisoned arrays, one record more than needed), once cleared.  EXACT: the
    outputs are the same bytes.  FAST: the palette index is; its dB is not reproducible to the last bit from run to run whatever
    is set (float accumulation order, DESIGN.md §8: 1.5e-5 dB observed), so dB and peak lists are compared to 1e-4 dB, the
    mode's own accuracy.  Returns (level records [S, Cr], cross records [pairs, Cr] or None)."""
    level = np.full(S * Cr + 1, 0xA5, np.uint8).repeat(24).view(emspec.LEVEL_DTYPE)
    cross = np.full(pairs * Cr + 1, 0xA5, np.uint8).repeat(16).view(emspec.CROSS_DTYPE) if pairs else None
    e.set_level_out(level)
    try:
        if pairs:
            e.set_cross_out(ab[0], ab[1], cross)
        with_ = run()
    finally:
        e.set_level_out(None)
        e.set_cross_out(0, 0, None)
    poison = np.full(24, 0xA5, np.uint8)
    assert level[-1].tobytes() == poison.tobytes() and (cross is None or cross[-1].tobytes() == poison[:16].tobytes())
    kept = level.copy(), None if cross is None else cross.copy()
    without = run()
    assert LR.same(level, kept[0]) and (cross is None or LR.same(cross, kept[1])), "a cleared setting was written"
    assert with_.keys() == without.keys()
    for k in with_:
        a, b = with_[k], without[k]
        assert (a is None) == (b is None)
        if a is None:
            continue
        if is_exact or a.dtype == np.uint8:
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{k} differs with the settings on"
        else:
            assert a.shape == b.shape and np.allclose(a, b, rtol=0, atol=1e-4, equal_nan=True), f"{k} differs with the settings on"
    return level[:-1].reshape(S, Cr), None if cross is None else cross[:-1].reshape(pairs, Cr)


@pytest.mark.parametrize("f", [1, 3])
def test_host_pipeline_entries(pipe, f, monkeypatch):
    e, is_exact = pipe
    monkeypatch.setenv("EMSPEC_PIPE_CHUNKS", "3")
    S = 5
    e.set_time_reduce(f)
    try:
        # emspec_batch, index out: 5 streams in 3 units
        n, hop, L = 1024, 255, 1024 + 255 * 70 + 11
        x = LR.signal(S, L, n, hop, f, seed=6, finite=True)
        Cr = emspec.reduced_columns(emspec.num_columns(L, n, hop), f)
        got, _ = _with_and_without(e, is_exact, lambda: e.batch(x, n, hop, True, want=("index", "db")), S, Cr)
        assert LR.same(got, LR.levels(x, n, hop, f))
        # emspec_batch_pcm: 3 stereo S16 sources -> L R M S at 4096 / 256, level records of the 12 views and the cross records
        # of (left, right) of each source; the float streams exist in no host buffer (tests/pcm_ref.py decodes them)
        n, hop, sources = 4096, 256, 3
        frames = n + hop * 29 + 3
        fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
        rng = np.random.default_rng(11 + f)
        raw = rng.integers(-20000, 20000, (sources, frames * 2), dtype=np.int16)
        raw[1, 1::2] = -raw[1, 0::2]                          # source 1: right = -left
        raw[2, 1::2] = raw[2, 0::2]                           # source 2: right = left
        raw[0, 2 * (n // 2 + 20 * hop)] = 32767
        raw[0, 2 * (n // 2 + 20 * hop) + 1] = -32768
        dec = PR.decode(raw.view(np.uint8), PR.S16, 2, fmt.matrix)
        Cr = emspec.reduced_columns(emspec.num_columns(frames, n, hop), f)
        got, cgot = _with_and_without(e, is_exact, lambda: e.batch_pcm(raw, fmt, n, hop, True, want=("index", "db")), sources * 4, Cr,
                                      pairs=sources, ab=(0, 1))
        want = LR.levels(dec, n, hop, f)
        assert LR.same(got, want) and LR.same(cgot, LR.crosses(dec, 4, 0, 1, n, hop, f))
        # ... and the helpers read them: the inverted source correlates -1, the copied one +1, and its side view is silent
        lv = got.reshape(sources, 4, Cr)
        assert emspec.cross_correlation(lv[1, 0, 0], lv[1, 1, 0], cgot[1, 0]) == -1.0
        assert emspec.cross_correlation(lv[2, 0, 0], lv[2, 1, 0], cgot[2, 0]) == 1.0
        assert emspec.level_values(lv[2, 3, 0], emspec.level_window(frames, n, hop, f, 0)) == (-np.inf, -np.inf)
        assert not (want["odd"] > 0).any() and (want["peak"] > 0).any()
        # emspec_batch_multires at 16384 / 4096 / 256: the column grid is the long band's
        n_low, n_high, hop = 16384, 4096, 256
        L = n_low + hop * 21 + 1
        x = LR.signal(S, L, n_low, hop, f, seed=7, finite=True)
        Cr = emspec.reduced_columns(emspec.multires_columns(L, n_low, n_high, hop), f)
        split = e.split_row_for_hz(250.0)
        got, _ = _with_and_without(e, is_exact, lambda: e.batch_multires(x, n_low, n_high, hop, split, True, want=("index",)), S, Cr)
        assert LR.same(got, LR.levels(x, n_low, hop, f))
        # emspec_batch_peaks (full rate only)
        if f == 1:
            n, hop, L = 4096, 256, 4096 + 256 * 30 + 9
            x = (synth.streams(S, L) * F(0.5)).astype(F)
            Cn = emspec.num_columns(L, n, hop)
            got, _ = _with_and_without(e, is_exact, lambda: {"peaks": e.batch_peaks(x, n, hop, True, 4, -60.0)}, S, Cn)
            assert LR.same(got, LR.levels(x, n, hop, 1))
    finally:
        e.set_time_reduce(1)


@pytest.mark.parametrize("f", [1, 3])
def test_one_long_stream_cut_into_runs(pipe, f, monkeypatch):
    """ONE stream of 2^18 samples at 256 / 7: 37,413 columns, the fewest streams and about the fewest columns the pipeline cuts
    into runs of columns (two, of 16,384 or more, with a halo); the windows start `skip` columns into each run's staged samples,
    and with f = 3 the runs start on multiples of 3."""
    e, is_exact = pipe
    monkeypatch.setenv("EMSPEC_PIPE_CHUNKS", "3")
    n, hop, L = 256, 7, 2 ** 18
    Cn = emspec.num_columns(L, n, hop)
    assert Cn // 16384 == 2
    x = LR.signal(1, L, n, hop, f, seed=5, finite=True)
    e.set_time_reduce(f)
    try:
        got, _ = _with_and_without(e, is_exact, lambda: e.batch(x, n, hop, True, want=("index",)), 1, emspec.reduced_columns(Cn, f))
    finally:
        e.set_time_reduce(1)
    assert LR.same(got, LR.levels(x, n, hop, f))


# ---- 5. state and refusals
def _refused(code, call, word):
    with pytest.raises(emspec.EmspecError) as ei:
        call()
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def test_refusals_through_the_engine(exact):
    S, L, n, hop = 4, 2 ** 13 + 1, 1024, 256
    x = LR.signal(S, L, n, hop, 1, seed=8, finite=True)
    Cn = emspec.num_columns(L, n, hop)
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right"))
    raw = np.random.default_rng(3).integers(-9000, 9000, (2, L * 2), dtype=np.int16)
    gather = lambda: exact._chk(exact._lib.emspec_batch_gather(exact._h, x.ctypes.data_as(C.c_void_p), S, L, n, hop, 1, 0, None, None, None))
    db = np.full((S, Cn, exact.rows), 7.0, F)
    level = np.zeros(S * Cn - 1, emspec.LEVEL_DTYPE)
    cross = np.zeros(2 * Cn, emspec.CROSS_DTYPE)
    try:
        # one record short: refused before anything runs
        exact.set_level_out(level)
        _refused(emspec.ERR_INVALID_ARG, lambda: exact.batch(x, n, hop, True, want=("db",), db_out=db), "emspec_set_level_out")
        assert np.all(db == 7.0) and not level.view(np.uint8).any()
        _refused(emspec.ERR_STATE, gather, "emspec_set_level_out")
        exact.set_level_out(None)
        # cross records: a state error on float streams and for the gather; bad views and a short array are refused on PCM
        exact.set_cross_out(0, 1, cross)
        _refused(emspec.ERR_STATE, lambda: exact.batch(x, n, hop, True, want=("db",), db_out=db), "emspec_set_cross_out")
        _refused(emspec.ERR_STATE, lambda: exact.batch_peaks(x, n, hop, True, 4, -60.0), "emspec_set_cross_out")
        _refused(emspec.ERR_STATE, gather, "emspec_set_cross_out")
        assert np.all(db == 7.0)
        exact.batch_pcm(raw, fmt, n, hop, True, want=("index",))
        assert LR.same(cross.reshape(2, Cn), LR.crosses(PR.decode(raw.view(np.uint8), PR.S16, 2, fmt.matrix), 2, 0, 1, n, hop, 1))
        exact.set_cross_out(0, 2, cross)
        _refused(emspec.ERR_INVALID_ARG, lambda: exact.batch_pcm(raw, fmt, n, hop, True, want=("index",)), "views")
        exact.set_cross_out(1, 0, cross[:2 * Cn - 1])
        _refused(emspec.ERR_INVALID_ARG, lambda: exact.batch_pcm(raw, fmt, n, hop, True, want=("index",)), "emspec_set_cross_out")
    finally:
        exact.set_level_out(None)
        exact.set_cross_out(0, 0, None)
    # cleared: nothing is written, the engine is usable, and the gather's refusal is the communicator's again
    kept = cross.copy()
    out = exact.batch(x, n, hop, True, want=("db",), db_out=db)
    assert out["db"] is db and not np.any(db == 7.0) and LR.same(cross, kept) and not level.view(np.uint8).any()
    _refused(emspec.ERR_STATE, gather, "communicator")
    # the setters' and the device entries' refusals: every one INVALID_ARG with a message, nothing written
    lib, h = exact._lib, exact._h
    lp, cp = level.ctypes.data_as(C.c_void_p), cross.ctypes.data_as(C.c_void_p)
    assert lib.emspec_set_level_out(h, lp, -1) == emspec.ERR_INVALID_ARG and lib.emspec_set_cross_out(h, 0, 1, cp, -1) == emspec.ERR_INVALID_ARG
    assert lib.emspec_set_level_out(h, C.c_void_p(level.ctypes.data + 4), 1) == emspec.ERR_INVALID_ARG and "8-byte" in lib.emspec_last_error(h).decode()
    assert lib.emspec_set_cross_out(h, 0, 64, cp, 1) == emspec.ERR_INVALID_ARG and lib.emspec_set_cross_out(h, -1, 0, cp, 1) == emspec.ERR_INVALID_ARG
    t = torch.from_numpy(x).cuda()
    o = torch.full((S * Cn * 24 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, q = t.data_ptr(), o.data_ptr()
    for args, word in [((p, S, L, n, hop, 1, q + 4), "8-byte"), ((p + 2, S, L - 1, n, hop, 1, q), "4-byte"), ((p, S, L, n, hop, 0, q), "factor"),
                       ((p, S, L, n, hop, 65537, q), "factor"), ((p, S, L, n, 0, 1, q), "hop"), ((p, S, L, n, n + 1, 1, q), "hop"),
                       ((p, S, L, 1000, hop, 1, q), "fft size"), ((p, 65536, L, n, hop, 1, q), "streams"), ((None, S, L, n, hop, 1, q), "null"),
                       ((p, S, L, n, hop, 1, None), "null")]:
        a = list(args)
        rc = lib.emspec_level_device(h, C.c_void_p(a[0]), *a[1:6], C.c_void_p(a[6]), st)
        assert rc == emspec.ERR_INVALID_ARG and word in lib.emspec_last_error(h).decode(), (args, lib.emspec_last_error(h).decode())
    for args, word in [((p, 2, 2, 0, 1, L, n, hop, 1, q + 4), "8-byte"), ((p, 2, 0, 0, 0, L, n, hop, 1, q), "views"), ((p, 1, 65, 0, 0, L, n, hop, 1, q), "views"),
                       ((p, 2, 2, 2, 0, L, n, hop, 1, q), "a and b"), ((p, 2, 2, 0, -1, L, n, hop, 1, q), "a and b"),
                       ((p, 1024, 64, 0, 1, L, n, hop, 1, q), "pairs x views"), ((p, 2, 2, 0, 1, L, n, hop, 0, q), "factor"),
                       ((p, 2, 2, 0, 1, L, 1000, hop, 1, q), "fft size"), ((None, 2, 2, 0, 1, L, n, hop, 1, q), "null")]:
        a = list(args)
        rc = lib.emspec_cross_device(h, C.c_void_p(a[0]), *a[1:9], C.c_void_p(a[9]), st)
        assert rc == emspec.ERR_INVALID_ARG and word in lib.emspec_last_error(h).decode(), (args, lib.emspec_last_error(h).decode())
    assert lib.emspec_level_device(h, None, 0, L, n, hop, 1, None, st) == 0 and lib.emspec_cross_device(h, None, 2, 2, 0, 1, n - 1, n, hop, 1, None, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(o == 0xA5))
    got = exact.level_device(t, n, hop, 1).cpu().numpy().view(emspec.LEVEL_DTYPE)[..., 0]
    assert LR.same(got, LR.levels(x, n, hop, 1))


def test_device_entries_report_the_first_broken_rule(exact):
    """With more than one rule broken the three device entries report the same one as the host forms (tests/test_level_cpu.py):
    the pair's rules (cross), then streams, length, FFT size, hop, factor.  Refused before anything is read or written."""
    lib, h = exact._lib, exact._h
    t = torch.zeros(4 * 1000, dtype=torch.float32, device="cuda")
    o = torch.full((4 * 8 * 24,), 0xA5, dtype=torch.uint8, device="cuda")
    p, q, st = C.c_void_p(t.data_ptr()), C.c_void_p(o.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (S, L, n, hop, f), word in PRECEDENCE:
        for call in (lambda: lib.emspec_wave_device(h, p, S, L, n, hop, f, q, st), lambda: lib.emspec_level_device(h, p, S, L, n, hop, f, q, st),
                     lambda: lib.emspec_cross_device(h, p, S, 1, 0, 0, L, n, hop, f, q, st)):
            msg = (call(), lib.emspec_last_error(h).decode())
            assert msg[0] == emspec.ERR_INVALID_ARG and word in msg[1], ((S, L, n, hop, f), msg)
    assert lib.emspec_cross_device(h, p, -1, 0, 0, 0, -1, 300, 0, 0, q, st) == emspec.ERR_INVALID_ARG and "views" in lib.emspec_last_error(h).decode()
    torch.cuda.synchronize()
    assert bool(torch.all(o == 0xA5))
