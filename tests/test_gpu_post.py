"""The display post-process (post.hip.inc, live_launch.hip.inc) at its limits against binary64.

Every comparison: an EXACT-mode engine (the raw columns are the same bytes in every call) delivers `raw` with the display
off; with the display on, its dB must lie within post_ref.bound(sm, agc, max |reference|) of
post_ref.reference(raw, ...), the law evaluated sequentially in binary64.  tests/test_post_cpu.py shows on the CPU that the
bound holds for correct float32 evaluations and that a warm-up of 128 columns, other AGC constants, a clamp of 39 dB or a
chunk restarted from zero leave it.  Every case prints its max error / bound.
"""
import numpy as np
import pytest

import emspec
import oracle as O
import post_ref as P

pytestmark = pytest.mark.gpu

N, HOP = 1024, 256
D = 2                                       # emspec.latency_columns(1024, 256, True), asserted below
SETTINGS = [(0.95, 1.0), (0.95, 0.0), (0.0, 1.0), (0.6, 0.8)]
COLUMNS = [1, 2, 3, 5, 1023, 1024, 1025, 1537, 2049]
TOP_DEFAULT, TOP_LOW = 0.0, -60.0           # as tests/test_post_cpu.py: +40 dB is reached at the first, -40 dB at the second
FAST_TOL_DB = 8.7e-4                        # the project's FAST-mode dB tolerance ("Tolerances in the tests")


def _samples(columns):
    return N + HOP * (columns - 1)


_pcm_cache = {}


def _pcm(S, columns):
    """signals() is a prefix of any longer signals(): one array per S, grown on demand."""
    L = _samples(columns)
    if S not in _pcm_cache or _pcm_cache[S].shape[1] < L:
        _pcm_cache[S] = P.signals(S, L, HOP)
    return np.ascontiguousarray(_pcm_cache[S][:, :L])


@pytest.fixture(scope="module")
def engines(engine):
    """EXACT-mode engines by (db_top, rows), made on demand, closed with the module.  (`engine`: the session's engine has
    settled the torch / HIP load order.)"""
    made = {}

    def get(top=TOP_DEFAULT, rows=1024):
        if (top, rows) not in made:
            made[top, rows] = emspec.Engine(mode=emspec.MODE_EXACT, db_top=top, rows=rows)
        e = made[top, rows]
        e.reset()
        e.set_display(0.0, 0.0)
        return e
    yield get
    for e in made.values():
        e.close()


_raw_cache = {}


def _raw(e, key, pcm):
    """The engine's own raw columns (display off), once per (engine, signal)."""
    if key not in _raw_cache:
        e.set_display(0.0, 0.0)
        db = e.batch(pcm, N, HOP, True, want=("db",))["db"]
        db.setflags(write=False)
        _raw_cache[key] = db
    return _raw_cache[key]


def _within(got, want, sm, agc, label, scale=1.0, extra=0.0):
    """max |got - want| against scale * bound + extra; prints the ratio, returns it."""
    lim = scale * P.bound(sm, agc, np.max(np.abs(want))) + extra
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"{label}: max error {err:.3e} dB / bound {lim:.3e} dB = {err / lim:.3f}")
    assert err <= lim, (label, err, lim)
    return err / lim


def test_latency_of_the_shape():
    assert emspec.latency_columns(N, HOP, True) == D


# ---- batch: host and device entry ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("top", [TOP_DEFAULT, TOP_LOW], ids=["top0", "top-60"])
@pytest.mark.parametrize("columns", COLUMNS)
@pytest.mark.parametrize("sm,agc", SETTINGS)
def test_batch_against_binary64(engines, sm, agc, columns, top):
    """Column counts around the 4-way unroll (1, 2, 3, 5) and the chunk arithmetic (1023 .. 2049: one chunk, one chunk and a
    column, a warm-up that starts at column 0 / 512 / 1536), smoothing at its maximum, both clamps active."""
    import torch
    e = engines(top)
    pcm = _pcm(2, columns)
    raw = _raw(e, (top, 1024, 2, columns), pcm)
    want, gain = P.reference(raw, sm, agc, top)
    e.set_display(sm, agc)
    host = e.batch(pcm, N, HOP, True, want=("db",))["db"]
    _within(host, want, sm, agc, f"batch host sm={sm} agc={agc} C={columns} db_top={top}")
    dev = torch.empty((2, columns, 1024), dtype=torch.float32, device="cuda")
    e.batch_device(torch.from_numpy(pcm).cuda(), N, HOP, True, db=dev)
    torch.cuda.synchronize()
    _within(dev.cpu().numpy(), want, sm, agc, f"batch device sm={sm} agc={agc} C={columns} db_top={top}")
    if agc > 0.0:
        clamp = 40.0 if top == TOP_DEFAULT else -40.0
        at = gain == clamp
        assert at.any(), "the clamp is not active in any column"
        if sm == 0.0:   # nothing but the gain between raw and output: those columns are raw + clamp, one rounding
            beyond = np.where(at, np.abs(float(np.float32(agc)) * (top - P.level(raw))), 0.0)   # where it is clamped by the most
            s, c = np.unravel_index(np.argmax(beyond), beyond.shape)
            assert beyond[s, c] > 41.0
            assert np.max(np.abs(host[s, c].astype(np.float64) - (raw[s, c].astype(np.float64) + clamp))) <= P.U * np.max(np.abs(want))


@pytest.mark.parametrize("rows", [64, 1000, 4096])
def test_rows(engines, rows):
    """64 rows: 16 quads, 48 lanes of column_max_kernel's wave keep the seed; 1000: 250 quads, gid % qpc wraps inside a wave;
    4096.  1100 columns: two chunks."""
    e = engines(TOP_DEFAULT, rows)
    pcm = _pcm(2, 1100)
    raw = _raw(e, (TOP_DEFAULT, rows, 2, 1100), pcm)
    assert raw.shape == (2, 1100, rows)
    want, _ = P.reference(raw, 0.95, 1.0, TOP_DEFAULT)
    e.set_display(0.95, 1.0)
    _within(e.batch(pcm, N, HOP, True, want=("db",))["db"], want, 0.95, 1.0, f"rows={rows}")


@pytest.mark.parametrize("S", [1, 65])
def test_streams(engines, S):
    """agc_scan_kernel: one thread per stream, 64 per block - 65 streams are two blocks; every stream differs."""
    e = engines(TOP_DEFAULT, 64)
    pcm = _pcm(S, 300)
    assert len({pcm[s].tobytes() for s in range(S)}) == S
    raw = _raw(e, (TOP_DEFAULT, 64, S, 300), pcm)
    want, _ = P.reference(raw, 0.95, 1.0, TOP_DEFAULT)
    e.set_display(0.95, 1.0)
    got = e.batch(pcm, N, HOP, True, want=("db",))["db"]
    for s in range(S):
        assert np.max(np.abs(got[s].astype(np.float64) - want[s])) <= P.bound(0.95, 1.0, np.max(np.abs(want))), f"stream {s}"
    _within(got, want, 0.95, 1.0, f"S={S}")


def test_silence_beside_a_live_stream(engines):
    """Digital silence: the raw dB sits at the -200 dB floor, the column peak equals every cell, the gain is +40 throughout."""
    e = engines()
    columns = 300
    pcm = np.stack([np.zeros(_samples(columns), np.float32), _pcm(1, columns)[0]])
    raw = _raw(e, ("silence",), pcm)
    assert np.all(raw[0] == raw[0, 0, 0]) and abs(float(raw[0, 0, 0]) + 200.0) < 1e-4
    want, gain = P.reference(raw, 0.95, 1.0, TOP_DEFAULT)
    assert np.all(gain[0] == 40.0)
    e.set_display(0.95, 1.0)
    out = e.batch(pcm, N, HOP, True, want=("db", "index"))
    _within(out["db"], want, 0.95, 1.0, "silence")
    floor = float(raw[0, 0, 0]) + 40.0
    assert np.max(np.abs(out["db"][0].astype(np.float64) - floor)) <= P.bound(0.95, 1.0, np.max(np.abs(want)))
    # -160 dB is below the gate (-80 dB): palette index 0, as the restatement says
    assert np.all(out["index"][0] == 0)
    assert np.array_equal(out["index"][0], P.cell_index_f32(out["db"][0], TOP_DEFAULT))


@pytest.mark.parametrize("sm,agc", [(0.95, 1.0), (0.6, 0.8)])
def test_index_and_rgba_follow_the_returned_db(sm, agc, engine):
    columns = 1025
    pcm = _pcm(2, columns)
    lut = emspec.make_colormap(0.8)
    lut[:, 3] = np.arange(256, dtype=np.uint8)                   # every entry distinct, not the default ramp
    assert not np.array_equal(lut, O.default_lut()) and len({r.tobytes() for r in lut}) == 256
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_colormap(lut)
        e.set_display(sm, agc)
        out = e.batch(pcm, N, HOP, True, want=("db", "index", "rgba"))
        only_idx = e.batch(pcm, N, HOP, True, want=("index",))["index"]
        only_db = e.batch(pcm, N, HOP, True, want=("db",))["db"]
        only_rgba = e.batch(pcm, N, HOP, True, want=("rgba",))["rgba"]
    want_idx = P.cell_index_f32(out["db"], TOP_DEFAULT)
    differ = out["index"] != want_idx
    edge = P.index_borderline(out["db"], TOP_DEFAULT)
    print(f"sm={sm} agc={agc}: {int(differ.sum())} indices differ from the restatement, {float(edge.mean()):.2e} of the cells on a palette step")
    assert edge.mean() < 1e-3
    assert not np.any(differ & ~edge)
    assert np.all(np.abs(out["index"][differ].astype(np.int32) - want_idx[differ].astype(np.int32)) == 1)
    assert np.array_equal(out["rgba"], lut[out["index"]])
    assert np.array_equal(only_idx, out["index"])
    assert np.array_equal(only_db.view(np.uint32), out["db"].view(np.uint32))
    assert np.array_equal(only_rgba, out["rgba"])


def test_fast_mode_against_binary64(engine):
    """FAST mode, one case: the raw columns are the float32 bit model's within the project's 8.7e-4 dB; the output is a convex
    combination of raw cells plus a gain that moves by at most agc times that."""
    columns, sm, agc = 2049, 0.95, 1.0
    pcm = _pcm(2, columns)
    raw, _, _ = O.batch_f32(O.make_cfg(N, HOP, True), pcm, want=("db",))
    want, _ = P.reference(raw, sm, agc, TOP_DEFAULT)
    engine.reset()
    engine.set_display(sm, agc)
    try:
        got = engine.batch(pcm, N, HOP, True, want=("db",))["db"]
    finally:
        engine.set_display(0.0, 0.0)
    _within(got, want, sm, agc, "FAST C=2049", extra=2 * FAST_TOL_DB)


# ---- streaming -----------------------------------------------------------------------------------------------------------

LIVE_S, LIVE_C, LIVE_SET = 3, 640, (0.95, 1.0)


def _fed_for(columns):
    """Samples after which a stream has emitted `columns` columns."""
    return _samples(columns + D)


@pytest.fixture(scope="module")
def live(engines):
    e = engines()
    pcm = _pcm(LIVE_S, LIVE_C)
    raw = _raw(e, ("live",), pcm)
    want, gain = P.reference(raw, *LIVE_SET, TOP_DEFAULT)
    e.set_display(*LIVE_SET)
    batch = e.batch(pcm, N, HOP, True, want=("db",))["db"]
    e.set_display(0.0, 0.0)
    return dict(pcm=pcm, raw=raw, want=want, gain=gain, batch=batch, sessions={})


def _feed(e, pcm, start, stop, block, sinks, restarted=()):
    """Feeds samples [start, stop) of every stream in blocks; sinks[s]: the stream's columns so far, in emission order."""
    for a in range(start, stop, block):
        cnt = min(block, stop - a)
        db, _, counts, firsts = e.push_samples_multi(pcm, N, HOP, True, count=cnt, offset=a)
        for s in range(pcm.shape[0]):
            if counts[s]:
                assert firsts[s] == len(sinks[s])
            for i in range(int(counts[s])):
                sinks[s].append(db[s, i].copy())


def _flush(e, sinks):
    for _ in range(D):
        db, _, cols = e.columns_flush()
        for s in range(len(sinks)):
            assert cols[s] == len(sinks[s])
            sinks[s].append(db[s].copy())


def _push_session(pcm, block):
    sinks = [[] for _ in range(pcm.shape[0])]
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_display(*LIVE_SET)
        _feed(e, pcm, 0, pcm.shape[1], block, sinks)
        _flush(e, sinks)
    return np.stack([np.stack(c) for c in sinks])


def _hop_session(live):
    if "hop" not in live["sessions"]:
        live["sessions"]["hop"] = _push_session(live["pcm"], HOP)
    return live["sessions"]["hop"]


def _first_column_passes_through(got0, live):
    """y_0 = raw_0 + g_0: no smoothing towards anything (one rounding of the sum, one of the gain's product)."""
    x0 = live["raw"][:, 0].astype(np.float64) + live["gain"][:, 0, None]
    assert np.max(np.abs(got0.astype(np.float64) - x0)) <= 2 * P.U * np.max(np.abs(x0))


@pytest.mark.parametrize("block", [HOP, 1000], ids=["hop", "1000"])
def test_streaming_blocks_against_binary64(live, block):
    got = _hop_session(live) if block == HOP else _push_session(live["pcm"], block)
    assert got.shape == live["want"].shape
    _within(got, live["want"], *LIVE_SET, f"streaming, blocks of {block}")
    _first_column_passes_through(got[:, 0], live)


def test_streaming_per_frame_form_against_binary64(live):
    pcm = live["pcm"]
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        empty, _, cols = e.columns(pcm[:, :N], HOP, True)          # display off: the raw empty column
        assert np.all(cols == -1)
        empty = empty.copy()
        e.reset()
        e.set_display(*LIVE_SET)
        got = np.empty(live["want"].shape, np.float32)
        for j in range(LIVE_C):
            db, _, cols = e.columns(pcm[:, j * HOP:j * HOP + N], HOP, True)
            if j < D:   # the empty leading columns pass through raw and do not start the state
                assert np.all(cols == -1) and np.array_equal(db.view(np.uint32), empty.view(np.uint32))
            else:
                assert np.all(cols == j - D)
                got[:, j - D] = db
        for i in range(D):
            db, _, cols = e.columns_flush()
            assert np.all(cols == LIVE_C - D + i)
            got[:, LIVE_C - D + i] = db
    _within(got, live["want"], *LIVE_SET, "streaming, per-frame form")
    _first_column_passes_through(got[:, 0], live)


def test_batch_equals_streaming(live):
    got = _hop_session(live)
    lim = 2 * P.bound(*LIVE_SET, np.max(np.abs(live["want"])))
    err = float(np.max(np.abs(got.astype(np.float64) - live["batch"])))
    print(f"batch vs streaming: max difference {err:.3e} dB / (2 x bound) {lim:.3e} dB = {err / lim:.3f}")
    assert err <= lim
    _within(live["batch"], live["want"], *LIVE_SET, "batch on the streaming signal")


def test_streaming_state_reset_stream_reset_and_a_change_of_settings(live, engines):
    """One engine, in this order: emspec_reset_stream(1) after 200 columns (stream 1 restarts the law from its next column,
    streams 0 and 2 continue unbroken); emspec_reset and a new session of the same three streams (equal to a fresh engine's
    output: a stale d_pstate would show); emspec_set_display at column 300 of a session - the library accepts it, the state
    carries over and the columns from 300 on follow the new settings."""
    pcm, want = live["pcm"], live["want"]
    L = pcm.shape[1]
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        # 1. reset of one stream
        e.set_display(*LIVE_SET)
        sinks = [[] for _ in range(LIVE_S)]
        cut = _fed_for(200)
        _feed(e, pcm, 0, cut, HOP, sinks)
        assert [len(c) for c in sinks] == [200] * LIVE_S
        e.reset_stream(1)
        old1, sinks[1] = sinks[1], []
        _feed(e, pcm, cut, L, HOP, sinks)
        _flush(e, sinks)
        new_cols = emspec.num_columns(L - cut, N, HOP)
        assert [len(c) for c in sinks] == [LIVE_C, new_cols, LIVE_C]
        for s in (0, 2):
            _within(np.stack(sinks[s]), want[s], *LIVE_SET, f"stream {s} beside a reset stream")
        _within(np.stack(old1), want[1, :200], *LIVE_SET, "stream 1 before its reset")
        raw1 = _raw(engines(), ("live, stream 1 restarted",), np.ascontiguousarray(pcm[1:2, cut:]))
        want1, _ = P.reference(raw1, *LIVE_SET, TOP_DEFAULT)
        _within(np.stack(sinks[1]), want1[0], *LIVE_SET, "stream 1 after its reset")

        # 2. reset of the engine, then the same streams again: a fresh engine's bytes
        upto = _fed_for(150)
        fresh = [[] for _ in range(LIVE_S)]
        with emspec.Engine(mode=emspec.MODE_EXACT) as f:
            f.set_display(*LIVE_SET)
            _feed(f, pcm, 0, upto, HOP, fresh)
        e.reset()
        assert e.live_streams == 0
        again = [[] for _ in range(LIVE_S)]
        _feed(e, pcm, 0, upto, HOP, again)
        fresh, again = np.stack([np.stack(c) for c in fresh]), np.stack([np.stack(c) for c in again])
        assert again.shape == (LIVE_S, 150, 1024)
        assert np.array_equal(again.view(np.uint32), fresh.view(np.uint32))
        _within(again, want[:, :150], *LIVE_SET, "a new session after emspec_reset")

        # 3. other settings from column 300 on
        e.reset()
        e.set_display(*LIVE_SET)
        sinks = [[] for _ in range(LIVE_S)]
        _feed(e, pcm, 0, _fed_for(300), HOP, sinks)
        assert [len(c) for c in sinks] == [300] * LIVE_S
        e.set_display(0.6, 0.5)                                     # accepted mid-session
        _feed(e, pcm, _fed_for(300), _fed_for(450), HOP, sinks)
        got = np.stack([np.stack(c) for c in sinks])
        assert got.shape == (LIVE_S, 450, 1024)
        sm = np.where(np.arange(450) < 300, LIVE_SET[0], 0.6)
        agc = np.where(np.arange(450) < 300, LIVE_SET[1], 0.5)
        want2, _ = P.reference(live["raw"][:, :450], sm, agc, TOP_DEFAULT)
        _within(got, want2, sm, agc, "settings changed at column 300")
        assert np.array_equal(want2[:, :300], want[:, :300])
        # ... and it is the new law that is followed: the old one is far away by then
        assert np.max(np.abs(want2[:, 300:] - want[:, 300:450])) > 100 * P.bound(sm, agc, np.max(np.abs(want2)))
