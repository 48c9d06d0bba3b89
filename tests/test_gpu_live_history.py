"""GPU: the live history (include/emspec.h: emspec_set_live_history, emspec_live_history, emspec_history_view*; DESIGN.md
§3.14, §4.16): a ring on the device of the dB columns the streaming calls deliver, and views of it reduced in time and coloured.

The reference is the dB the calls themselves delivered, collected here column by column and fed to the numpy model
tests/history_ref.py (rings by slot; views = overview_ref.reduce_db of the stored columns, post_ref.cell_index_f32 of dB +
shift).  Everything is compared on bytes, in FAST and in EXACT mode: the history is a function of bytes the host holds.  Only
where two RUNS of a script are held against each other (test 5: a run that delivers no dB) does the FAST mode get the
run-to-run bound of tests/test_gpu_live_overlay.py - its dB is not the same from run to run, with or without a history.

Shapes: 64 rows (68 once; 128 / 192 where two / three bands need 64 rows each), FFT 1024 / hop 256, three streams whose levels
jump (post_ref.signals at a short hold), W = 5, sessions of 23 or more columns: the ring wraps several times."""
import numpy as np
import pytest

import emspec
import history_ref as H
import overview_ref as V
import post_ref as P

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
N, HOP, S, W, R = 1024, 256, 3, 5, 64
FRAMES = 27                                   # 25 columns with the flushes (D = 2)
MODES = pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
TOL_DB = 8.7e-4                               # the project's FAST-mode bound against the float32 bit model (tests/test_gpu_live.py)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """(tests/conftest.py: torch's HIP runtime is initialised before the first engine is created)"""
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()


def _engine(exact, rows=R, **kw):
    return emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST, rows=rows, **kw)


def _pcm(streams=S, frames=FRAMES, n=N, hop=HOP):
    return H.signal(streams, n + hop * (frames - 1))


def _same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


def _refused(code, call):
    with pytest.raises(emspec.EmspecError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


class Run:
    """One session with a history: feeds, keeps per stream every delivered column in order, feeds the model the same, and after
    every call holds emspec_live_history against the model's held range."""

    def __init__(self, e, streams=S, width=W, session="multi"):
        self.e, self.S, self.session = e, streams, session
        self.model = H.History(streams, width, e.rows)
        self.got = [[] for _ in range(streams)]          # delivered columns per stream

    def took(self, per_stream):
        """per_stream[s]: [count][rows] delivered to stream s by the call just made (None: the call delivered no dB)."""
        if per_stream is not None:
            self.model.launch(per_stream)
            for s, cols in enumerate(per_stream):
                self.got[s] += [c.copy() for c in np.asarray(cols, F).reshape(-1, self.e.rows)]
        for s in range(self.S):
            assert self.e.live_history(s, self.session) == self.model.held(s), (s, self.e.live_history(s, self.session), self.model.held(s))

    # ---- the feeding forms ----
    def push(self, pcm, a, cnt, feed=None, **kw):
        feed = feed or (lambda: self.e.push_samples_multi(pcm, N, HOP, True, count=cnt, offset=a, **kw))
        db, _, counts, firsts = feed()
        for s in range(self.S):
            assert counts[s] == 0 or firsts[s] == self.model.held(s)[0], "first_columns is the history's column number"
        self.took([db[s, :counts[s]] for s in range(self.S)])
        return counts

    def frame(self, pcm, j):
        db, _, cols = self.e.columns(pcm[:, j * HOP:j * HOP + N], HOP, True)
        self.took([db[s:s + 1] if cols[s] >= 0 else db[:0] for s in range(self.S)])

    def flush_all(self):
        while True:
            try:
                db, _, cols = self.e.columns_flush()
            except emspec.EmspecError as err:
                assert err.code == emspec.ERR_STATE
                return
            self.took([db[s:s + 1] if cols[s] >= 0 else db[:0] for s in range(self.S)])

    def delivered(self, s0=0, s1=None):
        """[streams][columns][rows] of streams [s0, s1) (equal counts)."""
        return np.stack([np.stack(g) for g in self.got[s0:s1]])

    def check_views(self, factors=(1,), stream0=0, streams=None):
        """Every valid first_column at every factor: the view's dB is reduce_db of the delivered columns, byte for byte."""
        n = self.S - stream0 if streams is None else streams
        ends = {self.model.held(s) for s in range(stream0, stream0 + n)}
        assert len(ends) == 1
        end, first = ends.pop()
        full = self.delivered(stream0, stream0 + n)
        assert full.shape[1] == end
        for f in factors:
            for a in range(first, end):
                groups = -(-(end - a) // f)
                got = self.e.history_view(a, f, groups, stream0, streams, session=self.session)["db"]
                assert _same(got, V.reduce_db(full[:, a:end], f)), (f, a, groups)
                assert _same(got, self.model.view(a, f, groups, stream0, streams)["db"]), (f, a, groups)


def _block_session(e, pcm, block=HOP, **kw):
    """Per-hop block form plus flush on the multi-stream session -> the Run."""
    r = Run(e, pcm.shape[0], **kw)
    for a in range(0, pcm.shape[1], block):
        r.push(pcm, a, min(block, pcm.shape[1] - a))
    r.flush_all()
    return r


# ---- 1. every feeding form: the held range after every call, and the f = 1 view of what is held ----
@MODES
@pytest.mark.parametrize("form", ["block", "frame", "one"])
def test_held_range_and_the_last_columns(exact, form):
    pcm = _pcm()
    with _engine(exact) as e:
        assert e.live_history(0) is None                   # no history
        e.set_live_history(W)
        assert e.live_history(0) is None and e.live_history(0, "one") is None   # a session that has not started has no streams
        if form == "block":
            r = _block_session(e, pcm)
        elif form == "frame":
            r = Run(e)
            for j in range(FRAMES):
                r.frame(pcm, j)
            r.flush_all()
        else:
            r = Run(e, 1, session="one")
            for j in range(FRAMES):
                db, col = e.column(pcm[0, j * HOP:j * HOP + N], HOP, True)
                r.took([db[None] if col >= 0 else db[None][:0]])
            for _ in range(2):
                db, col = e.flush()
                assert col >= 0
                r.took([db[None]])
            assert e.live_history(0, "multi") is None and e.live_history(1, "one") is None
        for s in range(r.S):
            assert r.model.held(s) == (FRAMES, FRAMES - W)
        got = e.history_view(FRAMES - W, 1, W, session=r.session)["db"]
        assert _same(got, r.delivered()[:, -W:])
        r.check_views()
        e.reset()                                           # empties every ring
        assert e.live_history(0, r.session) is None
        _refused(emspec.ERR_STATE, lambda: e.history_view(0, 1, 1, session=r.session))


# ---- 2. factors, from every valid first column, and a sub-range of streams ----
@MODES
@pytest.mark.parametrize("rows", [64, 68])
def test_factors_from_every_first_column(exact, rows):
    pcm = _pcm()
    with _engine(exact, rows=rows) as e:
        e.set_live_history(W)
        r = _block_session(e, pcm, block=3 * HOP + 17)
        r.check_views(factors=(1, 2, 3, 5, 7))
        r.check_views(factors=(1, 2, 3, 5, 7), stream0=1, streams=2)
        r.check_views(factors=(2,), stream0=2, streams=1)
        # pinned outputs are written in place
        pin = emspec.PinnedArray((S, 2, rows), F)
        try:
            e.history_view(FRAMES - W, 3, 2, db=pin.array, want=())
            assert _same(pin.array, V.reduce_db(r.delivered()[:, -W:], 3))
        finally:
            pin.close()


# ---- 3. more columns than W in one launch, unequal counts, reset_stream ----
@MODES
def test_long_push_unequal_counts_and_reset_stream(exact):
    pcm = _pcm(frames=60)
    with _engine(exact) as e:
        e.set_live_history(W)
        r = Run(e)
        first = N + HOP * 13                               # 14 frames = 12 columns in one launch, into W = 5
        assert e.push_columns_multi(first, N, HOP, True) == 12
        assert list(r.push(pcm, 0, first)) == [12] * S
        assert r.model.held(0) == (12, 7)
        r.check_views(factors=(1, 2))
        r.push(pcm, first, 3 * HOP)
        e.reset_stream(1)                                   # empties stream 1 only, restarts its numbering
        r.model.reset_stream(1)
        r.got[1] = []
        r.took(None)
        assert e.live_history(1) == (0, 0) and e.live_history(0) == (15, 10)
        msg = _refused(emspec.ERR_INVALID_ARG, lambda: e.history_view(10, 1, 1))
        assert "stream 1" in msg and "[0, 0)" in msg, msg
        _refused(emspec.ERR_INVALID_ARG, lambda: e.history_view(0, 1, 1, stream0=1, streams=1))
        r.check_views(stream0=0, streams=1)
        r.check_views(stream0=2, streams=1)
        a = first + 3 * HOP
        counts = r.push(pcm, a, N + 6 * HOP)               # streams 0 and 2: 10 columns, stream 1 (restarted): 5
        assert list(counts) == [10, 5, 10]
        assert [r.model.held(s) for s in range(S)] == [(25, 20), (5, 0), (25, 20)]
        for s in range(S):
            r.check_views(factors=(1, 3), stream0=s, streams=1)
        _refused(emspec.ERR_INVALID_ARG, lambda: e.history_view(20, 1, 1))      # stream 1 holds [0, 5)
        counts = r.push(pcm, a + N + 6 * HOP, 20 * HOP)    # 20 more columns each: stream 1 wraps too, at its own numbers
        assert list(counts) == [20, 20, 20]
        for s in range(S):
            r.check_views(factors=(1, 2), stream0=s, streams=1)


# ---- 4. colour ----
@MODES
def test_colour_law_of_a_view(exact):
    """index = cell_index_f32(dB + shift) under a map that differs from the configuration in all four fields - exactly, outside
    the cells post_ref.index_borderline excuses (within one step there; at most 1e-3 of the cells: tests/test_history_cpu.py
    shows the reference's own share on this signal is below that) - and rgba = LUT[index] exactly, with an uploaded colour map."""
    pcm = _pcm()
    lut = H.colour_map()
    with _engine(exact) as e:
        e.set_colormap(lut)
        e.set_live_history(32)
        r = _block_session(e, pcm, width=32)
        cfgmap = (e.cfg.db_top, e.cfg.db_range, e.cfg.gate_db, 0.0)
        assert all(a != b for a, b in zip(H.VIEW_MAP, cfgmap))
        excused = cells = 0
        for m, law in ((H.VIEW_MAP, H.VIEW_MAP), (None, cfgmap), (emspec.ViewMap(*H.VIEW_MAP), H.VIEW_MAP)):
            for f, groups in ((1, FRAMES), (3, 9), (FRAMES, 1)):
                got = e.history_view(0, f, groups, map=m, want=("db", "index", "rgba"))
                want = r.model.view(0, f, groups, map=law, lut=lut)
                assert _same(got["db"], want["db"])                      # the dB output is not shifted
                border = P.index_borderline(want["shifted"], *law[:3])
                diff = got["index"].astype(int) - want["index"].astype(int)
                assert np.all(diff[~border] == 0) and np.all(np.abs(diff) <= 1), (f, int(np.abs(diff).max()))
                assert np.array_equal(got["rgba"], lut[got["index"]])
                excused += int(np.count_nonzero(diff))
                cells += diff.size
                only = e.history_view(0, f, groups, map=m, want=("rgba",))
                assert only["db"] is None and np.array_equal(only["rgba"], got["rgba"])
        print("cells", cells, "excused", excused)
        assert excused <= 1e-3 * cells, (excused, cells)
        assert len(np.unique(got["index"])) > 8                         # (the law is exercised: not one colour)


# ---- 5. where the delivered dB comes from ----
def _overlay_run(exact, post, peaks, kind, history):
    """Per-hop block pushes + flushes; kind: "pinned" | "pageable" | "none" (out_db = NULL).  -> (delivered dB or None,
    the peaks of every column [S][columns][k][2] or None, the last W columns through the history or None)."""
    pcm = _pcm()
    k = 4
    keep = []

    def alloc(shape):
        if kind == "pinned":
            keep.append(emspec.PinnedArray(shape, F))
            return keep[-1].array
        return np.empty(shape, F)
    with _engine(exact) as e:
        if post:
            e.set_display(0.5, 0.6)
        if history:
            e.set_live_history(W)
        pk = alloc((S, 1, k, 2)) if peaks else None
        if peaks:
            e.set_live_peaks(k, -70.0, pk)
        dbbuf = alloc((S, 1, R)) if kind != "none" else None
        cols, pks, views = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]

        def took(db, counts):
            for s in range(S):
                for i in range(int(counts[s])):
                    if db is not None:
                        cols[s].append(db[s, i].copy())
                    if peaks:
                        pks[s].append(pk[s, i].copy())
                    if history:       # the newest column through the ring, after every call
                        end = e.live_history(s)[0]
                        views[s].append(e.history_view(end - 1, 1, 1, stream0=s, streams=1)["db"][0, 0])
        for a in range(0, pcm.shape[1], HOP):
            db, _, counts, _ = e.push_samples_multi(pcm, N, HOP, True, count=HOP, offset=a, db=dbbuf, want_db=kind != "none")
            assert db is dbbuf
            took(db, counts)
        for _ in range(2):
            if kind == "none":
                db, _, c = e.columns_flush(want_db=False)
            else:
                db, _, c = e.columns_flush(db=dbbuf[:, 0])
                db = db[:, None]
            took(db, (c >= 0).astype(int))              # (the flush writes pk[s][0] like a one-column call)
        if history:
            assert e.live_history(0) == (FRAMES, FRAMES - W)
        e.set_live_peaks(1, 0.0, None)
        out = (np.array(cols) if kind != "none" else None, np.array(pks) if peaks else None, np.array(views) if history else None)
    for p in keep:
        p.close()
    return out


@MODES
@pytest.mark.parametrize("post", [False, True], ids=["raw", "post"])
@pytest.mark.parametrize("peaks", [False, True], ids=["nopeaks", "peaks"])
def test_every_source_of_the_delivered_db(exact, post, peaks):
    """Display post-process on / off x live peaks on / off: the four places the delivered dB comes from.  For page-locked
    outputs, pageable outputs and out_db = NULL: every column read back through the ring right after its call is the column
    the call delivered, byte for byte; the peaks are emspec.peaks_host of that column with and without a history.  Across runs
    (a run without out_db has nothing delivered to compare with; peaks with a history against peaks without): EXACT is
    reproducible, so the bytes are equal; FAST differs from run to run by up to 2 TOL_DB raw and 4 TOL_DB with the display
    (tests/test_gpu_live_overlay.py: _same_run), with or without a history, and gets that bound."""
    runs = {kind: _overlay_run(exact, post, peaks, kind, True) for kind in ("pinned", "pageable", "none")}
    plain = _overlay_run(exact, post, peaks, "pageable", False)
    for kind, (db, pk, view) in runs.items():
        assert view.shape == (S, FRAMES, R)
        if db is not None:
            assert _same(view, db), kind
        if peaks:
            assert _same(pk, emspec.peaks_host(view, 4, -70.0)), kind
    ref = runs["pageable"][2]
    bound = (4 if post else 2) * TOL_DB
    for kind, (db, pk, view) in runs.items():
        err = float(np.max(np.abs(view - ref)))
        print(kind, "max |dB difference| to the pageable run:", err)
        assert _same(view, ref) if exact else err <= bound, (kind, err)
    err = float(np.max(np.abs(plain[0] - ref)))
    assert _same(plain[0], ref) if exact else err <= bound, err            # a history changes no delivered byte
    if peaks and exact:
        for kind in runs:
            assert _same(runs[kind][1], plain[1]), kind                     # peaks_out unchanged from a run without history


# ---- 6. the other session types ----
def _generic_session(e, streams, feed, total, block):
    r = Run(e, streams)
    for a in range(0, total, block):
        cnt = min(block, total - a)
        r.push(None, a, cnt, feed=lambda: feed(cnt, a))
    r.flush_all()
    return r


@MODES
def test_multires_session(exact):
    """The multi-resolution entry at its smallest accepted shape (n_low is 8192 or 16384: 8192 / 1024, hop 256)."""
    n_low, n_high, rows, split = 8192, 1024, 128, 64
    frames = 23 + 2 * emspec.latency_columns(n_low, HOP, True)
    pcm = _pcm(frames=frames, n=n_low)
    with _engine(exact, rows=rows) as e:
        e.set_live_history(W)
        r = _generic_session(e, S, lambda cnt, a: e.push_samples_multires(pcm, n_low, n_high, HOP, split, True, count=cnt, offset=a),
                             pcm.shape[1], 9 * HOP + 3)
        assert r.model.held(0)[0] == frames >= 23
        r.check_views(factors=(1, 3))


@MODES
def test_two_band_session_4096_1024(exact):
    """Two bands, 4096 below row 64 and 1024 above, hop 256: the two-band live session at sizes the multi-resolution entry itself
    does not take, through the band entry with K = 2 (include/emspec.h: its columns are the two-band session's)."""
    n, rows, split = (4096, 1024), 128, (64,)
    frames = 23 + 2 * emspec.latency_columns(n[0], HOP, True)
    pcm = _pcm(frames=frames, n=n[0])
    with _engine(exact, rows=rows) as e:
        e.set_live_history(W)
        r = _generic_session(e, S, lambda cnt, a: e.push_samples_multiband(pcm, n, split, HOP, True, count=cnt, offset=a),
                             pcm.shape[1], 5 * HOP + 3)
        assert r.model.held(0)[0] == frames >= 23
        r.check_views(factors=(1, 3))


@MODES
def test_multiband_session(exact):
    n, rows, split = (4096, 2048, 1024), 192, (64, 128)
    frames = 23 + 2 * emspec.latency_columns(n[0], HOP, True)
    pcm = _pcm(frames=frames, n=n[0])
    with _engine(exact, rows=rows) as e:
        e.set_live_history(W)
        r = _generic_session(e, S, lambda cnt, a: e.push_samples_multiband(pcm, n, split, HOP, True, count=cnt, offset=a),
                             pcm.shape[1], 4 * HOP + 1)
        assert r.model.held(0)[0] == frames
        r.check_views(factors=(1, 2))


@MODES
def test_pcm_session(exact):
    """S16 stereo -> L R M S: the history holds the decoded views' columns."""
    total = N + HOP * (FRAMES - 1)
    x = _pcm(2, FRAMES)
    raw = np.round(np.stack([x[0], x[1]], -1).reshape(1, -1) * 32767).astype("<i2")
    fmt = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
    with _engine(exact) as e:
        e.set_live_history(W)
        r = _generic_session(e, 4, lambda cnt, a: e.push_samples_pcm(raw, fmt, N, HOP, True, count=cnt, offset=a), total, 2 * HOP + 5)
        assert e.live_streams == 4 and r.model.held(3) == (FRAMES, FRAMES - W)
        r.check_views(factors=(1, 3))
        r.check_views(factors=(2,), stream0=2, streams=2)


# ---- 7. refusals, each followed by a successful call on the same engine ----
def test_refusals_leave_the_engine_usable():
    pcm = _pcm()
    with _engine(True) as e:
        ok = lambda: e.history_view(e.live_history(0)[1], 1, 1)["db"]
        _refused(emspec.ERR_STATE, lambda: e.history_view(0, 1, 1))                 # a view without a history
        _refused(emspec.ERR_INVALID_ARG, lambda: e.set_live_history(-1))
        _refused(emspec.ERR_INVALID_ARG, lambda: e.set_live_history((1 << 20) + 1))
        e.set_live_history(1 << 20)                                                  # the largest W is accepted (nothing allocated yet)
        e.set_live_history(W)
        _refused(emspec.ERR_STATE, lambda: e.history_view(0, 1, 1))                 # a session that does not exist
        _refused(emspec.ERR_STATE, lambda: e.history_view(0, 1, 1, session="one", streams=1))
        r = Run(e)
        r.push(pcm, 0, N + 8 * HOP)                                                  # 7 columns: holds [2, 7)
        assert e.live_history(0) == (7, 2)
        for call in (lambda: e.history_view(1, 1, 1), lambda: e.history_view(7, 1, 1), lambda: e.history_view(2, 1, 6),
                     lambda: e.history_view(2, 2, 4), lambda: e.history_view(-1, 1, 1)):
            msg = _refused(emspec.ERR_INVALID_ARG, call)
            assert "stream 0" in msg and "[2, 7)" in msg, msg
            assert _same(ok(), r.delivered()[:, 2:3])
        for call in (lambda: e.history_view(2, 0, 1), lambda: e.history_view(2, 65537, 1), lambda: e.history_view(2, 1, 0),
                     lambda: e.history_view(2, 1, 1, streams=0), lambda: e.history_view(2, 1, 1, stream0=2, streams=2),
                     lambda: e.history_view(2, 1, 1, stream0=-1, streams=1), lambda: e.history_view(2, 1, 1, want=()),
                     lambda: e.history_view(2, 1, 1, map=(0.0, 0.0, -80.0, 0.0))):
            _refused(emspec.ERR_INVALID_ARG, call)
            assert _same(ok(), r.delivered()[:, 2:3])
        assert _same(e.history_view(2, 65536, 1)["db"], V.reduce_db(r.delivered()[:, 2:], 65536))
        _refused(emspec.ERR_STATE, lambda: e.set_live_history(W))                   # set while frames are fed
        _refused(emspec.ERR_STATE, lambda: e.set_live_history(9))
        assert _same(ok(), r.delivered()[:, 2:3])
        # a push that does not fit max_columns is refused before anything is fed, like one with an output
        before = e.live_history(0)
        _refused(emspec.ERR_INVALID_ARG, lambda: e.push_samples_multi(pcm, N, HOP, True, want_db=False, count=2 * HOP, offset=N + 8 * HOP,
                                                                      db=None, rgba=np.empty((S, 1, R, 4), np.uint8)))
        lib, h = e._lib, e._h
        assert lib.emspec_push_samples_multi(h, pcm.ctypes.data + 4 * (N + 8 * HOP), S, 2 * HOP, pcm.shape[1], N, HOP, 1, None, None, R, 0,
                                             None, None) == emspec.ERR_INVALID_ARG      # no output at all: still refused
        assert e.live_history(0) == before
        r.push(pcm, N + 8 * HOP, 2 * HOP)
        assert e.live_history(0) == (9, 4)
        r.check_views(factors=(1, 2))
        e.set_live_history(0)                                                        # clearing is always allowed; frees the rings
        assert e.live_history(0) is None
        _refused(emspec.ERR_STATE, lambda: e.history_view(4, 1, 1))
        db, _, counts, _ = e.push_samples_multi(pcm, N, HOP, True, count=HOP, offset=N + 10 * HOP)   # the session goes on without it
        assert list(counts) == [1] * S
        e.reset()
        e.set_live_history(3)
        r = Run(e, width=3)
        r.push(pcm, 0, N + 5 * HOP)
        r.check_views()
    # a time reduction stays refused by the streaming calls, with or without a history
    with _engine(False) as e:
        e.set_live_history(W)
        e.set_time_reduce(4)
        _refused(emspec.ERR_STATE, lambda: e.push_samples_multi(pcm, N, HOP, True))
        e.set_time_reduce(1)
        r = Run(e)
        r.push(pcm, 0, N + 4 * HOP)
        r.check_views()


# ---- 8. the device entry ----
@MODES
def test_device_entry_gives_the_host_entrys_bytes(exact):
    import torch
    pcm = _pcm()
    lut = H.colour_map()
    with _engine(exact) as e:
        e.set_colormap(lut)
        e.set_live_history(16)
        r = _block_session(e, pcm, width=16)
        st = torch.cuda.Stream()
        for f, first, groups in ((1, FRAMES - 16, 16), (3, FRAMES - 16, 6), (16, FRAMES - 16, 1), (2, FRAMES - 3, 2)):
            host = e.history_view(first, f, groups, map=H.VIEW_MAP, want=("db", "index", "rgba"))
            db = torch.full((S, groups, R), 7.0, dtype=torch.float32, device="cuda")
            idx = torch.full((S, groups, R), 9, dtype=torch.uint8, device="cuda")
            rgba = torch.full((S, groups, R, 4), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            e.history_view_device(first, f, groups, map=H.VIEW_MAP, db=db, index=idx, rgba=rgba, stream=st)
            st.synchronize()
            assert _same(db.cpu().numpy(), host["db"]) and np.array_equal(idx.cpu().numpy(), host["index"])
            assert np.array_equal(rgba.cpu().numpy(), host["rgba"])
            assert _same(host["db"], r.model.view(first, f, groups)["db"])
        # a sub-range of streams, the index alone, on the current stream
        idx = torch.empty((2, 4, R), dtype=torch.uint8, device="cuda")
        e.history_view_device(FRAMES - 4, 1, 4, stream0=1, streams=2, index=idx)
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy(), e.history_view(FRAMES - 4, 1, 4, stream0=1, streams=2, want=("index",))["index"])
        _refused(emspec.ERR_INVALID_ARG, lambda: e.history_view_device(0, 1, 1, db=torch.empty((S, 1, R), device="cuda")))


# ---- the split-group path: one wide group per stream ----
@MODES
def test_one_wide_group_is_cut_over_waves_without_changing_a_byte(exact):
    """One group of all W = 96 held columns per stream - too few threads to fill the device, so the group's columns are cut over
    the waves of a workgroup - gives the bytes of the unsplit definition (the model), from a first column past the wrap too."""
    frames = 130
    pcm = _pcm(frames=frames)
    with _engine(exact) as e:
        e.set_live_history(96)
        r = _block_session(e, pcm, block=16 * HOP, width=96)
        end, first = r.model.held(0)
        assert (end, first) == (frames, frames - 96)
        for a, f in ((first, 96), (first + 1, 95), (first + 30, 66), (first, 48), (first + 5, 33)):
            groups = -(-(end - a) // f)
            got = e.history_view(a, f, groups, map=H.VIEW_MAP, want=("db", "index"))
            want = r.model.view(a, f, groups, map=H.VIEW_MAP)
            assert _same(got["db"], want["db"]), (a, f)
            assert _same(got["db"], V.reduce_db(r.delivered()[:, a:end], f)), (a, f)
            assert np.max(np.abs(got["index"].astype(int) - want["index"].astype(int))) <= 1
