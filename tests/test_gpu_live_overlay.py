"""GPU: the overlays of the live calls (include/emspec.h: emspec_set_live_peaks, emspec_set_live_wave): beside
every column a streaming call delivers, its spectral peaks and the envelope pair of the samples under it.

References, all on bytes: the peaks are emspec.peaks_host (tests/peaks_ref.py on a sample of them) of the dB the SAME call
delivered; the envelope is emspec.wave_host (tests/wave_ref.py on one session) of the samples fed.  Neither has a tolerance:
both overlays are functions of bits the host holds, in FAST and in EXACT mode.  Only where two RUNS of a script are held
against each other (overlays set against cleared) does the FAST mode get the bound of _same_run: its dB is not the same from
run to run, with or without overlays."""
import numpy as np
import pytest

import emspec
import peaks_ref as P
import pcm_ref
import wave_ref as W
import worst_signals as WS
from emspec import synth

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
MIN_DB = -60.0
EMPTY_PAIR = np.array([np.inf, -np.inf], F).view(U)
MODES = pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])


def _engine(exact, **kw):
    return emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST, **kw)


def _same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


TOL_DB = 8.7e-4   # the project's FAST-mode bound against the float32 bit model (tests/test_gpu_live.py)


def _same_run(a, b, exact, what, terms=2):
    """Two runs of the same script.  EXACT: the same bytes.  FAST: a launch's float adds arrive in any order, so two runs differ
    with or without overlays; each raw dB is within TOL_DB of the bit model, hence two runs within 2 TOL_DB (terms = 2).  With the
    display on (terms = 4): the smoothing is a convex combination and does not widen that, the gain follows the column peaks
    with a strength <= 1 and adds at most another 2 TOL_DB."""
    a, b = np.array(a), np.array(b)
    assert a.shape == b.shape, what
    if a.dtype == np.uint8:
        frac = float(np.mean(a != b)) if a.size else 0.0
        print(what, "rgba bytes that differ:", frac)
        assert frac == 0.0 if exact else frac < 1e-3, (what, frac)
        return
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    print(what, "max |dB difference| between runs:", err, "byte-equal:", _same(a, b))
    assert _same(a, b) if exact else err <= terms * TOL_DB, (what, err)


class Session:
    """One engine session with both overlays on: feeds, and keeps per stream what every call delivered, column by column."""
    FILL = 7.0

    def __init__(self, e, S, k, pairs, min_db=MIN_DB, pinned=False, peaks=True, wave=True, want_db=True, want_rgba=False,
                 single=False):
        self.e, self.S, self.k, self.single = e, S, k, single
        self.want_db, self.want_rgba = want_db, want_rgba
        self.pinned = pinned
        self.keep = []
        self.pk = self.wv = None
        if peaks:
            self.pk = self._alloc(pairs * k * 2)
            e.set_live_peaks(k, min_db, self.pk)
        if wave:
            self.wv = self._alloc(pairs * 2)
            e.set_live_wave(self.wv)
        self.rec = [dict(col=[], db=[], rgba=[], pk=[], wv=[]) for _ in range(S)]
        # page-locked dB for the push calls too: with every output page-locked the kernels write the caller's blocks in place
        self.dbbuf = self._alloc(pairs * e.rows) if pinned and want_db and not single else None

    def _alloc(self, count):
        if self.pinned:
            self.keep.append(emspec.PinnedArray((count,), F))
            a = self.keep[-1].array
        else:
            a = np.empty(count, F)
        a[:] = self.FILL
        return a

    def close(self):
        self.e.set_live_peaks(1, 0.0, None)
        self.e.set_live_wave(None)
        for p in self.keep:
            p.close()

    def _take(self, cols, counts, firsts, db, rgba):
        """After a call that delivered [S][cols]: the written slots of every stream; the others must be untouched."""
        S, k = self.S, self.k
        pk = self.pk[:S * cols * k * 2].reshape(S, cols, k, 2) if self.pk is not None else None
        wv = self.wv[:S * cols * 2].reshape(S, cols, 2) if self.wv is not None else None
        for s in range(S):
            for i in range(int(counts[s])):
                r = self.rec[s]
                r["col"].append(int(firsts[s]) + i if firsts[s] >= 0 else -1)
                if db is not None:
                    r["db"].append(db[s, i].copy())
                if rgba is not None:
                    r["rgba"].append(rgba[s, i].copy())
                if pk is not None:
                    r["pk"].append(pk[s, i].copy())
                if wv is not None:
                    r["wv"].append(wv[s, i].copy())
            for a in (pk, wv):
                if a is not None:
                    assert np.all(a[s, int(counts[s]):] == self.FILL), "a slot the call did not write was touched"
                    a[s] = self.FILL

    # ---- the calls ----
    def frame(self, frames, hop, reassign, n_high=0, split=0):
        if self.single:
            out = self.e.column(frames[0], hop, reassign, want_rgba=self.want_rgba)
            db, rgba, cols = out[0][None, None], (out[1][None, None] if self.want_rgba else None), np.array([out[-1]])
        else:
            kw = dict(want_db=self.want_db, want_rgba=self.want_rgba)
            db, rgba, cols = self.e.columns_multires(frames, n_high, hop, split, reassign, **kw) if n_high else \
                self.e.columns(frames, hop, reassign, **kw)
            db, rgba = (db[:, None] if db is not None else None), (rgba[:, None] if rgba is not None else None)
        self._take(1, np.ones(self.S, int), cols, db, rgba)     # (the per-frame form always writes its slot: column -1 is the empty one)
        return cols

    def flush(self):
        if self.single:
            out = self.e.flush(want_rgba=self.want_rgba)
            db, rgba, cols = out[0][None, None], (out[1][None, None] if self.want_rgba else None), np.array([out[-1]])
        else:
            db, rgba, cols = self.e.columns_flush(want_db=self.want_db, want_rgba=self.want_rgba)
            db, rgba = (db[:, None] if db is not None else None), (rgba[:, None] if rgba is not None else None)
        self._take(1, np.ones(self.S, int), cols, db, rgba)
        return cols

    def push(self, pcm, a, cnt, n, hop, reassign, n_high=0, split=0):
        if self.single:
            out = self.e.push_samples(pcm[0, a:a + cnt], n, hop, reassign, want_rgba=self.want_rgba)
            db, rgba = out[0][None], (out[1][None] if self.want_rgba else None)
            counts, firsts = np.array([db.shape[1]]), np.array([out[-1]])
        elif n_high:
            db, rgba, counts, firsts = self.e.push_samples_multires(pcm, n, n_high, hop, split, reassign, want_db=self.want_db,
                                                                    want_rgba=self.want_rgba, count=cnt, offset=a)
        else:
            db = None
            if self.dbbuf is not None:
                kc = self.e.push_columns_multi(cnt, n, hop, reassign)
                db = self.dbbuf[:self.S * kc * self.e.rows].reshape(self.S, kc, self.e.rows)
            db, rgba, counts, firsts = self.e.push_samples_multi(pcm, n, hop, reassign, want_db=self.want_db, want_rgba=self.want_rgba,
                                                                 db=db, count=cnt, offset=a)
        cols = (db if db is not None else rgba).shape[1] if (db is not None or rgba is not None) else int(max(counts))
        self._take(cols, counts, firsts, db, rgba)
        return counts

    def flush_all(self):
        while True:
            try:
                self.flush()
            except emspec.EmspecError as ex:
                assert ex.code == emspec.ERR_STATE
                return

    # ---- what was delivered ----
    def emitted(self, s, key):
        """Stream s's real columns (not the empty ones), in order."""
        r = self.rec[s]
        return np.array([v for c, v in zip(r["col"], r[key]) if c >= 0])

    def check_peaks(self, ref_sample=4):
        for s in range(self.S):
            r = self.rec[s]
            if not r["db"]:
                continue
            db, pk = np.array(r["db"]), np.array(r["pk"])
            assert _same(pk, emspec.peaks_host(db, self.k, MIN_DB)), ("peaks differ from peaks_host of the delivered dB", s)
            idx = np.linspace(0, len(db) - 1, min(ref_sample, len(db))).astype(int)
            assert _same(pk[idx], P.peaks(db[idx], self.k, MIN_DB)), s

    def check_wave(self, fed, n, hop):
        """fed: [S][L] what every stream was fed (since its last reset); the session is flushed."""
        want = emspec.wave_host(fed, n, hop)
        for s in range(self.S):
            r = self.rec[s]
            cols = [c for c in r["col"] if c >= 0]
            assert cols == list(range(want.shape[1])), (s, cols[:5], want.shape)
            assert _same(self.emitted(s, "wv"), want[s]), ("envelope differs from wave_host", s)
            for c, v in zip(r["col"], r["wv"]):
                if c < 0:
                    assert np.array_equal(v.view(U), EMPTY_PAIR), "the empty column's pair is (+inf, -inf)"


def _frames(pcm, j, n, hop):
    return np.ascontiguousarray(pcm[:, j * hop:j * hop + n])


def _run_frames(t, pcm, n, hop, reassign, frames, **kw):
    for j in range(frames):
        t.frame(_frames(pcm, j, n, hop), hop, reassign, **kw)
    t.flush_all()


def _run_blocks(t, pcm, n, hop, reassign, blocks, **kw):
    a = 0
    for b in blocks:
        t.push(pcm, a, b, n, hop, reassign, **kw)
        a += b
    assert a == pcm.shape[1]
    t.flush_all()


def _blocks(total, size):
    return [size] * (total // size) + ([total % size] if total % size else [])


# ---- 1. per-frame form ----
@MODES
@pytest.mark.parametrize("rows", [64, 260, 1024, 4096])
def test_per_frame_form(exact, rows):
    """n = 1024 / hop 256, reassign on and off, S = 3, 12 frames and the flush; k = 1, 8, 32.  rows = 260: a partial 65th quad;
    4096: 16 quads per lane.  The empty columns' peaks and (+inf, -inf) pairs are part of every comparison."""
    S, n, hop, frames = 3, 1024, 256, 12
    pcm = synth.streams(S, n + hop * (frames - 1))
    with _engine(exact, rows=rows) as e:
        for reassign in (True, False):
            for k in (1, 8, 32):
                e.reset()
                t = Session(e, S, k, S)
                _run_frames(t, pcm, n, hop, reassign, frames)
                D = emspec.latency_columns(n, hop, reassign)
                assert [c for c in t.rec[0]["col"]] == [-1] * D + list(range(frames))
                t.check_peaks()
                t.check_wave(pcm, n, hop)
                assert any(p[0, 0] >= 0 for p in t.rec[0]["pk"]) and all(np.all(p[:, 0] == -1) for p in t.rec[0]["pk"][:D])
                t.close()
    if rows == 1024 and exact:
        assert W.same(W.envelope(pcm, n, hop), emspec.wave_host(pcm, n, hop))


# ---- 2. block form ----
@MODES
def test_block_form(exact):
    """n = 4096 / hop 256, S = 4: blocks of 128 (no launch for most), 256, 20000 (several rounds and the deferred finalize) and an
    irregular list; pinned and pageable overlay arrays give the same bytes; one 60000-sample block and the same hop by hop."""
    S, n, hop, L, k = 4, 4096, 256, 60000, 8
    pcm = synth.streams(S, L)
    short = np.ascontiguousarray(pcm[:, :24000])
    irregular = [1, 127, 300, 5000, 4096, 77, 256, 257, 9000, 2886, 2000]
    assert sum(irregular) == short.shape[1]
    got = {}
    with _engine(exact) as e:
        for name, sig, blocks, pinned in (("128", short, _blocks(24000, 128), False), ("256", short, _blocks(24000, 256), True),
                                          ("20000", short, [20000, 4000], False), ("20000p", short, [20000, 4000], True),
                                          ("irregular", short, irregular, False), ("one", pcm, [L], False), ("hops", pcm, _blocks(L, hop), True)):
            e.reset()
            t = Session(e, S, k, S * 256, pinned=pinned)
            _run_blocks(t, sig, n, hop, True, blocks)
            t.check_peaks()
            t.check_wave(sig, n, hop)
            got[name] = [(t.emitted(s, "db"), t.emitted(s, "pk"), t.emitted(s, "wv")) for s in range(S)]
            t.close()
    for a, b in (("20000", "20000p"), ("one", "hops"), ("128", "irregular"), ("256", "irregular")):
        for s in range(S):
            assert _same(got[a][s][2], got[b][s][2]), (a, b, s)
            if exact:   # (FAST: the dB itself depends on the arrival order of a launch's float adds; its peaks are checked above)
                assert _same(got[a][s][0], got[b][s][0]) and _same(got[a][s][1], got[b][s][1]), (a, b, s)


# ---- 3. staggered streams and a reset ----
@MODES
@pytest.mark.parametrize("form", ["frames", "blocks"])
def test_reset_of_one_stream(exact, form):
    """S = 5; stream 2 is reset after `cut` samples and fed another signal from its start: its envelope restarts as wave_host of
    what it was fed afterwards; the other streams' overlays are those of the uninterrupted streams."""
    S, n, hop, k = 5, 1024, 256, 8
    frames, cutf = 30, 11
    L = n + hop * (frames - 1)
    pcm = synth.streams(S, L)
    other = synth.streams(7, L)[6:7]
    with _engine(exact) as e:
        t = Session(e, S, k, S * 64)
        if form == "frames":
            for j in range(frames):
                if j == cutf:
                    e.reset_stream(2)
                    before = {key: list(v) for key, v in t.rec[2].items()}
                    t.rec[2] = dict(col=[], db=[], rgba=[], pk=[], wv=[])
                fr = _frames(pcm, j, n, hop)
                if j >= cutf:
                    fr[2] = other[0, (j - cutf) * hop:(j - cutf) * hop + n]
                t.frame(fr, hop, True)
            fed2 = other[:, :n + hop * (frames - cutf - 1)]
        else:
            cut = n + hop * (cutf - 1) + 100
            sig = pcm.copy()
            sig[2, cut:] = other[0, :L - cut]
            a = 0
            for b in [cut, 300, 2000, L - cut - 2300]:
                if a == cut:
                    e.reset_stream(2)
                    before = {key: list(v) for key, v in t.rec[2].items()}
                    t.rec[2] = dict(col=[], db=[], rgba=[], pk=[], wv=[])
                t.push(sig, a, b, n, hop, True)
                a += b
            fed2 = other[:, :L - cut]
        t.flush_all()
        t.check_peaks()
        # the reset stream: its life before the reset is a prefix of the uninterrupted stream's envelope ...
        whole = emspec.wave_host(pcm, n, hop)
        cols = [c for c in before["col"] if c >= 0]
        assert cols == list(range(len(cols))) and len(cols) > 0
        assert _same(np.array([v for c, v in zip(before["col"], before["wv"]) if c >= 0]), whole[2, :len(cols)])
        # ... and its life after it is a stream of its own; the others never noticed
        want2 = emspec.wave_host(fed2, n, hop)[0]
        assert _same(t.emitted(2, "wv"), want2) and [c for c in t.rec[2]["col"] if c >= 0] == list(range(len(want2)))
        for s in (0, 1, 3, 4):
            assert _same(t.emitted(s, "wv"), whole[s]), s
        t.close()


# ---- 4. the envelope's order ----
def _order_signals(n, hop, frames):
    L = WS.length(n, hop, frames)
    rng = np.random.default_rng(5)
    x = np.stack([WS.signal("poisoned", n, hop, frames), WS.signal("step", n, hop, frames), synth.streams(1, L)[0], synth.streams(2, L)[1]])
    x[0, L // 2] = -np.inf                                     # (poisoned carries a NaN and +inf)
    x[1] = np.where(rng.integers(0, 2, L) == 1, F(0.0), F(-0.0))   # windows that hold only -0.0 and +0.0
    off = n // 2 - hop // 2
    x[2, off + 5 * hop:off + 6 * hop] = np.nan                 # one window that is all NaN
    x[2, off + 7 * hop + 3] = np.nan
    x[3, ::3] = -x[3, ::3]
    return x


@MODES
def test_envelope_order_and_batch_envelope(exact):
    """NaN, +-inf, signed zeros and an all-NaN window: the live pairs are wave_host's bits in both feeding forms; in EXACT mode
    the flushed session's pair list is the envelope emspec_set_wave_out delivers from emspec_batch on the same samples."""
    n, hop, frames, S = 1024, 256, 20, 4
    pcm = _order_signals(n, hop, frames)
    ref = emspec.wave_host(pcm, n, hop)
    assert W.same(W.envelope(pcm, n, hop), ref)
    assert np.array_equal(ref[2, 5].view(U), EMPTY_PAIR) and np.signbit(ref[1, :, 0]).all() and not np.signbit(ref[1, :, 1]).any()
    with _engine(exact) as e:
        lists = []
        for form in ("frames", "blocks"):
            e.reset()
            t = Session(e, S, 4, S * 32, peaks=False)
            if form == "frames":
                _run_frames(t, pcm, n, hop, True, frames)
            else:
                _run_blocks(t, pcm, n, hop, True, [700, 256, 3000, pcm.shape[1] - 3956])
            t.check_wave(pcm, n, hop)
            lists.append(np.array([t.emitted(s, "wv") for s in range(S)]))
            t.close()
        if exact:
            wave = np.full((S, frames, 2), 7.0, F)
            e.set_wave_out(wave)
            e.batch(pcm, n, hop, True)
            e.set_wave_out(None)
            for got in lists:
                assert _same(got, wave)


# ---- 5. the peaks against the batch entry ----
def test_peaks_equal_batch_peaks_exact():
    n, hop, S, L, k = 2048, 128, 2, 1 << 15, 8
    pcm = synth.streams(S, L)
    with _engine(True) as e:
        want = e.batch_peaks(pcm, n, hop, True, k, MIN_DB)
        for form in ("frames", "blocks"):
            e.reset()
            t = Session(e, S, k, S * 256, wave=False)
            if form == "frames":
                _run_frames(t, pcm, n, hop, True, emspec.num_columns(L, n, hop))
            else:
                _run_blocks(t, pcm, n, hop, True, [9000, 128, 20000, L - 29128])
            for s in range(S):
                assert _same(t.emitted(s, "pk"), want[s]), (form, s)
            t.close()
        # a known answer (the statement of tests/test_gpu_peaks.py): a 440 Hz sine's first peak lies in the row that holds 440 Hz
        tone = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(L) / 48000.0)).astype(F)[None]
        e.reset()
        t = Session(e, 1, 4, 256, wave=False, single=True)
        _run_blocks(t, tone, n, hop, True, [L])
        edges = e.row_edges_hz().astype(np.float64)
        pk = t.emitted(0, "pk")
        D = emspec.latency_columns(n, hop, True)
        assert len(pk) > D + 10
        for c in range(D, len(pk)):
            pos = float(pk[c, 0, 0])
            r = int(np.floor(pos))
            assert 0 <= r < e.rows and edges[r] <= 440.0 < edges[r + 1] and edges[r] <= e.position_hz(pos) <= edges[r + 1], (c, pos)
        t.close()


# ---- 6. / 7. the display post-process; RGBA only ----
def _script(e, pcm, n, hop, form, overlays, want_db=True, want_rgba=True, k=8):
    e.reset()
    S = pcm.shape[0]
    t = Session(e, S, k, S * 64, peaks=overlays, wave=overlays, want_db=want_db, want_rgba=want_rgba)
    if form == "frames":
        _run_frames(t, pcm, n, hop, True, (pcm.shape[1] - n) // hop + 1)
    else:
        _run_blocks(t, pcm, n, hop, True, [300, 256, 6000, pcm.shape[1] - 6556])
    t.close()
    return t


@MODES
@pytest.mark.parametrize("form", ["frames", "blocks"])
def test_display_on(exact, form):
    """emspec_set_display(0.6, 0.5): the peaks are peaks_host of the delivered, post-processed dB; the delivered dB and RGBA are
    those of the same script with the overlays cleared."""
    n, hop, S = 1024, 256, 3
    pcm = synth.streams(S, n + hop * 29)
    with _engine(exact) as e:
        e.set_display(0.6, 0.5)
        on = _script(e, pcm, n, hop, form, True)
        off = _script(e, pcm, n, hop, form, False)
        on.check_peaks()
        on.check_wave(pcm, n, hop)
        e.set_display(0.0, 0.0)
        raw = _script(e, pcm, n, hop, form, False)
    for s in range(S):
        assert on.rec[s]["col"] == off.rec[s]["col"]
        _same_run(on.rec[s]["db"], off.rec[s]["db"], exact, "display on, overlays set / cleared, stream %d" % s, terms=4)
        _same_run(on.rec[s]["rgba"], off.rec[s]["rgba"], exact, "display on, overlays set / cleared, stream %d" % s)
        assert not _same(np.array(on.rec[s]["db"]), np.array(raw.rec[s]["db"]))   # the post-process did run


@MODES
@pytest.mark.parametrize("form", ["frames", "blocks"])
@pytest.mark.parametrize("display", [False, True], ids=["raw", "display"])
def test_rgba_only(exact, form, display):
    """out_db NULL, RGBA wanted: the peaks are those of the run that also took dB, the RGBA bytes those with overlays cleared."""
    n, hop, S = 1024, 256, 3
    pcm = synth.streams(S, n + hop * 29)
    with _engine(exact) as e:
        if display:
            e.set_display(0.6, 0.5)
        both = _script(e, pcm, n, hop, form, True)
        only = _script(e, pcm, n, hop, form, True, want_db=False)
        off = _script(e, pcm, n, hop, form, False, want_db=False)
    both.check_peaks()
    for s in range(S):
        assert only.rec[s]["col"] == both.rec[s]["col"] and not only.rec[s]["db"]
        assert _same(np.array(only.rec[s]["wv"]), np.array(both.rec[s]["wv"]))
        if exact:   # (the peaks are a function of the dB bytes, and only the EXACT mode's are the same from run to run)
            assert _same(np.array(only.rec[s]["pk"]), np.array(both.rec[s]["pk"])), s
        _same_run(only.rec[s]["rgba"], off.rec[s]["rgba"], exact, "rgba only, overlays set / cleared, stream %d" % s)


# ---- 8. multi-resolution session ----
@MODES
def test_multires_session(exact):
    """8192 / 2048, hop 256, split 128 of 256 rows, S = 2: the peaks are those of the composed column, the envelope is on the
    n_low grid; a priming block without outputs is served or refused exactly as max_columns says."""
    S, n, nh, hop, split, k = 2, 8192, 2048, 256, 128, 8
    frames = 40
    pcm = synth.streams(S, n + hop * (frames - 1))
    with _engine(exact, rows=256) as e:
        t = Session(e, S, k, S * 64)
        _run_frames(t, pcm, n, hop, True, frames, n_high=nh, split=split)
        t.check_peaks()
        t.check_wave(pcm, n, hop)
        t.close()
        e.reset()
        t = Session(e, S, k, S * 64)
        # priming without outputs: max_columns = 0 serves a block that completes no column and writes nothing ...
        db, rgba, counts, firsts = e.push_samples_multires(pcm, n, nh, hop, split, True, want_db=False, want_rgba=False, count=n + hop, offset=0,
                                                           max_columns=0)
        assert db is None and np.all(counts == 0) and np.all(t.pk == t.FILL) and np.all(t.wv == t.FILL)
        # ... and refuses one that completes some, before anything is fed
        D = emspec.latency_columns(n, hop, True)
        with pytest.raises(emspec.EmspecError) as ei:
            e.push_samples_multires(pcm, n, nh, hop, split, True, want_db=False, want_rgba=False, count=(D + 2) * hop, offset=n + hop, max_columns=0)
        assert ei.value.code == emspec.ERR_INVALID_ARG and np.all(t.pk == t.FILL)
        a = n + hop
        for b in [(D + 2) * hop, 100, 3000, pcm.shape[1] - a - (D + 2) * hop - 3100]:
            t.push(pcm, a, b, n, hop, True, n_high=nh, split=split)
            a += b
        t.flush_all()
        t.check_peaks()
        t.check_wave(pcm, n, hop)
        t.close()


# ---- 9. PCM session ----
@MODES
def test_pcm_session_envelope(exact):
    """S16 stereo -> L R M S of 2 sources: the envelope is wave_host of the decoded views (tests/pcm_ref.py), which exist in no host buffer."""
    n, hop, frames, k = 1024, 256, 30, 4
    L = n + hop * (frames - 1)
    rng = np.random.default_rng(11)
    raw = rng.integers(-32768, 32768, (2, L * 2)).astype(np.int16)
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
    views = pcm_ref.decode(raw.view(np.uint8), pcm_ref.S16, 2, fmt.matrix)
    S = 8
    with _engine(exact) as e:
        t = Session(e, S, k, S * 64)
        a = 0
        for b in [100, 2000, 77, 256, L - 2433]:
            db, rgba, counts, firsts = e.push_samples_pcm(raw, fmt, n, hop, True, count=b, offset=a)
            t._take(db.shape[1], counts, firsts, db, None)
            a += b
        t.flush_all()
        t.check_peaks()
        t.check_wave(views, n, hop)
        t.close()


# ---- 10. the single-stream session beside a multi-stream one ----
@MODES
def test_single_stream_session_beside_a_live_one(exact):
    n, hop, frames, k = 1024, 256, 14, 8
    L = n + hop * (frames - 1)
    pcm = synth.streams(4, L)
    one, many = pcm[3:4], np.ascontiguousarray(pcm[:3])
    with _engine(exact) as e:
        # two recorders on one engine: the settings are the engine's, so they share the arrays - each call rewrites its own slots
        tm = Session(e, 3, k, 3 * 64)
        t1 = Session(e, 1, k, 64, peaks=False, wave=False, single=True)
        t1.pk, t1.wv = tm.pk, tm.wv
        for j in range(frames):
            tm.frame(_frames(many, j, n, hop), hop, True)
            t1.frame(_frames(one, j, n, hop), hop, True)
        t1.flush_all()
        tm.flush_all()
        for t, sig in ((tm, many), (t1, one)):
            t.check_peaks()
            t.check_wave(sig, n, hop)
        e.reset()
        t1.rec = [dict(col=[], db=[], rgba=[], pk=[], wv=[])]
        _run_blocks(t1, one, n, hop, True, [500, 256, 1500, L - 2256])
        t1.check_peaks()
        t1.check_wave(one, n, hop)
        tm.close()


# ---- 11. guards ----
def test_guards():
    """Every refusal of the two setters and of the calls' capacity rule, with its code and a message; the engine and the session
    are usable afterwards."""
    n, hop, S, k = 1024, 256, 2, 4
    pcm = synth.streams(S, n + hop * 9)
    D = emspec.latency_columns(n, hop, True)
    buf, wbuf = np.full(S * k * 2, 7.0, F), np.full(S * 2, 7.0, F)

    def refused(code, fn, *a, **kw):
        with pytest.raises(emspec.EmspecError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code and len(str(ei.value)) > 25, str(ei.value)

    with _engine(False) as e:
        for bad_k in (0, 33, -1):
            refused(emspec.ERR_INVALID_ARG, e.set_live_peaks, bad_k, MIN_DB, buf)
        refused(emspec.ERR_INVALID_ARG, e.set_live_peaks, k, float("nan"), buf)
        lib, h = e._lib, e._h
        assert lib.emspec_set_live_peaks(h, k, MIN_DB, buf.ctypes.data, -1) == emspec.ERR_INVALID_ARG
        assert lib.emspec_set_live_wave(h, wbuf.ctypes.data, -1) == emspec.ERR_INVALID_ARG
        assert b"capacity" in lib.emspec_last_error(h)
        # capacity one pair short: refused before anything is fed, and the session stays as it was
        e.set_live_peaks(k, MIN_DB, buf[:-2])
        refused(emspec.ERR_INVALID_ARG, e.columns, _frames(pcm, 0, n, hop), hop, True)
        assert e.live_streams == 0
        e.set_live_peaks(k, MIN_DB, buf)
        e.set_live_wave(wbuf[:-2])
        refused(emspec.ERR_INVALID_ARG, e.columns, _frames(pcm, 0, n, hop), hop, True)
        e.set_live_wave(wbuf)
        db0, _, cols = e.columns(_frames(pcm, 0, n, hop), hop, True)
        assert np.all(cols == -1) and np.array_equal(wbuf.reshape(S, 2).view(U), np.tile(EMPTY_PAIR, (S, 1)))
        # mid-session: the envelope cannot start (its history is gone), peaks can; clearing is always allowed
        e.set_live_wave(None)
        refused(emspec.ERR_STATE, e.set_live_wave, wbuf)
        assert "emspec_reset" in e._lib.emspec_last_error(e._h).decode()
        e.set_live_peaks(k, MIN_DB, None)
        got = [e.columns(_frames(pcm, j, n, hop), hop, True)[0] for j in range(1, 5)]
        e.set_live_peaks(k, MIN_DB, buf)
        got += [e.columns(_frames(pcm, j, n, hop), hop, True)[0] for j in range(5, 10)]
        assert _same(buf.reshape(S, k, 2), emspec.peaks_host(got[-1], k, MIN_DB))
        # a push whose block completes more columns than the arrays' capacity allows
        e.reset()
        e.set_live_wave(wbuf)
        refused(emspec.ERR_INVALID_ARG, e.push_samples_multi, pcm, n, hop, True, count=n + hop * (D + 1), offset=0)
        assert e.live_streams == 0
        e.set_live_wave(None)
        e.set_live_peaks(k, MIN_DB, None)
        e.reset()
        # a time reduction: the streaming calls refuse anyway, and so does the envelope's setter
        e.set_time_reduce(4)
        refused(emspec.ERR_STATE, e.set_live_wave, wbuf)
        e.set_time_reduce(1)
        e.set_live_wave(wbuf)
        e.set_live_wave(None)
    # peaks set and cleared mid-session change no dB byte (byte equality of the dB across runs is the EXACT mode's)
    with _engine(True) as x:
        x.set_live_peaks(k, MIN_DB, buf)
        a = [x.columns(_frames(pcm, j, n, hop), hop, True)[0] for j in range(5)]
        x.set_live_peaks(k, MIN_DB, None)
        a += [x.columns(_frames(pcm, j, n, hop), hop, True)[0] for j in range(5, 10)]
        x.reset()
        b = [x.columns(_frames(pcm, j, n, hop), hop, True)[0] for j in range(10)]
        assert _same(np.array(a), np.array(b))
    # (engine rows that break the rule of emspec_peaks_device cannot be shown: emspec_create accepts multiples of 4 in 64 .. 4096
    # only, all of which the rule admits; the setter's check stands behind that)
