"""GPU: the live level meters (include/emspec.h: emspec_set_live_level, emspec_set_live_cross): beside
every column a streaming call delivers, the level record of the samples under it and, per pair of streams, their cross record.

The reference is tests/level_ref.py (levels, crosses: Python-integer definitions, vectorised) of the samples fed, and every
comparison is on bytes: the records are integer sums and maxima, the same in FAST and EXACT mode, in both feeding forms, however
the samples were cut into calls.  Nothing here has a tolerance."""
import numpy as np
import pytest

import emspec
import level_ref as LR
import pcm_ref
import worst_signals as WS
from emspec import synth

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
LEVEL, CROSS = emspec.LEVEL_DTYPE, emspec.CROSS_DTYPE
MODES = pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
FILL = 0x5A   # every byte of a slot no call has written


def _engine(exact, **kw):
    return emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST, **kw)


def _same(a, b):
    return LR.same(np.asarray(a), np.asarray(b))


class Meters:
    """One engine session with the meters on: feeds, and keeps per stream (per pair) the record every call delivered, column by
    column; a slot a call did not write must still hold FILL."""

    def __init__(self, e, S, cols, level=True, cross=None, pinned=False, single=False, want_db=True, want_rgba=False):
        self.e, self.S, self.single, self.keep = e, S, single, []
        self.want = dict(want_db=want_db, want_rgba=want_rgba)
        self.views = cross[0] if cross else 1
        self.P = S // self.views
        self.lv = self._alloc(S * cols, LEVEL, pinned) if level else None
        self.cr = self._alloc(self.P * cols, CROSS, pinned) if cross else None
        if level:
            e.set_live_level(self.lv)
        if cross:
            e.set_live_cross(*cross, self.cr)
        self.col = [[] for _ in range(S)]
        self.level = [[] for _ in range(S)]
        self.cross = [[] for _ in range(self.P)]
        self.db, self.rgba = [[] for _ in range(S)], [[] for _ in range(S)]

    def _alloc(self, count, dtype, pinned):
        if pinned:
            self.keep.append(emspec.PinnedArray((count,), dtype))
            a = self.keep[-1].array
        else:
            a = np.empty(count, dtype)
        a.view(np.uint8)[:] = FILL
        return a

    def close(self):
        self.e.set_live_level(None)
        self.e.set_live_cross(0, 0, 0, None)
        for p in self.keep:
            p.close()

    def take(self, cols, counts, firsts, db=None, rgba=None):
        """After a call that delivered [S][cols]: the written slots of every stream and pair; the others must be untouched."""
        for s in range(self.S):
            for i in range(int(counts[s])):
                self.col[s].append(int(firsts[s]) + i if firsts[s] >= 0 else -1)
                if db is not None:
                    self.db[s].append(db[s, i].copy())
                if rgba is not None:
                    self.rgba[s].append(rgba[s, i].copy())
        for arr, rows, per, sink in ((self.lv, self.S, 1, self.level), (self.cr, self.P, self.views, self.cross)):
            if arr is None:
                continue
            a = arr[:rows * cols].reshape(rows, cols)
            for r in range(rows):
                k = int(counts[r * per])
                sink[r].extend(a[r, :k].copy())
                assert np.all(a[r, k:].view(np.uint8) == FILL), "a slot the call did not write was touched"
            assert np.all(arr[rows * cols:].view(np.uint8) == FILL)
            a.view(np.uint8)[:] = FILL

    # ---- the calls ----
    def frame(self, frames, hop, reassign):
        if self.single:
            db, c = self.e.column(frames[0], hop, reassign)
            db, rgba, cols = db[None], None, np.array([c])
        else:
            db, rgba, cols = self.e.columns(frames, hop, reassign, **self.want)
        self.take(1, np.ones(self.S, int), cols, db[:, None] if db is not None else None, rgba[:, None] if rgba is not None else None)

    def flush(self):
        if self.single:
            db, c = self.e.flush()
            db, rgba, cols = db[None], None, np.array([c])
        else:
            db, rgba, cols = self.e.columns_flush(**self.want)
        self.take(1, np.ones(self.S, int), cols, db[:, None] if db is not None else None, rgba[:, None] if rgba is not None else None)

    def push(self, pcm, a, cnt, n, hop, reassign):
        if self.single:
            db, first = self.e.push_samples(pcm[0, a:a + cnt], n, hop, reassign)
            db, rgba, counts, firsts = db[None], None, np.array([db.shape[0]]), np.array([first])
        else:
            db, rgba, counts, firsts = self.e.push_samples_multi(pcm, n, hop, reassign, count=cnt, offset=a, **self.want)
        cols = (db if db is not None else rgba).shape[1]
        self.take(cols, counts, firsts, db, rgba)

    def flush_all(self):
        while True:
            try:
                self.flush()
            except emspec.EmspecError as ex:
                assert ex.code == emspec.ERR_STATE
                return

    # ---- what was delivered ----
    def emitted(self, r, sink, per=1):
        """row r's records of real columns (not the empty ones), in order"""
        return np.array([v for c, v in zip(self.col[r * per], sink[r]) if c >= 0], dtype=LEVEL if sink is self.level else CROSS)

    def check(self, fed, n, hop, cross=None):
        """fed: [S][L] what every stream was fed; the session is flushed."""
        want = LR.levels(fed, n, hop)
        for s in range(self.S):
            assert [c for c in self.col[s] if c >= 0] == list(range(want.shape[1])), (s, self.col[s][:5], want.shape)
            if self.lv is not None:
                assert _same(self.emitted(s, self.level), want[s]), ("level records differ from level_ref.levels", s)
                assert all(v.tobytes() == bytes(24) for c, v in zip(self.col[s], self.level[s]) if c < 0), "the empty column's record is zero"
        if cross:
            wantx = LR.crosses(fed, *cross, n, hop)
            for p in range(self.P):
                assert _same(self.emitted(p, self.cross, self.views), wantx[p]), ("cross records differ from level_ref.crosses", p)
                assert all(v.tobytes() == bytes(16) for c, v in zip(self.col[p * self.views], self.cross[p]) if c < 0)


def _frames(pcm, j, n, hop):
    return np.ascontiguousarray(pcm[:, j * hop:j * hop + n])


def _run_frames(t, pcm, n, hop, reassign, frames):
    for j in range(frames):
        t.frame(_frames(pcm, j, n, hop), hop, reassign)
    t.flush_all()


def _run_blocks(t, pcm, n, hop, reassign, blocks):
    a = 0
    for b in blocks:
        t.push(pcm, a, b, n, hop, reassign)
        a += b
    assert a == pcm.shape[1]
    t.flush_all()


# ---- 3. per-frame form ----
@MODES
@pytest.mark.parametrize("n,hop,reassign", [(1024, 256, True), (256, 100, False)])
def test_per_frame_form(exact, n, hop, reassign):
    """S = 3, D + 12 frames and the flushes.  1024 / 256 with reassignment: D = 2, the records wait in the ring; 256 / 100
    without: D = 0, a column's record is its own frame's, and the hop is no multiple of 64 or of 4."""
    S = 3
    D = emspec.latency_columns(n, hop, reassign)
    frames = D + 12
    pcm = synth.streams(S, n + hop * (frames - 1))
    with _engine(exact) as e:
        t = Meters(e, S, 1)
        _run_frames(t, pcm, n, hop, reassign, frames)
        assert t.col[0] == [-1] * D + list(range(frames))
        t.check(pcm, n, hop)
        assert all(np.all(t.emitted(s, t.level)["sq_lo"] > 0) for s in range(S))
        t.close()
    # (the reference against the library's own host form, once)
    assert _same(LR.levels(pcm, n, hop), emspec.level_host(pcm, n, hop))


# ---- 4. block form ----
@MODES
def test_block_form(exact):
    """S = 4, 4096 / 256: blocks of 1, 255, 257, 4096, 20000 and 777 samples, then the flush.  mmax = 64 frames at S = 4, so the
    20000-sample block is more than one launch, and a launch of 64 frames takes its first D = 8 columns' records from the ring
    and the other 56 from its own samples.  Pageable and page-locked arrays give the same bytes."""
    S, n, hop = 4, 4096, 256
    blocks = [1, 255, 257, 4096, 20000, 777]
    pcm = synth.streams(S, sum(blocks))
    got = {}
    with _engine(exact) as e:
        for pinned in (False, True):
            e.reset()
            t = Meters(e, S, 128, cross=(2, 0, 1), pinned=pinned)
            _run_blocks(t, pcm, n, hop, True, blocks)
            t.check(pcm, n, hop, cross=(2, 0, 1))
            assert len(t.level[0]) == emspec.num_columns(sum(blocks), n, hop) > 64 + 8
            got[pinned] = (np.array(t.level, dtype=LEVEL), np.array(t.cross, dtype=CROSS))
            t.close()
    assert got[False][0].tobytes() == got[True][0].tobytes() and got[False][1].tobytes() == got[True][1].tobytes()


# ---- 5. signals ----
def _signals(n, hop, frames):
    L = WS.length(n, hop, frames)
    off = n // 2 - hop // 2
    x = np.stack([synth.streams(1, L)[0], WS.signal("poisoned", n, hop, frames), WS.signal("loud", n, hop, frames),
                  synth.streams(2, L)[1], np.where((np.arange(L) // 37) % 2 == 0, F(1.0), F(-1.0))]).astype(F)
    x[0, off + 3 * hop - 5:off + 5 * hop + 7] = np.nan              # a NaN run over more than a whole column
    x[1, L // 2] = -np.inf                                           # (poisoned carries a NaN and +inf)
    x[2, off + 2 * hop:off + 2 * hop + 9] = [128.0, -128.0, 127.99999, 200.0, -1e30, 129.0, -127.99999, 3e38, 130.0]
    tiny = np.array([0x00000001, 0x807fffff, 0x00400000, 0x80000000, 0x33000000, 0x32ffffff, 0x33800000, 0xb3000001], U).view(F)
    x[3, off:off + 4 * hop] = np.tile(tiny, 4 * hop // 8)            # -0.0, denormals and the values around 2^-25, where k rounds to 0 or 1
    return x


@MODES
@pytest.mark.parametrize("form", ["frames", "blocks"])
def test_signals(exact, form):
    """A NaN run, +-Inf, |x| >= 128 inside a level of 30, -0.0 and denormals, a full-scale square (k^2 = 2^48: sq_hi counts):
    odd, peak and both limbs are the reference's."""
    n, hop, frames = 1024, 256, 16
    pcm = _signals(n, hop, frames)
    S = pcm.shape[0]
    want = LR.levels(pcm, n, hop)
    assert want["odd"][0].max() == hop and want["odd"][1].sum() == 3 and want["odd"][2].sum() == 7 and want["peak"][2].max() == LR.KMAX
    assert np.all(want["sq_hi"][4] == hop << 16) and np.all(want["sq_lo"][4] == 0) and want["peak"][3, :4].max() == 1
    with _engine(exact) as e:
        t = Meters(e, S, 32, cross=(1, 0, 0))
        if form == "frames":
            _run_frames(t, pcm, n, hop, True, frames)
        else:
            _run_blocks(t, pcm, n, hop, True, [700, 256, 3000, pcm.shape[1] - 3956])
        t.check(pcm, n, hop, cross=(1, 0, 0))      # (views = 1, a = b = 0: every stream against itself)
        t.close()


# ---- 6. cross ----
def _pairs(L):
    base = synth.streams(4, L + 1)
    x = np.empty((6, L), F)
    x[0], x[1] = base[0, :L], -base[0, :L]             # the inverted copy
    x[2], x[3] = base[1, :L], base[2, :L]              # an independent signal
    x[4], x[5] = base[3, 1:], base[3, :L]              # a copy delayed by one sample
    return x


@MODES
@pytest.mark.parametrize("ab", [(0, 1), (1, 1)])
def test_cross(exact, ab):
    """S = 6 as three pairs of views = 2: records equal level_ref.crosses in both forms; the summed records of the inverted pair
    give a correlation of exactly -1."""
    n, hop, frames, S = 1024, 256, 14, 6
    L = n + hop * (frames - 1)
    pcm = _pairs(L)
    with _engine(exact) as e:
        for form in ("frames", "blocks"):
            e.reset()
            t = Meters(e, S, 32, cross=(2,) + ab)
            if form == "frames":
                _run_frames(t, pcm, n, hop, True, frames)
            else:
                _run_blocks(t, pcm, n, hop, True, [1500, 100, 256, L - 1856])
            t.check(pcm, n, hop, cross=(2,) + ab)
            la, lb = emspec.level_sum(t.emitted(0, t.level)), emspec.level_sum(t.emitted(1, t.level))
            x = emspec.cross_sum(t.emitted(0, t.cross, 2))
            rho = emspec.cross_correlation(la, lb, x)
            assert rho == (-1.0 if ab == (0, 1) else 1.0), rho
            assert LR.sum_ab(x) == (-LR.sum_sq(la) if ab == (0, 1) else LR.sum_sq(lb))
            t.close()


# ---- 7. PCM session ----
@MODES
def test_pcm_session(exact):
    """S16 stereo -> L R M S of 2 sources: the level of all 8 streams and the cross of (0, 1) and of (2, 3) are level_ref's on the
    decoded views (tests/pcm_ref.py), which exist in no host buffer."""
    n, hop, frames = 1024, 256, 24
    L = n + hop * (frames - 1)
    rng = np.random.default_rng(11)
    raw = rng.integers(-32768, 32768, (2, L * 2)).astype(np.int16)
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
    views = pcm_ref.decode(raw.view(np.uint8), pcm_ref.S16, 2, fmt.matrix)
    S = 8
    with _engine(exact) as e:
        for ab in ((0, 1), (2, 3)):
            e.reset()
            t = Meters(e, S, 32, cross=(4,) + ab)
            a = 0
            for b in [100, 2000, 77, 256, L - 2433]:
                db, rgba, counts, firsts = e.push_samples_pcm(raw, fmt, n, hop, True, count=b, offset=a)
                t.take(db.shape[1], counts, firsts)
                a += b
            t.flush_all()
            t.check(views, n, hop, cross=(4,) + ab)
            t.close()


# ---- 8. other sessions ----
def test_multiband_session():
    """16384 / 4096 / 1024 at hop 256, S = 2: the records lie on the grid of n[0]."""
    n, hop, S, frames = (16384, 4096, 1024), 256, 2, 40
    L = n[0] + hop * (frames - 1)
    pcm = synth.streams(S, L)
    with _engine(False) as e:
        split = tuple(e.split_row_for_hz(f) for f in (250.0, 2000.0))
        t = Meters(e, S, 64, cross=(2, 0, 1))
        a = 0
        for b in [n[0] + 300, 256, 5000, L - n[0] - 5556]:
            db, _, counts, firsts = e.push_samples_multiband(pcm, n, split, hop, True, count=b, offset=a)
            t.take(db.shape[1], counts, firsts)
            a += b
        t.flush_all()
        t.check(pcm, n[0], hop, cross=(2, 0, 1))
        t.close()


@MODES
def test_single_stream_session_beside_a_live_one(exact):
    n, hop, frames = 1024, 256, 14
    L = n + hop * (frames - 1)
    pcm = synth.streams(4, L)
    one, many = pcm[3:4], np.ascontiguousarray(pcm[:3])
    with _engine(exact) as e:
        # two recorders on one engine: the setting is the engine's, so they share the array - each call rewrites its own slots
        tm = Meters(e, 3, 64)
        t1 = Meters(e, 1, 64, level=False, single=True)
        t1.lv = tm.lv
        for j in range(frames):
            tm.frame(_frames(many, j, n, hop), hop, True)
            t1.frame(_frames(one, j, n, hop), hop, True)
        t1.flush_all()
        tm.flush_all()
        tm.check(many, n, hop)
        t1.check(one, n, hop)
        e.reset()
        t1.col, t1.level = [[]], [[]]
        _run_blocks(t1, one, n, hop, True, [500, 256, 1500, L - 2256])
        t1.check(one, n, hop)
        tm.close()


# ---- 9. emspec_reset_stream ----
@MODES
@pytest.mark.parametrize("form", ["frames", "blocks"])
def test_reset_of_one_stream(exact, form):
    """The script of the overlay tests: S = 5, stream 2 is reset and fed another signal from its start - its records restart as
    those of what it was fed afterwards, the other streams' are those of the uninterrupted streams."""
    S, n, hop = 5, 1024, 256
    frames, cutf = 30, 11
    L = n + hop * (frames - 1)
    pcm = synth.streams(S, L)
    other = synth.streams(7, L)[6:7]
    with _engine(exact) as e:
        t = Meters(e, S, 64)
        if form == "frames":
            for j in range(frames):
                if j == cutf:
                    e.reset_stream(2)
                    before = (list(t.col[2]), list(t.level[2]))
                    t.col[2], t.level[2] = [], []
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
                    before = (list(t.col[2]), list(t.level[2]))
                    t.col[2], t.level[2] = [], []
                t.push(sig, a, b, n, hop, True)
                a += b
            fed2 = other[:, :L - cut]
        t.flush_all()
        whole = LR.levels(pcm, n, hop)
        cols = [c for c in before[0] if c >= 0]
        assert cols == list(range(len(cols))) and len(cols) > 0
        assert _same(np.array([v for c, v in zip(*before) if c >= 0], dtype=LEVEL), whole[2, :len(cols)])
        want2 = LR.levels(fed2, n, hop)[0]
        assert _same(t.emitted(2, t.level), want2) and [c for c in t.col[2] if c >= 0] == list(range(len(want2)))
        for s in (0, 1, 3, 4):
            assert _same(t.emitted(s, t.level), whole[s]), s
        t.close()


def test_reset_stream_is_refused_while_a_cross_is_set():
    """EMSPEC_ERR_STATE, nothing changes: the next push gives the bytes of an undisturbed session."""
    S, n, hop = 4, 1024, 256
    L = n + hop * 19
    pcm = synth.streams(S, L)
    with _engine(True) as e:
        t = Meters(e, S, 64, cross=(2, 0, 1))
        t.push(pcm, 0, 3000, n, hop, True)
        with pytest.raises(emspec.EmspecError) as ei:
            e.reset_stream(1)
        assert ei.value.code == emspec.ERR_STATE and "emspec_set_live_cross" in str(ei.value)
        t.push(pcm, 3000, L - 3000, n, hop, True)
        t.flush_all()
        t.check(pcm, n, hop, cross=(2, 0, 1))
        db = np.array(t.db)
        t.close()
        e.reset()
        u = Meters(e, S, 64, level=False)
        _run_blocks(u, pcm, n, hop, True, [3000, L - 3000])
        assert np.array_equal(db.view(U), np.array(u.db).view(U))        # (EXACT: the dB is the same from run to run)
        # cleared, the stream restarts alone again
        e.reset_stream(1)


# ---- 10. all overlays at once ----
def test_all_overlays_at_once():
    """Peaks (k = 8) + envelope + level + cross + history W = 64 + audio history, out_db NULL and RGBA only (EXACT: its dB is the
    same from run to run).  Level and cross equal level_ref; the envelope equals wave_host; the peaks equal peaks_host of the dB
    the history kept; the audio history holds the samples fed; and peaks and envelope are those of the same script with level
    and cross cleared."""
    S, n, hop, k, frames = 4, 1024, 256, 8, 30
    L = n + hop * (frames - 1)
    pcm = synth.streams(S, L)
    runs = {}
    with _engine(True) as e:
        for meters in (True, False):
            e.reset()
            e.set_live_history(64)
            e.set_live_audio(1 << 15)
            pk, wv = np.full(S * 64 * k * 2, 7.0, F), np.full(S * 64 * 2, 7.0, F)
            e.set_live_peaks(k, -60.0, pk)
            e.set_live_wave(wv)
            t = Meters(e, S, 64, level=meters, cross=(2, 0, 1) if meters else None, want_db=False, want_rgba=True)
            peaks, waves = [[] for _ in range(S)], [[] for _ in range(S)]
            a = 0
            for b in [300, 256, 6000, L - 6556]:
                _, rgba, counts, firsts = e.push_samples_multi(pcm, n, hop, True, want_db=False, want_rgba=True, count=b, offset=a)
                cols = rgba.shape[1]
                t.take(cols, counts, firsts, None, rgba)
                for s in range(S):
                    peaks[s].extend(pk[:S * cols * k * 2].reshape(S, cols, k, 2)[s, :counts[s]].copy())
                    waves[s].extend(wv[:S * cols * 2].reshape(S, cols, 2)[s, :counts[s]].copy())
                a += b
            while True:
                try:
                    _, rgba, cols = e.columns_flush(want_db=False, want_rgba=True)
                except emspec.EmspecError:
                    break
                t.take(1, np.ones(S, int), cols, None, rgba[:, None])
                for s in range(S):
                    peaks[s].append(pk[:S * k * 2].reshape(S, k, 2)[s].copy())
                    waves[s].append(wv[:S * 2].reshape(S, 2)[s].copy())
            runs[meters] = (np.array(peaks), np.array(waves), np.array(t.rgba))
            if meters:
                t.check(pcm, n, hop, cross=(2, 0, 1))
                assert np.array_equal(np.array(waves).view(U), emspec.wave_host(pcm, n, hop).view(U))
                kept = e.history_view(0, 1, frames)["db"]
                assert np.array_equal(np.array(peaks).view(U), emspec.peaks_host(kept, k, -60.0).view(U))
                assert np.array_equal(e.audio_view(0, L).view(U), pcm.view(U))
            t.close()
            e.set_live_peaks(k, -60.0, None)
            e.set_live_wave(None)
    for i in range(3):
        assert np.array_equal(runs[True][i].view(np.uint8), runs[False][i].view(np.uint8)), i


# ---- 11. guards ----
def test_guards():
    n, hop, S = 1024, 256, 4
    pcm = synth.streams(S, n + hop * 9)
    D = emspec.latency_columns(n, hop, True)
    lbuf, xbuf = np.zeros(S + 1, LEVEL), np.zeros(S // 2 + 1, CROSS)
    lbuf.view(np.uint8)[:] = FILL

    def refused(code, fn, *a, **kw):
        with pytest.raises(emspec.EmspecError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code and len(str(ei.value)) > 25, str(ei.value)

    with _engine(False) as e:
        lib, h = e._lib, e._h
        # a NULL engine; misaligned outputs; a negative capacity
        assert lib.emspec_set_live_level(None, lbuf.ctypes.data, S) == emspec.ERR_INVALID_ARG
        assert lib.emspec_set_live_cross(None, 2, 0, 1, xbuf.ctypes.data, S) == emspec.ERR_INVALID_ARG
        assert lib.emspec_set_live_level(h, lbuf.ctypes.data + 4, S) == emspec.ERR_INVALID_ARG and b"8-byte" in lib.emspec_last_error(h)
        assert lib.emspec_set_live_cross(h, 2, 0, 1, xbuf.ctypes.data + 4, 2) == emspec.ERR_INVALID_ARG and b"8-byte" in lib.emspec_last_error(h)
        assert lib.emspec_set_live_level(h, lbuf.ctypes.data, -1) == emspec.ERR_INVALID_ARG and b"capacity" in lib.emspec_last_error(h)
        assert lib.emspec_set_live_cross(h, 2, 0, 1, xbuf.ctypes.data, -1) == emspec.ERR_INVALID_ARG and b"capacity" in lib.emspec_last_error(h)
        # the pair rule, at set time
        for views, a, b in ((0, 0, 0), (65, 0, 1), (2, 2, 0), (2, 0, 2), (2, -1, 0)):
            refused(emspec.ERR_INVALID_ARG, e.set_live_cross, views, a, b, xbuf)
        # capacity one record short: refused before anything is fed, and the session stays as it was
        e.set_live_level(lbuf[:S - 1])
        refused(emspec.ERR_INVALID_ARG, e.columns, _frames(pcm, 0, n, hop), hop, True)
        assert e.live_streams == 0
        e.set_live_level(lbuf)
        e.set_live_cross(2, 0, 1, xbuf[:S // 2 - 1])
        refused(emspec.ERR_INVALID_ARG, e.columns, _frames(pcm, 0, n, hop), hop, True)
        assert e.live_streams == 0
        # S = 5 with views = 2: no pairs
        e.set_live_cross(2, 0, 1, xbuf)
        refused(emspec.ERR_INVALID_ARG, e.columns, np.zeros((5, n), F), hop, True)
        assert e.live_streams == 0 and "multiple" in lib.emspec_last_error(h).decode()
        e.set_live_cross(0, 0, 0, None)
        # a push whose block completes more columns than max_columns (here: than the arrays hold)
        refused(emspec.ERR_INVALID_ARG, e.push_samples_multi, pcm, n, hop, True, count=n + hop * (D + 1), offset=0)
        assert e.live_streams == 0
        assert lib.emspec_push_samples_multi(h, pcm.ctypes.data, S, n + hop * (D + 2), pcm.shape[1], n, hop, 1, None, None, e.rows, 1, None,
                                             None) == emspec.ERR_INVALID_ARG and b"fewer columns" in lib.emspec_last_error(h)
        # fed: one frame - the empty column's records, and the slot behind them untouched
        e.columns(_frames(pcm, 0, n, hop), hop, True)
        assert np.all(lbuf[:S].view(np.uint8) == 0) and np.all(lbuf[S:].view(np.uint8) == FILL)
        refused(emspec.ERR_STATE, e.set_live_level, lbuf[:S])            # setting while frames are fed is refused ...
        assert e.live_streams == S
        e.set_live_level(None)                                           # ... clearing succeeds
        e.set_live_cross(0, 0, 0, None)
        refused(emspec.ERR_STATE, e.set_live_level, lbuf)
        assert "emspec_reset" in lib.emspec_last_error(h).decode()
        refused(emspec.ERR_STATE, e.set_live_cross, 2, 0, 1, xbuf)
        _, _, cols = e.columns(_frames(pcm, 1, n, hop), hop, True)      # the session goes on
        assert np.all(cols == -1)
        e.reset()
        # streams moved apart before any frame, then a cross: the pairs are out of step until emspec_reset
        e.push_samples_multi(pcm, n, hop, True, count=100, offset=0)
        e.reset_stream(1)
        e.set_live_cross(2, 0, 1, xbuf)
        refused(emspec.ERR_STATE, e.push_samples_multi, pcm, n, hop, True, count=100, offset=100)
        e.set_live_cross(0, 0, 0, None)
        e.reset()
        # a time reduction of 2
        e.set_time_reduce(2)
        refused(emspec.ERR_STATE, e.set_live_level, lbuf)
        refused(emspec.ERR_STATE, e.set_live_cross, 2, 0, 1, xbuf)
        e.set_time_reduce(1)
        e.set_live_level(lbuf)
        e.set_live_cross(2, 0, 1, xbuf)
        e.set_live_level(None)
        e.set_live_cross(0, 0, 0, None)
