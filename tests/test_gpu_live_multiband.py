"""GPU: the live multi-band session (include/emspec.h: emspec_columns_multiband, emspec_push_samples_multiband,
emspec_push_columns_multiband, emspec_push_samples_pcm_multiband) - the multi-band image column by column
while the audio arrives.  The reference is the definition, tests/multiband_ref.py: compose(...) on the CPU bit models (EXACT: equal
bytes; FAST: the live tests' bounds, sums in arrival order) - except where a test says it compares two calls of the engine.

Shapes: 3 streams of n[0] + 119 hops unless said otherwise, 1024 rows, split rows from split_row_for_hz.  The ladders:
    A (4096, 2048, 1024) / 256          the smallest; the 1024 band makes every launch defer to the bands kernel
    B (16384, 4096, 1024) / 256         60 and 48 priming frames
    C (8192, 4096, 2048) / 128          no band defers at one hop per call: every band finalises in place
    D (16384, 8192, 4096, 2048) / 512   four bands
"""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec
import multiband_ref as B
import oracle as O
import pcm_ref as P
from emspec import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_DB = 8.7e-4          # FAST dB (tests/test_gpu_live_multires.py)
RGBA_SHARE = 1e-3        # FAST: share of RGBA bytes that may differ (tests/test_gpu_live_multires.py)
BOOST = 2.0
R = 1024
FRAMES = 120
LADDERS = {"A": ((4096, 2048, 1024), 256, (250.0, 2000.0)), "B": ((16384, 4096, 1024), 256, (250.0, 2000.0)),
           "C": ((8192, 4096, 2048), 128, (250.0, 2000.0)), "D": ((16384, 8192, 4096, 2048), 512, (120.0, 500.0, 2000.0))}
MODES = pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
U = np.uint32


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """(tests/conftest.py: torch's HIP runtime is initialised before the first engine is created)"""
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()


def _engine(exact, boost=None):
    e = emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST)
    if boost is not None:
        e.set_row_edges_hz(emspec.warped_edges_hz(e.rows, 20.0, 24000.0, boost))
    return e


def _split(e, hz):
    return tuple(e.split_row_for_hz(f) for f in hz)


@functools.lru_cache(maxsize=None)
def _pcm(S, L):
    x = synth.streams(S, L)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(S, L, n, hop, split, reassign, exact, boost):
    """compose() of _pcm(S, L): db and rgba, computed once per shape and shared (read-only)."""
    edges = None if boost is None else emspec.warped_edges_hz(R, 20.0, 24000.0, boost)
    out = B.compose(_pcm(S, L), n, split, hop, reassign, exact=exact, edges_hz=edges, want=("db", "rgba"))
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def _same_db(got, want, exact):
    assert got.shape == want.shape, (got.shape, want.shape)
    if exact:
        assert np.array_equal(got.view(U), want.view(U))
    else:
        err = float(np.max(np.abs(got - want)))
        print(f"max dB err {err:.2e}")
        assert err < TOL_DB, err


def _same_rgba(got, want, exact):
    assert got.shape == want.shape, (got.shape, want.shape)
    if exact:
        assert np.array_equal(got, want)
    else:
        share = float(np.mean(got != want))
        print(f"rgba share {share:.2e}")
        assert share < RGBA_SHARE, share


def _expected_counts(seen_before, count, n0, hop, D):
    before = max(emspec.num_columns(seen_before, n0, hop) - D, 0)
    after = max(emspec.num_columns(seen_before + count, n0, hop) - D, 0)
    return after - before, before


def _push_session(e, pcm, n, hop, split, reassign, block, want_rgba=True, a0=0, feed=None):
    """Feeds pcm[:, a0:] in blocks, flushes; returns (db [S][J][R], rgba) and checks counts / first columns / prediction."""
    S, L = pcm.shape[0], pcm.shape[1] - a0
    J = emspec.multiband_columns(L, n, hop)
    assert J == emspec.num_columns(L, n[0], hop)
    D = emspec.latency_columns(n[0], hop, reassign)
    got_db = np.empty((S, J, R), np.float32)
    got_rgba = np.empty((S, J, R, 4), np.uint8)
    feed = feed or (lambda cnt, off: e.push_samples_multiband(pcm, n, split, hop, reassign, want_rgba=want_rgba, count=cnt, offset=off))
    nxt = 0
    for a in range(0, L, block):
        cnt = min(block, L - a)
        want_k, want_first = _expected_counts(a, cnt, n[0], hop, D)
        k = e.push_columns_multiband(cnt, n, hop, reassign)
        assert k == want_k, (a, k, want_k)
        db, rgba, counts, firsts = feed(cnt, a0 + a)
        assert np.all(counts == k) and db.shape[1] == k
        assert np.all(firsts == (want_first if k else -1))
        if k:
            got_db[:, nxt:nxt + k] = db
            if want_rgba:
                got_rgba[:, nxt:nxt + k] = rgba
            nxt += k
    assert nxt == max(J - D, 0)
    for i in range(min(D, J)):
        db, rgba, cols = e.columns_flush(want_rgba=want_rgba)
        assert np.all(cols == nxt)
        got_db[:, nxt] = db
        if want_rgba:
            got_rgba[:, nxt] = rgba
        nxt += 1
    assert nxt == J
    return got_db, got_rgba


# ---- 1. per-frame form ----
@MODES
def test_per_frame_form_equals_the_composition(exact):
    (n, hop, hz), S, L = LADDERS["A"], 2, 1 << 15
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n[0], hop, True)
    J = emspec.multiband_columns(L, n, hop)
    got_db = np.empty((S, J, R), np.float32)
    got_rgba = np.empty((S, J, R, 4), np.uint8)
    with _engine(exact) as e:
        split = _split(e, hz)
        for j in range(J):
            db, rgba, cols = e.columns_multiband(pcm[:, j * hop:j * hop + n[0]], n, split, hop, True, want_rgba=True)
            assert e.live_streams == S
            assert np.all(cols == (j - D if j >= D else -1))
            if j >= D:
                got_db[:, j - D], got_rgba[:, j - D] = db, rgba
            else:   # the empty column, written whole: constant dB, constant RGBA - every band wrote its part
                assert np.all(db == db[0, 0]) and np.all(rgba == rgba[0, 0])
        for i in range(D):
            db, rgba, cols = e.columns_flush(want_rgba=True)
            assert np.all(cols == J - D + i)
            got_db[:, J - D + i], got_rgba[:, J - D + i] = db, rgba
        with pytest.raises(emspec.EmspecError) as ei:
            e.columns_flush()
        assert ei.value.code == emspec.ERR_STATE
        with pytest.raises(emspec.EmspecError) as ei:   # a flushed stream is at its end
            e.columns_multiband(pcm[:, :n[0]], n, split, hop, True)
        assert ei.value.code == emspec.ERR_STATE
    want = _ref(S, L, n, hop, split, True, exact, None)
    _same_db(got_db, want["db"], exact)
    _same_rgba(got_rgba, want["rgba"], exact)


# ---- 2. sample-block form ----
def _block_case(name, block, reassign, exact, boost):
    n, hop, hz = LADDERS[name]
    S, L = 3, n[0] + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    with _engine(exact, boost) as e:
        split = _split(e, hz)
        got_db, got_rgba = _push_session(e, pcm, n, hop, split, reassign, hop if block == "hop" else block)
    want = _ref(S, L, n, hop, split, reassign, exact, boost)
    _same_db(got_db, want["db"], exact)
    _same_rgba(got_rgba, want["rgba"], exact)


@MODES
@pytest.mark.parametrize("block", [128, "hop", 1000, 20000])
@pytest.mark.parametrize("name", list(LADDERS))
def test_sample_blocks_equal_the_composition(name, block, exact):
    _block_case(name, block, True, exact, None)


@MODES
@pytest.mark.parametrize("block", ["hop", 1000])
def test_sample_blocks_without_reassignment(block, exact):
    _block_case("A", block, False, exact, None)


@MODES
def test_sample_blocks_on_the_warped_axis(exact):
    _block_case("B", 1000, True, exact, BOOST)


# ---- 3. K = 2 through the multi-band entry: the two-band live session's bytes ----
@pytest.mark.parametrize("n_low,n_high,hop", [(16384, 4096, 256), (8192, 2048, 128)])
@pytest.mark.parametrize("block", ["hop", 1000])
def test_two_bands_equal_the_two_band_session(n_low, n_high, hop, block):
    S, L = 3, n_low + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    block = hop if block == "hop" else block
    D = emspec.latency_columns(n_low, hop, True)
    with _engine(True) as e:
        split = e.split_row_for_hz(250.0)
        got_db, got_rgba = _push_session(e, pcm, (n_low, n_high), hop, (split,), True, block)
        e.reset()
        ref_db, ref_rgba = [], []
        for a in range(0, L, block):
            db, rgba, counts, _ = e.push_samples_multires(pcm, n_low, n_high, hop, split, True, want_rgba=True, count=min(block, L - a), offset=a)
            ref_db.append(db), ref_rgba.append(rgba)
        for i in range(D):
            db, rgba, _ = e.columns_flush(want_rgba=True)
            ref_db.append(db[:, None]), ref_rgba.append(rgba[:, None])
    assert np.array_equal(got_db.view(U), np.concatenate(ref_db, 1).view(U))
    assert np.array_equal(got_rgba, np.concatenate(ref_rgba, 1))


# ---- 4. 64 streams x 200 hops, page-locked against ordinary buffers ----
def test_64_streams_200_hops_pinned_equals_pageable_equals_the_composition():
    (n, hop, hz), S, hops = LADDERS["B"], 64, 200
    L = n[0] + hop * (hops - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n[0], hop, True)
    pin_in = emspec.PinnedArray((S, hop), np.float32)
    pin_db = emspec.PinnedArray((S, 1, R), np.float32)
    pin_rgba = emspec.PinnedArray((S, 1, R, 4), np.uint8)
    got = np.empty((S, hops, R), np.float32)
    got_rgba = np.empty((S, hops, R, 4), np.uint8)
    try:
        with _engine(True) as a, _engine(True) as b:
            split = _split(a, hz)
            # the first n[0] - hop samples complete no frame; then one hop per call
            a.push_samples_multiband(pcm, n, split, hop, True, want_db=False, count=n[0] - hop, offset=0)
            b.push_samples_multiband(pcm, n, split, hop, True, want_db=False, count=n[0] - hop, offset=0)
            nxt = 0
            for j in range(hops):
                off = n[0] - hop + j * hop
                pin_in.array[:] = pcm[:, off:off + hop]
                _, _, c1, f1 = a.push_samples_multiband(pin_in.array, n, split, hop, True, want_rgba=True, db=pin_db.array,
                                                        rgba=pin_rgba.array)
                db2, rgba2, c2, f2 = b.push_samples_multiband(pcm, n, split, hop, True, want_rgba=True, count=hop, offset=off,
                                                              db=np.empty((S, 1, R), np.float32), rgba=np.empty((S, 1, R, 4), np.uint8))
                assert np.array_equal(c1, c2) and np.array_equal(f1, f2)
                assert np.all(c1 == (1 if j >= D else 0))
                if j >= D:
                    assert np.all(f1 == j - D)
                    assert np.array_equal(pin_db.array.view(U), db2.view(U))
                    assert np.array_equal(pin_rgba.array, rgba2)
                    got[:, nxt], got_rgba[:, nxt] = pin_db.array[:, 0], pin_rgba.array[:, 0]
                    nxt += 1
            for i in range(D):
                db1, rgba1, cols1 = a.columns_flush(want_rgba=True)
                db2, rgba2, cols2 = b.columns_flush(want_rgba=True)
                assert np.all(cols1 == nxt) and np.all(cols2 == nxt)
                assert np.array_equal(db1.view(U), db2.view(U)) and np.array_equal(rgba1, rgba2)
                got[:, nxt], got_rgba[:, nxt] = db1, rgba1
                nxt += 1
            assert nxt == hops
    finally:
        for p in (pin_in, pin_db, pin_rgba):
            p.close()
    want = _ref(S, L, n, hop, split, True, True, None)
    _same_db(got, want["db"], True)
    _same_rgba(got_rgba, want["rgba"], True)


# ---- 5. reset_stream mid-session ----
@pytest.mark.parametrize("form", ["frames", "blocks"])
def test_reset_stream_restarts_one_stream_only(form):
    """Stream 1 restarts mid-session: its later columns are the composition of the samples fed after the restart - every band's ring
    was cleared, and its first call re-primes every shorter band while the others run one frame; the other streams never notice."""
    (n, hop, hz), S, hops, K = LADDERS["A"], 3, FRAMES, 37
    L = n[0] + hop * (hops - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n[0], hop, True)
    block, P0 = 1000, 10000                          # blocks form: stream 1 restarts after P0 samples
    a0 = K * hop if form == "frames" else P0
    got = [[] for _ in range(S)]
    with _engine(True) as e:
        split = _split(e, hz)
        if form == "frames":
            for j in range(hops):
                if j == K:
                    e.reset_stream(1)
                db, _, cols = e.columns_multiband(pcm[:, j * hop:j * hop + n[0]], n, split, hop, True)
                for s in range(S):
                    base = K if (s == 1 and j >= K) else 0
                    assert cols[s] == (j - base - D if j - base >= D else -1)
                    if cols[s] >= 0:
                        got[s].append(db[s].copy())
        else:
            for a in range(0, L, block):
                if a == P0:
                    e.reset_stream(1)
                cnt = min(block, L - a)
                db, _, counts, firsts = e.push_samples_multiband(pcm, n, split, hop, True, count=cnt, offset=a)
                for s in range(S):
                    seen = a - P0 if (s == 1 and a >= P0) else a
                    k, first = _expected_counts(seen, cnt, n[0], hop, D)
                    assert counts[s] == k and firsts[s] == (first if k else -1), (a, s)
                    for i in range(k):
                        got[s].append(db[s, i].copy())
        for i in range(D):
            db, _, cols = e.columns_flush()
            assert np.all(cols >= 0)
            for s in range(S):
                got[s].append(db[s].copy())
    full = _ref(S, L, n, hop, split, True, True, None)["db"]
    for s in (0, 2):
        assert np.array_equal(np.stack(got[s]).view(U), full[s].view(U)), s
    before = K - D if form == "frames" else emspec.num_columns(P0, n[0], hop) - D   # columns stream 1 emitted before the reset
    g1 = np.stack(got[1])
    assert np.array_equal(g1[:before].view(U), full[1, :before].view(U))
    restarted = B.compose(pcm[1:2, a0:], n, split, hop, True, exact=True, want=("db",))["db"][0]
    assert np.array_equal(g1[before:].view(U), restarted.view(U))


# ---- 6. display post-process ----
@MODES
def test_display_postprocess_runs_once_over_the_composed_column(exact):
    """EXACT: the bytes of batch_multiband with the same set_display on the same samples.  FAST: the post-process law
    (oracle.postprocess) on the bit model's composed raw dB, with the two-band test's bounds."""
    (n, hop, hz), S = LADDERS["A"], 3
    L = n[0] + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    with _engine(exact) as e:
        split = _split(e, hz)
        e.set_display(0.6, 0.8)
        got_db, got_rgba = _push_session(e, pcm, n, hop, split, True, 3 * hop)
        e.reset()
        batch = e.batch_multiband(pcm, n, split, hop, True, want=("db", "rgba"))
    if exact:
        assert np.array_equal(got_db.view(U), batch["db"].view(U)) and np.array_equal(got_rgba, batch["rgba"])
        return
    raw = _ref(S, L, n, hop, split, True, exact, None)["db"]
    pdb, pidx, _ = O.postprocess(raw, 0.6, 0.8, O.make_cfg(n[0], hop, True))
    err = float(np.max(np.abs(got_db - pdb)))
    print(f"post-process max dB err {err:.2e}")
    assert err < 2e-3, err
    lut = O.default_lut()
    near = (got_rgba == lut[pidx]).all(-1) | (got_rgba == lut[np.minimum(pidx.astype(np.int32) + 1, 255)]).all(-1) | \
        (got_rgba == lut[np.maximum(pidx.astype(np.int32) - 1, 0)]).all(-1)
    assert near.all()   # palette index within one step


def test_display_postprocess_into_an_oversized_pinned_block():
    (n, hop, hz), S, cap = LADDERS["A"], 3, 40
    L = n[0] + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n[0], hop, True)
    pin = emspec.PinnedArray((S, cap, R), np.float32)
    got = np.empty((S, FRAMES, R), np.float32)
    try:
        with _engine(True) as e:
            split = _split(e, hz)
            e.set_display(0.6, 0.8)
            nxt = 0
            for a in range(0, L, 3 * hop):
                cnt = min(3 * hop, L - a)
                pin.array[...] = -1.0
                _, _, counts, _ = e.push_samples_multiband(pcm, n, split, hop, True, db=pin.array, count=cnt, offset=a)
                k = int(counts[0])
                assert np.all(counts == k) and k <= 3
                assert np.all(pin.array[:, k:] == -1.0)          # nothing beyond the completed columns is touched
                got[:, nxt:nxt + k] = pin.array[:, :k]
                nxt += k
            assert nxt == FRAMES - D
            e.reset()
            batch = e.batch_multiband(pcm, n, split, hop, True, want=("db",))["db"]
    finally:
        pin.close()
    assert np.array_equal(got[:, :nxt].view(U), batch[:, :nxt].view(U))


# ---- 7. overlays ----
@MODES
@pytest.mark.parametrize("form", ["frames", "hop", "blocks"])   # in-place launches of one frame; deferred launches; both end in flushes
def test_overlays_follow_the_delivered_columns(form, exact):
    """set_live_peaks(k = 8): byte-equal to peaks_host of the dB the same call delivered; set_live_wave: byte-equal to wave_host of
    the samples on the n[0] grid."""
    (n, hop, hz), S, k, min_db = LADDERS["A"], 3, 8, -60.0
    if form == "frames":
        n, hop, hz = LADDERS["C"]        # (ladder C at one frame per call: every band finalises in place)
    L = n[0] + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n[0], hop, True)
    block = {"frames": hop, "hop": hop, "blocks": 5 * hop}[form]
    cols_max = 8
    pk = np.full((S, cols_max, k, 2), 7.0, np.float32)
    wv = np.full((S, cols_max, 2), 7.0, np.float32)
    dbs, pks, wvs = [], [], []

    def take(db, count, cols, keep=True):
        """the first `count` of the call's `cols` slots were written; the rest must be untouched"""
        p, w = pk.reshape(-1)[:S * cols * k * 2].reshape(S, cols, k, 2), wv.reshape(-1)[:S * cols * 2].reshape(S, cols, 2)
        assert np.all(p[:, count:] == 7.0) and np.all(w[:, count:] == 7.0)
        if count and keep:
            dbs.append(db[:, :count].copy()), pks.append(p[:, :count].copy()), wvs.append(w[:, :count].copy())
        pk[...] = 7.0
        wv[...] = 7.0

    with _engine(exact) as e:
        split = _split(e, hz)
        e.set_live_peaks(k, min_db, pk.reshape(-1))
        e.set_live_wave(wv.reshape(-1))
        if form == "frames":
            for j in range(FRAMES):
                db, _, cols = e.columns_multiband(pcm[:, j * hop:j * hop + n[0]], n, split, hop, True)
                take(db[:, None], 1, 1, keep=j >= D)     # (the per-frame form always writes its slot: the empty column's too)
        else:
            for a in range(0, L, block):
                db, _, counts, _ = e.push_samples_multiband(pcm, n, split, hop, True, count=min(block, L - a), offset=a)
                assert db.shape[1] <= cols_max
                take(db, int(counts[0]), db.shape[1])
        for i in range(D):
            db, _, cols = e.columns_flush()
            take(db[:, None], 1, 1)
        e.set_live_peaks(1, 0.0, None)
        e.set_live_wave(None)
    db, p, w = np.concatenate(dbs, 1), np.concatenate(pks, 1), np.concatenate(wvs, 1)
    assert db.shape[1] == FRAMES
    assert np.array_equal(p.view(U), np.ascontiguousarray(emspec.peaks_host(db, k, min_db), np.float32).reshape(p.shape).view(U))
    assert np.array_equal(w.view(U), np.ascontiguousarray(emspec.wave_host(pcm, n[0], hop), np.float32).reshape(w.shape).view(U))
    _same_db(db, _ref(S, L, n, hop, split, True, exact, None)["db"], exact)


# ---- 8. PCM ----
def test_pcm_session_equals_the_float_session():
    """2 stereo s16 sources -> L R M S = 8 streams, EXACT: the bytes of the float push of the decoded views (tests/pcm_ref.py)."""
    (n, hop, hz), sources = LADDERS["A"], 2
    total = n[0] + hop * (FRAMES - 1)
    t = np.arange(total)
    x = np.stack([np.stack([0.35 * np.sin(2 * np.pi * 110.0 * (1 + s) * (1 + 0.5 * c) * t / 48000.0 + s) +
                            0.1 * np.sin(2 * np.pi * (3000 + 40 * s) * (1 + c) * t / 48000.0) for c in range(2)], -1) for s in range(sources)])
    raw = np.round(x.reshape(sources, -1) * 32767).astype("<i2")
    fmt = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
    pcm = P.decode(raw.view(np.uint8).reshape(sources, -1), P.S16, 2, fmt.matrix)
    assert pcm.shape == (8, total)
    with _engine(True) as e:
        split = _split(e, hz)
        want = _push_session(e, pcm, n, hop, split, True, 1000)
        e.reset()
        got = _push_session(e, pcm, n, hop, split, True, 1000,
                            feed=lambda cnt, off: e.push_samples_pcm(raw, fmt, n, hop, True, split_rows=split, want_rgba=True, count=cnt,
                                                                     offset=off))
        assert e.live_streams == 8
    assert np.array_equal(got[0].view(U), want[0].view(U)) and np.array_equal(got[1], want[1])


# ---- 9. rejections and guards ----
@pytest.mark.parametrize("n,hop,split,rule", [
    ((4096,), 256, (), "bands must be in 2..4"),
    ((16384, 8192, 4096, 2048, 1024), 256, (100, 200, 300, 400), "bands must be in 2..4"),
    ((4096, 512), 256, (368,), "every fft size must be"),
    ((2048, 4096), 256, (368,), "strictly decreasing"),
    ((4096, 2048, 1024), 2048, (368, 668), "hop must be in"),
    ((4096, 2048, 1024), 1000, (368, 668), "must be an integer"),
    ((4096, 2048, 1024), 256, (366, 668), "multiple of 4"),
    ((4096, 2048, 1024), 256, (668, 368), "strictly increasing"),
    ((4096, 2048, 1024), 256, (60, 668), "at least 64 rows"),
    ((4096, 2048, 1024), 256, (368, 964), "at least 64 rows"),
])
def test_rejections_name_the_rule_and_leave_the_engine_usable(n, hop, split, rule):
    pcm = _pcm(2, 4096 + 256 * 40)
    with _engine(True) as e:
        with pytest.raises(emspec.EmspecError) as ei:
            e.columns_multiband(pcm[:, :n[0]], n, split, hop, True)
        assert ei.value.code == emspec.ERR_INVALID_ARG and rule in str(ei.value), str(ei.value)
        with pytest.raises(emspec.EmspecError) as ei:
            e.push_samples_multiband(pcm[:, :4096], n, split, hop, True)
        assert ei.value.code == emspec.ERR_INVALID_ARG and rule in str(ei.value), str(ei.value)
        shape_rule = emspec.multiband_columns(1 << 20, n, hop) < 0   # (a split rule: the shape itself is accepted)
        assert (e.push_columns_multiband(4096, n, hop, True) == -1) == shape_rule
        assert e.live_streams == 0                                    # nothing was fed
        got, _ = _push_session(e, pcm, (4096, 2048, 1024), 256, (368, 668), True, 2048, want_rgba=False)
    want = _ref(2, 4096 + 256 * 40, (4096, 2048, 1024), 256, (368, 668), True, True, None)["db"]
    assert np.array_equal(got.view(U), want.view(U))


def test_session_guards():
    (n, hop, hz), S = LADDERS["A"], 2
    L = n[0] + hop * 40
    pcm = _pcm(S, L)
    fr = pcm[:, :n[0]]

    def refused(code, fn):
        with pytest.raises(emspec.EmspecError) as ei:
            fn()
        assert ei.value.code == code, str(ei.value)

    with _engine(True) as e:
        split = _split(e, hz)
        s2 = e.split_row_for_hz(250.0)
        # max_columns too small, outputs or not, display on or off: rejected before anything is fed
        for display in ((0.6, 0.8), (0.0, 0.0)):
            e.set_display(*display)
            refused(emspec.ERR_INVALID_ARG, lambda: e.push_samples_multiband(pcm, n, split, hop, True, want_db=False, max_columns=0))
            refused(emspec.ERR_INVALID_ARG, lambda: e.push_samples_multiband(pcm, n, split, hop, True, db=np.empty((S, 2, R), np.float32)))
            assert e.live_streams == 0
        # a multi-band call on a single-resolution or a two-band session
        e.columns(pcm[:, :4096], hop, True)
        refused(emspec.ERR_STATE, lambda: e.columns_multiband(fr, n, split, hop, True))
        refused(emspec.ERR_STATE, lambda: e.push_samples_multiband(pcm[:, :512], n, split, hop, True))
        e.reset()
        e.columns_multires(pcm[:, :8192], 2048, hop, s2, True)
        refused(emspec.ERR_STATE, lambda: e.columns_multiband(pcm[:, :8192], (8192, 2048), (s2,), hop, True))
        e.reset()
        # the reverse, and any change, on a multi-band session
        e.columns_multiband(fr, n, split, hop, True)
        for bad in (lambda: e.columns(fr, hop, True),
                    lambda: e.push_samples_multi(pcm[:, :512], n[0], hop, True),
                    lambda: e.columns_multires(pcm[:, :8192], 2048, hop, s2, True),
                    lambda: e.push_samples_multires(pcm[:, :512], 8192, 2048, hop, s2, True),
                    lambda: e.columns_multiband(fr, n[:2], split[:1], hop, True),                  # other band count
                    lambda: e.columns_multiband(fr, (4096, 2048, 1024)[:1] + (1024,), split[:1], hop, True),
                    lambda: e.columns_multiband(pcm[:, :8192], (8192, 2048, 1024), split, hop, True),   # other n[0]
                    lambda: e.columns_multiband(fr, n, split, 128, True),                          # other hop
                    lambda: e.columns_multiband(fr, n, (split[0] + 4, split[1]), hop, True),       # other split rows
                    lambda: e.columns_multiband(fr, n, (split[0], split[1] - 4), hop, True),
                    lambda: e.columns_multiband(fr, n, split, hop, False),                         # other reassign
                    lambda: e.columns_multiband(fr[:1], n, split, hop, True),                      # other stream count
                    lambda: e.push_samples_multiband(pcm[:, :512], n, split, hop, True)):          # other feeding form
            refused(emspec.ERR_STATE, bad)
        db, _, cols = e.columns_multiband(pcm[:, hop:hop + n[0]], n, split, hop, True)   # the session itself goes on
        assert np.all(cols == -1)
        e.reset()
        # while a time reduction is set
        e.set_time_reduce(4)
        refused(emspec.ERR_STATE, lambda: e.columns_multiband(fr, n, split, hop, True))
        refused(emspec.ERR_STATE, lambda: e.push_samples_multiband(pcm[:, :512], n, split, hop, True))
        e.set_time_reduce(1)
        got, _ = _push_session(e, pcm, n, hop, split, True, 777, want_rgba=False)
    want = _ref(S, L, n, hop, split, True, True, None)["db"]
    assert np.array_equal(got.view(U), want.view(U))


# ---- 10. a long session against the engine's own batch ----
def test_long_session_equals_the_device_batch_bytes():
    """2 streams x 2,000 hops, one hop per call, EXACT: the bytes of emspec_batch_multiband_device on the same engine (every ring
    wraps many times)."""
    import torch
    (n, hop, hz), S, hops = LADDERS["A"], 2, 2000
    L = n[0] + hop * (hops - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n[0], hop, True)
    got = np.empty((S, hops, R), np.float32)
    got_rgba = np.empty((S, hops, R, 4), np.uint8)
    db1, rgba1 = np.empty((S, 1, R), np.float32), np.empty((S, 1, R, 4), np.uint8)
    with _engine(True) as e:
        split = _split(e, hz)
        e.push_samples_multiband(pcm, n, split, hop, True, want_db=False, count=n[0] - hop, offset=0)
        nxt = 0
        for j in range(hops):
            _, _, counts, firsts = e.push_samples_multiband(pcm, n, split, hop, True, db=db1, rgba=rgba1, count=hop,
                                                            offset=n[0] - hop + j * hop)
            if j >= D:
                assert np.all(counts == 1) and np.all(firsts == nxt)
                got[:, nxt], got_rgba[:, nxt] = db1[:, 0], rgba1[:, 0]
                nxt += 1
        for i in range(D):
            db, rgba, cols = e.columns_flush(want_rgba=True)
            got[:, nxt], got_rgba[:, nxt] = db, rgba
            nxt += 1
        assert nxt == hops
        e.reset()
        x = torch.from_numpy(np.array(pcm, np.float32)).cuda()
        tdb = torch.empty((S, hops, R), dtype=torch.float32, device="cuda")
        trgba = torch.empty((S, hops, R, 4), dtype=torch.uint8, device="cuda")
        e.batch_multiband_device(x, n, split, hop, True, db=tdb, rgba=trgba)
        torch.cuda.synchronize()
        e.device_status()
        want_db, want_rgba = tdb.cpu().numpy(), trgba.cpu().numpy()
    assert np.array_equal(got.view(U), want_db.view(U))
    assert np.array_equal(got_rgba, want_rgba)


# ---- 11. one engine, one session kind after another ----
def test_session_kinds_in_turn_on_one_engine():
    """A single-resolution live session, a two-band one and a multi-band one, each after reset(), then the first two again: the
    bytes of fresh engines (the rings and counters the kinds share are sized and cleared per session)."""
    hop, S, hops = 256, 2, 60
    L = 16384 + hop * (hops - 1)
    pcm = _pcm(S, L)
    n3, hz = LADDERS["B"][0], LADDERS["B"][2]

    def single(e):
        return [e.push_samples_multi(pcm, 4096, hop, True, count=c, offset=a)[0] for a, c in ((0, 9000), (9000, L - 9000))]

    def two(e):
        s = e.split_row_for_hz(250.0)
        return [e.push_samples_multires(pcm, 16384, 4096, hop, s, True, count=c, offset=a)[0] for a, c in ((0, 17000), (17000, L - 17000))]

    splits = []

    def three(e):
        splits.append(_split(e, hz))
        return [e.push_samples_multiband(pcm, n3, _split(e, hz), hop, True, count=c, offset=a)[0] for a, c in ((0, 17000), (17000, L - 17000))]

    fresh = []
    for kind in (single, two, three):
        with _engine(True) as e:
            fresh.append(kind(e))
    with _engine(True) as e:
        runs = []
        for kind in (single, two, three, single, two):
            runs.append(kind(e))
            e.reset()
    for got, want in zip(runs, fresh + fresh[:2]):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a.view(U), b.view(U))
    want = _ref(S, L, n3, hop, splits[0], True, True, None)["db"]
    D = emspec.latency_columns(n3[0], hop, True)
    assert np.array_equal(np.concatenate(runs[2], 1).view(U), want[:, :hops - D].view(U))


# ---- 12. Node ----
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_push_samples_multiband_matches_ctypes(tmp_path):
    """engine.pushSamplesMultiband on 4 streams (js/test_live_multiband.js, EXACT engine) returns the ctypes calls' bytes."""
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_live_multiband.js", str(tmp_path)], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    S, L, J = res["S"], res["L"], res["columns"]
    pcm = np.fromfile(str(tmp_path / "pcm.f32"), np.float32).reshape(S, L)
    node_db = np.fromfile(str(tmp_path / "db.f32"), np.float32).reshape(S, J, R)
    node_rgba = np.fromfile(str(tmp_path / "rgba.u8"), np.uint8).reshape(S, J, R, 4)
    with _engine(True) as e:
        split = _split(e, res["splitHz"])
        assert list(split) == res["splitRows"]
        got_db, got_rgba = _push_session(e, pcm, tuple(res["fftSizes"]), res["hop"], split, True, res["block"])
    assert J == got_db.shape[1]
    assert np.array_equal(got_db.view(U), node_db.view(U))
    assert np.array_equal(got_rgba, node_rgba)
