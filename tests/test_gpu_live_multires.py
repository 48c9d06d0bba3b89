"""GPU: the live multi-resolution session (include/emspec.h: emspec_columns_multires, emspec_push_samples_multires,
emspec_push_columns_multires) - the multi-resolution image column by column while the audio arrives.
Every comparison is against the definition, tests/multires_ref.py: compose(...) on the CPU bit model (EXACT: equal bytes;
FAST: the live tests' tolerances, sums in arrival order), never against the engine's own batch call - except the long
session at the end, a self-consistency check on top of the others.
"""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec
import multires_ref as M
import oracle as O
from emspec import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_DB = 8.7e-4          # FAST dB (tests/test_gpu_live.py)
RGBA_SHARE = 1e-3        # FAST: share of RGBA bytes that may differ (tests/test_gpu_live.py)
BOOST = 2.0              # the warped axis of tests/test_gpu_multires.py: moves the 250 Hz split row
R = 1024


def _engine(exact, boost=None):
    e = emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST)
    edges = None
    if boost is not None:
        edges = emspec.warped_edges_hz(e.rows, 20.0, 24000.0, boost)
        e.set_row_edges_hz(edges)
    return e, edges


@functools.lru_cache(maxsize=None)
def _pcm(S, L):
    return synth.streams(S, L)


@functools.lru_cache(maxsize=None)
def _ref(S, L, n_low, n_high, hop, split, reassign, exact, boost):
    """compose() of _pcm(S, L): db and rgba."""
    edges = None if boost is None else emspec.warped_edges_hz(R, 20.0, 24000.0, boost)
    return M.compose(_pcm(S, L), n_low, n_high, hop, split, reassign, exact=exact, edges_hz=edges, want=("db", "rgba"))


def _same_db(got, want, exact):
    assert got.shape == want.shape, (got.shape, want.shape)
    if exact:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
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


def _expected_counts(seen_before, count, n_low, hop, D):
    """Columns a block of `count` samples completes for a stream that had `seen_before` samples: from emspec_num_columns."""
    before = max(emspec.num_columns(seen_before, n_low, hop) - D, 0)
    after = max(emspec.num_columns(seen_before + count, n_low, hop) - D, 0)
    return after - before, before


def _push_session(e, pcm, n_low, n_high, hop, split, reassign, block, want_rgba=True, a0=0):
    """Feeds pcm[:, a0:] in blocks, flushes; returns (db [S][J][R], rgba) and checks counts / first columns / prediction."""
    S, L = pcm.shape[0], pcm.shape[1] - a0
    J = emspec.multires_columns(L, n_low, n_high, hop)
    D = emspec.latency_columns(n_low, hop, reassign)
    got_db = np.empty((S, J, R), np.float32)
    got_rgba = np.empty((S, J, R, 4), np.uint8)
    nxt = 0
    for a in range(0, L, block):
        cnt = min(block, L - a)
        want_k, want_first = _expected_counts(a, cnt, n_low, hop, D)
        k = e.push_columns_multires(cnt, n_low, n_high, hop, reassign)
        assert k == want_k, (a, k, want_k)
        db, rgba, counts, firsts = e.push_samples_multires(pcm, n_low, n_high, hop, split, reassign, want_rgba=want_rgba,
                                                           count=cnt, offset=a0 + a)
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
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_per_frame_form_equals_the_composition(exact):
    S, L, n_low, n_high, hop = 4, 1 << 17, 16384, 4096, 256
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n_low, hop, True)
    J = emspec.multires_columns(L, n_low, n_high, hop)
    assert J == emspec.num_columns(L, n_low, hop)
    got_db = np.empty((S, J, R), np.float32)
    got_rgba = np.empty((S, J, R, 4), np.uint8)
    with _engine(exact)[0] as e:
        split = e.split_row_for_hz(250.0)
        for j in range(J):
            db, rgba, cols = e.columns_multires(pcm[:, j * hop:j * hop + n_low], n_high, hop, split, True, want_rgba=True)
            assert e.live_streams == S
            assert np.all(cols == (j - D if j >= D else -1))
            if j >= D:
                got_db[:, j - D], got_rgba[:, j - D] = db, rgba
            else:   # the empty column: constant dB, constant RGBA - both bands wrote their part
                assert np.all(db == db[0, 0]) and np.all(rgba == rgba[0, 0])
        for i in range(D):
            db, rgba, cols = e.columns_flush(want_rgba=True)
            assert np.all(cols == J - D + i)
            got_db[:, J - D + i], got_rgba[:, J - D + i] = db, rgba
        with pytest.raises(emspec.EmspecError) as ei:
            e.columns_flush()
        assert ei.value.code == emspec.ERR_STATE
        with pytest.raises(emspec.EmspecError) as ei:   # a flushed stream is at its end
            e.columns_multires(pcm[:, :n_low], n_high, hop, split, True)
        assert ei.value.code == emspec.ERR_STATE
    want = _ref(S, L, n_low, n_high, hop, split, True, exact, None)
    _same_db(got_db, want["db"], exact)
    _same_rgba(got_rgba, want["rgba"], exact)


# ---- 2. sample-block form ----
SHAPES = [(16384, 4096, 256), (8192, 2048, 128), (16384, 1024, 512)]   # (the last: a small transform defers its finalize)
FRAMES = 120


def _block_case(n_low, n_high, hop, block, reassign, exact, boost):
    S, L = 3, n_low + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    e, _ = _engine(exact, boost)
    with e:
        split = e.split_row_for_hz(250.0)
        got_db, got_rgba = _push_session(e, pcm, n_low, n_high, hop, split, reassign, block)
    want = _ref(S, L, n_low, n_high, hop, split, reassign, exact, boost)
    _same_db(got_db, want["db"], exact)
    _same_rgba(got_rgba, want["rgba"], exact)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("block", [128, "hop", 1000, 20000])
@pytest.mark.parametrize("n_low,n_high,hop", SHAPES)
def test_sample_blocks_equal_the_composition(n_low, n_high, hop, block, exact):
    _block_case(n_low, n_high, hop, hop if block == "hop" else block, True, exact, None)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("block", [256, 1000])
def test_sample_blocks_without_reassignment(block, exact):
    _block_case(16384, 4096, 256, block, False, exact, None)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("n_low,n_high,hop", SHAPES[:2])
def test_sample_blocks_on_the_warped_axis(n_low, n_high, hop, exact):
    _block_case(n_low, n_high, hop, 1000, True, exact, BOOST)


# ---- 3. 64 streams x 200 hops, page-locked against ordinary buffers ----
def test_64_streams_200_hops_pinned_equals_pageable_equals_the_composition():
    S, n_low, n_high, hop, hops = 64, 16384, 4096, 256, 200
    L = n_low + hop * (hops - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n_low, hop, True)
    pin_in = emspec.PinnedArray((S, hop), np.float32)
    pin_db = emspec.PinnedArray((S, 1, R), np.float32)
    pin_rgba = emspec.PinnedArray((S, 1, R, 4), np.uint8)
    got = np.empty((S, hops, R), np.float32)
    got_rgba = np.empty((S, hops, R, 4), np.uint8)
    try:
        with emspec.Engine(mode=emspec.MODE_EXACT) as a, emspec.Engine(mode=emspec.MODE_EXACT) as b:
            split = a.split_row_for_hz(250.0)
            # the first n_low - hop samples complete no frame; then one hop per call
            a.push_samples_multires(pcm, n_low, n_high, hop, split, True, want_db=False, count=n_low - hop, offset=0)
            b.push_samples_multires(pcm, n_low, n_high, hop, split, True, want_db=False, count=n_low - hop, offset=0)
            nxt = 0
            for j in range(hops):
                off = n_low - hop + j * hop
                pin_in.array[:] = pcm[:, off:off + hop]
                _, _, c1, f1 = a.push_samples_multires(pin_in.array, n_low, n_high, hop, split, True, want_rgba=True,
                                                       db=pin_db.array, rgba=pin_rgba.array)
                db2, rgba2, c2, f2 = b.push_samples_multires(pcm, n_low, n_high, hop, split, True, want_rgba=True, count=hop,
                                                             offset=off, db=np.empty((S, 1, R), np.float32),
                                                             rgba=np.empty((S, 1, R, 4), np.uint8))
                assert np.array_equal(c1, c2) and np.array_equal(f1, f2)
                assert np.all(c1 == (1 if j >= D else 0))
                if j >= D:
                    assert np.all(f1 == j - D)
                    assert np.array_equal(pin_db.array.view(np.uint32), db2.view(np.uint32))
                    assert np.array_equal(pin_rgba.array, rgba2)
                    got[:, nxt], got_rgba[:, nxt] = pin_db.array[:, 0], pin_rgba.array[:, 0]
                    nxt += 1
            for i in range(D):
                db1, rgba1, cols1 = a.columns_flush(want_rgba=True)
                db2, rgba2, cols2 = b.columns_flush(want_rgba=True)
                assert np.all(cols1 == nxt) and np.all(cols2 == nxt)
                assert np.array_equal(db1.view(np.uint32), db2.view(np.uint32)) and np.array_equal(rgba1, rgba2)
                got[:, nxt], got_rgba[:, nxt] = db1, rgba1
                nxt += 1
            assert nxt == hops
    finally:
        for p in (pin_in, pin_db, pin_rgba):
            p.close()
    want = _ref(S, L, n_low, n_high, hop, split, True, True, None)
    _same_db(got, want["db"], True)
    _same_rgba(got_rgba, want["rgba"], True)


# ---- 4. reset_stream mid-session ----
@pytest.mark.parametrize("form", ["frames", "blocks"])
def test_reset_stream_restarts_one_stream_only(form):
    """Stream 1 restarts after K hops: its later columns are the composition of the samples fed after the restart (its first
    call re-primes the short band's 2 shift + 1 frames while the others run one); the other streams never notice."""
    S, n_low, n_high, hop, hops, K = 3, 16384, 4096, 256, 200, 37
    L = n_low + hop * (hops - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n_low, hop, True)
    block, P = 1000, 30000                          # blocks form: stream 1 restarts after P samples
    a0 = K * hop if form == "frames" else P         # stream 1's signal after the restart is pcm[1, a0:]
    got = [[] for _ in range(S)]
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        split = e.split_row_for_hz(250.0)
        if form == "frames":
            for j in range(hops):
                if j == K:
                    e.reset_stream(1)
                db, _, cols = e.columns_multires(pcm[:, j * hop:j * hop + n_low], n_high, hop, split, True)
                for s in range(S):
                    base = K if (s == 1 and j >= K) else 0
                    assert cols[s] == (j - base - D if j - base >= D else -1)
                    if cols[s] >= 0:
                        got[s].append(db[s].copy())
            for i in range(D):
                db, _, cols = e.columns_flush()
                for s in range(S):
                    got[s].append(db[s].copy())
        else:
            # every stream goes on receiving its row of pcm; stream 1 is reset after P samples, so what it receives from
            # then on, pcm[1, P:], is a new signal on a sample clock of its own
            for a in range(0, L, block):
                if a == P:
                    e.reset_stream(1)
                cnt = min(block, L - a)
                db, _, counts, firsts = e.push_samples_multires(pcm, n_low, n_high, hop, split, True, count=cnt, offset=a)
                for s in range(S):
                    seen = a - P if (s == 1 and a >= P) else a
                    k, first = _expected_counts(seen, cnt, n_low, hop, D)
                    assert counts[s] == k and firsts[s] == (first if k else -1), (a, s)
                    for i in range(k):
                        got[s].append(db[s, i].copy())
            for i in range(D):
                db, _, cols = e.columns_flush()
                assert np.all(cols >= 0)
                for s in range(S):
                    got[s].append(db[s].copy())
    full = _ref(S, L, n_low, n_high, hop, split, True, True, None)["db"]
    for s in (0, 2):
        assert np.array_equal(np.stack(got[s]).view(np.uint32), full[s].view(np.uint32)), s
    before = K - D if form == "frames" else emspec.num_columns(P, n_low, hop) - D   # columns stream 1 emitted before the reset
    g1 = np.stack(got[1])
    assert np.array_equal(g1[:before].view(np.uint32), full[1, :before].view(np.uint32))
    restarted = M.compose(pcm[1:2, a0:], n_low, n_high, hop, split, True, exact=True, want=("db",))["db"][0]
    assert np.array_equal(g1[before:].view(np.uint32), restarted.view(np.uint32))


# ---- 5. display post-process ----
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_display_postprocess_runs_once_over_the_composed_column(exact):
    S, n_low, n_high, hop = 3, 16384, 4096, 256
    L = n_low + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    with _engine(exact)[0] as e:
        split = e.split_row_for_hz(250.0)
        e.set_display(0.6, 0.8)
        got_db, got_rgba = _push_session(e, pcm, n_low, n_high, hop, split, True, 3 * hop)
    raw = _ref(S, L, n_low, n_high, hop, split, True, exact, None)["db"]
    pdb, pidx, _ = O.postprocess(raw, 0.6, 0.8, O.make_cfg(n_low, hop, True))
    err = float(np.max(np.abs(got_db - pdb)))
    print(f"post-process max dB err {err:.2e}")
    assert err < 2e-3, err
    lut = O.default_lut()
    near = (got_rgba == lut[pidx]).all(-1) | (got_rgba == lut[np.minimum(pidx.astype(np.int32) + 1, 255)]).all(-1) | \
        (got_rgba == lut[np.maximum(pidx.astype(np.int32) - 1, 0)]).all(-1)
    assert near.all()   # palette index within one step


def test_display_postprocess_into_an_oversized_pinned_block():
    S, n_low, n_high, hop, cap = 3, 16384, 4096, 256, 40
    L = n_low + hop * (FRAMES - 1)
    pcm = _pcm(S, L)
    D = emspec.latency_columns(n_low, hop, True)
    pin = emspec.PinnedArray((S, cap, R), np.float32)
    got = np.empty((S, FRAMES, R), np.float32)
    try:
        with emspec.Engine() as e:
            split = e.split_row_for_hz(250.0)
            e.set_display(0.6, 0.8)
            nxt = 0
            for a in range(0, L, 3 * hop):
                cnt = min(3 * hop, L - a)
                pin.array[...] = -1.0
                _, _, counts, _ = e.push_samples_multires(pcm, n_low, n_high, hop, split, True, db=pin.array, count=cnt, offset=a)
                k = int(counts[0])
                assert np.all(counts == k) and k <= 3
                assert np.all(pin.array[:, k:] == -1.0)          # nothing beyond the completed columns is touched
                got[:, nxt:nxt + k] = pin.array[:, :k]
                nxt += k
            assert nxt == FRAMES - D
    finally:
        pin.close()
    raw = _ref(S, L, n_low, n_high, hop, split, True, False, None)["db"]
    pdb = O.postprocess(raw, 0.6, 0.8, O.make_cfg(n_low, hop, True))[0]
    assert np.max(np.abs(got[:, :nxt] - pdb[:, :nxt])) < 2e-3


# ---- 6. guards ----
@pytest.mark.parametrize("args,rule", [
    ((16384, 2048, 1000, 368), "integer"),
    ((4096, 2048, 256, 368), "n_low"),
    ((16384, 16384, 256, 368), "n_high"),
    ((16384, 8192, 256, 368), "n_high"),
    ((16384, 4096, 256, 366), "split_row"),
    ((16384, 4096, 256, 60), "split_row"),
    ((16384, 4096, 256, 964), "split_row"),
])
def test_rejections_name_the_rule_and_leave_the_engine_usable(args, rule):
    n_low, n_high, hop, split = args
    pcm = _pcm(2, 16384 + 256 * 40)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        with pytest.raises(emspec.EmspecError) as ei:
            e.columns_multires(pcm[:, :n_low], n_high, hop, split, True)
        assert ei.value.code == emspec.ERR_INVALID_ARG and rule in str(ei.value), str(ei.value)
        with pytest.raises(emspec.EmspecError) as ei:
            e.push_samples_multires(pcm[:, :4096], n_low, n_high, hop, split, True)
        assert ei.value.code == emspec.ERR_INVALID_ARG and rule in str(ei.value), str(ei.value)
        assert e.live_streams == 0
        got, _ = _push_session(e, pcm, 16384, 4096, 256, 368, True, 2048, want_rgba=False)
    want = _ref(2, 16384 + 256 * 40, 16384, 4096, 256, 368, True, True, None)["db"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_session_guards():
    S, n_low, n_high, hop, split = 2, 16384, 4096, 256, 368
    pcm = _pcm(S, n_low + hop * 40)
    fr = pcm[:, :n_low]
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        fresh_cols = [e.columns(pcm[:, j * hop:j * hop + 4096], hop, True)[0].copy() for j in range(20)]
        fresh_batch = e.batch(pcm, 4096, hop, True, want=("db", "index"))
        e.reset()
        # a multi-resolution call on a single-resolution session
        e.columns(pcm[:, :4096], hop, True)
        for bad in (lambda: e.columns_multires(fr, n_high, hop, split, True),
                    lambda: e.push_samples_multires(pcm[:, :512], n_low, n_high, hop, split, True)):
            with pytest.raises(emspec.EmspecError) as ei:
                bad()
            assert ei.value.code == emspec.ERR_STATE
        e.reset()
        # a single-resolution call, or any change, on a multi-resolution session
        e.columns_multires(fr, n_high, hop, split, True)
        for bad in (lambda: e.columns(fr, hop, True),
                    lambda: e.columns(pcm[:, :4096], hop, True),
                    lambda: e.push_samples_multi(pcm[:, :512], n_low, hop, True),
                    lambda: e.columns_multires(fr, 2048, hop, split, True),              # other n_high
                    lambda: e.columns_multires(pcm[:, :8192], n_high, hop, split, True),  # other n_low
                    lambda: e.columns_multires(fr, n_high, 512, split, True),            # other hop
                    lambda: e.columns_multires(fr, n_high, hop, split + 4, True),        # other split row
                    lambda: e.columns_multires(fr, n_high, hop, split, False),           # other reassign
                    lambda: e.columns_multires(fr[:1], n_high, hop, split, True),        # other stream count
                    lambda: e.push_samples_multires(pcm[:, :512], n_low, n_high, hop, split, True)):   # other feeding form
            with pytest.raises(emspec.EmspecError) as ei:
                bad()
            assert ei.value.code == emspec.ERR_STATE
        with pytest.raises(emspec.EmspecError) as ei:        # the row table is pinned while columns are pending
            e.set_row_edges_hz(emspec.warped_edges_hz(e.rows, 20.0, 24000.0, BOOST))
        assert ei.value.code == emspec.ERR_STATE
        db, _, cols = e.columns_multires(pcm[:, hop:hop + n_low], n_high, hop, split, True)   # the session itself goes on
        assert np.all(cols == -1)
        e.reset()
        # NULL outputs, no room for the columns the block completes, post-process on: rejected before any state changes
        e.set_display(0.6, 0.8)
        with pytest.raises(emspec.EmspecError) as ei:
            e.push_samples_multires(pcm, n_low, n_high, hop, split, True, want_db=False, max_columns=0)
        assert ei.value.code == emspec.ERR_INVALID_ARG
        assert e.live_streams == 0
        e.set_display(0.0, 0.0)
        with pytest.raises(emspec.EmspecError) as ei:        # ... and with the post-process off as well
            e.push_samples_multires(pcm, n_low, n_high, hop, split, True, want_db=False, max_columns=0)
        assert ei.value.code == emspec.ERR_INVALID_ARG
        assert e.live_streams == 0
        got, _ = _push_session(e, pcm, n_low, n_high, hop, split, True, 777, want_rgba=False)
        # after a multi-resolution session and reset(): the single-resolution session and the batch, byte for byte
        e.reset()
        again_cols = [e.columns(pcm[:, j * hop:j * hop + 4096], hop, True)[0].copy() for j in range(20)]
        again_batch = e.batch(pcm, 4096, hop, True, want=("db", "index"))
    want = _ref(S, n_low + hop * 40, n_low, n_high, hop, split, True, True, None)["db"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for x, y in zip(fresh_cols, again_cols):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(fresh_batch["db"].view(np.uint32), again_batch["db"].view(np.uint32))
    assert np.array_equal(fresh_batch["index"], again_batch["index"])


# ---- 7. a long session against the engine's own batch ----
def test_long_session_equals_the_batch_bytes():
    """2 streams x 4,000 hops by sample blocks, EXACT: the bytes of emspec_batch_multires on the same engine (the ring slots
    wrap hundreds of times).  On top of the bit-model tests above, not instead of them."""
    S, n_low, n_high, hop, hops = 2, 16384, 4096, 256, 4000
    L = n_low + hop * (hops - 1)
    pcm = _pcm(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        split = e.split_row_for_hz(250.0)
        got_db, got_rgba = _push_session(e, pcm, n_low, n_high, hop, split, True, 3000)
        e.reset()
        want = e.batch_multires(pcm, n_low, n_high, hop, split, True, want=("db", "rgba"))
    assert np.array_equal(got_db.view(np.uint32), want["db"].view(np.uint32))
    assert np.array_equal(got_rgba, want["rgba"])


# ---- 8. Node ----
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_push_samples_multires_matches_ctypes(tmp_path):
    """engine.pushSamplesMultires on 4 streams (js/test_live_multires.js, EXACT engine) returns the ctypes calls' bytes."""
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_live_multires.js", str(tmp_path)], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    S, L, J = res["S"], res["L"], res["columns"]
    pcm = np.fromfile(str(tmp_path / "pcm.f32"), np.float32).reshape(S, L)
    node_db = np.fromfile(str(tmp_path / "db.f32"), np.float32).reshape(S, J, R)
    node_rgba = np.fromfile(str(tmp_path / "rgba.u8"), np.uint8).reshape(S, J, R, 4)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        split = e.split_row_for_hz(res["splitHz"])
        assert split == res["splitRow"]
        got_db, got_rgba = _push_session(e, pcm, res["lowFftSize"], res["fftSize"], res["hop"], split, True, res["block"])
    assert J == got_db.shape[1]
    assert np.array_equal(got_db.view(np.uint32), node_db.view(np.uint32))
    assert np.array_equal(got_rgba, node_rgba)
