"""GPU: the stereo image (include/emspec.h: emspec_stereo_device, emspec_batch_stereo_device, emspec_batch_pcm_stereo,
emspec_history_view_stereo*), in FAST and in EXACT mode.

Wherever the test holds the dB bytes an image is made of - emspec_stereo_device on an array it uploads, the history views of
columns the session delivered - every output is compared byte for byte with the host twin emspec_stereo_host and the numpy
restatement tests/stereo_ref.py (which tests/test_stereo_cpu.py holds against each other on the CPU).  The batch entries make
their image of dB that never leaves the engine; the reference is then the image of the dB a second call (emspec_batch_device)
delivers.  EXACT mode is reproducible, so that comparison is on bytes too.  FAST mode sums in arrival order and its dB differs
from call to call within twice the project's bound against the float32 bit model (tests/test_gpu_live_overlay.py: 2 x 8.7e-4 dB
raw, 4 x with the display post-process): there the delivered level must lie within that bound of the other call's, index and
balance must be equal except on cells that bound can move across a step of the law (at most one step then) or across the gate,
and what is a function of delivered bytes - the index of the delivered level, RGBA of the delivered balance and index - is
still exact.

Shapes: FFT 1024 / hop 256, rows 64 and 68, 27 frames, two stereo S16 sources decoded to L R M S (stereo_ref.raw_signal);
1,700 cells = 425 quads where the compose kernel's last workgroup is ragged."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import chunk_ref as K
import emspec
import overview_ref as V
import post_ref as P
import stereo_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
N, HOP, FRAMES = T.N, T.HOP, T.FRAMES
MODES = pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
ALL = ("level", "index", "pan", "rgba")
MAPS = (T.DEFAULT_MAP, T.VIEW_MAP)
TOL_DB = 8.7e-4                               # the project's FAST-mode bound against the float32 bit model (tests/test_gpu_live.py)
DISPLAY = (0.6, 0.8)
LRMS = ["left", "right", "mid", "side"]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """(tests/conftest.py: torch's HIP runtime is initialised before the first engine is created)"""
    if torch.cuda.is_available():
        torch.cuda.init()


def _engine(exact, rows=64, **kw):
    return emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST, rows=rows, **kw)


def _np(out):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _equal(got, want, what):
    for k in ALL:
        if got.get(k) is None:
            continue
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k]).reshape(got[k].shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k, int(np.count_nonzero(g.view(np.uint8) != w.view(np.uint8))))


def _batch_db(e, x):
    db = torch.empty((x.shape[0], emspec.num_columns(x.shape[1], N, HOP), e.rows), dtype=torch.float32, device="cuda")
    e.batch_device(x, N, HOP, True, db=db)
    torch.cuda.synchronize()
    return db


def _refused(code, call, needle=""):
    with pytest.raises(emspec.EmspecError) as ei:
        call()
    assert ei.value.code == code and needle in str(ei.value), (ei.value.code, str(ei.value))
    return str(ei.value)


def _own_bytes_consistent(got, map, pal):
    """What is a function of delivered bytes is exact in either mode: the index of the delivered level, RGBA of (pan, index)."""
    top, rng, gate, shift = (F(v) for v in map[:4])
    with np.errstate(invalid="ignore"):
        s = (got["level"] + shift).astype(F)
        idx = P.cell_index_f32(np.where(np.isnan(s), gate, s).astype(F), top, rng, gate)
        idx[np.isnan(s)] = 0
        assert np.array_equal(got["index"], idx)
        assert np.all(got["pan"][s < gate] == 16)
    assert np.array_equal(got["rgba"], pal[got["pan"], got["index"]])


def _image_of(got, db_other, case, map, pal, exact, post, what):
    """got: an image made of dB inside the engine; db_other: the dB another call delivered (see the head of this file)."""
    views, a, b = case
    want = T.compose(db_other, views, a, b, map, pal)
    _own_bytes_consistent(got, map, pal)
    if exact:
        return _equal(got, want, what)
    bound = (4 if post else 2) * TOL_DB
    top, rng, gate, shift, pan_range = (float(F(v)) for v in map)
    x = db_other.astype(np.float64).reshape((-1, views) + db_other.shape[1:])
    xa, xb = x[:, a], x[:, b]
    s = np.maximum(xa, xb) + shift
    near_gate = np.abs(s - gate) <= bound
    t = np.clip((xb - xa) / pan_range, -1, 1) * 16
    near_tie = np.abs(t - np.floor(t) - 0.5) <= 16 / pan_range * 2 * bound + 1e-6
    v = np.clip((s - (top - rng)) / rng, 0, 1) * 255 + 0.5
    near_step = np.abs(v - np.round(v)) <= 255 / rng * bound + 1e-4
    err = float(np.max(np.abs(got["level"].astype(np.float64) - want["level"])))
    dp = got["pan"].astype(int) - want["pan"].astype(int)
    di = got["index"].astype(int) - want["index"].astype(int)
    print(what, "FAST against another call's dB: max |level difference| %.3e (bound %.3e); balance differs on %d, index on %d of %d cells"
          % (err, bound, np.count_nonzero(dp), np.count_nonzero(di), dp.size))
    assert err <= bound, (what, err)
    assert np.all(dp[~(near_tie | near_gate)] == 0) and np.all(np.abs(dp[~near_gate]) <= 1), what
    assert np.all(di[~(near_step | near_gate)] == 0) and np.all(np.abs(di[~near_gate]) <= 1), what


def _signal_t(views=4, **kw):
    return torch.from_numpy(T.decoded_signal(views, **kw)).cuda()


# ---- 1. emspec_stereo_device against the host twin and the restatement ----
@MODES
@pytest.mark.parametrize("rows", [64, 68])
def test_device_entry_on_bytes_the_test_holds(exact, rows):
    pal = T.random_palette()
    with _engine(exact, rows) as e:
        # a new engine holds the built palette at its default colour map's brightness: 0 dB against -12, -6, 0 and -3 dB
        four = torch.tensor([[0.0, 0.0, 0.0, 0.0], [-12.0, -6.0, 0.0, -3.0]], device="cuda")
        assert np.array_equal(_np(e.stereo_device(four, want=("rgba",)))["rgba"][0], emspec.make_stereo_colormap(0.5)[[0, 8, 16, 12], 255])
        e.set_stereo_colormap(pal)
        dm = e.stereo_default_map()
        assert (dm.db_top, dm.db_range, dm.gate_db, dm.shift_db, dm.pan_range_db) == T.DEFAULT_MAP
        # the constructed array: 1,700 cells = 425 quads, a ragged second workgroup
        for map in (T.DEFAULT_MAP[:4] + (16.0,), T.VIEW_MAP[:4] + (16.0,), T.VIEW_MAP):
            db = T.special_cases(map, cells=1700)
            want = T.compose(db, 2, 0, 1, map, pal)
            got = _np(e.stereo_device(torch.from_numpy(db).cuda(), 2, 0, 1, map, want=ALL))
            _equal(got, want, ("special", map))
            _equal(got, emspec.stereo_host(db, 2, 0, 1, map, pal, want=ALL), ("special, host twin", map))
        assert np.array_equal(got["rgba"], pal[got["pan"], got["index"]])
        # the engine's own dB of the decoded signal; rows 68: also 25 columns of it, 1,700 cells per stream
        full = _batch_db(e, _signal_t(4))
        assert full.shape == (8, FRAMES, rows)
        for db_t in ([full] if rows == 64 else [full, full[:, :25].contiguous()]):
            db = db_t.cpu().numpy()
            for views, a, b in T.CASES:
                x_t = db_t if views == 4 else db_t.reshape(2, 4, -1)[:, :2].reshape(4, *db_t.shape[1:]).contiguous()
                x = x_t.cpu().numpy()
                for map in MAPS:
                    want = T.compose(x, views, a, b, map, pal)
                    T.exercised(want)
                    got = _np(e.stereo_device(x_t, views, a, b, map, want=ALL))
                    _equal(got, want, (views, a, b, map))
                    _equal(got, emspec.stereo_host(x, views, a, b, map, pal, want=ALL), ("host twin", views, a, b))
            # each output asked for alone gives the same bytes; None = the default map
            want = T.compose(db, 4, 2, 3, T.DEFAULT_MAP, pal)
            for k in ALL:
                only = _np(e.stereo_device(db_t, 4, 2, 3, want=(k,)))
                assert all(only[o] is None for o in ALL if o != k)
                _equal(only, want, ("alone", k))
        assert len(np.unique(got["rgba"].reshape(-1, 4), axis=0)) > 64
        # no pairs: a no-op; refusals leave the engine usable
        lib, h, m = e._lib, e._h, emspec.StereoMap(*T.DEFAULT_MAP)
        out = torch.full((2, 1700), 7, dtype=torch.uint8, device="cuda")
        p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
        x = torch.from_numpy(T.special_cases(T.DEFAULT_MAP, cells=1700)).cuda()
        assert lib.emspec_stereo_device(h, p(x), 0, 2, 0, 1, 1700, C.byref(m), None, p(out), None, None, None) == emspec.OK
        for args, needle in (((1, 1, 0, 0, 1700), "views >= 2"), ((1, 2, 0, 2, 1700), "0 .. views - 1"), ((1, 2, 1, 1, 1700), "differ"),
                             ((1, 2, 0, 1, 1698), "cells % 4"), ((65536, 2, 0, 1, 4), "pairs"), ((-1, 2, 0, 1, 4), "pairs")):
            assert lib.emspec_stereo_device(h, p(x), *args, C.byref(m), None, p(out), None, None, None) == emspec.ERR_INVALID_ARG
            assert needle in lib.emspec_last_error(h).decode(), (args, lib.emspec_last_error(h))
        for bad in ((0.0, 0.0, -80.0, 0.0, 12.0), (0.0, 80.0, -80.0, 0.0, 0.0), (float("nan"), 80.0, -80.0, 0.0, 12.0),
                    (0.0, 80.0, -80.0, float("nan"), 12.0), (0.0, 80.0, -80.0, 0.0, float("nan"))):
            bm = emspec.StereoMap(*bad)
            assert lib.emspec_stereo_device(h, p(x), 1, 2, 0, 1, 1700, C.byref(bm), None, p(out), None, None, None) == emspec.ERR_INVALID_ARG
        assert lib.emspec_stereo_device(h, p(x), 1, 2, 0, 1, 1700, C.byref(m), None, None, None, None, None) == emspec.ERR_INVALID_ARG
        assert "at least one output" in lib.emspec_last_error(h).decode()
        for kw in (dict(db=4), dict(index=2), dict(pan=1)):
            rc = lib.emspec_stereo_device(h, p(x, kw.get("db", 0)), 1, 2, 0, 1, 1696, C.byref(m), None, p(out, kw.get("index", 0)),
                                          p(out, 1700 + kw["pan"]) if "pan" in kw else None, None, None)
            assert rc == emspec.ERR_INVALID_ARG and "aligned" in lib.emspec_last_error(h).decode(), kw
        torch.cuda.synchronize()
        assert bool((out == 7).all())                                        # no refusal wrote anything
        got = _np(e.stereo_device(x, 2, 0, 1, T.DEFAULT_MAP, want=ALL))
        _equal(got, T.compose(x.cpu().numpy(), 2, 0, 1, T.DEFAULT_MAP, pal), "after the refusals")


# ---- 2. emspec_batch_stereo_device ----
@MODES
@pytest.mark.parametrize("rows,display", [(64, False), (68, False), (64, True)], ids=["r64", "r68", "display"])
def test_batch_device_entry(exact, rows, display):
    pal = T.random_palette()
    with _engine(exact, rows) as e:
        e.set_stereo_colormap(pal)
        if display:
            e.set_display(*DISPLAY)
        x = _signal_t(4)
        db = _batch_db(e, x).cpu().numpy()
        for case in T.CASES:
            views, a, b = case
            x_t = x if views == 4 else x.reshape(2, 4, -1)[:, :2].reshape(4, -1).contiguous()
            d = db if views == 4 else np.ascontiguousarray(db.reshape(2, 4, *db.shape[1:])[:, :2].reshape(4, *db.shape[1:]))
            for map in MAPS:
                got = _np(e.batch_stereo_device(x_t, N, HOP, True, views, a, b, map, want=ALL))
                assert got["level"].shape == (2, FRAMES, rows)
                _image_of(got, d, case, map, pal, exact, display, ("batch device", case, rows, display))
        only = _np(e.batch_stereo_device(x, N, HOP, True, 4, 0, 1, want=("pan",)))
        assert only["index"] is None and only["pan"].shape == (2, FRAMES, rows)
        # refusals: whole pairs, a time reduction
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_stereo_device(x[:6], N, HOP, True, 4, 0, 1), "S % views")
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_stereo_device(x, N, HOP, True, 4, 0, 4), "views - 1")
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_stereo_device(x, N, HOP, True, 4, 0, 1, want=()), "at least one output")
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_stereo_device(x, N, HOP, True, 4, 0, 1, (0.0, 80.0, -80.0, 0.0, -1.0)), "pan_range_db")
        e.set_time_reduce(4)
        _refused(emspec.ERR_STATE, lambda: e.batch_stereo_device(x, N, HOP, True, 4, 0, 1), "time reduction")
        e.set_time_reduce(1)
        got = _np(e.batch_stereo_device(x, N, HOP, True, 4, 2, 3, T.VIEW_MAP, want=ALL))
        _image_of(got, db, (4, 2, 3), T.VIEW_MAP, pal, exact, display, "after the refusals")


@MODES
def test_batch_device_entry_in_chunks_of_whole_pairs(exact, monkeypatch):
    """Three pairs of four views on the diagnostic library at a workspace budget that holds 2.3 .. 2.65 pairs (chunk_ref.budget_for;
    a pair needs views x columns x rows x 4 bytes of the workspace): chunks of (2, 1) pairs - the boundary falls between pairs, the
    last chunk is short - and at budget 0 one pair per chunk; both give the unbudgeted run's image."""
    rows, views, pairs = 64, 4, 3
    Cn, budget = K.frames_for(lambda c: views * K.peaks_bytes(c, rows))
    per_pair = views * K.peaks_bytes(Cn, rows)
    assert K.chunks(budget, per_pair, pairs) == (2, 1) and K.chunks(0, per_pair, pairs) == (1, 1, 1)
    print("columns", Cn, "budget", budget, "MiB;", per_pair, "B per pair -> chunks", K.chunks(budget, per_pair, pairs))
    x = _signal_t(4, frames=Cn, sources=pairs)
    assert x.shape[0] == pairs * views
    pal = emspec.make_stereo_colormap(0.5)
    runs = []
    for v in (None, budget, 0):
        if v is None:
            monkeypatch.delenv(K_ENV, raising=False)
        else:
            monkeypatch.setenv(K_ENV, str(v))
        with _engine(exact, rows, diag=True) as e:
            out = {k: torch.full((pairs, Cn, rows) + ((4,) if k == "rgba" else ()), 0x5A, dtype=torch.float32 if k == "level" else torch.uint8,
                                 device="cuda") for k in ALL}
            e.batch_stereo_device(x, N, HOP, True, views, 2, 3, T.VIEW_MAP, **out)
            got = _np(out)
            e.device_status()
            db = _batch_db(e, x).cpu().numpy() if v is None else None
        runs.append(got)
        if v is None:
            _image_of(got, db, (views, 2, 3), T.VIEW_MAP, pal, exact, False, "unbudgeted")
            ref_db = db
        elif exact:
            _equal(got, runs[0], ("budget", v))
        else:
            _image_of(got, ref_db, (views, 2, 3), T.VIEW_MAP, pal, exact, False, ("budget", v))
    monkeypatch.delenv(K_ENV, raising=False)


K_ENV = "EMSPEC_RECORD_BUDGET_MB"


# ---- 3. emspec_batch_pcm_stereo ----
def _pcm_stereo(e, raw, fmt, case, map, pinned):
    """One call into pageable or page-locked outputs pre-filled with a pattern."""
    sources, Cn = raw.shape[0], emspec.num_columns(raw.shape[1] // 2, N, HOP)
    shape = (sources, Cn, e.rows)
    pins = []

    def alloc(sh, dt):
        if pinned:
            pins.append(emspec.PinnedArray(sh, dt))
            a = pins[-1].array
        else:
            a = np.empty(sh, dt)
        a.view(np.uint8)[...] = 0x5A
        return a
    try:
        src = raw
        if pinned:
            src = alloc(raw.shape, raw.dtype)
            src[...] = raw
        out = {"level": alloc(shape, F), "index": alloc(shape, np.uint8), "pan": alloc(shape, np.uint8), "rgba": alloc(shape + (4,), np.uint8)}
        got = e.batch_pcm_stereo(src, fmt, N, HOP, True, case[1], case[2], map, **out)
        return {k: v.copy() for k, v in got.items()}
    finally:
        for pn in pins:
            pn.close()


@MODES
@pytest.mark.parametrize("display", [False, True], ids=["raw", "display"])
def test_host_entry_from_raw_frames(exact, display):
    raw = T.raw_signal()
    pal = T.random_palette()
    with _engine(exact, 64) as e:
        e.set_stereo_colormap(pal)
        if display:
            e.set_display(*DISPLAY)
        for views, a, b in T.CASES:
            fmt = emspec.PcmFormat.make("s16", 2, views=LRMS[:views])
            x = _signal_t(views)
            db = _batch_db(e, x).cpu().numpy()
            dev = _np(e.batch_stereo_device(x, N, HOP, True, views, a, b, T.VIEW_MAP, want=ALL))
            for pinned in (False, True):
                got = _pcm_stereo(e, raw, fmt, (views, a, b), T.VIEW_MAP, pinned)
                if exact:
                    _equal(got, dev, ("host entry = device entry", views, a, b, pinned))
                _image_of(got, db, (views, a, b), T.VIEW_MAP, pal, exact, display, ("host entry", views, a, b, pinned))
        # only what is asked for is written; the default map
        fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
        only = e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 1, want=("index", "pan"))
        assert only["level"] is None and only["rgba"] is None
        if exact:
            ref = T.compose(db, 4, 0, 1, T.DEFAULT_MAP)
            assert np.array_equal(only["index"], ref["index"]) and np.array_equal(only["pan"], ref["pan"])
        # with the envelope set, the same call also delivers emspec_batch_pcm's envelope (a function of the samples alone)
        wave_a, wave_b = np.full((8, FRAMES, 2), 7.0, F), np.full((8, FRAMES, 2), 9.0, F)
        e.set_wave_out(wave_a)
        e.batch_pcm(raw, fmt, N, HOP, True, want=("index",))
        e.set_wave_out(wave_b)
        got = e.batch_pcm_stereo(raw, fmt, N, HOP, True, 2, 3, T.VIEW_MAP, want=ALL)
        e.set_wave_out(None)
        assert np.array_equal(wave_a.view(U), wave_b.view(U)) and not np.any(wave_a == 7.0)
        _image_of(got, db, (4, 2, 3), T.VIEW_MAP, pal, exact, display, "beside the envelope")
        # refusals
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 4), "views - 1")
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_pcm_stereo(raw, fmt, N, HOP, True, 1, 1), "differ")
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_pcm_stereo(raw, emspec.PcmFormat.make("s16", 2, views=["mono"]), N, HOP), "views >= 2")
        _refused(emspec.ERR_INVALID_ARG, lambda: e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 1, want=()), "at least one output")
        e.set_time_reduce(2)
        _refused(emspec.ERR_STATE, lambda: e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 1), "time reduction")
        e.set_time_reduce(1)
        got = e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 1, T.VIEW_MAP, want=ALL)
        _image_of(got, db, (4, 0, 1), T.VIEW_MAP, pal, exact, display, "after the refusals")


@MODES
def test_host_entry_one_long_source_cut_into_runs_of_columns(exact, monkeypatch):
    """ONE source of 2 x 16,384 columns - the fewest the pipeline cuts into runs (emspec_pipe_plan.h: pipe_items) - on the
    diagnostic library with the unit count forced to two, so that the cut is certain: both views of the pair come from the same
    run's columns, the halo columns of a run are composed and left on the device.  The device entry on the decoded samples gives
    the reference."""
    Cn = 2 * 16384
    frames = N + HOP * (Cn - 1)
    short = T.raw_signal(frames=250, sources=1)                               # 64,768 frames, tiled: levels jump every ~6 columns
    raw = np.ascontiguousarray(np.tile(short, (1, -(-frames * 2 // short.shape[1])))[:, :frames * 2])
    fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
    pal = emspec.make_stereo_colormap(0.5)
    monkeypatch.setenv("EMSPEC_PIPE_CHUNKS", "2")
    with _engine(exact, 64, diag=True) as e:
        x = e.pcm_decode_device(torch.from_numpy(raw.view(np.uint8)).cuda(), fmt, 1, frames)
        assert x.shape == (4, frames)
        dev = _np(e.batch_stereo_device(x, N, HOP, True, 4, 0, 1, T.VIEW_MAP, want=("index", "pan")))
        got = e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 1, T.VIEW_MAP, want=("index", "pan"))
        assert got["pan"].shape == (1, Cn, 64)
        if exact:
            _equal(got, dev, "runs of columns")
        else:
            db = _batch_db(e, x).cpu().numpy()
            full = e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 1, T.VIEW_MAP, want=ALL)
            _image_of(full, db, (4, 0, 1), T.VIEW_MAP, pal, exact, False, "runs of columns")
        assert len(np.unique(got["pan"])) >= 24 and len(np.unique(got["index"])) > 8


# ---- 4. the stereo history views ----
class Session:
    """A PCM live session (2 sources x L R M S) with a history, fed per hop and flushed; keeps every delivered column."""

    def __init__(self, e, W, frames=FRAMES, sources=2):
        self.e, self.W = e, W
        self.raw = T.raw_signal(frames=frames, sources=sources)
        self.fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
        self.S = 4 * sources
        self.got = [[] for _ in range(self.S)]
        e.set_live_history(W)
        total = N + HOP * (frames - 1)
        for a in range(0, total, HOP):
            db, _, counts, _ = e.push_samples_pcm(self.raw, self.fmt, N, HOP, True, count=min(HOP, total - a), offset=a)
            self.took(db, counts)
        while True:
            try:
                db, _, cols = e.columns_flush()
            except emspec.EmspecError as err:
                assert err.code == emspec.ERR_STATE
                break
            self.took(db[:, None], (cols >= 0).astype(int))
        self.end = frames
        assert all(len(g) == frames for g in self.got) and e.live_history(0) == (frames, max(0, frames - W))

    def took(self, db, counts):
        for s in range(self.S):
            self.got[s] += [db[s, i].copy() for i in range(int(counts[s]))]

    def delivered(self):
        return np.stack([np.stack(g) for g in self.got])                     # [S][columns][rows]

    def want(self, first, f, groups, case, map, pal, stream0=0, pairs=None):
        views, a, b = case
        pairs = (self.S - stream0) // views if pairs is None else pairs
        full = self.delivered()[stream0:stream0 + pairs * views, first:self.end]
        held = V.reduce_db(full, f)
        assert held.shape[1] == groups
        return T.compose(held, views, a, b, map, pal)


@MODES
@pytest.mark.parametrize("rows", [64, 68])
def test_history_views_of_the_delivered_columns(exact, rows):
    W = 5
    pal = T.random_palette()
    with _engine(exact, rows) as e:
        e.set_stereo_colormap(pal)
        ss = Session(e, W)
        first = ss.end - W
        mono_before = e.history_view(first, 2, 3, want=("db", "index"))
        exercised = False
        for case in T.CASES:
            views = case[0]
            for f in (1, 2, W):
                for a0 in range(first, ss.end):
                    groups = -(-(ss.end - a0) // f)
                    map = MAPS[(a0 + f) % 2]
                    want = ss.want(a0, f, groups, case, map, pal)
                    got = e.history_view_stereo(a0, f, groups, *case, map=map, want=ALL)
                    assert got["pan"].shape == (8 // views, groups, rows)
                    _equal(got, want, ("host view", case, f, a0))
                    if a0 == first and f == 1:
                        dev = _np(e.history_view_stereo_device(a0, f, groups, *case, map=map, want=ALL, stream=torch.cuda.Stream()))
                        _equal(dev, want, ("device view", case))
                        # (a window of five columns: fewer balance values than the whole image's 24, still both ends and the centre)
                        T.exercised(want, min_pans=12, min_cells=100)
                        exercised = True
        assert exercised
        # a sub-range: the second source's pair alone, one output, the default map; page-locked outputs are written in place
        want = ss.want(first + 1, 3, 2, (4, 2, 3), T.DEFAULT_MAP, pal, stream0=4, pairs=1)
        got = e.history_view_stereo(first + 1, 3, 2, 4, 2, 3, stream0=4, pairs=1, want=("pan",))
        assert got["index"] is None and np.array_equal(got["pan"], want["pan"])
        pin = [emspec.PinnedArray((2, 2, rows), F), emspec.PinnedArray((2, 2, rows, 4), np.uint8)]
        try:
            e.history_view_stereo(first + 1, 3, 2, 4, 0, 1, map=T.VIEW_MAP, want=(), level=pin[0].array, rgba=pin[1].array)
            _equal({"level": pin[0].array, "rgba": pin[1].array}, ss.want(first + 1, 3, 2, (4, 0, 1), T.VIEW_MAP, pal), "pinned")
        finally:
            for p in pin:
                p.close()
        # the mono view of the same session returns what it did before
        mono = e.history_view(first, 2, 3, want=("db", "index"))
        assert np.array_equal(mono["db"].view(U), mono_before["db"].view(U)) and np.array_equal(mono["index"], mono_before["index"])
        assert np.array_equal(mono["db"].view(U), V.reduce_db(ss.delivered()[:, first:], 2).view(U))
        # refusals: those of the mono view, for both streams of every pair; nothing written
        ok = lambda: e.history_view_stereo(first, 1, 1, 4, 0, 1, want=("pan",))["pan"]
        good = ok()
        for call in (lambda: e.history_view_stereo(first - 1, 1, 1, 4, 0, 1), lambda: e.history_view_stereo(first, 1, W + 1, 4, 0, 1),
                     lambda: e.history_view_stereo(first, 0, 1, 4, 0, 1), lambda: e.history_view_stereo(first, 1, 0, 4, 0, 1),
                     lambda: e.history_view_stereo(first, 1, 1, 4, 0, 1, pairs=3), lambda: e.history_view_stereo(first, 1, 1, 4, 0, 1, stream0=5, pairs=1),
                     lambda: e.history_view_stereo(first, 1, 1, 4, 0, 0), lambda: e.history_view_stereo(first, 1, 1, 1, 0, 0, pairs=1),
                     lambda: e.history_view_stereo(first, 1, 1, 4, 0, 1, want=()), lambda: e.history_view_stereo(first, 1, 1, 4, 0, 1, pairs=0),
                     lambda: e.history_view_stereo(first, 1, 1, 4, 0, 1, map=(0.0, 80.0, -80.0, 0.0, 0.0))):
            _refused(emspec.ERR_INVALID_ARG, call)
            assert np.array_equal(ok(), good)
        e.reset_stream(5)                                                     # the second source's right channel
        patt = {k: np.full((2, 1, rows) + ((4,) if k == "rgba" else ()), 0x5A, F if k == "level" else np.uint8) for k in ALL}
        keep = {k: v.copy() for k, v in patt.items()}
        msg = _refused(emspec.ERR_INVALID_ARG, lambda: e.history_view_stereo(first, 1, 1, 4, 0, 1, want=(), **patt), "stream 5")
        assert "[0, 0)" in msg and all(np.array_equal(patt[k], keep[k]) for k in ALL)
        dev = {k: torch.from_numpy(v).cuda() for k, v in keep.items()}
        _refused(emspec.ERR_INVALID_ARG, lambda: e.history_view_stereo_device(first, 1, 1, 4, 0, 1, want=(), **dev), "stream 5")
        assert all(np.array_equal(_np(dev)[k], keep[k]) for k in ALL)
        # ... the pairs that do not touch it still view: the first source, and mid / side of the second
        _equal(e.history_view_stereo(first, 1, W, 4, 0, 1, pairs=1, map=T.VIEW_MAP, want=ALL), ss.want(first, 1, W, (4, 0, 1), T.VIEW_MAP, pal, pairs=1),
               "the first source after reset_stream")
        _equal(e.history_view_stereo(first, 1, W, 4, 2, 3, map=T.VIEW_MAP, want=ALL), ss.want(first, 1, W, (4, 2, 3), T.VIEW_MAP, pal), "mid / side")
    with _engine(exact, rows) as e:
        _refused(emspec.ERR_STATE, lambda: e.history_view_stereo(0, 1, 1, 4, 0, 1, pairs=1), "no live history")


@MODES
def test_history_view_of_wide_groups_is_cut_over_waves_without_changing_a_byte(exact):
    """W = 64, factors of 32 and more: too few threads to fill the device, so each channel's group is cut over the waves of a
    workgroup (the SPLIT form) - the bytes of the unsplit definition, from a first column past the wrap too."""
    W, frames = 64, 80
    pal = T.random_palette()
    with _engine(exact, 64) as e:
        e.set_stereo_colormap(pal)
        ss = Session(e, W, frames=frames)
        first = frames - W
        assert e.live_streams == 8
        for a0, f in ((first, 64), (first + 1, 63), (first, 32), (first + 7, 33), (first + 20, 40)):
            groups = -(-(frames - a0) // f)
            for case in ((4, 0, 1), (4, 2, 3), (2, 1, 0)):
                want = ss.want(a0, f, groups, case, T.VIEW_MAP, pal)
                _equal(e.history_view_stereo(a0, f, groups, *case, map=T.VIEW_MAP, want=ALL), want, ("split", a0, f, case))
                dev = _np(e.history_view_stereo_device(a0, f, groups, *case, map=T.VIEW_MAP, want=ALL))
                _equal(dev, want, ("split, device", a0, f, case))


# ---- 5. Node: the addon returns the ctypes binding's bytes ----
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_stereo_matches_ctypes(tmp_path):
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    R, W = 64, 5
    raw = T.raw_signal()
    frames = raw.shape[1] // 2
    feed, out = tmp_path / "feed.s16", tmp_path / "stereo.bin"
    raw.tofile(feed)
    r = subprocess.run(["node", "test_stereo.js", str(feed), str(out)] + [str(v) for v in (2, frames, N, HOP, R, W)], cwd=js,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["columns"] == FRAMES and res["emitted"] == FRAMES
    fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
    want = [emspec.make_stereo_colormap(0.7).tobytes()]
    with _engine(True, R) as e:
        for v in (e.batch_pcm_stereo(raw, fmt, N, HOP, True, 0, 1, want=ALL), e.batch_pcm_stereo(raw, fmt, N, HOP, True, 2, 3, T.VIEW_MAP, want=("index", "pan"))):
            want += [v[k].tobytes() for k in ALL if v[k] is not None]
        e.set_stereo_colormap(emspec.make_stereo_colormap(0.7))
        Session(e, W)
        first = FRAMES - W
        views = (e.history_view_stereo(first, 1, W, 4, 0, 1, want=ALL),
                 e.history_view_stereo(first + 1, 2, 2, 4, 2, 3, map=T.VIEW_MAP, stream0=4, pairs=1, want=ALL))
        for v in views:
            want += [v[k].tobytes() for k in ALL]
        assert len(np.unique(views[0]["pan"])) > 4 and len(np.unique(views[0]["index"])) > 8   # (not one colour)
    got = out.read_bytes()
    assert len(got) == sum(len(w) for w in want)
    at = 0
    for i, w in enumerate(want):
        assert got[at:at + len(w)] == w, ("piece", i)
        at += len(w)
