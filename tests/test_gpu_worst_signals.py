"""GPU: the worst-case signals of tests/worst_signals.py through every accumulator of the project.

The other parity tests feed emspec.synth.streams, whose energy is spread over the image.  Here a stationary tone piles its skirts
into one cell, an impulse puts every bin of n / hop frames into one column, a 30 Hz tone lives in the lowest rows, a level of 30
crosses the EXACT mode's upper power gate, a chirp reaches past +-D - on the fused kernels of every fft size, the records path
with its walking and tile scatters, the EXACT kernels with the low rows in their L2 scratch, the live kernels and both bands of
the multi-resolution batch.  tests/test_worst_signals_cpu.py asserts on the bit model that each signal provokes what it is meant
to at each shape used here.

S = 2 streams (the signal and half of it; live: a quarter as well), 3 (2D + 2) frames so that every column ring wraps twice.
FAST: per-bin dump equal to the float32 bit model, dB within 8.7e-4, palette within one step at a share bounded per case in
tests/golden/palette_bounds.json.  EXACT: every byte equal to the binary64 bit model.  The bit-model references are computed once
per (signal, shape) and shared by the tests of this module."""
import functools

import numpy as np
import pytest

import emspec
import multires_ref as M
import oracle as O
import worst_signals as WS
from palette import palette_close

pytestmark = pytest.mark.gpu

TOL_DB = 8.7e-4
LINEAR_AXIS = np.linspace(40.0, 23000.0, 1025).astype(np.float32)     # test_exact_axes_the_row_split_does_not_serve's


@functools.lru_cache(maxsize=None)
def _pcm(kind, n, hop, S=2):
    x = WS.signal(kind, n, hop, WS.frames_for(n, hop))
    pcm = np.stack([x * np.float32(0.5 ** s) for s in range(S)])      # (halving is exact in float32)
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def _ref_fast(kind, n, hop, rows=1024, S=2):
    db, _, idx = O.batch_f32(O.make_cfg(n, hop, True, rows=rows), _pcm(kind, n, hop, S), want=("db", "index"))
    for a in (db, idx):
        a.setflags(write=False)
    return db, idx


@functools.lru_cache(maxsize=None)
def _ref_exact(kind, n, hop, rows=1024, S=2, power_floor=None, linear=False):
    kw = {} if power_floor is None else {"power_floor": power_floor}
    if linear:
        O.set_custom_edges_hz(LINEAR_AXIS)
    try:
        db, _, idx, _ = O.batch_exact(O.make_cfg(n, hop, True, rows=rows, **kw), _pcm(kind, n, hop, S), want=("db", "index"))
    finally:
        if linear:
            O.set_custom_edges_hz(None)
    for a in (db, idx):
        a.setflags(write=False)
    return db, idx


@pytest.fixture(scope="module")
def engines():
    import torch   # torch's HIP runtime first (tests/conftest.py:_torch_first)
    if torch.cuda.is_available():
        torch.cuda.init()
    made = {}

    def get(mode, rows=1024, **kw):
        key = (mode, rows, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = emspec.Engine(mode=mode, rows=rows, **kw)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- FAST ------------------------------------------------------------------------------------------------------------------
FAST_FUSED = {(4096, 256, 1024): True, (1024, 256, 1024): True, (4096, 512, 1024): True, (2048, 128, 1024): True,
              (2048, 300, 1024): True, (8192, 512, 1024): True, (16384, 512, 1024): True,
              (16384, 256, 1024): False,        # test_generic_records_path_still_serves_n16384_small_hop's shape
              (4096, 256, 2048): False}         # test_generic_path_at_4096_with_many_rows'
FAST_CASES = [(n, hop, rows, kind) for n, hop, rows, kinds in WS.FAST_SHAPES for kind in kinds]


@pytest.mark.parametrize("n,hop,rows,kind", FAST_CASES)
def test_fast_matches_the_float32_bit_model(engines, n, hop, rows, kind):
    e = engines(emspec.MODE_FAST, rows)
    assert e.fused(n, hop, True) == FAST_FUSED[(n, hop, rows)]
    pcm = _pcm(kind, n, hop)
    frames = WS.frames_for(n, hop)
    last = min(frames, 8)
    cfg = O.make_cfg(n, hop, True, rows=rows)
    pw, col, row = e.parity_dump(pcm, n, hop, True, frames - last, last)
    for s in range(pcm.shape[0]):
        opw, ocol, orow = O.frames_f32(cfg, pcm[s], frames - last, last)
        assert np.array_equal(col[s], ocol), f"stream {s}: column differs in {int(np.sum(col[s] != ocol))} bins, first (frame, bin) {tuple(np.argwhere(col[s] != ocol)[0])}"
        assert np.array_equal(row[s], orow), f"stream {s}: row differs in {int(np.sum(row[s] != orow))} bins, first (frame, bin) {tuple(np.argwhere(row[s] != orow)[0])}"
        assert np.array_equal(pw[s], opw, equal_nan=True), f"stream {s}: power differs in {int(np.sum(~((pw[s] == opw) | (np.isnan(pw[s]) & np.isnan(opw)))))} bins"
    out = e.batch(pcm, n, hop, True, want=("db", "index"))
    odb, oidx = _ref_fast(kind, n, hop, rows)
    assert out["db"].shape == odb.shape == (2, frames, rows)
    assert not np.isnan(out["db"]).any()
    err = float(np.max(np.abs(out["db"] - odb)))
    print(f"MEASURED worst-signal dB error {kind} N={n} hop={hop} rows={rows}: {err:.3e}")
    assert err < TOL_DB, err
    palette_close(out["index"], oidx)


# ---- EXACT -----------------------------------------------------------------------------------------------------------------
EXACT_FUSED = {(4096, 256, 1024): True, (2048, 128, 1024): True, (1024, 256, 1024): True, (16384, 512, 1024): False,
               (8192, 512, 1024): False, (4096, 128, 1024): False, (4096, 256, 2048): False}
EXACT_CASES = [(n, hop, rows, kind, "plain") for n, hop, rows, kinds in WS.EXACT_SHAPES for kind in kinds] + \
    [(4096, 256, 1024, kind, variant) for variant in ("linear_axis", "no_floor") for kind in WS.CORE_KINDS]


@pytest.mark.parametrize("n,hop,rows,kind,variant", EXACT_CASES)
def test_exact_equals_the_binary64_bit_model(engines, n, hop, rows, kind, variant):
    """plain: exact_fused_lr (4096 / 2048 / 1024), the records path with the walking scatter (16384, 8192, 4096 / 128) and the
    tile scatter (2048 rows); linear_axis: the parked-ring exact_fused kernel; no_floor: the generic per-bin core."""
    pcm = _pcm(kind, n, hop)
    frames = WS.frames_for(n, hop)
    last = min(frames, 8)
    if variant == "linear_axis":
        e = emspec.Engine(mode=emspec.MODE_EXACT)
        e.set_row_edges_hz(LINEAR_AXIS)
        cfg = O.make_cfg(n, hop, True)
        odb, oidx = _ref_exact(kind, n, hop, linear=True)
    elif variant == "no_floor":
        e = engines(emspec.MODE_EXACT, rows, power_floor=0.0)
        assert e.fused(n, hop, True)
        cfg = O.make_cfg(n, hop, True, power_floor=0.0)
        odb, oidx = _ref_exact(kind, n, hop, power_floor=0.0)
    else:
        e = engines(emspec.MODE_EXACT, rows)
        assert e.fused(n, hop, True) == EXACT_FUSED[(n, hop, rows)]
        cfg = O.make_cfg(n, hop, True, rows=rows)
        odb, oidx = _ref_exact(kind, n, hop, rows)
    try:
        pw, col, row, q = e.parity_dump_exact(pcm, n, hop, True, frames - last, last)
        out = e.batch(pcm, n, hop, True, want=("db", "index"))
        again = e.batch(pcm, n, hop, True, want=("db", "index"))
    finally:
        if variant == "linear_axis":
            e.close()
    if variant == "linear_axis":
        O.set_custom_edges_hz(LINEAR_AXIS)
    try:
        model = [O.frames_exact(cfg, pcm[s], frames - last, last) for s in range(pcm.shape[0])]
    finally:
        O.set_custom_edges_hz(None)
    for s, (opw, ocol, orow, oq) in enumerate(model):
        for name, got, want in (("column", col[s], ocol), ("row", row[s], orow), ("q", q[s], oq)):
            assert np.array_equal(got, want), f"stream {s}: {name} differs in {int(np.sum(got != want))} bins, first (frame, bin) {tuple(np.argwhere(got != want)[0])}"
        same = (pw[s].view(np.uint64) == opw.view(np.uint64)) | (np.isnan(pw[s]) & np.isnan(opw))
        assert same.all(), f"stream {s}: power bits differ in {int(np.sum(~same))} bins, first (frame, bin) {tuple(np.argwhere(~same)[0])}"
    assert out["db"].shape == odb.shape
    assert np.array_equal(out["index"], oidx), f"{int(np.sum(out['index'] != oidx))} palette indices differ, first (stream, column, row) {tuple(np.argwhere(out['index'] != oidx)[0])}"
    d = out["db"].view(np.uint32) != odb.view(np.uint32)
    assert not d.any(), f"{int(d.sum())} dB cells differ, first (stream, column, row) {tuple(np.argwhere(d)[0])}"
    for k in ("db", "index"):
        assert _same_bits(out[k], again[k]), f"{k} differs between two runs of the same call"


@pytest.mark.parametrize("kind", ["loud", "impulses"])
def test_exact_short_odd_segments(kind, monkeypatch):
    """N = 4096 / hop 256 cut into segments of 33 columns (diagnostic build, as test_exact_fused_kernel_shapes): every segment
    restarts the ring and recomputes its halo."""
    n, hop = 4096, 256
    monkeypatch.setenv("EMSPEC_SEGLEN", "33")
    pcm = _pcm(kind, n, hop)
    with emspec.Engine(mode=emspec.MODE_EXACT, diag=True) as e:
        assert e.fused(n, hop, True)
        out = e.batch(pcm, n, hop, True, want=("db", "index"))
        again = e.batch(pcm, n, hop, True, want=("db", "index"))
    odb, oidx = _ref_exact(kind, n, hop)
    assert np.array_equal(out["index"], oidx) and _same_bits(out["db"], odb)
    assert _same_bits(out["db"], again["db"]) and _same_bits(out["index"], again["index"])


# ---- live ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("kind", ["tone_centre", "impulses", "loud"])
@pytest.mark.parametrize("n,hop", [(4096, 256), (1024, 256)])
def test_live_blocks_of_1000_samples(n, hop, kind, exact):
    """emspec_push_samples_multi, S = 3, blocks of 1,000 samples (ragged against the hop: 3 or 4 frames a launch), then the flush.
    EXACT: the batch's bytes (the bit model's, which the batch test above pins); FAST: the convention of tests/test_gpu_live.py."""
    S = 3
    pcm = np.ascontiguousarray(_pcm(kind, n, hop, S))
    L = pcm.shape[1]
    frames = WS.frames_for(n, hop)
    odb = (_ref_exact(kind, n, hop, S=S) if exact else _ref_fast(kind, n, hop, S=S))[0]
    D = emspec.latency_columns(n, hop, True)
    got = np.full((S, frames, 1024), np.nan, np.float32)
    nxt = 0
    with emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST) as e:
        for a in range(0, L, 1000):
            cnt = min(1000, L - a)
            db, _, counts, firsts = e.push_samples_multi(pcm, n, hop, True, count=cnt, offset=a)
            k = int(counts[0])
            assert np.all(counts == k)
            if k:
                assert np.all(firsts == nxt)
                got[:, nxt:nxt + k] = db[:, :k]
                nxt += k
        assert nxt == frames - D
        for _ in range(D):
            db, _, cols = e.columns_flush()
            assert np.all(cols == nxt)
            got[:, nxt] = db
            nxt += 1
    if exact:
        d = got.view(np.uint32) != odb.view(np.uint32)
        assert not d.any(), f"{int(d.sum())} dB cells differ, first (stream, column, row) {tuple(np.argwhere(d)[0])}"
    else:
        assert not np.isnan(got).any()
        assert np.max(np.abs(got - odb)) < TOL_DB, float(np.max(np.abs(got - odb)))


# ---- multi-resolution -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tone_low+impulses", "loud"])
def test_multires_exact_equals_the_composition(kind):
    """16384 below 250 Hz, 4096 above, hop 256: the 30 Hz tone lives in the long band, the impulses fill both; `loud` crosses the
    upper power gate of both bands (each has its own fixed-point scale)."""
    n_low, n_high, hop = 16384, 4096, 256
    frames = WS.frames_for(n_low, hop)
    if kind == "loud":
        x = WS.signal("loud", n_low, hop, frames)
    else:
        x = (WS.signal("tone_low", n_low, hop, frames).astype(np.float64) + WS.signal("impulses", n_low, hop, frames)).astype(np.float32)
    pcm = np.stack([x, x * np.float32(0.5)])
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        split = e.split_row_for_hz(250.0)
        got = e.batch_multires(pcm, n_low, n_high, hop, split, True, want=("db", "index"))
        again = e.batch_multires(pcm, n_low, n_high, hop, split, True, want=("db", "index"))
    want = M.compose(pcm, n_low, n_high, hop, split, True, exact=True, want=("db", "index"))
    for k in ("db", "index"):
        assert _same_bits(got[k], want[k]), f"{k}: {int(np.sum(got[k].view(np.uint8) != want[k].view(np.uint8)))} bytes differ from the composition"
        assert _same_bits(got[k], again[k]), f"{k} differs between two runs"
