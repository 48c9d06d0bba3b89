"""GPU: every column kernel on other sample rates and log axes (tests/axis_cases.py: 44.1, 8, 32, 96 and 192 kHz and a one-octave
zoom at 48 kHz; every shape at 1024 rows, one per kernel at 68 rows, the records paths at 4092 rows).
tests/test_axis_cases_cpu.py shows on the oracle alone that at least 10 % of every case's cells and the top row quad of at least
95 % of its columns (`zoom`: 50 %) are non-zero, and that on `tel` and `wide32` the clamp of the top edge to N / 2 decides where
the Nyquist bin - far above the power floor on this signal - belongs: to no row.

For every case Engine.fused() is the route tests/golden/kernel_plans.json records, and the columns equal the oracle's by the
comparison the suite uses for the mode - FAST: |dB error| < 8.7e-4, palette index within one step, at most max(8, cells / 1000)
cells off by one; EXACT: dB bits and palette index (RGBA on one case per kernel) byte-equal to the binary64 bit model.  The per-bin
dump of the first 6 frames is array_equal to the bit model's, bins 0 and N / 2 included.  On `tel` the EXACT streaming calls
(exact_frames_kernel, which visits the Nyquist bin) deliver the batch's bytes (the one-kernel routes, which do not).  The row
lookup of the FAST kernels equals bisection on every axis, on axes within 1 % of the bound of hint_rows_ok and past it.
S = 2 streams, max(41, 2 D + 9) columns.  Every FAST case prints a MEASURED line."""
import ctypes as C

import numpy as np
import pytest

import axis_cases as A
import emspec
import oracle as O

pytestmark = pytest.mark.gpu

FAST_TOL_DB = 8.7e-4
ALL = ("db", "rgba", "index")


@pytest.fixture(scope="module")
def engines(engine):
    """One engine per (mode, diag) at a time, on the axis and rows last asked for (the cases come grouped by them); closed with
    the module.  (`engine`: the session's engine has settled the torch / HIP load order.)"""
    made = {}

    def get(exact, axis, rows, diag=False):
        slot, key = (bool(exact), bool(diag)), (A.kw(axis)["sample_rate"], A.kw(axis)["fmin_hz"], A.kw(axis)["fmax_hz"], rows)
        if slot in made and made[slot][0] != key:
            made.pop(slot)[1].close()
        if slot not in made:
            made[slot] = (key, emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST, rows=rows, diag=diag, **A.kw(axis)))
        e = made[slot][1]
        e.reset()
        return e
    yield get
    for _, e in made.values():
        e.close()


def _cfg(axis, n, hop, rows):
    return O.make_cfg(n, hop, True, rows=rows, **A.kw(axis))


def _grouped(cases):
    return sorted(cases, key=lambda c: (list(A.AXES).index(c[0]), c[3]))


def _fast_close(label, db, index, odb, oidx):
    assert db.shape == odb.shape and index.shape == oidx.shape
    worst = float(np.max(np.abs(db - odb)))
    d = np.abs(index.astype(int) - oidx.astype(int))
    off = int(np.count_nonzero(d))
    print(f"MEASURED {label}: worst |dB error| {worst:.2e}, cells off by one {off} of {d.size}")
    assert worst < FAST_TOL_DB, (label, worst)
    assert d.max() <= 1 and off <= max(8, d.size // 1000), (label, int(d.max()), off)


@pytest.mark.parametrize("axis,n,hop,rows", _grouped(A.FAST_CASES))
def test_fast_columns_on_other_axes(engines, axis, n, hop, rows):
    plan = A.fast_plan(axis, n, hop, rows)
    pcm = A.case_signal(axis, n, hop, rows)
    cfg = _cfg(axis, n, hop, rows)
    e = engines(False, axis, rows)
    assert e.rows == rows and bool(e.fused(n, hop, True)) == (plan["route"] != "records_f32")
    out = e.batch(pcm, n, hop, True, want=("db", "index"))
    pw, col, row = e.parity_dump(pcm, n, hop, True, 0, A.DUMP_FRAMES)
    e.device_status()
    odb, _, oidx = O.batch_f32(cfg, pcm, want=("db", "index"))
    assert out["db"].shape == (A.STREAMS, A.columns(n, hop), rows)
    _fast_close(f"{plan['route']} {axis} {n}/{hop} rows {rows}", out["db"], out["index"], odb, oidx)
    for s in range(A.STREAMS):
        opw, ocol, orow = O.frames_f32(cfg, pcm[s], 0, A.DUMP_FRAMES)
        assert np.array_equal(col[s], ocol) and np.array_equal(row[s], orow) and np.array_equal(pw[s], opw), \
            (s, int(np.sum(col[s] != ocol)), int(np.sum(row[s] != orow)), int(np.sum(pw[s] != opw)))
        assert np.all(orow[:, n // 2] == -1)


@pytest.mark.parametrize("axis,n,hop,rows", _grouped(A.EXACT_CASES))
def test_exact_columns_on_other_axes(engines, axis, n, hop, rows):
    plan = A.exact_plan(axis, n, hop, rows)
    pcm = A.case_signal(axis, n, hop, rows)
    cfg = _cfg(axis, n, hop, rows)
    rgba = (axis, n, hop, rows) in A.EXACT_RGBA
    x = engines(True, axis, rows)
    assert bool(x.fused(n, hop, True)) == (plan["route"] != "exact_records") == bool(plan["uses_fused"])
    out = x.batch(pcm, n, hop, True, want=ALL if rgba else ("db", "index"))
    pw, col, row, q = x.parity_dump_exact(pcm, n, hop, True, 0, A.DUMP_FRAMES)
    x.device_status()
    label = f"{plan['route']} {axis} {n}/{hop} rows {rows} rl {plan['rl']}"
    odb, orgba, oidx, _ = O.batch_exact(cfg, pcm, want=ALL if rgba else ("db", "index"))
    assert out["db"].shape == odb.shape == (A.STREAMS, A.columns(n, hop), rows)
    assert np.array_equal(out["index"], oidx), f"{label}: {np.sum(out['index'] != oidx)} palette indices differ " \
        f"(top row: {np.sum(out['index'][..., -1] != oidx[..., -1])})"
    assert np.array_equal(out["db"].view(np.uint32), odb.view(np.uint32)), \
        f"{label}: {np.sum(out['db'].view(np.uint32) != odb.view(np.uint32))} dB cells differ from the bit model"
    if rgba:
        assert np.array_equal(out["rgba"], orgba), f"{label}: RGBA differs"
    for s in range(A.STREAMS):
        opw, ocol, orow, oq = O.frames_exact(cfg, pcm[s], 0, A.DUMP_FRAMES)
        assert np.array_equal(col[s], ocol) and np.array_equal(row[s], orow) and np.array_equal(pw[s], opw) and np.array_equal(q[s], oq), \
            (label, s, int(np.sum(col[s] != ocol)), int(np.sum(row[s] != orow)), int(np.sum(pw[s] != opw)), int(np.sum(q[s] != oq)))


@pytest.mark.parametrize("axis,n,hop,rows", A.STREAMING)
def test_exact_streaming_equals_batch_bytes_on_tel(engines, axis, n, hop, rows):
    """emspec_column (frame by frame + flush) and emspec_push_samples (ragged blocks) run exact_frames_kernel, which visits the
    Nyquist bin; the batch runs a one-kernel route, which does not.  Same samples, same bytes - and the bit model's."""
    plan = A.exact_plan(axis, n, hop, rows)
    assert plan["route"] in ("exact_lr", "exact_parked")
    pcm = A.case_signal(axis, n, hop, rows)[0]
    frames = A.columns(n, hop)
    pcm = pcm[:n + (frames - 1) * hop]
    D = emspec.latency_columns(n, hop, True)
    x = engines(True, axis, rows)
    assert x.fused(n, hop, True)
    want = x.batch(pcm[None], n, hop, True, want=("db", "rgba"))
    odb, orgba, _, _ = O.batch_exact(_cfg(axis, n, hop, rows), pcm[None], want=("db", "rgba"))
    assert np.array_equal(want["db"].view(np.uint32), odb.view(np.uint32)) and np.array_equal(want["rgba"], orgba)
    x.reset()
    got_db, got_rgba = np.full((frames, rows), np.nan, np.float32), np.zeros((frames, rows, 4), np.uint8)
    for j in range(frames):
        db, rgba, c = x.column(pcm[j * hop:j * hop + n], hop, True, want_rgba=True)
        assert c == (j - D if j >= D else -1)
        if c >= 0:
            got_db[c], got_rgba[c] = db, rgba
    for j in range(D):
        db, rgba, c = x.flush(want_rgba=True)
        assert c == frames - D + j
        got_db[c], got_rgba[c] = db, rgba
    top = int(np.sum(got_db[:, -1].view(np.uint32) != want["db"][0][:, -1].view(np.uint32)))
    assert np.array_equal(got_db.view(np.uint32), want["db"][0].view(np.uint32)), f"emspec_column: top row differs in {top} columns"
    assert np.array_equal(got_rgba, want["rgba"][0])
    x.reset()
    cols, pos, i = [], 0, 0
    while pos < pcm.size:
        blk = (100, 3 * n - 1, 256, 700)[i % 4]
        db, first = x.push_samples(pcm[pos:pos + blk], n, hop, True)
        if db.shape[0]:
            assert first == len(cols)
            cols.extend(db)
        pos, i = pos + blk, i + 1
    for _ in range(D):
        cols.append(x.flush()[0])
    x.device_status()
    x.reset()
    assert len(cols) == frames
    assert np.array_equal(np.stack(cols).view(np.uint32), want["db"][0].view(np.uint32)), "emspec_push_samples differs from the batch"


# ---- the row lookup of the FAST kernels --------------------------------------------------------------------------------------

def _probe(e, n):
    """emspec_debug_row_lookup on every edge, its neighbours at 1 and 2 ulp, the row midpoints, 200,000 log-uniform values from
    half the first edge to twice the last, and zeros, negatives, inf and NaN: (values, the plan's lookup, the search)."""
    f = emspec.load(diag=True).emspec_debug_row_lookup
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    _, eb = e.tables(n)
    rng = np.random.default_rng(n)
    kh = np.ascontiguousarray(np.concatenate([
        A.probe_values(eb), np.exp(rng.uniform(np.log(eb[0] * 0.5), np.log(eb[-1] * 2.0), 200000)).astype(np.float32),
        np.array([0.0, -0.0, -1.0, 1e-30, 1e30, np.inf, -np.inf, np.nan], np.float32)]), np.float32)
    a, b = np.empty(kh.size, np.int32), np.empty(kh.size, np.int32)
    assert f(e._h, n, kh.ctypes.data, kh.size, a.ctypes.data, b.ctypes.data) == 0
    return eb, kh, a, b


def _lookup_is_bisection(e, n, label):
    eb, kh, a, b = _probe(e, n)
    assert np.array_equal(a, b), f"{label} n={n}: {np.sum(a != b)} of {a.size} rows differ from the search"
    ok = (kh >= eb[0]) & (kh < eb[-1])
    ref = A.bisect_rows(eb, kh)
    assert np.array_equal(b[ok], ref[ok]) and np.all(b[~ok] == -1), label


@pytest.mark.parametrize("rows", A.PROBE_ROWS)
@pytest.mark.parametrize("axis", list(A.AXES))
def test_row_lookup_equals_binary_search_on_other_axes(engines, axis, rows):
    e = engines(False, axis, rows, diag=True)
    for n in A.PROBE_SIZES:
        _lookup_is_bisection(e, n, f"{axis} rows {rows}")


@pytest.mark.parametrize("n", A.PROBE_SIZES)
def test_row_lookup_on_the_narrowest_hinted_axes(engines, n):
    """Within 1 % of the bound of hint_rows_ok for this n (tests/test_tables_cpu.py pins that): the hinted lookup, where the
    derivation leaves it a quarter of a row."""
    _lookup_is_bisection(engines(False, A.NARROW_HINTED[n], A.NARROW_ROWS, diag=True), n, f"narrow {A.NARROW_HINTED[n]}")


@pytest.mark.parametrize("axis,rows", A.NARROW_SEARCHED)
def test_row_lookup_past_the_hint_bound_is_searched(engines, axis, rows):
    """Axes a numpy model of the hint gets wrong (629 of 4,096 and 1,033 of 16,384 probes): the plan has log_rows = 0 there, the
    lookup searches, and the FAST columns still equal the oracle's."""
    e = engines(False, axis, rows, diag=True)
    for n in A.PROBE_SIZES:
        _lookup_is_bisection(e, n, f"searched {axis} rows {rows}")


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("which", list(A.NARROW_COLUMNS))
def test_columns_on_narrow_axes(engines, which, exact):
    """N = 4096, hop 256 on a 500 Hz wide axis below Nyquist (past the bound: log_rows = 0, the searched lookup and the generic
    per-bin core) and on the narrow hinted one: noise and a 23.8 kHz cosine, against the bit model of the mode."""
    axis, rows, share = A.NARROW_COLUMNS[which]
    n, hop = 4096, 256
    L = A.length(n, hop)
    pcm = (A.signal(A.STREAMS, L, nyquist=0.0).astype(np.float64) + 0.3 * np.cos(2 * np.pi * 23800.0 / 48000.0 * np.arange(L))).astype(np.float32)
    cfg = _cfg(axis, n, hop, rows)
    e = engines(exact, axis, rows)
    assert e.fused(n, hop, True)
    out = e.batch(pcm, n, hop, True, want=("db", "index"))
    e.device_status()
    if exact:
        odb, _, oidx, _ = O.batch_exact(cfg, pcm, want=("db", "index"))
        assert np.array_equal(out["index"], oidx) and np.array_equal(out["db"].view(np.uint32), odb.view(np.uint32))
    else:
        odb, _, oidx = O.batch_f32(cfg, pcm, want=("db", "index"))
        _fast_close(f"narrow ({which}) {axis} rows {rows}", out["db"], out["index"], odb, oidx)
        pw, col, row = e.parity_dump(pcm, n, hop, True, 0, A.DUMP_FRAMES)
        for s in range(A.STREAMS):
            opw, ocol, orow = O.frames_f32(cfg, pcm[s], 0, A.DUMP_FRAMES)
            assert np.array_equal(col[s], ocol) and np.array_equal(row[s], orow) and np.array_equal(pw[s], opw)
    assert float(np.mean(oidx != 0)) >= share and np.all((oidx != 0).any(axis=2))     # not vacuous: every column holds something
