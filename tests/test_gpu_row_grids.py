"""GPU: every column kernel on row counts that are no power of two (tests/row_grid_cases.py: 68, 100, 516, 1000 and 1020 rows on
every route of tests/golden/kernel_plans.json, both sides of every row threshold it records, 2052 and 4092 rows on the records
paths, and rows 68 and 1020 again with segments of 33 columns).  tests/test_row_grid_cases_cpu.py shows on the oracle alone that
the last row quad of every column, and at least 85 % of all row quads, are non-zero in every case's image: a kernel that drops or
misplaces the last quad of a column, writes a cell past its ring at full occupancy or mishandles a 4-row low split cannot pass.

For every case Engine.fused() is the route the fixture records, and the columns equal the oracle's by the comparison the suite uses
for the mode - FAST: |dB error| < 8.7e-4, palette index within one step, at most max(8, cells / 1000) cells off by one (the bounds
of tests/test_gpu_route.py); EXACT: dB bits, palette index and RGBA byte-equal to the binary64 bit model.  S = 2 streams,
max(41, 2 D + 9) columns.  Every FAST case prints a MEASURED line."""
import functools

import numpy as np
import pytest

import emspec
import multiband_ref as B
import oracle as O
import row_grid_cases as G

pytestmark = pytest.mark.gpu

FAST_TOL_DB = 8.7e-4
ALL = ("db", "rgba", "index")


@pytest.fixture(scope="module")
def engines(engine):
    """Engines by (mode, rows, diag), made on demand, closed with the module; handed out reset, on the configured log axis.
    (`engine`: the session's engine has settled the torch / HIP load order.)"""
    made = {}

    def get(exact, rows, diag=False):
        key = (bool(exact), rows, bool(diag))
        if key not in made:
            made[key] = emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST, rows=rows, diag=diag)
        e = made[key]
        e.reset()
        e.set_row_edges_hz(None)
        return e
    yield get
    for e in made.values():
        e.close()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _fast_ref(n, hop, rows, reassign):
    """The float32 oracle's (db, rgba, index) of a case, computed once and shared read-only."""
    return _frozen(*O.batch_f32(O.make_cfg(n, hop, bool(reassign), rows=rows), G.case_signal(n, hop, rows, reassign), want=ALL))


@functools.lru_cache(maxsize=None)
def _exact_ref(n, hop, rows, axis):
    O.set_custom_edges_hz(G.edges_hz(axis, rows))
    try:
        return _frozen(*O.batch_exact(O.make_cfg(n, hop, True, rows=rows), G.case_signal(n, hop, rows), want=ALL)[:3])
    finally:
        O.set_custom_edges_hz(None)


def _fast_close(label, db, index, odb, oidx):
    assert db.shape == odb.shape and index.shape == oidx.shape
    worst = float(np.max(np.abs(db - odb)))
    d = np.abs(index.astype(int) - oidx.astype(int))
    off = int(np.count_nonzero(d))
    print(f"MEASURED {label}: worst |dB error| {worst:.2e}, cells off by one {off} of {d.size}")
    assert worst < FAST_TOL_DB, (label, worst)
    assert d.max() <= 1 and off <= max(8, d.size // 1000), (label, int(d.max()), off)


def _exact_same(label, out, odb, orgba, oidx):
    assert out["db"].shape == odb.shape
    assert np.array_equal(out["index"], oidx), f"{label}: {np.sum(out['index'] != oidx)} palette indices differ"
    assert np.array_equal(out["db"].view(np.uint32), odb.view(np.uint32)), \
        f"{label}: {np.sum(out['db'].view(np.uint32) != odb.view(np.uint32))} dB cells differ from the bit model"
    assert np.array_equal(out["rgba"], orgba), f"{label}: RGBA differs"


def _run_fast(e, case, label):
    n, hop, rows, reassign = case
    plan = G.fast_plan(*case)
    pcm = G.case_signal(n, hop, rows, reassign)
    rgba = case in G.FAST_RGBA
    assert e.rows == rows and bool(e.fused(n, hop, bool(reassign))) == (plan["route"] != "records_f32")
    out = e.batch(pcm, n, hop, bool(reassign), want=ALL if rgba else ("db", "index"))
    e.device_status()
    odb, _, oidx = _fast_ref(*case)
    assert out["db"].shape == (G.STREAMS, G.columns(n, hop, reassign), rows)
    _fast_close(f"{plan['route']} {label}{n}/{hop} rows {rows} reassign {reassign}", out["db"], out["index"], odb, oidx)
    if rgba:
        assert np.array_equal(out["rgba"], O.default_lut()[out["index"]])
    return plan


@pytest.mark.parametrize("n,hop,rows,reassign", G.FAST_CASES)
def test_fast_columns_on_odd_row_grids(engines, n, hop, rows, reassign):
    case = (n, hop, rows, reassign)
    e = engines(False, rows)
    _run_fast(e, case, "")
    if rows in (68, 1020) and case in G.FAST_SWEEP:
        # the per-bin records of the first and the last three frames: (column, row) and power equal to the bit model's
        pcm, frames = G.case_signal(n, hop, rows, reassign), G.columns(n, hop, reassign)
        cfg = O.make_cfg(n, hop, bool(reassign), rows=rows)
        for f0 in (0, frames - 3):
            pw, col, row = e.parity_dump(pcm, n, hop, bool(reassign), f0, 3)
            for s in range(G.STREAMS):
                opw, ocol, orow = O.frames_f32(cfg, pcm[s], f0, 3)
                assert np.array_equal(col[s], ocol) and np.array_equal(row[s], orow) and np.array_equal(pw[s], opw), (f0, s)


@pytest.mark.parametrize("n,hop,rows,axis", G.EXACT_CASES)
def test_exact_columns_on_odd_row_grids(engines, n, hop, rows, axis):
    plan = G.exact_plan(n, hop, rows, axis)
    pcm = G.case_signal(n, hop, rows)
    x = engines(True, rows)
    try:
        x.set_row_edges_hz(G.edges_hz(axis, rows))
        assert bool(x.fused(n, hop, True)) == (plan["route"] != "exact_records") == bool(plan["uses_fused"])
        out = x.batch(pcm, n, hop, True, want=ALL)
        x.device_status()
    finally:
        x.set_row_edges_hz(None)
    _exact_same(f"{plan['route']} {n}/{hop} rows {rows} axis {axis} rl {plan['rl']}", out, *_exact_ref(n, hop, rows, axis))


@pytest.mark.parametrize("n,hop,rows,reassign", G.FAST_FORCED)
def test_fast_short_segments_on_odd_row_grids(engines, n, hop, rows, reassign, monkeypatch):
    """Two segments per stream (EMSPEC_SEGLEN is a switch of the diagnostic build, read per launch): the finalize's [c0, c1) test
    and the ring restart at an odd R."""
    monkeypatch.setenv("EMSPEC_SEGLEN", str(G.SEGLEN))
    assert G.columns(n, hop, reassign) > G.SEGLEN + 1
    plan = _run_fast(engines(False, rows, diag=True), (n, hop, rows, reassign), f"seglen {G.SEGLEN} ")
    assert plan["route"] != "records_f32"


@pytest.mark.parametrize("n,hop,rows,axis,parked", G.EXACT_FORCED)
def test_exact_short_segments_on_odd_row_grids(engines, n, hop, rows, axis, parked, monkeypatch):
    monkeypatch.setenv("EMSPEC_SEGLEN", str(G.SEGLEN))
    if parked:
        monkeypatch.setenv("EMSPEC_EXACT_PARKED", "1")     # the parked kernel where the no-parking one would serve (read per call)
    plan = G.exact_plan(n, hop, rows, axis, parked)
    assert plan["route"] == ("exact_parked" if parked else "exact_lr")
    pcm = G.case_signal(n, hop, rows)
    x = engines(True, rows, diag=True)
    try:
        x.set_row_edges_hz(G.edges_hz(axis, rows))
        assert x.fused(n, hop, True)
        out = x.batch(pcm, n, hop, True, want=ALL)
        x.device_status()
    finally:
        x.set_row_edges_hz(None)
    _exact_same(f"{plan['route']} seglen {G.SEGLEN} {n}/{hop} rows {rows} axis {axis}", out, *_exact_ref(n, hop, rows, axis))


# ---- the other entries that run a column kernel, small and few --------------------------------------------------------------

@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("n,hop", [(4096, 256), (1024, 256)])
@pytest.mark.parametrize("rows", [100, 1020])
def test_live_sample_blocks_on_odd_row_grids(engines, rows, n, hop, exact):
    """emspec_push_samples_multi in blocks of 100, 256 and 700 samples in rotation, then the flush, against the oracle's batch
    columns by the comparison of tests/test_gpu_live.py."""
    pcm = G.case_signal(n, hop, rows)
    odb, orgba, _ = _exact_ref(n, hop, rows, G.LOG) if exact else _fast_ref(n, hop, rows, 1)
    S, frames = odb.shape[:2]
    D = G.latency(n, hop, 1)
    got_db = np.full(odb.shape, np.nan, np.float32)
    got_rgba = np.zeros(orgba.shape, np.uint8)
    e = engines(exact, rows)
    nxt = a = i = 0
    L = pcm.shape[1]
    try:
        while a < L:
            cnt = min((100, 256, 700)[i % 3], L - a)
            db, rgba, counts, firsts = e.push_samples_multi(pcm, n, hop, True, want_rgba=True, count=cnt, offset=a)
            k = int(counts[0])
            assert np.all(counts == k) and (k == 0 or np.all(firsts == nxt))
            got_db[:, nxt:nxt + k], got_rgba[:, nxt:nxt + k] = db[:, :k], rgba[:, :k]
            nxt, a, i = nxt + k, a + cnt, i + 1
        assert nxt == frames - D
        for _ in range(D):
            db, rgba, cols = e.columns_flush(want_rgba=True)
            assert np.all(cols == nxt)
            got_db[:, nxt], got_rgba[:, nxt] = db, rgba
            nxt += 1
        e.device_status()
    finally:
        e.reset()
    if exact:
        assert np.array_equal(got_db.view(np.uint32), odb.view(np.uint32)) and np.array_equal(got_rgba, orgba)
    else:
        worst = float(np.max(np.abs(got_db - odb)))
        print(f"MEASURED live {n}/{hop} rows {rows}: worst |dB error| {worst:.2e}, RGBA cells that differ {float(np.mean(got_rgba != orgba)):.2e}")
        assert worst < FAST_TOL_DB and np.mean(got_rgba != orgba) < 1e-3


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_multiband_on_a_1000_row_engine(engines, exact):
    """Three bands of an engine with 1000 rows: each band kernel is handed a row count of its own, none a power of two.  Against
    the stitch of the bit model's single-resolution images (tests/multiband_ref.py); EXACT also against the stitch of the
    engine's own."""
    n, hop, rows = (16384, 4096, 1024), 256, 1000
    pcm = G.signal(G.STREAMS, n[0] + 40 * hop + 3)
    e = engines(exact, rows)
    split = tuple(e.split_row_for_hz(f) for f in (250.0, 2000.0))
    widths = np.diff([0, *split, rows])
    assert widths.min() >= 64 and all(w & (w - 1) for w in widths), widths
    got = e.batch_multiband(pcm, n, split, hop, True, want=ALL)
    e.device_status()
    Cm = emspec.multiband_columns(pcm.shape[1], n, hop)
    assert Cm == 41 and got["db"].shape == (G.STREAMS, Cm, rows)
    model = O.batch_exact if exact else O.batch_f32
    singles = [dict(zip(ALL, model(O.make_cfg(v, hop, True, rows=rows), pcm, want=ALL)[:3])) for v in n]
    want = {k: B.stitch([s[k] for s in singles], n, split, hop, Cm) for k in ALL}
    if exact:
        _exact_same("multiband", got, want["db"], want["rgba"], want["index"])
        own = [e.batch(pcm, v, hop, True, want=ALL) for v in n]
        _exact_same("multiband, the engine's own stitch", got, *(B.stitch([s[k] for s in own], n, split, hop, Cm) for k in ALL))
    else:
        _fast_close(f"multiband {n} rows {rows} splits {split}", got["db"], got["index"], want["db"], want["index"])
        assert np.array_equal(got["rgba"], O.default_lut()[got["index"]])


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_host_entry_equals_the_device_entry_at_1020_rows(engines, exact):
    """emspec_batch (staging, chunks, copies out) against emspec_batch_device of the same engine on the same samples - EXACT: bytes;
    FAST: the comparison of tests/test_gpu_host.py."""
    import torch
    n, hop, rows = 4096, 256, 1020
    pcm = G.case_signal(n, hop, rows)
    e = engines(exact, rows)
    got = e.batch(pcm, n, hop, True, want=("db", "index"))
    S, Cn = got["db"].shape[:2]
    db = torch.full((S, Cn, rows), -1.0, dtype=torch.float32, device="cuda")
    ix = torch.full((S, Cn, rows), 0x5A, dtype=torch.uint8, device="cuda")
    e.batch_device(torch.from_numpy(np.array(pcm)).cuda(), n, hop, True, db=db, index=ix)
    torch.cuda.synchronize()
    e.device_status()
    rdb, rix = db.cpu().numpy(), ix.cpu().numpy()
    if exact:
        assert np.array_equal(got["index"], rix) and np.array_equal(got["db"].view(np.uint32), rdb.view(np.uint32))
    else:
        d = np.abs(got["index"].astype(int) - rix.astype(int))
        assert d.max() <= 1 and np.mean(d != 0) < 1e-4
        assert np.max(np.abs(got["db"] - rdb)) < 1e-3
