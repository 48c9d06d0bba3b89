"""GPU: every stream-chunked engine workspace across a chunk boundary ("Kernel plan": EMSPEC_RECORD_BUDGET_MB).

Six loops cut a batch into chunks of streams (tests/chunk_ref.py lists them).  Each case here runs one call three times on
engines of the diagnostic library: unbudgeted (one chunk), at an integer budget that holds 2.25 .. 2.75 streams of the call's
outermost workspace (chunk_ref.budget_for aims at 2.3 .. 2.65, so that a size that drifts by 10 % still gives two; S = 5: chunks
(2, 2, 1) - a boundary and a short last chunk whose stream count differs from the stride of the sub-arrays), and at budget 0
(one stream per chunk whatever the sizes).  The expected chunk lists are printed from
chunk_ref, whose formulas tests/test_chunk_ref_cpu.py ties to the headers.

EXACT: the three results are byte-equal and equal the CPU reference of the entry (oracle.batch_exact, multires_ref /
multiband_ref.compose, overview_ref.reduce, peaks_ref.peaks); with the display post-process on, the reference comparison is by
the bounds of tests/test_gpu_multiband.py (< 2e-3 dB, index within one step).  FAST sums in arrival order, so each run is held to
the oracle by the bounds of tests/test_gpu_route.py: |dB error| < 8.7e-4, index within one step on at most max(8, cells / 1000)
cells.  A reduced column is the maximum of its group: a maximum of values within eps of their references is within eps of the
references' maximum, and a reduced index differs only where a full-rate one does - so the same bounds hold behind the time
reduction, the cell count being that of the full-rate image.

Columns per case: the fewest >= 25 at which an integer number of MiB meets the budget rule (chunk_ref.columns_and_budget) - 25
to 33 for the records shapes, 41 to 97 for the composed entries and the time reduction, 387 where a stream needs only C x rows
bytes (index or RGBA alone behind the time reduction).  The whole file runs in about four seconds."""
import functools

import numpy as np
import pytest
import torch

import chunk_ref as K
import emspec
import multiband_ref as B
import multires_ref as M
import oracle as O
import overview_ref as V
import peaks_ref as P
from emspec import synth

pytestmark = pytest.mark.gpu

S = 5
ENV = "EMSPEC_RECORD_BUDGET_MB"
DISPLAY = (0.6, 0.8)
TWO = {"8192": (8192, 2048, 256, 368), "16384": (16384, 4096, 512, 368)}          # split_row_for_hz(250) on the default axis
LADDERS = {"3x512": ((8192, 2048, 1024), 512, (368, 668)), "4x128": ((16384, 8192, 4096, 2048), 128, (260, 468, 668))}


def test_the_diagnostic_library_is_the_one_loaded():
    """EMSPEC_RECORD_BUDGET_MB is read by the diagnostic build only: without it every case below would run one chunk."""
    lib = emspec.load(diag=True)
    assert hasattr(lib, "emspec_debug_row_lookup") and not hasattr(emspec.load(), "emspec_debug_row_lookup")
    with emspec.Engine(diag=True) as e:
        assert e._lib is lib


def case(entry, shape, exact, **kw):
    return dict(entry=entry, shape=tuple(shape), exact=exact, **kw)


def _n0_hop(c):
    sh = c["shape"]
    return (sh[0][0], sh[1]) if c["entry"] == "multi" else (sh[0], sh[1] if c["entry"] == "single" else sh[2])


def _freeze(d):
    return tuple(sorted((k, v) for k, v in d.items()))


@functools.lru_cache(maxsize=None)
def _pcm(streams, L):
    x = synth.streams(streams, L)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(frozen, streams, L):
    """The CPU reference of a case: the bit model (EXACT) or the float32 oracle (FAST) of the entry at full rate, the display
    post-process behind it, the time reduction behind that.  Computed once, shared read-only."""
    c = dict(frozen)
    pcm, exact, R = _pcm(streams, L), c["exact"], c.get("rows", 1024)
    n0, hop = _n0_hop(c)
    if c["entry"] == "single":
        cfg = O.make_cfg(n0, hop, True, rows=R)
        got = O.batch_exact(cfg, pcm)[:3] if exact else O.batch_f32(cfg, pcm)
        full = dict(zip(("db", "rgba", "index"), got))
    elif c["entry"] == "two":
        n_low, n_high, hop, split = c["shape"]
        full = M.compose(pcm, n_low, n_high, hop, split, True, exact=exact)
    else:
        n, hop, splits = c["shape"]
        full = B.compose(pcm, n, splits, hop, True, exact=exact)
    if c.get("display"):
        db, idx, rgba = O.postprocess(full["db"], *DISPLAY, O.make_cfg(n0, hop, True, rows=R))
        full = {"db": db, "rgba": rgba, "index": idx}
    out = V.reduce(full, c["f"], O.default_lut()) if c.get("f", 1) > 1 else full
    for v in out.values():
        v.setflags(write=False)
    return out


def _engine(c):
    e = emspec.Engine(mode=emspec.MODE_EXACT if c["exact"] else emspec.MODE_FAST, diag=True, rows=c.get("rows", 1024))
    if c.get("display"):
        e.set_display(*DISPLAY)
    if c.get("f", 1) > 1:
        e.set_time_reduce(c["f"])
    return e


def _call(e, c, x, columns):
    """One device call into outputs pre-filled with a pattern (an unwritten stream shows) -> numpy arrays."""
    want, streams, R = c.get("want", ("db", "index")), x.shape[0], e.rows
    if c.get("peaks"):
        out = torch.full((streams, columns, 8, 2), 7.0, dtype=torch.float32, device="cuda")
        e.batch_peaks_device(x, *c["shape"], True, 8, -60.0, out=out)
        torch.cuda.synchronize()
        e.device_status()
        return {"peaks": out.cpu().numpy()}
    Cr = e.out_columns(columns)
    t = {"db": torch.full((streams, Cr, R), -1.0, dtype=torch.float32, device="cuda") if "db" in want else None,
         "rgba": torch.full((streams, Cr, R, 4), 0x5A, dtype=torch.uint8, device="cuda") if "rgba" in want else None,
         "index": torch.full((streams, Cr, R), 0x5A, dtype=torch.uint8, device="cuda") if "index" in want else None}
    if c["entry"] == "single":
        e.batch_device(x, *c["shape"], True, **t)
    elif c["entry"] == "two":
        e.batch_multires_device(x, *c["shape"], True, **t)
    else:
        n, hop, splits = c["shape"]
        e.batch_multiband_device(x, n, splits, hop, True, **t)
    torch.cuda.synchronize()
    e.device_status()
    return {k: v.cpu().numpy() for k, v in t.items() if v is not None}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _where(a, b, name):
    """The first differing (stream, column): which chunk and which plane offset a mismatch belongs to."""
    d = np.argwhere(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], a.shape[1], -1) !=
                    np.ascontiguousarray(b).view(np.uint8).reshape(b.shape[0], b.shape[1], -1))
    return f"{name}: {len(d)} bytes differ, first at stream {d[0][0]} column {d[0][1]} byte {d[0][2]}" if len(d) else f"{name}: equal"


def _plan(c, streams=S, budgets=None):
    """Columns, samples and the budgets of a case; prints the chunk lists expected at each and checks that the budgeted run has
    at least two chunks and a short last one."""
    columns, b = K.columns_and_budget(c)
    n0, hop = _n0_hop(c)
    L = n0 + hop * (columns - 1) + 3
    budgets = [None, b, 0] if budgets is None else budgets
    for v in budgets:
        print(f"EXPECTED {c['entry']} {c['shape']} S = {streams}, {columns} columns:")
        for line in K.expected(c, columns, v, streams):
            print("   ", line)
    lists = K.outer_chunks(c, columns, b, streams)
    assert len(lists) >= 2 and lists[-1] < lists[0] == 2, lists
    assert set(K.outer_chunks(c, columns, 0, streams)) == {1}
    return columns, L, budgets


def _set_budget(monkeypatch, v):
    if v is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, str(v))


def _three_runs(c, monkeypatch, fused=None):
    """The call of case c on a fresh diag engine per budget -> ([result per budget], columns, samples).  fused: whether
    Engine.fused() must say that one kernel serves the (single-resolution) shape."""
    columns, L, budgets = _plan(c)
    x = torch.from_numpy(np.array(_pcm(S, L))).cuda()
    runs = []
    for v in budgets:
        _set_budget(monkeypatch, v)
        with _engine(c) as e:
            if fused is not None:
                assert bool(e.fused(*c["shape"], True)) == fused, "the shape left the route this case is about"
            runs.append(_call(e, c, x, columns))
    return runs, columns, L


def _check_exact(c, runs, ref):
    """Chunked = unchunked, byte for byte; against the reference: bytes, or with the display post-process on its bounds."""
    for k in runs[0]:
        for i, r in enumerate(runs[1:], 1):
            assert _same(r[k], runs[0][k]), _where(r[k], runs[0][k], f"run {i} against the unbudgeted one, {k}")
    got = runs[0]
    if c.get("display"):
        if "db" in got:
            err = float(np.max(np.abs(got["db"] - ref["db"])))
            print(f"MEASURED display {c['entry']} {c['shape']}: max |dB error| {err:.2e}")
            assert err < 2e-3, err
        if "index" in got:
            assert np.max(np.abs(got["index"].astype(np.int32) - ref["index"].astype(np.int32))) <= 1
        return
    for k in got:
        assert _same(got[k], ref[k]), _where(got[k], ref[k], f"unbudgeted run against the reference, {k}")


def _check_fast(c, runs, ref, full_cells):
    for i, got in enumerate(runs):
        err = float(np.max(np.abs(got["db"] - ref["db"]))) if "db" in got else 0.0
        d = np.abs(got["index"].astype(np.int32) - ref["index"].astype(np.int32))
        off, bound = int(np.count_nonzero(d)), max(8, full_cells // 1000)
        print(f"MEASURED FAST {c['entry']} {c['shape']} run {i}: max |dB error| {err:.2e}, index cells off by one {off} (bound {bound}), "
              f"max index step {int(d.max())}")
        assert err < 8.7e-4, err
        assert d.max() <= 1 and off <= bound, (int(d.max()), off, bound)
        if "rgba" in got:
            assert np.array_equal(got["rgba"], O.default_lut()[got["index"]])


def _run_case(c, monkeypatch, fused=None):
    runs, columns, L = _three_runs(c, monkeypatch, fused)
    ref = _reference(_freeze(c), S, L)
    if c["exact"]:
        _check_exact(c, runs, ref)
    else:
        _check_fast(c, runs, ref, S * columns * c.get("rows", 1024))


# ---- the cases: CASES["group:name"] = (case, whether Engine.fused() must hold for the shape or None); the tests below take
# their parameters from it, and tests/test_chunk_ref_cpu.py runs the headers over every one of them
CASES = {}
ALL3 = ("db", "rgba", "index")


def _add(group, name, c, fused=None):
    CASES[f"{group}:{name}"] = (c, fused)


def _ids(group):
    return [k for k in CASES if k.startswith(group + ":")]


# 1. FAST records (d_hist): the ring stops fitting, the rows gate, D = 64
_add("fast_records", "4096/227", case("single", (4096, 227), False, records=True, want=ALL3), False)
_add("fast_records", "4096/512-2048rows", case("single", (4096, 512), False, rows=2048, records=True, want=ALL3), False)
_add("fast_records", "16384/128", case("single", (16384, 128), False, records=True, want=ALL3), False)
# 2. EXACT records (d_hist: two arrays; 16384 / 512 keeps the scatter's low rows in d_xlow, sized for both chunk sizes)
for _n, _hop in ((16384, 512), (8192, 512), (4096, 128)):
    _add("exact_records", f"{_n}/{_hop}", case("single", (_n, _hop), True, records=True, want=ALL3), False)
# 3. the time reduction of the device entry (d_full: dB, then the index at second_array_offset(dB bytes, chunk)).  4096 / 227 is
# a records shape in FAST mode only - EXACT runs it in one kernel - so the EXACT nest d_full -> d_hist takes 8192 / 512
for _f in (4, 64):
    _add("reduce", f"exact-db-index-f{_f}", case("single", (4096, 256), True, f=_f, want=("db", "index")), True)
    _add("reduce", f"exact-index-f{_f}", case("single", (4096, 256), True, f=_f, want=("index",)), True)
    _add("reduce", f"exact-rgba-f{_f}", case("single", (4096, 256), True, f=_f, want=("rgba",)), True)
    _add("reduce", f"exact-display-f{_f}", case("single", (4096, 256), True, f=_f, display=True, want=("db", "index")), True)
    _add("reduce", f"exact-records-8192/512-f{_f}", case("single", (8192, 512), True, f=_f, records=True, want=("db", "index")), False)
    _add("reduce", f"fast-db-index-f{_f}", case("single", (4096, 256), False, f=_f, want=("db", "index")), True)
    _add("reduce", f"fast-records-4096/227-f{_f}", case("single", (4096, 227), False, f=_f, records=True, want=("db", "index")), False)
# 4. the peaks' device entry (d_full)
_add("peaks", "fused-4096/256", case("single", (4096, 256), True, peaks=True), True)
_add("peaks", "records-8192/512", case("single", (8192, 512), True, peaks=True, records=True), False)
# 5. the two-band device entry (d_mres: low plane, high plane, raw plane, each strided by the chunk; with the display
# post-process d_peak + sc * C, and d_post reused per chunk when only the index is wanted)
for _name, _shape in TWO.items():
    _add("two_band", f"exact-{_name}-plain", case("two", _shape, True, want=ALL3))
    _add("two_band", f"exact-{_name}-display", case("two", _shape, True, display=True, want=("db", "index")))
    _add("two_band", f"exact-{_name}-display-index-only", case("two", _shape, True, display=True, want=("index",)))
    _add("two_band", f"fast-{_name}-plain", case("two", _shape, False, want=ALL3))
# 6. the multi-band device entry (d_mres by band_layout); reduce4-display: d_full chunks around d_mres chunks around the records
# bands' d_hist chunks
for _name, _shape in LADDERS.items():
    _add("multi_band", f"exact-{_name}-plain", case("multi", _shape, True, want=ALL3))
    _add("multi_band", f"exact-{_name}-display", case("multi", _shape, True, display=True, want=("db", "index")))
    _add("multi_band", f"exact-{_name}-reduce4-display", case("multi", _shape, True, display=True, f=4, want=("db", "index")))
    _add("multi_band", f"fast-{_name}-plain", case("multi", _shape, False, want=ALL3))
# 7. the host entries, S = 9
_add("host", "batch", case("single", (8192, 512), True, records=True, want=("db", "index")), False)
_add("host", "multires", case("two", TWO["8192"], True, want=("db", "index")))
_add("host", "multiband", case("multi", LADDERS["3x512"], True, want=("db", "index")))
# 8. the one-kernel EXACT routes under the time reduction with short segments (EMSPEC_SEGLEN = 33): their low-row scratch is
# sized per chunk of d_full
_add("short_segments", "1024/64", case("single", (1024, 64), True, f=4, want=("db", "index")), True)
_add("short_segments", "4096/256", case("single", (4096, 256), True, f=4, want=("db", "index")), True)


@pytest.mark.parametrize("key", _ids("fast_records") + _ids("exact_records") + _ids("reduce") + _ids("two_band") + _ids("multi_band"))
def test_three_budgets(key, monkeypatch):
    _run_case(CASES[key][0], monkeypatch, fused=CASES[key][1])


def run_exact_records(n, hop, monkeypatch):
    """What tests/test_gpu_exact.py::test_exact_record_path_stream_chunks runs."""
    c, fused = CASES[f"exact_records:{n}/{hop}"]
    _run_case(c, monkeypatch, fused=fused)


@pytest.mark.parametrize("key", _ids("peaks"))
def test_exact_batch_peaks_device(key, monkeypatch):
    c, fused = CASES[key]
    runs, columns, L = _three_runs(c, monkeypatch, fused=fused)
    db = _reference(_freeze(case("single", c["shape"], True)), S, L)["db"]
    want = P.peaks(db, 8, -60.0)
    assert (want[..., 0] >= 0).any()
    for i, r in enumerate(runs):
        assert _same(r["peaks"], want), _where(r["peaks"].reshape(S, columns, -1), want.reshape(S, columns, -1), f"run {i}, peaks")


def test_exact_multi_band_triple_nest_at_the_band_workspaces_budget(monkeypatch):
    """The triple nest again at the budget that gives d_mres - not d_full - chunks of two: d_full then runs (4, 1)."""
    c = CASES["multi_band:exact-3x512-reduce4-display"][0]
    columns, b = K.frames_for(lambda cols: K.path(c, cols)[1][1])
    inner = K.path(c, columns)[1]
    assert inner[0].startswith("d_mres")
    L = 8192 + 512 * (columns - 1) + 3
    for line in K.expected(c, columns, b, S):
        print("EXPECTED", line)
    outer = K.outer_chunks(c, columns, b, S)
    assert len(outer) >= 2 and K.chunks(b, inner[1], outer[0])[0] == 2 and K.chunks(b, inner[1], outer[0])[-1] <= 2
    x = torch.from_numpy(np.array(_pcm(S, L))).cuda()
    runs = []
    for v in (None, b):
        _set_budget(monkeypatch, v)
        with _engine(c) as e:
            runs.append(_call(e, c, x, columns))
    _check_exact(c, runs, _reference(_freeze(c), S, L))


def _host(e, c, pcm):
    want = c["want"]
    if c["entry"] == "single":
        return e.batch(pcm, *c["shape"], True, want=want)
    if c["entry"] == "two":
        return e.batch_multires(pcm, *c["shape"], True, want=want)
    n, hop, splits = c["shape"]
    return e.batch_multiband(pcm, n, splits, hop, True, want=want)


@pytest.mark.parametrize("key", _ids("host"))
def test_exact_host_entries_over_a_budget(key, monkeypatch):
    """S = 9: the pipeline cuts units of whole streams (the two composed entries: at least four per unit), and every unit is
    chunked by the budget inside.  The bytes are the device entry's unbudgeted ones."""
    c, streams = CASES[key][0], 9
    columns, b = K.columns_and_budget(c)
    n0, hop = _n0_hop(c)
    L = n0 + hop * (columns - 1) + 3
    pcm = _pcm(streams, L)
    for unit in (9, 5, 4, 1):
        print(f"EXPECTED in a unit of {unit} streams:", "; ".join(K.expected(c, columns, b, unit)))
    assert K.outer_chunks(c, columns, b, 4) == (2, 2) and K.outer_chunks(c, columns, b, 9)[-1] == 1
    _set_budget(monkeypatch, None)
    with _engine(c) as e:
        want = _call(e, c, torch.from_numpy(np.array(pcm)).cuda(), columns)
    for v in (b, 0):
        _set_budget(monkeypatch, v)
        with _engine(c) as e:
            got = _host(e, c, pcm)
            e.device_status()
        for k in want:
            assert _same(got[k], want[k]), _where(got[k], want[k], f"host entry at budget {v}, {k}")


@pytest.mark.parametrize("key", _ids("short_segments"))
def test_exact_fused_routes_under_the_time_reduction_with_short_segments(key, monkeypatch):
    monkeypatch.setenv("EMSPEC_SEGLEN", "33")
    _run_case(CASES[key][0], monkeypatch, fused=CASES[key][1])
