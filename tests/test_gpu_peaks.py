"""GPU: the spectral peaks (include/emspec.h: emspec_peaks_device, emspec_batch_peaks*,
emspec_position_hz).  The standalone kernel and every batch entry against tests/peaks_ref.py - byte for byte wherever the dB
is the same bytes: always for the standalone kernel, in EXACT mode for the batch entries - the FAST mode within the bounds that
follow from the project's dB tolerance, a known answer, the refusals, and the Node addon."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emspec
import oracle as O
import peaks_ref as P
from emspec import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPS_DB = 8.7e-4          # the project's dB tolerance of the FAST mode against the float32 bit model
K, MIN_DB = 8, -60.0     # the batch tests' parameters


def _same(a, b):
    return a.shape == b.shape and np.array_equal(P.bits(a), P.bits(b))


def _dev_peaks(e, db, k, min_db):
    """emspec_peaks_device on a numpy dB array -> numpy peaks; the output is poisoned first."""
    t = torch.from_numpy(np.ascontiguousarray(db, F)).cuda()
    out = torch.full(tuple(t.shape[:-1]) + (k, 2), 7.0, dtype=torch.float32, device="cuda")
    e.peaks_device(t, k, min_db, out=out)
    torch.cuda.synchronize()
    e.device_status()
    return out.cpu().numpy()


def _batch_peaks_device(e, x, n, hop, reassign=True, k=K, min_db=MIN_DB):
    out = torch.full((x.shape[0], emspec.num_columns(x.shape[1], n, hop), k, 2), 7.0, dtype=torch.float32, device="cuda")
    e.batch_peaks_device(x, n, hop, reassign, k, min_db, out=out)
    torch.cuda.synchronize()
    e.device_status()
    return out.cpu().numpy()


def _batch_db_device(e, x, n, hop, reassign=True):
    db = torch.empty((x.shape[0], emspec.num_columns(x.shape[1], n, hop), e.rows), dtype=torch.float32, device="cuda")
    e.batch_device(x, n, hop, reassign, db=db)
    torch.cuda.synchronize()
    return db


def _pinned_batch_peaks(e, pcm, n, hop, k=K, min_db=MIN_DB):
    S, L = pcm.shape
    Cn = emspec.num_columns(L, n, hop)
    pin = [emspec.PinnedArray((S, L), np.float32), emspec.PinnedArray((S, Cn, k, 2), np.float32)]
    try:
        pin[0].array[:] = pcm
        pin[1].array[:] = 7.0
        return e.batch_peaks(pin[0].array, n, hop, True, k, min_db, out=pin[1].array).copy()
    finally:
        for p in pin:
            p.close()


# ---- 1. the standalone kernel on the CPU tests' columns
@pytest.mark.parametrize("R", [4, 64, 100, 1024, 4096])
def test_kernel_equals_the_reference_on_the_cpu_cases(engine, R):
    """Every column of peaks_ref.cases(R), repeated (rotated) to 1, 3, 257 and 1,000 columns, k = 1, 8 and 32."""
    ref = {}
    for min_db, cols in P.all_columns(R).items():
        for count in (1, 3, 257, 1000):
            first = (count * 7) % cols.shape[0]
            db = np.take(cols, np.arange(first, first + count) % cols.shape[0], axis=0)
            for k in (1, 8, 32):
                got = _dev_peaks(engine, db, k, min_db)
                key = (min_db, k)
                if key not in ref:
                    ref[key] = P.peaks(cols, k, min_db)
                want = np.take(ref[key], np.arange(first, first + count) % cols.shape[0], axis=0)
                bad = np.nonzero(np.any(P.bits(got) != P.bits(want), axis=(1, 2)))[0]
                assert bad.size == 0, (R, min_db, count, k, bad[:4], got[bad[:1]], want[bad[:1]])


def test_kernel_on_a_range_16_bytes_into_an_allocation(engine):
    R, cols, k = 100, 41, 8
    db = np.concatenate([c for _, c, m in P.cases(R) if m == -60.0])[:cols]
    buf = torch.zeros(4 + cols * R + 4, dtype=torch.float32, device="cuda")
    view = buf[4:4 + cols * R].view(cols, R)
    view.copy_(torch.from_numpy(db))
    assert buf.data_ptr() % 256 == 0 and view.data_ptr() == buf.data_ptr() + 16
    got = engine.peaks_device(view, k, -60.0)
    torch.cuda.synchronize()
    assert _same(got.cpu().numpy(), P.peaks(db, k, -60.0))
    assert emspec.OK == engine._lib.emspec_peaks_device(engine._h, None, 0, R, k, -60.0, None, None)   # no columns: a no-op


def test_kernel_past_2_to_31_cells(engine):
    """2^19 + 1 columns of 4,096 rows: the last column starts at cell 2^31, byte 2^33.  Column c holds case column c % 37 -
    2^18 = -1 and 2^19 = -2 (mod 37), so an offset that wrapped at 2^32 bytes or 2^31 cells reads another column."""
    R, k, cols = 4096, 8, (1 << 19) + 1
    need = cols * R * 4 + cols * k * 8 + (1 << 28)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
    base = np.concatenate([c for _, c, m in P.cases(R) if m == -60.0])[:37]
    assert base.shape == (37, R)
    tb = torch.from_numpy(base).cuda()
    big = torch.empty((cols, R), dtype=torch.float32, device="cuda")
    whole = cols // 37
    big[:whole * 37].view(whole, 37, R).copy_(tb.unsqueeze(0).expand(whole, 37, R))
    big[whole * 37:].copy_(tb[:cols - whole * 37])
    out = engine.peaks_device(big, k, -60.0)
    torch.cuda.synchronize()
    engine.device_status()
    want = P.peaks(base, k, -60.0)
    chosen = np.array([0, 1, 36, 37, 4095, 4096, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 19) - 2, (1 << 19) - 1, 1 << 19])
    got = out[torch.from_numpy(chosen).cuda()].cpu().numpy()
    assert _same(got, want[chosen % 37])
    # and every column, on the device: the output is the 37 lists repeated
    tw = torch.from_numpy(want).cuda().view(torch.int32)
    oi = out.view(torch.int32)
    assert torch.equal(oi[:whole * 37].view(whole, 37, k, 2), tw.unsqueeze(0).expand(whole, 37, k, 2))
    assert torch.equal(oi[whole * 37:], tw[:cols - whole * 37])


# ---- 2. EXACT, device entry: the bytes of peaks_ref over the binary64 bit model's dB
@pytest.mark.parametrize("n,hop,reassign,L", [(1024, 256, True, 1 << 15), (4096, 256, True, 1 << 15), (4096, 256, False, 1 << 15),
                                              (16384, 512, True, 1 << 16)])
def test_exact_device_entry_equals_the_bit_model(n, hop, reassign, L):
    pcm = synth.streams(3, L)
    odb = O.batch_exact(O.make_cfg(n, hop, reassign), pcm, want=("db",))[0]
    want = P.peaks(odb, K, MIN_DB)
    assert (want[..., 0] >= 0).mean() > 0.25            # the signal has peaks above min_db: the comparison is not of empty lists
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        got = _batch_peaks_device(e, torch.from_numpy(pcm).cuda(), n, hop, reassign)
    assert _same(got, want)


# ---- 3. EXACT, host entry = the device entry: pinned and pageable, whole streams, several units, runs of one long stream
@pytest.mark.parametrize("S,L", [(3, 1 << 15), (40, 1 << 17)])
def test_exact_host_entry_equals_the_device_entry(S, L):
    n, hop = 4096, 256
    pcm = synth.streams(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        dev = _batch_peaks_device(e, torch.from_numpy(pcm).cuda(), n, hop)
        assert (dev[..., 0] >= 0).any()
        assert _same(e.batch_peaks(pcm, n, hop, True, K, MIN_DB, out=np.full(dev.shape, 7.0, F)), dev), "pageable"
        assert _same(_pinned_batch_peaks(e, pcm, n, hop), dev), "pinned"


def test_exact_one_long_stream_cut_into_runs():
    """ONE stream of 49,158 columns (the length tests/test_gpu_overview.py cuts into three runs of >= 16,384 columns)."""
    n, hop = 4096, 256
    Cn = 3 * 16384 + 6
    pcm = synth.streams(1, n + hop * (Cn - 1))
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        x = torch.from_numpy(pcm).cuda()
        dev = _batch_peaks_device(e, x, n, hop)
        ref = P.peaks(_batch_db_device(e, x, n, hop).cpu().numpy(), K, MIN_DB)
        del x
        assert _same(dev, ref), "device entry vs the reference on the engine's own dB"
        assert _same(e.batch_peaks(pcm, n, hop, True, K, MIN_DB), dev), "pageable"
        assert _same(_pinned_batch_peaks(e, pcm, n, hop), dev), "pinned"


# ---- 4. EXACT with the display post-process on
def test_exact_display_postprocess_on():
    n, hop, S, L = 4096, 256, 6, 1 << 17
    pcm = synth.streams(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_display(0.6, 0.8)
        want = P.peaks(e.batch(pcm, n, hop, True, want=("db",))["db"], K, MIN_DB)
        assert (want[..., 0] >= 0).any()
        assert _same(_batch_peaks_device(e, torch.from_numpy(pcm).cuda(), n, hop), want), "device"
        assert _same(e.batch_peaks(pcm, n, hop, True, K, MIN_DB), want), "pageable"
        assert _same(_pinned_batch_peaks(e, pcm, n, hop), want), "pinned"


# ---- 5. EXACT, multi-resolution: the standalone kernel on the composed dB
def test_exact_multires_db_through_the_standalone_kernel():
    n_low, n_high, hop, S, L = 16384, 4096, 256, 3, 1 << 16
    pcm = synth.streams(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        split = e.split_row_for_hz(250.0)
        x = torch.from_numpy(pcm).cuda()
        db = torch.empty((S, emspec.multires_columns(L, n_low, n_high, hop), e.rows), dtype=torch.float32, device="cuda")
        e.batch_multires_device(x, n_low, n_high, hop, split, True, db=db)
        got = e.peaks_device(db, K, MIN_DB)
        torch.cuda.synchronize()
        e.device_status()
        want = P.peaks(db.cpu().numpy(), K, MIN_DB)
        assert (want[..., 0] >= 0).any()
        assert _same(got.cpu().numpy(), want)
        # the host twin on the host entry's columns
        hdb = e.batch_multires(pcm, n_low, n_high, hop, split, True, want=("db",))["db"]
        assert _same(emspec.peaks_host(hdb, K, MIN_DB), want)


# ---- 6. FAST
def test_fast_kernel_on_the_engines_own_db(engine):
    """(a) Cell sums arrive in any order in FAST mode, so two launches may differ in the last bits: the kernel is compared on
    ONE dB array the engine wrote, byte for byte."""
    n, hop = 4096, 256
    x = torch.from_numpy(synth.streams(3, 1 << 16)).cuda()
    db = _batch_db_device(engine, x, n, hop)
    got = engine.peaks_device(db, K, MIN_DB)
    torch.cuda.synchronize()
    want = P.peaks(db.cpu().numpy(), K, MIN_DB)
    assert (want[..., 0] >= 0).any()
    assert _same(got.cpu().numpy(), want)


def test_fast_end_to_end_on_four_tones(engine):
    """(b) Four steady tones 4.4 dB apart or more, k = 4, min_db = -60 (the float32 bit model's next local maximum is below
    -67 dB).  Against peaks_ref of the float32 bit model's dB: the same rows; dB within EPS_DB; pos within 3 EPS_DB / |u| + 2 ulp,
    u the reference's denominator - the numerator of d moves by at most EPS_DB (half of 2 EPS_DB), the denominator by at most
    4 EPS_DB, and |d| <= 0.5, so d moves by (EPS_DB + 0.5 * 4 EPS_DB) / |u| to first order."""
    n, hop, L, k = 4096, 256, 1 << 15, 4
    t = np.arange(L) / 48000.0
    pcm = sum(a * np.sin(2 * np.pi * f * t) for f, a in ((440.0, 0.5), (1000.0, 0.3), (2500.0, 0.18), (6100.0, 0.1)))
    pcm = pcm.astype(F)[None]
    odb = O.batch_f32(O.make_cfg(n, hop, True), pcm, want=("db",))[0]
    want = P.peaks(odb, k, MIN_DB)
    assert np.all(want[..., 0] >= 0)                     # four peaks in every column
    got = _batch_peaks_device(engine, torch.from_numpy(pcm).cuda(), n, hop, True, k, MIN_DB)
    host = engine.batch_peaks(pcm, n, hop, True, k, MIN_DB)
    _, _, _, u = P.parts(odb[0], MIN_DB)
    for name, g in (("device", got), ("host", host)):
        rows_w, rows_g = np.floor(want[0, :, :, 0]).astype(int), np.floor(g[0, :, :, 0]).astype(int)
        db_err = float(np.max(np.abs(g[0, :, :, 1] - want[0, :, :, 1])))
        uu = np.abs(np.take_along_axis(u, rows_w, axis=1))
        bound = 3 * EPS_DB / uu + 2 * np.spacing(want[0, :, :, 0])
        pos_err = np.abs(g[0, :, :, 0].astype(np.float64) - want[0, :, :, 0])
        print(f"{name}: rows differ in {int((rows_w != rows_g).sum())} of {rows_w.size} slots; max dB error {db_err:.3e} "
              f"(bound {EPS_DB:.1e}); max pos error / bound {float(np.max(pos_err / bound)):.3f}; min |u| {float(uu.min()):.2f}")
        assert np.array_equal(rows_w, rows_g), name
        assert db_err <= EPS_DB, (name, db_err)
        assert np.all(pos_err <= bound), (name, float(np.max(pos_err / bound)))


# ---- 7. a known answer
def test_known_answer_440_hz():
    """A 440 Hz sine, EXACT, N = 4096 / hop 256: from column D on, the first peak's row holds 440 Hz between its edges, and so
    does emspec_position_hz of its position - the half-row statement of the header and no stronger."""
    n, hop, L = 4096, 256, 1 << 15
    pcm = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(L) / 48000.0)).astype(F)[None]
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        p = _batch_peaks_device(e, torch.from_numpy(pcm).cuda(), n, hop)[0]
        edges = e.row_edges_hz().astype(np.float64)
        D = emspec.latency_columns(n, hop, True)
        assert p.shape[0] > D + 10
        for c in range(D, p.shape[0]):
            pos = float(p[c, 0, 0])
            r = int(np.floor(pos))
            assert 0 <= r < e.rows and edges[r] <= 440.0 < edges[r + 1], (c, pos, edges[r], edges[r + 1])
            hz = e.position_hz(pos)
            assert edges[r] <= hz <= edges[r + 1], (c, pos, hz)
        # the formula, against the edge table: edges at integer positions, the geometric centre at r + 0.5
        for r in (0, 1, 511, e.rows - 1):
            assert abs(e.position_hz(float(r)) / edges[r] - 1) < 1e-12
            assert abs(e.position_hz(r + 0.5) / np.sqrt(edges[r] * edges[r + 1]) - 1) < 1e-12
        assert abs(e.position_hz(float(e.rows)) / edges[e.rows] - 1) < 1e-12
        for bad in (-0.001, e.rows + 0.5, float("nan")):
            with pytest.raises(emspec.EmspecError, match="pos must be"):
                e.position_hz(bad)
        assert e.position_hz(3.25) > 0


# ---- 8. refusals
def test_refusals_leave_the_engine_usable():
    n, hop, S, L, R = 4096, 256, 2, 1 << 15, 1024
    pcm = synth.streams(S, L)
    Cn = emspec.num_columns(L, n, hop)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        lib, h = e._lib, e._h
        x = torch.from_numpy(pcm).cuda()
        db = _batch_db_device(e, x, n, hop)
        good_dev = e.peaks_device(db, K, MIN_DB)
        torch.cuda.synchronize()
        good = good_dev.cpu().numpy()
        out = torch.zeros((S, Cn, 32, 2), dtype=torch.float32, device="cuda")
        hout = np.zeros((S, Cn, 32, 2), F)
        p = lambda t: C.c_void_p(t.data_ptr())
        hp = lambda a: C.c_void_p(a.ctypes.data)

        def refused(rc, word, code=emspec.ERR_INVALID_ARG):
            assert rc == code, (rc, word)
            assert word in lib.emspec_last_error(h).decode(), (word, lib.emspec_last_error(h).decode())
            # a good call on the same engine succeeds, with the same bytes
            again = e.peaks_device(db, K, MIN_DB)
            torch.cuda.synchronize()
            assert torch.equal(again.view(torch.int32), good_dev.view(torch.int32))

        standalone = lambda d, cols, rows, k, m, o: lib.emspec_peaks_device(h, d, cols, rows, k, m, o, None)
        bdev = lambda xx, k, m, o: lib.emspec_batch_peaks_device(h, xx, S, L, n, hop, 1, k, m, o, None)
        bhost = lambda xx, k, m, o: lib.emspec_batch_peaks(h, xx, S, L, n, hop, 1, k, m, o)
        for k in (0, 33, -3):
            refused(standalone(p(db), S * Cn, R, k, MIN_DB, p(out)), "k must be in [1, 32]")
            refused(bdev(p(x), k, MIN_DB, p(out)), "k must be in [1, 32]")
            refused(bhost(hp(pcm), k, MIN_DB, hp(hout)), "k must be in [1, 32]")
        nan = float("nan")
        refused(standalone(p(db), S * Cn, R, K, nan, p(out)), "NaN")
        refused(bdev(p(x), K, nan, p(out)), "NaN")
        refused(bhost(hp(pcm), K, nan, hp(hout)), "NaN")
        for rows in (0, 2, 1022, 4100, -8):
            refused(standalone(p(db), 4, rows, K, MIN_DB, p(out)), "rows % 4 == 0")
        refused(standalone(p(db), -1, R, K, MIN_DB, p(out)), "columns")
        refused(standalone(None, 4, R, K, MIN_DB, p(out)), "null")
        refused(standalone(p(db), 4, R, K, MIN_DB, None), "null")
        refused(bdev(None, K, MIN_DB, p(out)), "null")
        refused(bdev(p(x), K, MIN_DB, None), "null")
        refused(bhost(None, K, MIN_DB, hp(hout)), "null")
        refused(bhost(hp(pcm), K, MIN_DB, None), "null")
        refused(standalone(C.c_void_p(db.data_ptr() + 4), 4, R, K, MIN_DB, p(out)), "16-byte aligned")
        refused(standalone(p(db), 4, R, K, MIN_DB, C.c_void_p(out.data_ptr() + 4)), "8-byte aligned")
        refused(bdev(p(x), K, MIN_DB, C.c_void_p(out.data_ptr() + 4)), "8-byte aligned")
        refused(bhost(hp(pcm), K, MIN_DB, C.c_void_p(hout.ctypes.data + 4)), "8-byte aligned")
        refused(lib.emspec_batch_peaks_device(h, p(x), S, L, 4000, hop, 1, K, MIN_DB, p(out), None), "")      # a shape that is not accepted
        assert not out.any().item() and not hout.any()            # no refusal wrote anything
        # while a time reduction is set: the two batch entries are a state error, the standalone calls are not affected
        e.set_time_reduce(4)
        refused(bdev(p(x), K, MIN_DB, p(out)), "time reduction", emspec.ERR_STATE)
        refused(bhost(hp(pcm), K, MIN_DB, hp(hout)), "time reduction", emspec.ERR_STATE)
        assert _same(emspec.peaks_host(db.cpu().numpy(), K, MIN_DB), good)
        e.set_time_reduce(1)
        assert _same(_batch_peaks_device(e, x, n, hop), good)
        assert _same(e.batch_peaks(pcm, n, hop, True, K, MIN_DB), good)


def test_exact_rows_not_a_multiple_of_16():
    """rows = 1000 (every engine's rows are a multiple of 4 in [64, 4096], so the batch entries' rows always satisfy the kernel's
    rule): 250 quads, the last load round partly empty."""
    n, hop, S, L = 4096, 256, 2, 1 << 15
    pcm = synth.streams(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT, rows=1000) as e:
        x = torch.from_numpy(pcm).cuda()
        want = P.peaks(_batch_db_device(e, x, n, hop).cpu().numpy(), K, MIN_DB)
        assert (want[..., 0] >= 0).any()
        assert _same(_batch_peaks_device(e, x, n, hop), want)
        assert _same(e.batch_peaks(pcm, n, hop, True, K, MIN_DB), want)


# ---- 9. Node: the addon returns the ctypes binding's bytes
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_peaks_match_ctypes(tmp_path):
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_peaks.js", str(tmp_path)], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    S, L, n, hop, k, min_db = res["S"], res["L"], res["fftSize"], res["hop"], res["k"], res["minDb"]
    pcm = np.fromfile(str(tmp_path / "pcm.f32"), np.float32).reshape(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        Cn = emspec.num_columns(L, n, hop)
        assert Cn == res["columns"]
        want = e.batch_peaks(pcm, n, hop, True, k, min_db)
        assert (want[..., 0] >= 0).any()
        assert _same(np.fromfile(str(tmp_path / "peaks.f32"), np.float32).reshape(S, Cn, k, 2), want)
        db = e.batch(pcm, n, hop, True, want=("db",))["db"]
        assert _same(np.fromfile(str(tmp_path / "peaks_of.f32"), np.float32).reshape(S, Cn, k, 2), emspec.peaks_host(db, k, min_db))
        for pos, hz in zip(res["positions"], res["hz"]):
            assert abs(hz / e.position_hz(pos) - 1) < 1e-15
    notes = {round(v["hz"], 4): (v["name"], v["octave"], v["cents"]) for v in res["notes"]}
    assert notes[440.0] == ("A", 4, 0) and notes[27.5] == ("A", 0, 0)
    assert notes[261.6256][:2] == ("C", 4) and abs(notes[261.6256][2]) < 0.01
