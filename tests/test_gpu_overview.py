"""GPU: the time reduction (emspec_set_time_reduce) against its definition - tests/overview_ref.py applied to
the CPU bit models' full-rate columns - through every batch entry, with the display post-process, its refusals and its
memory bound."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emspec
import multires_ref as M
import oracle as O
import overview_ref as V
import pcm_ref as P
from emspec import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = ("db", "rgba", "index")
BOUNDS_PATH = os.path.join(ROOT, "tests", "golden", "overview_bounds.json")


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _device(e, x, n, hop, reassign=True, want=WANT, multires=None):
    """The device entry at the engine's factor -> numpy arrays [S][Cr][R] (+[4])."""
    S, L = x.shape
    Cn = emspec.num_columns(L, multires[0] if multires else n, hop)
    Cr = emspec.reduced_columns(Cn, e.time_reduce)
    t = {"db": torch.empty((S, Cr, e.rows), dtype=torch.float32, device="cuda") if "db" in want else None,
         "rgba": torch.empty((S, Cr, e.rows, 4), dtype=torch.uint8, device="cuda") if "rgba" in want else None,
         "index": torch.empty((S, Cr, e.rows), dtype=torch.uint8, device="cuda") if "index" in want else None}
    for v in t.values():
        if v is not None:
            v.fill_(0x5A if v.dtype == torch.uint8 else -1.0)
    if multires:
        e.batch_multires_device(x, multires[0], multires[1], hop, multires[2], reassign, **t)
    else:
        e.batch_device(x, n, hop, reassign, **t)
    torch.cuda.synchronize()
    e.device_status()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in t.items()}


def _pinned_batch(e, pcm, n, hop, Cr):
    S, L = pcm.shape
    pin = {"pcm": emspec.PinnedArray((S, L), np.float32), "db": emspec.PinnedArray((S, Cr, e.rows), np.float32),
           "rgba": emspec.PinnedArray((S, Cr, e.rows, 4), np.uint8), "index": emspec.PinnedArray((S, Cr, e.rows), np.uint8)}
    try:
        pin["pcm"].array[:] = pcm
        out = emspec.Out(pin["db"].array.ctypes.data, pin["rgba"].array.ctypes.data, pin["index"].array.ctypes.data)
        e._chk(e._lib.emspec_batch(e._h, C.c_void_p(pin["pcm"].array.ctypes.data), S, L, n, hop, 1, C.byref(out)))
        return {k: pin[k].array.copy() for k in WANT}
    finally:
        for p in pin.values():
            p.close()


def _unpack(e, wire, off, S, Cr):
    return np.stack([emspec.wire_unpack_host(wire[off[s]:off[s + 1]], Cr, e.rows) for s in range(S)])


# ---- 1. EXACT, device entry: the bytes of overview_ref over the binary64 bit model's columns
@pytest.mark.parametrize("n,hop,reassign", [(4096, 256, True), (1024, 256, False), (2048, 128, True), (8192, 512, True),
                                            (16384, 512, True)])
def test_exact_device_entry_equals_the_reduced_bit_model(n, hop, reassign):
    Cn = 100
    pcm = synth.streams(2, n + hop * (Cn - 1))
    full = dict(zip(("db", "rgba", "index"), O.batch_exact(O.make_cfg(n, hop, reassign), pcm, want=WANT)[:3]))
    x = torch.from_numpy(pcm).cuda()
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        for f in (2, 3, 16, 7, 128):      # 100 % 3, 100 % 16 and 100 % 7 != 0; 128 > C: a single column
            e.set_time_reduce(f)
            assert e.time_reduce == f
            want = V.reduce(full, f, O.default_lut())
            assert want["index"].shape == (2, emspec.reduced_columns(Cn, f), e.rows)
            got = _device(e, x, n, hop, reassign)
            for k in WANT:
                assert _same(got[k], want[k]), (f, k)
            # index / RGBA alone: the path that reads no dB
            alone = _device(e, x, n, hop, reassign, want=("rgba",))
            assert _same(alone["rgba"], want["rgba"]), (f, "rgba alone")
            alone = _device(e, x, n, hop, reassign, want=("db",))
            assert _same(alone["db"], want["db"]), (f, "db alone")


def test_exact_device_entry_rows_not_a_multiple_of_16():
    """rows = 1000 (a multiple of 4 only): the kernel's 4-row form."""
    n, hop, Cn = 4096, 256, 37
    pcm = synth.streams(2, n + hop * (Cn - 1))
    x = torch.from_numpy(pcm).cuda()
    with emspec.Engine(mode=emspec.MODE_EXACT, rows=1000) as e:
        full = _device(e, x, n, hop)
        e.set_time_reduce(5)
        got = _device(e, x, n, hop)
        lut = O.default_lut()
    want = V.reduce(full, 5, lut)
    for k in WANT:
        assert _same(got[k], want[k]), k


# ---- 2. EXACT: every host entry equals the device entry byte for byte
@pytest.mark.parametrize("f", [4, 7])
def test_exact_host_entries_equal_the_device_entry(f):
    n, hop, S, L = 4096, 256, 20, 1 << 18
    pcm = synth.streams(S, L)
    Cn = emspec.num_columns(L, n, hop)
    Cr = emspec.reduced_columns(Cn, f)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        x = torch.from_numpy(pcm).cuda()
        full = _device(e, x, n, hop)
        e.set_time_reduce(f)
        dev = _device(e, x, n, hop)
        ref = V.reduce(full, f, O.default_lut())
        for k in WANT:
            assert _same(dev[k], ref[k]), ("device vs the reduced full-rate output", k)
        got = e.batch(pcm, n, hop, True, want=WANT)                    # pageable: drainer and touchers
        for k in WANT:
            assert _same(got[k], dev[k]), ("pageable", k)
        got = _pinned_batch(e, pcm, n, hop, Cr)
        for k in WANT:
            assert _same(got[k], dev[k]), ("pinned", k)
        wire, off = e.batch_packed(pcm, n, hop, True)
        assert wire.size == S * emspec.wire_bound(Cr, e.rows)
        assert _same(_unpack(e, wire, off, S, Cr), dev["index"]), "packed"
        hdr = wire[:32].view(np.uint32)
        assert int(hdr[2]) | (int(hdr[3]) << 32) == Cr                 # the header's column count
        del x


@pytest.mark.parametrize("f", [3, 16])
def test_exact_pcm_entries_equal_the_device_entry_on_the_decoded_streams(f):
    n, hop, sources, frames = 4096, 256, 5, 1 << 17
    rng = np.random.default_rng(7)
    st = synth.streams(2 * sources, frames)
    raw = np.clip(np.round(st.reshape(sources, 2, frames).transpose(0, 2, 1) * 20000.0 + rng.integers(-3, 4, (sources, frames, 2))),
                  -32768, 32767).astype(np.int16)
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
    dec = P.decode(raw.reshape(sources, -1).view(np.uint8), P.S16, 2, fmt.matrix)
    S = sources * 4
    Cr = emspec.reduced_columns(emspec.num_columns(frames, n, hop), f)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_time_reduce(f)
        dev = _device(e, torch.from_numpy(dec).cuda(), n, hop)
        got = e.batch_pcm(raw.reshape(sources, -1), fmt, n, hop, True, want=WANT)
        for k in WANT:
            assert _same(got[k], dev[k]), ("batch_pcm", k)
        wire, off = e.batch_pcm_packed(raw.reshape(sources, -1), fmt, n, hop, True)
        assert _same(_unpack(e, wire, off, S, Cr), dev["index"]), "batch_pcm_packed"


@pytest.mark.parametrize("f", [2, 9])
def test_exact_multires_entries(f):
    """emspec_batch_multires_device at factor f = overview_ref of the bit model's composition; the host entry = its twin."""
    n_low, n_high, hop, S, L = 16384, 4096, 256, 8, 1 << 17
    pcm = synth.streams(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        split = e.split_row_for_hz(250.0)
        x = torch.from_numpy(pcm).cuda()
        e.set_time_reduce(f)
        dev = _device(e, x, None, hop, multires=(n_low, n_high, split))
        got = e.batch_multires(pcm, n_low, n_high, hop, split, True, want=WANT)
    want = V.reduce(M.compose(pcm, n_low, n_high, hop, split, True, exact=True), f, O.default_lut())
    for k in WANT:
        assert _same(dev[k], want[k]), ("device", k)
        assert _same(got[k], dev[k]), ("host", k)


@pytest.mark.parametrize("f", [7, 1000])
def test_one_long_stream_cut_into_runs(f):
    """ONE stream of 49,158 columns: fewer than sixteen streams, so the host pipeline cuts it into runs of >= 16,384 columns
    (three here: pipe_units asks for three units and C / 16384 = 3 allows them), whose starts are multiples of f.  Host entries
    (pageable and page-locked) = the device entry = overview_ref of the engine's own full-rate columns."""
    n, hop = 4096, 256
    Cn = 3 * 16384 + 6
    L = n + hop * (Cn - 1)
    pcm = synth.streams(1, L)
    Cr = emspec.reduced_columns(Cn, f)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        x = torch.from_numpy(pcm).cuda()
        full = _device(e, x, n, hop, want=("db", "index"))
        e.set_time_reduce(f)
        dev = _device(e, x, n, hop)
        del x
        ref = V.reduce(full, f, O.default_lut())
        assert _same(dev["db"], ref["db"]) and _same(dev["index"], ref["index"])
        assert np.array_equal(dev["rgba"], O.default_lut()[dev["index"]])
        got = e.batch(pcm, n, hop, True, want=WANT)
        for k in WANT:
            assert _same(got[k], dev[k]), ("pageable", k)
        got = _pinned_batch(e, pcm, n, hop, Cr)
        for k in WANT:
            assert _same(got[k], dev[k]), ("pinned", k)
        idx_only = e.batch(pcm, n, hop, True, want=("index",))
        assert _same(idx_only["index"], dev["index"])


# ---- 3. EXACT with the display post-process on: smoothing and AGC at full rate, the reduction behind them
def test_exact_display_postprocess_runs_at_full_rate():
    n, hop, S, L, f = 4096, 256, 6, 1 << 18, 5
    pcm = synth.streams(S, L)
    Cr = emspec.reduced_columns(emspec.num_columns(L, n, hop), f)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_display(0.6, 0.8)
        x = torch.from_numpy(pcm).cuda()
        full = _device(e, x, n, hop)
        e.set_time_reduce(f)
        want = V.reduce(full, f, O.default_lut())
        dev = _device(e, x, n, hop)
        for k in WANT:
            assert _same(dev[k], want[k]), ("device", k)
        got = e.batch(pcm, n, hop, True, want=WANT)
        for k in WANT:
            assert _same(got[k], want[k]), ("pageable", k)
        got = _pinned_batch(e, pcm, n, hop, Cr)
        for k in WANT:
            assert _same(got[k], want[k]), ("pinned", k)
        wire, off = e.batch_packed(pcm, n, hop, True)
        assert _same(_unpack(e, wire, off, S, Cr), want["index"]), "packed"
        split = e.split_row_for_hz(250.0)
        e.set_time_reduce(1)
        mfull = _device(e, x, None, hop, multires=(16384, 4096, split))
        e.set_time_reduce(f)
        mwant = V.reduce(mfull, f, O.default_lut())
        mdev = _device(e, x, None, hop, multires=(16384, 4096, split))
        mhost = e.batch_multires(pcm, 16384, 4096, hop, split, True, want=WANT)
        for k in WANT:
            assert _same(mdev[k], mwant[k]), ("multires device", k)
            assert _same(mhost[k], mwant[k]), ("multires host", k)


# ---- 4. FAST against overview_ref of the float32 bit model's columns
@pytest.mark.parametrize("n,hop,f", [(4096, 256, 3), (4096, 256, 16), (1024, 256, 3), (1024, 256, 16), (16384, 512, 3),
                                     (16384, 512, 16)])
def test_fast_within_the_design_tolerances(n, hop, f):
    """dB within the project's 8.7e-4 dB on the cells the bit model puts above -60 dB, the palette index at most one step
    off, on a share of the cells bounded at 2 x the share measured on an MI355X (tests/golden/overview_bounds.json: a maximum
    over f cells can differ wherever any of the f cells did, so the bound is measured per case, not derived)."""
    Cn = 480
    pcm = synth.streams(2, n + hop * (Cn - 1))
    db, rgba, idx = O.batch_f32(O.make_cfg(n, hop, True), pcm, want=WANT)
    want = V.reduce({"db": db, "rgba": rgba, "index": idx}, f, O.default_lut())
    with emspec.Engine() as e:
        e.set_time_reduce(f)
        got = e.batch(pcm, n, hop, True, want=WANT)
        dev = _device(e, torch.from_numpy(pcm).cuda(), n, hop)
    strong = want["db"] > -60.0
    err = float(np.max(np.abs(got["db"][strong] - want["db"][strong])))
    di = np.abs(got["index"].astype(np.int32) - want["index"].astype(np.int32))
    share = float(np.mean(di != 0))
    errd = float(np.max(np.abs(dev["db"][strong] - want["db"][strong])))
    did = np.abs(dev["index"].astype(np.int32) - want["index"].astype(np.int32))
    shared = float(np.mean(did != 0))
    print(f"MEASURED overview FAST {n}/{hop}/f{f}: cells {di.size}, max dB err {err:.3e} (device entry {errd:.3e}), "
          f"index share {share:.6e} (device entry {shared:.6e}), max step {int(di.max())}")
    assert np.array_equal(got["rgba"], O.default_lut()[got["index"]]) and np.array_equal(dev["rgba"], O.default_lut()[dev["index"]])
    assert err <= 8.7e-4 and errd <= 8.7e-4, (err, errd)
    assert di.max() <= 1 and did.max() <= 1
    bounds = json.load(open(BOUNDS_PATH))
    bound = bounds[f"{n}/{hop}/f{f}"]["index_share_bound"]
    assert share <= bound and shared <= bound, (share, shared, bound)


# ---- 5. factor 1 after factor 8: the bytes of an engine that never set it
def test_factor_one_after_factor_eight_is_the_untouched_engine():
    n, hop, S, L = 4096, 256, 3, 1 << 17
    pcm = synth.streams(S, L)
    x = torch.from_numpy(pcm).cuda()
    with emspec.Engine(mode=emspec.MODE_EXACT) as a, emspec.Engine(mode=emspec.MODE_EXACT) as b:
        assert a.time_reduce == 1 and b.time_reduce == 1
        a.set_time_reduce(8)
        assert a.time_reduce == 8
        small = a.batch(pcm, n, hop, True, want=WANT)
        assert small["index"].shape[1] == emspec.reduced_columns(emspec.num_columns(L, n, hop), 8)
        a.set_time_reduce(1)
        assert a.time_reduce == 1
        for k in WANT:
            assert _same(a.batch(pcm, n, hop, True, want=(k,))[k], b.batch(pcm, n, hop, True, want=(k,))[k]), k
        da, db_ = _device(a, x, n, hop), _device(b, x, n, hop)
        for k in WANT:
            assert _same(da[k], db_[k]), ("device", k)
        wa, oa = a.batch_packed(pcm, n, hop, True)
        wb, ob = b.batch_packed(pcm, n, hop, True)
        assert np.array_equal(oa, ob) and np.array_equal(wa[:oa[-1]], wb[:ob[-1]])
        # the streaming calls work again
        col, c = a.column(pcm[0, :n], hop, True)
        colb, cb = b.column(pcm[0, :n], hop, True)
        assert c == cb and _same(col, colb)


# ---- 6. refusals: status, message, and the engine stays usable
def test_refusals_leave_the_engine_usable():
    n, hop, S, L = 4096, 256, 2, 1 << 16
    pcm = synth.streams(S, L)
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right"))
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        for bad in (0, -1, 65537):
            with pytest.raises(emspec.EmspecError) as ei:
                e.set_time_reduce(bad)
            assert ei.value.code == emspec.ERR_INVALID_ARG and "65536" in str(ei.value)
            assert e.time_reduce == 1
        e.set_time_reduce(65536)
        e.set_time_reduce(1)
        # a live session with pending columns: the setter refuses, the session goes on
        D = emspec.latency_columns(n, hop, True)
        for j in range(3):
            e.columns(pcm[:, j * hop:j * hop + n], hop, True)
        with pytest.raises(emspec.EmspecError) as ei:
            e.set_time_reduce(4)
        assert ei.value.code == emspec.ERR_STATE and "pending" in str(ei.value) and e.time_reduce == 1
        e.columns(pcm[:, 3 * hop:3 * hop + n], hop, True)
        e.column(pcm[0, :n], hop, True)           # the single-stream session too
        with pytest.raises(emspec.EmspecError) as ei:
            e.set_time_reduce(4)
        assert ei.value.code == emspec.ERR_STATE
        e.reset()
        e.set_time_reduce(4)
        # every streaming call refuses while the factor is above 1
        calls = [
            lambda: e.column(pcm[0, :n], hop, True),
            lambda: e.flush(),
            lambda: e.push_samples(pcm[0, :n + hop], n, hop, True),
            lambda: e.columns(pcm[:, :n], hop, True),
            lambda: e._chk(e._lib.emspec_columns_flush(e._h, None, None, e.rows, None)),
            lambda: e.push_samples_multi(pcm[:, :n + hop], n, hop, True),
            lambda: e.columns_multires(pcm[:, :16384], 4096, hop, 368, True),
            lambda: e.push_samples_multires(pcm[:, :16384 + hop], 16384, 4096, hop, 368, True),
            lambda: e.push_samples_pcm(np.zeros((1, 2 * (n + hop)), np.int16), fmt, n, hop, True),
            lambda: e.push_samples_pcm(np.zeros((1, 2 * (16384 + hop)), np.int16), fmt, 16384, hop, True, n_high=4096, split_row=368),
        ]
        for i, call in enumerate(calls):
            with pytest.raises(emspec.EmspecError) as ei:
                call()
            assert ei.value.code == emspec.ERR_STATE and "emspec_set_time_reduce" in str(ei.value), (i, str(ei.value))
        assert e.live_streams == 0
        # ... and a batch call succeeds afterwards, with the right bytes
        x = torch.from_numpy(pcm).cuda()
        got = e.batch(pcm, n, hop, True, want=WANT)
        dev = _device(e, x, n, hop)
        e.set_time_reduce(1)
        want = V.reduce(_device(e, x, n, hop), 4, O.default_lut())
        for k in WANT:
            assert _same(got[k], want[k]) and _same(dev[k], want[k]), k
    # a wire buffer sized for Cr - 1 columns.  An image is as large as its non-zero cells make it, so the engine here maps every
    # cell - the empty ones at the dB floor included - to a non-zero index: each image then needs exactly its bound
    with emspec.Engine(mode=emspec.MODE_EXACT, db_range=400.0, gate_db=-1000.0) as e:
        e.set_time_reduce(4)
        Cr = emspec.reduced_columns(emspec.num_columns(L, n, hop), 4)
        ok = e.batch(pcm, n, hop, True, want=("index",))["index"]
        assert ok.min() > 0
        short = np.empty(S * emspec.wire_bound(Cr - 1, e.rows), np.uint8)
        with pytest.raises(emspec.EmspecError) as ei:
            e.batch_packed(pcm, n, hop, True, wire=short)
        assert ei.value.code == emspec.ERR_INVALID_ARG and "wire buffer too small" in str(ei.value)
        wire, off = e.batch_packed(pcm, n, hop, True)
        assert _same(_unpack(e, wire, off, S, Cr), ok)


# ---- 7. bounded memory: the bench shape at factor 64
def test_device_entry_memory_stays_within_the_chunk_budget():
    n, hop, S, L, f = 4096, 256, 64, 1 << 22, 64
    free0, total = torch.cuda.mem_get_info()
    need = 12 << 30
    print(f"MEASURED overview memory: free {free0 / 2**30:.2f} GiB of {total / 2**30:.2f} GiB before the test")
    if free0 < need:
        pytest.skip(f"needs 12 GB of free device memory, {free0 / 2**30:.2f} GiB free of {total / 2**30:.2f} GiB")
    Cn = emspec.num_columns(L, n, hop)
    Cr = emspec.reduced_columns(Cn, f)
    pcm = synth.streams(8, L)
    x = torch.from_numpy(pcm).cuda().repeat(8, 1).contiguous()
    x[8:] *= torch.linspace(0.3, 1.0, S - 8, device="cuda")[:, None]      # streams differ
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_time_reduce(f)
        db = torch.empty((S, Cr, e.rows), dtype=torch.float32, device="cuda")      # the caller's arrays: the reduced size
        idx = torch.empty((S, Cr, e.rows), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        budget = min(max(before // 4, 256 << 20), 4 << 30)                        # grow_chunked's rule (emspec_api.cpp)
        e.batch_device(x, n, hop, True, db=db, index=idx)
        torch.cuda.synchronize()
        e.device_status()
        after = torch.cuda.mem_get_info()[0]
        growth = before - after
        full_bytes = S * Cn * e.rows * 5
        print(f"MEASURED overview memory: growth {growth / 2**20:.1f} MiB, budget {budget / 2**20:.1f} MiB, full-rate columns "
              f"would be {full_bytes / 2**20:.1f} MiB, reduced outputs {(db.numel() * 4 + idx.numel()) / 2**20:.1f} MiB")
        assert growth <= budget + (64 << 20), (growth, budget)
        for s in (0, 9, 37, 63):
            d1 = torch.empty((1, Cr, e.rows), dtype=torch.float32, device="cuda")
            i1 = torch.empty((1, Cr, e.rows), dtype=torch.uint8, device="cuda")
            e.batch_device(x[s:s + 1], n, hop, True, db=d1, index=i1)
            torch.cuda.synchronize()
            assert torch.equal(d1[0].view(torch.int32), db[s].view(torch.int32)) and torch.equal(i1[0], idx[s]), s
        e.device_status()


# ---- 8. Node: the addon's reduced results are the ctypes binding's bytes
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_overview_matches_ctypes(tmp_path):
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_overview.js", str(tmp_path)], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    S, L, R, f = res["S"], res["L"], res["rows"], res["timeReduce"]
    pcm = np.fromfile(str(tmp_path / "pcm.f32"), np.float32).reshape(S, L)
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_time_reduce(f)
        Cr = emspec.reduced_columns(emspec.num_columns(L, res["fftSize"], res["hop"]), f)
        assert Cr == res["columns"]
        got = e.batch(pcm, res["fftSize"], res["hop"], True, want=("db", "index"))
        assert _same(np.fromfile(str(tmp_path / "index.u8"), np.uint8).reshape(S, Cr, R), got["index"])
        assert _same(np.fromfile(str(tmp_path / "db.f32"), np.float32).reshape(S, Cr, R), got["db"])
        assert _same(np.fromfile(str(tmp_path / "packed_index.u8"), np.uint8).reshape(S, Cr, R), got["index"])
        split = e.split_row_for_hz(res["splitHz"])
        Cm = emspec.reduced_columns(emspec.multires_columns(L, res["lowFftSize"], res["fftSize"], res["hop"]), f)
        assert Cm == res["multiresColumns"]
        m = e.batch_multires(pcm, res["lowFftSize"], res["fftSize"], res["hop"], split, True, want=("index",))["index"]
        assert _same(np.fromfile(str(tmp_path / "multires_index.u8"), np.uint8).reshape(S, Cm, R), m)
