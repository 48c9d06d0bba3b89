"""-m gpu: the PCM front end (include/emspec.h).  The decode kernel must BE the specification
(tests/pcm_ref.py, bit for bit), and every PCM entry point must give what the corresponding float entry point gives on the
decoded array: EXACT engines the same bytes, FAST engines the project's convention between two launches (palette index off
by at most 1 on a share of cells < 1e-4, |dB difference| < 1e-3: tests/test_gpu_host.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "em-spec_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import emspec  # noqa: E402
import pcm_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

LRMS = ["left", "right", "mid", "side"]
NAMES = {P.S16: "s16", P.S24: "s24", P.S32: "s32", P.F32: "f32"}


def _raw(rng, sample_type, sources, frames, channels, scale=1.0):
    """uint8 [sources][frames * frame_bytes]: full-range random integers; F32: normal-range floats (no NaN / denormal)."""
    nbytes = frames * P.frame_bytes(sample_type, channels)
    if sample_type == P.F32:
        x = (rng.standard_normal((sources, frames * channels)) * scale).astype("<f4")
        x[np.abs(x) < 1e-30] = 0.5
        return x.view(np.uint8).reshape(sources, nbytes)
    return rng.integers(0, 256, size=(sources, nbytes), dtype=np.uint8)


def _typed(raw, fmt):
    """the uint8 rows as the array type the binding takes for the format"""
    return raw if fmt.sample_type == P.S24 else raw.view(fmt.dtype)


def _audio(rng, sample_type, sources, frames, channels=2):
    """raw frames that look like audio (|x| < 1 after any +-1 / +-0.5 mix), as uint8 rows"""
    t = np.arange(frames)
    x = np.empty((sources, frames, channels))
    for s in range(sources):
        for c in range(channels):
            f0 = 110.0 * (1 + s) * (1 + 0.5 * c)
            x[s, :, c] = 0.35 * np.sin(2 * np.pi * f0 * t / 48000.0 + s) + 0.1 * np.sin(2 * np.pi * (3000 + 40 * s) * t / 48000.0 * (1 + c)) \
                + 0.02 * rng.standard_normal(frames)
    x = x.reshape(sources, frames * channels)
    if sample_type == P.S16:
        return np.round(x * 32767).astype("<i2").view(np.uint8).reshape(sources, -1)
    if sample_type == P.S24:
        return P.s24_pack(np.round(x * (2 ** 23 - 1)).astype(np.int64))
    if sample_type == P.S32:
        return np.round(x * (2 ** 31 - 1)).astype("<i4").view(np.uint8).reshape(sources, -1)
    return x.astype("<f4").view(np.uint8).reshape(sources, -1)


def _same(mode, got, ref, what=("db", "index")):
    if mode == "exact":
        if "index" in what:
            assert np.array_equal(got["index"], ref["index"])
        if "db" in what:
            assert np.array_equal(got["db"].view(np.uint32), ref["db"].view(np.uint32))
    else:
        if "index" in what:
            d = np.abs(got["index"].astype(np.int16) - ref["index"].astype(np.int16))
            assert d.max() <= 1 and np.mean(d != 0) < 1e-4
        if "db" in what:
            assert np.max(np.abs(got["db"] - ref["db"])) < 1e-3


def _engine(mode, **kw):
    return emspec.Engine(mode=emspec.MODE_EXACT if mode == "exact" else emspec.MODE_FAST, **kw)


# ---- 1. the decode kernel is the specification ----------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", [P.S16, P.S24, P.S32, P.F32])
def test_decode_is_the_specification(sample_type):
    import torch
    rng = np.random.default_rng(100 + sample_type)
    bps = P.BYTES[sample_type]
    offsets = (1, 2, 3) if sample_type == P.S24 else (bps,)
    cases = 0
    with emspec.Engine() as e:
        for channels in (1, 2, 3, 6, 8):
            for views in (1, 2, 4, 8):
                mix = rng.uniform(-1.5, 1.5, size=(views, channels)).astype(np.float32)
                fmt = emspec.PcmFormat.make(sample_type, channels, views=mix.tolist())
                fb = fmt.frame_bytes
                for frames in (1, 2, 3, 255, 4097, 100003):
                    sources = 3 if frames < 5000 else 2
                    raw = _raw(rng, sample_type, sources, frames, channels)
                    want = P.decode(raw, sample_type, channels, mix)
                    stride = frames * fb + bps * 5          # larger than a row, a multiple of the sample size only
                    for off in offsets:
                        host = np.zeros(256 + off + sources * stride, np.uint8)
                        dev = torch.empty(host.size, dtype=torch.uint8, device="cuda")
                        base = (-dev.data_ptr()) % 256 + off      # `off` bytes past a 256-byte aligned address
                        for i in range(sources):
                            host[base + i * stride: base + i * stride + frames * fb] = raw[i]
                        dev.copy_(torch.from_numpy(host))
                        got = e.pcm_decode_device(dev, fmt, sources, frames, src_stride_bytes=stride, offset_bytes=base)
                        torch.cuda.synchronize()
                        got = got.cpu().numpy()
                        assert got.shape == want.shape
                        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (NAMES[sample_type], channels, views, frames, off)
                        cases += 1
    assert cases == 5 * 4 * 6 * len(offsets)


def test_decode_reads_page_locked_host_memory_in_place():
    """the live path's form: the source is page-locked host memory, the kernel reads it over PCIe"""
    import torch
    rng = np.random.default_rng(7)
    fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
    raw = _raw(rng, P.S16, 3, 5001, 2)
    pin = emspec.PinnedArray(raw.shape, np.uint8)
    try:
        pin.array[...] = raw
        out = torch.empty((12, 5001), dtype=torch.float32, device="cuda")
        with emspec.Engine() as e:
            st = torch.cuda.current_stream()
            e._chk(e._lib.emspec_pcm_decode_device(e._h, C.c_void_p(pin.array.ctypes.data), C.byref(fmt), 3, 5001, 5001 * 4,
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
            torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), P.decode(raw, P.S16, 2, fmt.matrix).view(np.uint32))
    finally:
        pin.close()


def test_decode_argument_errors():
    import torch
    fmt = emspec.PcmFormat.make("s16", 2, views=["left"])
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with emspec.Engine() as e:
        for kw, field in ((dict(sample_type=9), "sample_type"), (dict(channels=0), "channels"), (dict(views=9), "views"),
                          (dict(reserved=3), "reserved")):
            bad = emspec.PcmFormat.make("s16", 2, views=["left"])
            for k, v in kw.items():
                setattr(bad, k, v)
            with pytest.raises(emspec.EmspecError) as ei:
                e.pcm_decode_device(dev, bad, 1, 16, src_stride_bytes=64, out=torch.empty((1, 16), dtype=torch.float32, device="cuda"))
            assert ei.value.code == emspec.ERR_INVALID_ARG and field in str(ei.value)
        nanw = emspec.PcmFormat.make("s16", 2, views=[[1.0, float("nan")]])
        with pytest.raises(emspec.EmspecError) as ei:
            e.pcm_decode_device(dev, nanw, 1, 16, src_stride_bytes=64)
        assert ei.value.code == emspec.ERR_INVALID_ARG and "mix" in str(ei.value)
        with pytest.raises(emspec.EmspecError) as ei:      # a stride shorter than a row
            e.pcm_decode_device(dev, fmt, 2, 16, src_stride_bytes=60)
        assert ei.value.code == emspec.ERR_INVALID_ARG
        with pytest.raises(emspec.EmspecError) as ei:      # an odd byte offset for 16-bit samples
            e.pcm_decode_device(dev, fmt, 1, 16, src_stride_bytes=64, offset_bytes=(-dev.data_ptr()) % 2 + 1)
        assert ei.value.code == emspec.ERR_INVALID_ARG
        assert e.pcm_decode_device(dev, fmt, 1, 16).shape == (1, 16)   # the engine is usable afterwards


# ---- 2. / 3. batch and packed batch = the float entries on the decoded array -------------------------------------------------
def _batch_pcm_pinned(e, raw, fmt, frames, n, hop, want):
    """emspec_batch_pcm with EVERY host buffer page-locked (the pipelined path without helper threads); returns copies"""
    sources = raw.shape[0]
    S, Cn = sources * fmt.views, emspec.num_columns(frames, n, hop)
    pin = emspec.PinnedArray(raw.shape, np.uint8)
    outs = {"db": emspec.PinnedArray((S, Cn, e.rows), np.float32) if "db" in want else None,
            "rgba": emspec.PinnedArray((S, Cn, e.rows, 4), np.uint8) if "rgba" in want else None,
            "index": emspec.PinnedArray((S, Cn, e.rows), np.uint8) if "index" in want else None}
    try:
        pin.array[...] = raw
        ptr = lambda k: outs[k].array.ctypes.data if outs[k] is not None else None
        out = emspec.Out(ptr("db"), ptr("rgba"), ptr("index"))
        e._chk(e._lib.emspec_batch_pcm(e._h, C.c_void_p(pin.array.ctypes.data), C.byref(fmt), sources, frames, n, hop, 1, C.byref(out)))
        return {k: (v.array.copy() if v is not None else None) for k, v in outs.items()}
    finally:
        pin.close()
        for v in outs.values():
            if v is not None:
                v.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("n,hop", [(4096, 256), (1024, 128)])
@pytest.mark.parametrize("sample_type", [P.S24, P.S16])
def test_batch_pcm_equals_float_batch_many_sources(mode, n, hop, sample_type):
    """23 stereo sources x (L, R, M, S) = 92 streams: many units of whole sources through the three staging sets; dB, palette
    index and RGBA; pageable and page-locked; twice per engine; then once with the display post-process; and the packed form."""
    rng = np.random.default_rng(11)
    frames = n + hop * 149 + 5
    raw = _audio(rng, sample_type, 23, frames)
    fmt = emspec.PcmFormat.make(sample_type, 2, views=LRMS)
    pcm = P.decode(raw, sample_type, 2, fmt.matrix)
    Cn = emspec.num_columns(frames, n, hop)
    with _engine(mode) as e:
        lut = emspec.make_colormap(0.7)
        e.set_colormap(lut)
        ref = e.batch(pcm, n, hop, True, want=("db", "rgba", "index"))
        for _ in range(2):
            got = e.batch_pcm(_typed(raw, fmt), fmt, n, hop, True, want=("db", "rgba", "index"))
            _same(mode, got, ref)
            assert np.array_equal(got["rgba"], np.asarray(lut).reshape(256, 4)[got["index"]])
            gotp = _batch_pcm_pinned(e, raw, fmt, frames, n, hop, ("db", "rgba", "index"))
            _same(mode, gotp, ref)
        # packed: every image expands to the index columns; offsets 16-byte aligned; a buffer too small is rejected
        wire, offs = e.batch_pcm_packed(_typed(raw, fmt), fmt, n, hop, True)
        assert offs.shape == (93,) and offs[0] == 0 and np.all(offs % 16 == 0) and np.all(np.diff(offs) > 0)
        unpacked = np.stack([emspec.wire_unpack_host(wire[offs[s]:offs[s + 1]], Cn, e.rows) for s in range(92)])
        _same(mode, {"index": unpacked}, ref, what=("index",))
        with pytest.raises(emspec.EmspecError) as ei:
            e.batch_pcm_packed(_typed(raw, fmt), fmt, n, hop, True, wire=np.empty(int(offs[-1]) - 64, np.uint8))
        assert ei.value.code == emspec.ERR_INVALID_ARG
        e.set_display(0.6, 0.5)
        refp = e.batch(pcm, n, hop, True, want=("db", "index"))
        gotp = e.batch_pcm(_typed(raw, fmt), fmt, n, hop, True, want=("db", "index"))
        _same(mode, gotp, refp)
        assert not np.array_equal(refp["db"], ref["db"])


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("n,hop,sample_type,columns,want", [(1024, 128, P.S24, 33100, ("db", "rgba", "index")),
                                                            (4096, 256, P.S16, 49200, ("db", "index"))])
def test_batch_pcm_equals_float_batch_one_long_source(mode, n, hop, sample_type, columns, want):
    """ONE source of more than 2^20 frames, long enough for units that are runs of columns of the source (at least 16,384 columns
    each): 33,100 columns are two runs, 49,200 three - the middle one has halo frames on both sides (columns skipped in front,
    left behind at the end).  Each run's raw frames start at first_sample * frame bytes in the caller's array and its four views
    leave the staging set one by one.  (The three-run case leaves RGBA out: 200 M cells x 4 bytes, three times over.)"""
    rng = np.random.default_rng(12)
    frames = n + hop * (columns - 1) + 7
    assert frames >= 1 << 20
    raw = _audio(rng, sample_type, 1, frames)
    fmt = emspec.PcmFormat.make(sample_type, 2, views=LRMS)
    pcm = P.decode(raw, sample_type, 2, fmt.matrix)
    with _engine(mode) as e:
        lut = emspec.make_colormap(0.7)
        e.set_colormap(lut)
        ref = e.batch(pcm, n, hop, True, want=want)
        for pinned in (False, True):
            got = _batch_pcm_pinned(e, raw, fmt, frames, n, hop, want) if pinned else e.batch_pcm(_typed(raw, fmt), fmt, n, hop, True, want=want)
            assert got["db"].shape == (4, columns, e.rows)
            _same(mode, got, ref)
            if "rgba" in want:
                assert np.array_equal(got["rgba"], np.asarray(lut).reshape(256, 4)[got["index"]])
            del got


# ---- 4. live ---------------------------------------------------------------------------------------------------------------
def _live_run(e, feed, flush_to, S, total, blocks, D, reset_at=None):
    """feeds [0, total) in blocks of the rotating sizes; returns per-stream lists of (first column, dB block, RGBA block)"""
    outs = [[] for _ in range(S)]
    pos, i = 0, 0
    while pos < total:
        count = min(blocks[i % len(blocks)], total - pos)
        db, rgba, counts, firsts = feed(pos, count)
        for s in range(S):
            if counts[s] > 0:
                outs[s].append((int(firsts[s]), db[s, :counts[s]].copy(), rgba[s, :counts[s]].copy()))
        pos += count
        i += 1
        if reset_at is not None and pos >= reset_at[0]:
            e.reset_stream(reset_at[1])
            outs[reset_at[1]].append("reset")
            reset_at = None
    for _ in range(flush_to):
        db, rgba, cols = e.columns_flush(want_rgba=True)
        for s in range(S):
            if cols[s] >= 0:
                outs[s].append((int(cols[s]), db[s][None].copy(), rgba[s][None].copy()))
    return outs


def _join(chunks):
    """[(first, db, rgba) ...] of one stream (after its last reset) -> (first column, db [k][rows], rgba)"""
    if "reset" in chunks:
        chunks = chunks[len(chunks) - chunks[::-1].index("reset"):]
    first = chunks[0][0]
    at = first
    for f, d, _ in chunks:
        assert f == at
        at += d.shape[0]
    return first, np.concatenate([c[1] for c in chunks]), np.concatenate([c[2] for c in chunks])


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("n,n_high,hop", [(4096, 0, 256), (16384, 4096, 256)])
@pytest.mark.parametrize("pinned", [False, True])
def test_live_pcm_equals_float_live_and_batch(mode, n, n_high, hop, pinned):
    """3 stereo sources x (L, R, M, S) = 12 streams in blocks of 128, 1000 and 4801 frames over more than 300 columns, then the
    flush: the columns of push_samples_multi / _multires fed the decoded floats in the same blocks, and batch_pcm's (a
    single-resolution session).  Stream 5 (source 1, view R) is reset mid-session while the others continue."""
    rng = np.random.default_rng(13)
    D = emspec.latency_columns(n, hop, True)
    total = n + hop * 330 + 17
    Cn = emspec.num_columns(total, n, hop)
    raw = _audio(rng, P.S16, 3, total)
    fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
    pcm = P.decode(raw, P.S16, 2, fmt.matrix)
    typed = _typed(raw, fmt)
    pin = None
    if pinned:
        pin = emspec.PinnedArray(typed.shape, typed.dtype)
        pin.array[...] = typed
        typed = pin.array
    blocks = (128, 1000, 4801)
    reset_frame = n + hop * 100 + 64
    try:
        with _engine(mode) as e:
            # a palette of 256 different colours: RGBA maps back to the palette index
            lut = np.zeros((256, 4), np.uint8)
            lut[:, 0] = np.arange(256)
            lut[:, 1] = 255 - np.arange(256)
            lut[:, 3] = 255
            e.set_colormap(lut)
            split = e.split_row_for_hz(250) if n_high else 0
            if n_high:
                feed_f = lambda pos, count: e.push_samples_multires(pcm, n, n_high, hop, split, True, want_rgba=True, count=count, offset=pos)
            else:
                feed_f = lambda pos, count: e.push_samples_multi(pcm, n, hop, True, want_rgba=True, count=count, offset=pos)
            feed_p = lambda pos, count: e.push_samples_pcm(typed, fmt, n, hop, True, n_high=n_high, split_row=split, want_rgba=True,
                                                           count=count, offset=pos)
            ref = _live_run(e, feed_f, D, 12, total, blocks, D, reset_at=(reset_frame, 5))
            e.reset()
            got = _live_run(e, feed_p, D, 12, total, blocks, D, reset_at=(reset_frame, 5))
            assert e.live_streams == 12
            e.reset()
            batch = None if n_high else e.batch_pcm(typed, fmt, n, hop, True, want=("db", "rgba"))
        for s in range(12):
            f0, gdb, grgba = _join(got[s])
            r0, rdb, rrgba = _join(ref[s])
            assert f0 == r0 == 0 and gdb.shape == rdb.shape
            if s != 5:
                assert gdb.shape[0] == Cn
            if mode == "exact":
                assert np.array_equal(gdb.view(np.uint32), rdb.view(np.uint32)) and np.array_equal(grgba, rrgba)
                if batch is not None and s != 5:
                    assert np.array_equal(gdb.view(np.uint32), batch["db"][s].view(np.uint32)) and np.array_equal(grgba, batch["rgba"][s])
            else:
                # the +-1 rule on the palette index (red channel = index in this palette)
                assert np.array_equal(grgba[..., 1], 255 - grgba[..., 0]) and np.all(grgba[..., 3] == 255)
                for other_db, other_rgba in ((rdb, rrgba),) + (((batch["db"][s], batch["rgba"][s]),) if batch is not None and s != 5 else ()):
                    d = np.abs(grgba[..., 0].astype(np.int16) - other_rgba[..., 0].astype(np.int16))
                    assert d.max() <= 1 and np.mean(d != 0) < 1e-4
                    assert np.max(np.abs(gdb - other_db)) < 1e-3
    finally:
        if pin is not None:
            pin.close()


# ---- 5. state and argument errors ---------------------------------------------------------------------------------------------
def test_live_pcm_state_and_argument_errors():
    rng = np.random.default_rng(14)
    n, hop = 4096, 256
    total = n + hop * 40
    raw = _audio(rng, P.S16, 2, total)
    fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
    other = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", [0.5, -0.25]])
    typed = _typed(raw, fmt)
    pcm = P.decode(raw, P.S16, 2, fmt.matrix)
    D = emspec.latency_columns(n, hop, True)

    def code(fn):
        with pytest.raises(emspec.EmspecError) as ei:
            fn()
        return ei.value.code

    with _engine("exact") as e:
        # undisturbed session
        a = e.push_samples_pcm(typed, fmt, n, hop, count=6000, offset=0)
        b = e.push_samples_pcm(typed, fmt, n, hop, count=total - 6000, offset=6000)
        e.reset()
        # the same, with every rejected call in between
        a2 = e.push_samples_pcm(typed, fmt, n, hop, count=6000, offset=0)
        assert code(lambda: e.push_samples_multi(pcm, n, hop, count=100, offset=6000)) == emspec.ERR_STATE        # float on PCM
        assert code(lambda: e.push_samples_pcm(typed, other, n, hop, count=100, offset=6000)) == emspec.ERR_STATE   # format change
        assert code(lambda: e.push_samples_pcm(typed, fmt, n, 128, count=100, offset=6000)) == emspec.ERR_STATE     # shape change
        need = e.push_columns_multi(total - 6000, n, hop)
        assert need > 1
        # max_columns too small with both outputs NULL: nothing fed
        assert code(lambda: e.push_samples_pcm(typed, fmt, n, hop, want_db=False, count=total - 6000, offset=6000,
                                               max_columns=need - 1)) == emspec.ERR_INVALID_ARG
        bad = emspec.PcmFormat.make("s16", 2, views=LRMS)
        bad.reserved = 1
        assert code(lambda: e.push_samples_pcm(typed, bad, n, hop, count=100, offset=6000)) == emspec.ERR_INVALID_ARG
        b2 = e.push_samples_pcm(typed, fmt, n, hop, count=total - 6000, offset=6000)
        for x, y in ((a, a2), (b, b2)):
            assert np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]) and np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32))
        assert np.all(b2[2] == need)
        for _ in range(D):
            e.columns_flush()
        assert code(lambda: e.columns_flush()) == emspec.ERR_STATE
        assert code(lambda: e.push_samples_pcm(typed, fmt, n, hop, count=100, offset=0)) == emspec.ERR_STATE        # fed after flush
        e.reset()
        # the reverse: PCM on a float session
        e.push_samples_multi(pcm, n, hop, count=5000, offset=0)
        assert code(lambda: e.push_samples_pcm(typed, fmt, n, hop, count=100, offset=5000)) == emspec.ERR_STATE
        e.reset()
        c = e.push_samples_pcm(typed, fmt, n, hop, count=6000, offset=0)     # usable afterwards
        assert np.array_equal(c[0].view(np.uint32), a[0].view(np.uint32))


# ---- 6. Node ------------------------------------------------------------------------------------------------------------------
def test_node_pcm_matches_ctypes(tmp_path):
    """js/test_pcm.js (EXACT engine): computeColumnsPcm from an Int16Array and pushSamplesPcm over blocks of 1000 frames return
    the ctypes calls' bytes (the script itself checks computeColumnsPcmPacked and the typed-array / format.type rule)."""
    import json
    import subprocess
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_pcm.js", str(tmp_path)], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sources, frames, J, R, n, hop = res["sources"], res["frames"], res["columns"], res["rows"], res["fftSize"], res["hop"]
    S = sources * res["views"]
    fmt = emspec.PcmFormat.make("s16", 2, views=LRMS)
    assert np.array_equal(np.array(res["mix"], np.float32).reshape(4, 2), fmt.matrix)
    src = np.fromfile(str(tmp_path / "src.i16"), np.int16).reshape(sources, frames * 2)
    node = {"batch_db": np.fromfile(str(tmp_path / "batch_db.f32"), np.float32).reshape(S, J, R),
            "batch_index": np.fromfile(str(tmp_path / "batch_index.u8"), np.uint8).reshape(S, J, R),
            "db": np.fromfile(str(tmp_path / "db.f32"), np.float32).reshape(S, J, R),
            "rgba": np.fromfile(str(tmp_path / "rgba.u8"), np.uint8).reshape(S, J, R, 4)}
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        assert e.rows == R
        got = e.batch_pcm(src, fmt, n, hop, True, want=("db", "index"))
        feed = lambda pos, count: e.push_samples_pcm(src, fmt, n, hop, True, want_rgba=True, count=count, offset=pos)
        live = _live_run(e, feed, emspec.latency_columns(n, hop, True), S, frames, (res["block"],), 0)
    assert np.array_equal(got["db"].view(np.uint32), node["batch_db"].view(np.uint32)) and np.array_equal(got["index"], node["batch_index"])
    for s in range(S):
        f0, ldb, lrgba = _join(live[s])
        assert f0 == 0 and ldb.shape[0] == J
        assert np.array_equal(ldb.view(np.uint32), node["db"][s].view(np.uint32)) and np.array_equal(lrgba, node["rgba"][s])
