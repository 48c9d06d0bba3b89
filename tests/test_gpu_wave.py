"""GPU: the waveform envelope (include/emspec.h: emspec_wave_device, emspec_set_wave_out).  The device
entry and every entry of the host pipeline against tests/wave_ref.py, byte for byte in both arithmetic modes (the envelope is a
function of the samples' bits); the images and dB of a call with the envelope set are those of the same call with it cleared;
the long-window split, offsets past 2^32 bytes, the refusals and the Node addon."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emspec
import pcm_ref as PR
import wave_ref as W
from emspec import synth
from window_cases import DEVICE_CASES, IDS, PATHS, SPLIT_CASES, _team

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
GB = 1e9


@pytest.fixture(scope="module")
def fast():
    with emspec.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def exact():
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        yield e
        e.set_wave_out(None)
        e.set_time_reduce(1)


def _dev_wave(e, x, n, hop, f):
    """emspec_wave_device on a numpy [S, L] array -> numpy [S, Cr, 2].  pcm_dev lies 4 bytes and wave_dev 8 bytes into an
    allocation; the output is poisoned, and a sentinel in front of and behind it must stay."""
    S, L = x.shape
    Cr = max(emspec.reduced_columns(max(emspec.num_columns(L, n, hop), 0), f), 0)
    buf = torch.empty(S * L + 1, dtype=torch.float32, device="cuda")
    src = buf[1:].view(S, L)
    src.copy_(torch.from_numpy(x))
    obuf = torch.full((S * Cr * 2 + 4,), 7.0, dtype=torch.float32, device="cuda")
    out = obuf[2:2 + S * Cr * 2].view(S, Cr, 2)
    assert src.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 8
    e.wave_device(src, n, hop, f, out=out)
    torch.cuda.synchronize()
    e.device_status()
    got = obuf.cpu().numpy()
    assert np.all(got[:2] == 7.0) and np.all(got[-2:] == 7.0), "the envelope was written outside [S][Cr] pairs"
    return got[2:-2].reshape(S, Cr, 2)


# ---- 1. the device entry on the cases shared with the level meters' suite (tests/window_cases.py): every team size and the split
def test_cases_cover_every_path():
    assert {_team(*c) for c in DEVICE_CASES} == PATHS == {1, 2, 4, 8, 16, 32, 64, "split"}
    assert _team(256, 1, 300, 1) == 1 and _team(4096, 4096, 5 * 4096 + 1, 1) == 64


@pytest.mark.parametrize("case", DEVICE_CASES, **IDS)
def test_wave_device_is_the_reference(fast, case):
    n, hop, L, f = case
    x = W.case_signal(case)
    assert W.same(_dev_wave(fast, x, n, hop, f), W.envelope(x, n, hop, f))


@pytest.mark.parametrize("case", SPLIT_CASES, **IDS)
def test_split_path(fast, case):
    """factor 300: three windows, two pieces each, the last one shorter than the split, so that its second piece lies past its
    end; factor 65536: one window of three pieces"""
    n, hop, L, f = case
    x = W.case_signal(case, seed=2)
    want = W.envelope(x, n, hop, f)
    assert _team(*case) == "split" and (f == 65536 or (want.shape[1] == 3 and 2560 < 16384 < 65536 < 300 * 256))
    assert W.same(_dev_wave(fast, x, n, hop, f), want)


def test_wave_device_is_the_same_on_an_exact_engine(exact):
    case = (4096, 257, 4096 + 257 * 20, 3)
    assert case in W.CASES
    x = W.case_signal(case)
    exact.set_time_reduce(5)     # the engine's time reduction plays no part: the factor is the call's own
    try:
        assert W.same(_dev_wave(exact, x, *case[:2], case[3]), W.envelope(x, *case[:2], case[3]))
    finally:
        exact.set_time_reduce(1)


# ---- 2. long windows: cut into pieces over workgroups, combined through the keys
@pytest.mark.parametrize("S,L,f", [(2, 2 ** 22 + 5, 4096), (2, 2 ** 22 + 5, 65536), (1, 2 ** 24 + 3, 65536)])
def test_long_windows(fast, S, L, f):
    n, hop = 4096, 256
    x = W.signal(S, L, n, hop, f, seed=3)
    want = W.envelope(x, n, hop, f)
    assert f * hop > 65536 and want.shape[1] >= 1
    assert W.same(_dev_wave(fast, x, n, hop, f), want)


# ---- 3. offsets past 2^32 bytes
@pytest.mark.parametrize("f", [1, 4096])
def test_offsets_past_4_gib(fast, f):
    """S = 3 streams of 2^29 - 3 samples (6.4 GB), generated on the device, free of NaN and zeros (every |x| in [0.5, 1.5), random
    sign), so that torch.amin / amax over the same windows is the reference by value and by bits."""
    S, L, n, hop = 3, 2 ** 29 - 3, 4096, 256
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < 10 * GB:
        pytest.skip(f"needs 10 GB of free device memory (6.4 GB of samples), {free / GB:.1f} of {total / GB:.1f} GB are free")
    gen = torch.Generator(device="cuda").manual_seed(29)
    x = torch.empty((S, L), dtype=torch.float32, device="cuda")
    for s in range(S):
        x[s].uniform_(0.5, 1.5, generator=gen)
        sign = torch.randint(0, 2, (L,), dtype=torch.int8, device="cuda", generator=gen).mul_(2).sub_(1)
        x[s].mul_(sign)
        del sign
    assert S * L * 4 > 2 ** 32
    Cn = emspec.num_columns(L, n, hop)
    Cr = emspec.reduced_columns(Cn, f)
    off = n // 2 - hop // 2
    out = torch.full((S * Cr * 2 + 2,), 7.0, dtype=torch.float32, device="cuda")
    got = out[:S * Cr * 2].view(S, Cr, 2)
    fast.wave_device(x, n, hop, f, out=got)
    torch.cuda.synchronize()
    fast.device_status()
    assert torch.all(out[-2:] == 7.0)
    full = (Cn // f) * f                                                   # the columns of the whole groups
    body = x[:, off:off + full * hop].unflatten(1, (Cn // f, f * hop))
    want = torch.empty((S, Cr, 2), dtype=torch.float32, device="cuda")
    want[:, :Cn // f, 0] = torch.amin(body, dim=2)
    want[:, :Cn // f, 1] = torch.amax(body, dim=2)
    if full < Cn:
        tail = x[:, off + full * hop:off + Cn * hop]
        want[:, -1, 0] = torch.amin(tail, dim=1)
        want[:, -1, 1] = torch.amax(tail, dim=1)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool((want[:, :, 0] < 0).all()) and bool((want[:, :, 1] > 0).all())
    del x, body, want, out
    torch.cuda.empty_cache()


# ---- 4. the host pipeline (EXACT engine: the images are the same bytes however a batch is cut)
def _batch_with_and_without(e, run, S, Cr):
    """run() -> dict of arrays.  Once with the envelope set (poisoned, one pair more than needed), once cleared: the outputs are
    the same bytes, and the cleared call writes nothing.  Returns (envelope [S, Cr, 2], outputs)."""
    wave = np.full((S * Cr + 1, 2), 7.0, F)
    e.set_wave_out(wave)
    try:
        with_ = run()
    finally:
        e.set_wave_out(None)
    assert np.all(wave[-1] == 7.0), "the envelope was written past streams x columns pairs"
    kept = wave.copy()
    without = run()
    assert np.array_equal(wave.view(U), kept.view(U)), "a cleared envelope was written"
    assert with_.keys() == without.keys()
    for k in with_:
        a, b = with_[k], without[k]
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{k} differs with the envelope set"
    return wave[:-1].reshape(S, Cr, 2), with_


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
@pytest.mark.parametrize("f", [1, 6])
def test_batch_delivers_the_envelope(exact, pinned, f):
    S, L, n, hop = 40, 2 ** 17, 4096, 256
    Cn = emspec.num_columns(L, n, hop)
    Cr = emspec.reduced_columns(Cn, f)
    x = W.signal(S, L, n, hop, f, seed=4, finite=True)
    want = W.envelope(x, n, hop, f)
    exact.set_time_reduce(f)
    pins = []
    try:
        if pinned:
            pins = [emspec.PinnedArray((S, L), F), emspec.PinnedArray((S * Cr + 1, 2), F), emspec.PinnedArray((S, Cr, exact.rows), F)]
            pins[0].array[...] = x
            src, wave, db = (p.array for p in pins)
            wave[...] = 7.0
            exact.set_wave_out(wave)
            got_db = exact.batch(src, n, hop, True, want=("db",), db_out=db)["db"].copy()
            got = wave.copy()
            exact.set_wave_out(None)
            assert np.all(got[-1] == 7.0) and W.same(got[:-1].reshape(S, Cr, 2), want)
            plain = exact.batch(x, n, hop, True, want=("db",))["db"]
            assert np.array_equal(got_db.view(U), plain.view(U))
        else:
            got, outs = _batch_with_and_without(exact, lambda: exact.batch(x, n, hop, True, want=("db", "index")), S, Cr)
            assert W.same(got, want) and outs["index"].shape == (S, Cr, exact.rows)
    finally:
        exact.set_wave_out(None)
        exact.set_time_reduce(1)
        for p in pins:
            p.close()


@pytest.mark.parametrize("f", [1, 6])
def test_one_long_stream_cut_into_runs(exact, f):
    """ONE stream of 49,158 columns (the length tests/test_gpu_peaks.py cuts into runs of >= 16,384 columns): the units are runs
    of columns with a halo, the envelope's windows start `skip` columns into the staged samples, and with f = 6 the runs start on
    multiples of 6."""
    n, hop, Cn = 4096, 256, 3 * 16384 + 6
    L = n + hop * (Cn - 1)
    Cr = emspec.reduced_columns(Cn, f)
    x = W.signal(1, L, n, hop, f, seed=5, finite=True)
    exact.set_time_reduce(f)
    try:
        got, _ = _batch_with_and_without(exact, lambda: exact.batch(x, n, hop, True, want=("index",)), 1, Cr)
    finally:
        exact.set_time_reduce(1)
    assert W.same(got, W.envelope(x, n, hop, f))


# ---- 5. the other entries
@pytest.mark.parametrize("f", [1, 3])
def test_pcm_packed_delivers_the_views_envelope(exact, f):
    """S16 stereo -> L R M S: the envelope is that of the decoded, mixed float streams (tests/pcm_ref.py), which exist in no host
    buffer; the wire images are the same with and without."""
    n, hop, sources = 4096, 256, 2
    frames = n + hop * 59 + 3
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
    rng = np.random.default_rng(11)
    raw = rng.integers(-20000, 20000, (sources, frames * 2), dtype=np.int16)
    raw[0, 2 * (n // 2 + 40 * hop)] = 32767
    raw[1, 2 * (n // 2 + 40 * hop) + 1] = -32768
    dec = PR.decode(raw.view(np.uint8), PR.S16, 2, fmt.matrix)
    S, Cr = sources * 4, emspec.reduced_columns(emspec.num_columns(frames, n, hop), f)
    assert dec.shape == (S, frames)
    exact.set_time_reduce(f)

    def run():
        wire, offsets = exact.batch_pcm_packed(raw, fmt, n, hop, True)
        return {"wire": wire[:offsets[-1]].copy(), "offsets": offsets}
    try:
        got, _ = _batch_with_and_without(exact, run, S, Cr)
        assert W.same(got, W.envelope(dec, n, hop, f))
        # ... and the unpacked PCM entry delivers the same pairs
        got2, _ = _batch_with_and_without(exact, lambda: exact.batch_pcm(raw, fmt, n, hop, True, want=("index",)), S, Cr)
        assert W.same(got2, got)
    finally:
        exact.set_time_reduce(1)


def test_packed_and_multires_and_peaks_deliver_the_envelope(exact):
    S = 5
    # emspec_batch_packed
    n, hop, L = 1024, 255, 1024 + 255 * 70 + 11
    x = W.signal(S, L, n, hop, 1, seed=6, finite=True)
    Cn = emspec.num_columns(L, n, hop)

    def packed():
        wire, offsets = exact.batch_packed(x, n, hop, True)
        return {"wire": wire[:offsets[-1]].copy(), "offsets": offsets}
    got, _ = _batch_with_and_without(exact, packed, S, Cn)
    assert W.same(got, W.envelope(x, n, hop, 1))
    # emspec_batch_multires at 16384 / 4096 / 256: the column grid is the long band's
    n_low, n_high, hop = 16384, 4096, 256
    L = n_low + hop * 45 + 1
    x = W.signal(S, L, n_low, hop, 1, seed=7, finite=True)
    Cn = emspec.multires_columns(L, n_low, n_high, hop)
    assert Cn == emspec.num_columns(L, n_low, hop)
    split = exact.split_row_for_hz(250.0)
    got, _ = _batch_with_and_without(exact, lambda: exact.batch_multires(x, n_low, n_high, hop, split, True, want=("db",)), S, Cn)
    assert W.same(got, W.envelope(x, n_low, hop, 1))
    exact.set_time_reduce(4)
    try:
        Cr = emspec.reduced_columns(Cn, 4)
        got, _ = _batch_with_and_without(exact, lambda: exact.batch_multires(x, n_low, n_high, hop, split, True, want=("index",)), S, Cr)
        assert W.same(got, W.envelope(x, n_low, hop, 4))
    finally:
        exact.set_time_reduce(1)
    # emspec_batch_peaks (full rate only)
    n, hop, L = 4096, 256, 4096 + 256 * 30 + 9
    x = (synth.streams(S, L) * F(0.5)).astype(F)
    Cn = emspec.num_columns(L, n, hop)
    got, outs = _batch_with_and_without(exact, lambda: {"peaks": exact.batch_peaks(x, n, hop, True, 4, -60.0)}, S, Cn)
    assert W.same(got, W.envelope(x, n, hop, 1)) and (outs["peaks"][..., 0] >= 0).any()


# ---- 6. state and refusals
def test_capacity_clearing_gather_and_alignment(exact):
    S, L, n, hop = 3, 2 ** 15 + 1, 1024, 256
    x = W.signal(S, L, n, hop, 1, seed=8, finite=True)
    Cn = emspec.num_columns(L, n, hop)
    # one pair short: refused before anything runs - the outputs and the envelope keep their sentinels
    wave = np.full((S * Cn - 1, 2), 7.0, F)
    db = np.full((S, Cn, exact.rows), 7.0, F)
    exact.set_wave_out(wave)
    try:
        with pytest.raises(emspec.EmspecError) as ei:
            exact.batch(x, n, hop, True, want=("db",), db_out=db)
        assert ei.value.code == emspec.ERR_INVALID_ARG and "emspec_set_wave_out" in str(ei.value)
        assert np.all(db == 7.0) and np.all(wave == 7.0)
        # a time reduction makes the same array large enough
        exact.set_time_reduce(2)
        exact.batch(x, n, hop, True, want=("index",))
        Cr = emspec.reduced_columns(Cn, 2)
        assert W.same(wave[:S * Cr].reshape(S, Cr, 2), W.envelope(x, n, hop, 2)) and np.all(wave[S * Cr:] == 7.0)
        exact.set_time_reduce(1)
        # the gather delivers none: a state error while set, in front of every other check (no communicator here)
        with pytest.raises(emspec.EmspecError) as ei:
            exact._chk(exact._lib.emspec_batch_gather(exact._h, x.ctypes.data_as(C.c_void_p), S, L, n, hop, 1, 0, None, None, None))
        assert ei.value.code == emspec.ERR_STATE and "emspec_set_wave_out" in str(ei.value)
    finally:
        exact.set_time_reduce(1)
        exact.set_wave_out(None)
    # cleared: nothing is written, the engine is usable, and the gather's refusal is the communicator's again
    wave[...] = 7.0
    out = exact.batch(x, n, hop, True, want=("db",), db_out=db)
    assert np.all(wave == 7.0) and not np.any(db == 7.0) and out["db"] is db
    with pytest.raises(emspec.EmspecError) as ei:
        exact._chk(exact._lib.emspec_batch_gather(exact._h, x.ctypes.data_as(C.c_void_p), S, L, n, hop, 1, 0, None, None, None))
    assert ei.value.code == emspec.ERR_STATE and "communicator" in str(ei.value)
    # a negative capacity, and the device entry's refusals: every one INVALID_ARG with a message, nothing written
    lib, h = exact._lib, exact._h
    assert lib.emspec_set_wave_out(h, wave.ctypes.data_as(C.c_void_p), -1) == emspec.ERR_INVALID_ARG
    t = torch.from_numpy(x).cuda()
    o = torch.full((S * Cn * 2 + 2,), 7.0, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, q = t.data_ptr(), o.data_ptr()
    for args, word in [((p, S, L, n, hop, 1, q + 4), "8-byte"), ((p + 2, S, L - 1, n, hop, 1, q), "4-byte"), ((p, S, L, n, hop, 0, q), "factor"),
                       ((p, S, L, n, hop, 65537, q), "factor"), ((p, S, L, n, 0, 1, q), "hop"), ((p, S, L, n, n + 1, 1, q), "hop"),
                       ((p, S, L, 1000, hop, 1, q), "fft size"), ((p, 65536, L, n, hop, 1, q), "streams"), ((None, S, L, n, hop, 1, q), "null"),
                       ((p, S, L, n, hop, 1, None), "null")]:
        a = list(args)
        rc = lib.emspec_wave_device(h, C.c_void_p(a[0]), *a[1:6], C.c_void_p(a[6]), st)
        assert rc == emspec.ERR_INVALID_ARG and word in lib.emspec_last_error(h).decode(), (args, lib.emspec_last_error(h).decode())
    assert lib.emspec_wave_device(h, None, 0, L, n, hop, 1, None, st) == 0 and lib.emspec_wave_device(h, None, S, n - 1, n, hop, 1, None, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(o == 7.0))
    assert W.same(exact.wave_device(t, n, hop, 1).cpu().numpy(), W.envelope(x, n, hop, 1))


# ---- 7. Node: setWaveOut with computeColumnsPcmPacked returns the ctypes binding's bytes
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_wave_matches_ctypes(exact, tmp_path):
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_wave.js", str(tmp_path)], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sources, frames, n, hop, f = res["sources"], res["frames"], res["fftSize"], res["hop"], res["factor"]
    raw = np.fromfile(str(tmp_path / "src.i16"), np.int16).reshape(sources, frames * 2)
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
    assert np.array_equal(fmt.matrix.ravel(), np.array(res["mix"], F))
    S, Cr = sources * 4, emspec.reduced_columns(res["columns"], f)
    wave = np.full((S, Cr, 2), 7.0, F)
    exact.set_time_reduce(f)
    exact.set_wave_out(wave)
    try:
        wire, offsets = exact.batch_pcm_packed(raw, fmt, n, hop, True)
    finally:
        exact.set_wave_out(None)
        exact.set_time_reduce(1)
    assert list(offsets) == [int(v) for v in res["offsets"]]
    assert np.array_equal(np.fromfile(str(tmp_path / "wire.u8"), np.uint8), wire[:offsets[-1]])
    got = np.fromfile(str(tmp_path / "wave.f32"), F).reshape(S, Cr, 2)
    assert W.same(got, wave) and W.same(got, W.envelope(PR.decode(raw.view(np.uint8), PR.S16, 2, fmt.matrix), n, hop, f))
    L = res["L"]
    pcm = np.fromfile(str(tmp_path / "pcm.f32"), F).reshape(3, L)
    assert W.same(np.fromfile(str(tmp_path / "wave_of.f32"), F).reshape(3, -1, 2), W.envelope(pcm, 1024, 255, 4))
