"""No GPU: the PCM front end's host-side contract - emspec_pcm_frame_bytes, format validation, the numpy restatement's known
answers (tests/pcm_ref.py), the named views of the bindings, and the argument checks that need no device."""
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


def test_symbols_exported():
    lib = emspec.load()
    for sym in ("emspec_pcm_frame_bytes", "emspec_pcm_decode_device", "emspec_batch_pcm", "emspec_batch_pcm_packed",
                "emspec_push_samples_pcm", "emspec_push_samples_pcm_multires"):
        assert hasattr(lib, sym) and sym in emspec.SYMBOLS


@pytest.mark.parametrize("name,per", [("s16", 2), ("s24", 3), ("s32", 4), ("f32", 4)])
def test_frame_bytes(name, per):
    for ch in range(1, 9):
        fmt = emspec.PcmFormat.make(name, ch, views=["mono"])
        assert emspec.pcm_frame_bytes(fmt) == per * ch == P.frame_bytes(fmt.sample_type, ch)


def test_frame_bytes_rejects_each_invalid_field():
    good = lambda: emspec.PcmFormat.make("s16", 2, views=["left", "right"])
    assert emspec.pcm_frame_bytes(good()) == 4
    assert emspec.pcm_frame_bytes(None) == -1
    for field, values in (("sample_type", (0, 5, -1)), ("channels", (0, 9, -2)), ("views", (0, 9, -1)), ("reserved", (1, -1))):
        for v in values:
            f = good()
            setattr(f, field, v)
            assert emspec.pcm_frame_bytes(f) == -1, (field, v)
    for bad in (float("nan"), float("inf"), -float("inf")):
        f = good()
        f.mix[3] = bad
        assert emspec.pcm_frame_bytes(f) == -1
    f = good()
    f.mix[4] = float("nan")   # beyond views * channels: not used
    assert emspec.pcm_frame_bytes(f) == 4


def test_restatement_known_answers():
    one = [[1.0]]
    s16 = np.array([-32768, 32767, 1, 0], "<i2").view(np.uint8)
    assert P.decode(s16, P.S16, 1, one)[0].tolist() == [-1.0, 32767 / 32768, 1 / 32768, 0.0]
    # S24: 0x800000 -> -1.0, 0x7FFFFF, and the byte order (least significant byte first)
    raw = np.array([0x00, 0x00, 0x80, 0xFF, 0xFF, 0x7F, 0x01, 0x00, 0x00, 0x00, 0x00, 0x01], np.uint8)
    assert P.decode(raw, P.S24, 1, one)[0].tolist() == [-1.0, (2 ** 23 - 1) / 2 ** 23, 2.0 ** -23, 2.0 ** -7]
    assert np.array_equal(P.s24_pack([-(1 << 23), (1 << 23) - 1, 1, 1 << 16]), raw)
    # S32: values that need rounding
    s32 = np.array([(1 << 24) + 1, -(1 << 31), (1 << 31) - 1, (1 << 24) + 3], "<i4").view(np.uint8)
    got = P.decode(s32, P.S32, 1, one)[0]
    assert got.tolist() == [2.0 ** -7, -1.0, 1.0, ((1 << 24) + 4) / 2.0 ** 31]   # 2^24+1 -> 2^24 (even), 2^24+3 -> 2^24+4
    f32 = np.array([0.25, -3.5], "<f4").view(np.uint8)
    assert P.decode(f32, P.F32, 1, one)[0].tolist() == [0.25, -3.5]


def test_mid_side_are_exact():
    rng = np.random.default_rng(5)
    ab = rng.integers(-32768, 32768, size=(4000, 2)).astype("<i2")
    ms = P.decode(ab.reshape(1, -1).view(np.uint8), P.S16, 2, [[0.5, 0.5], [0.5, -0.5]])
    a, b = ab[:, 0].astype(np.float64) / 32768, ab[:, 1].astype(np.float64) / 32768
    assert np.array_equal(ms[0].astype(np.float64), 0.5 * a + 0.5 * b)
    assert np.array_equal(ms[1].astype(np.float64), 0.5 * a - 0.5 * b)


def test_channel_order_is_ascending():
    """float32 addition does not associate: the restatement sums ((m0 x0 + m1 x1) + m2 x2), not another order."""
    x = np.array([1.0, 2.0 ** -24, 2.0 ** -24], "<f4").view(np.uint8)
    assert P.decode(x, P.F32, 3, [[1.0, 1.0, 1.0]])[0, 0] == np.float32(1.0)          # each small term is rounded away
    assert np.float32(1.0) + (np.float32(2.0 ** -24) + np.float32(2.0 ** -24)) != np.float32(1.0)


def test_named_views():
    m = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"]).matrix
    assert m.tolist() == [[1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [0.5, -0.5]]
    for ch in (1, 2, 3, 6, 8):
        w = emspec.PcmFormat.make("f32", ch, views=["mono"]).matrix
        assert w.shape == (1, ch) and np.all(w == np.float32(1.0) / np.float32(ch))
    mixed = emspec.PcmFormat.make(emspec.PCM_S24, 3, views=["left", [0.25, -1.5, 2.0]])
    assert mixed.views == 2 and mixed.matrix[1].tolist() == [0.25, -1.5, 2.0] and mixed.frame_bytes == 9
    with pytest.raises(ValueError):
        emspec.PcmFormat.make("s16", 1, views=["side"])
    with pytest.raises(ValueError):
        emspec.PcmFormat.make("s16", 2, views=[[1.0]])


def test_null_engine_is_an_error_not_a_crash():
    lib = emspec.load()
    fmt = emspec.PcmFormat.make("s16", 2, views=["left"])
    src = np.zeros(2 * 8192, np.int16)
    out = emspec.Out(None, None, None)
    offs = np.zeros(2, np.int64)
    wire = np.zeros(64, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.emspec_batch_pcm(None, p(src), C.byref(fmt), 1, 8192, 4096, 256, 1, C.byref(out)) == emspec.ERR_INVALID_ARG
    assert lib.emspec_batch_pcm_packed(None, p(src), C.byref(fmt), 1, 8192, 4096, 256, 1, p(wire), 64, p(offs)) == emspec.ERR_INVALID_ARG
    assert lib.emspec_pcm_decode_device(None, p(src), C.byref(fmt), 1, 8192, 4 * 8192, p(src), None) == emspec.ERR_INVALID_ARG
    cnt = np.zeros(1, np.int64)
    assert lib.emspec_push_samples_pcm(None, p(src), C.byref(fmt), 1, 128, 512, 4096, 256, 1, None, None, 1024, 0, p(cnt), p(cnt)) \
        == emspec.ERR_INVALID_ARG
    assert lib.emspec_push_samples_pcm_multires(None, p(src), C.byref(fmt), 1, 128, 512, 16384, 4096, 256, 256, 1, None, None, 1024,
                                                0, p(cnt), p(cnt)) == emspec.ERR_INVALID_ARG


def _node(script):
    """runs a script in em-spec_amd/js with node; None when node or the addon is absent"""
    import json
    import shutil
    import subprocess
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if shutil.which("node") is None or not os.path.exists(os.path.join(js, "emspec.node")):
        return None
    r = subprocess.run(["node", "-e", script], cwd=js, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_node_pcm_format_frame_bytes_and_named_views():
    """pcmFormat of the addon: emspec_pcm_frame_bytes through it (valid and invalid formats), and the named views' weights are
    the Python binding's floats.  Needs no device (the addon loads the library, no engine is made)."""
    res = _node("""
      const em = require('./index.js');
      const out = { bytes: {}, bad: [], views: {} };
      for (const type of ['s16', 's24', 's32', 'f32']) for (let ch = 1; ch <= 8; ch++) out.bytes[type + ch] = em.pcmFormat({ type, channels: ch }).frameBytes;
      out.bad.push(em.pcmFormat({ type: 'u8', channels: 2 }).frameBytes);
      out.bad.push(em.pcmFormat({ type: 's16', channels: 9, views: [[1, 0, 0, 0, 0, 0, 0, 0, 0]] }).frameBytes);
      out.bad.push(em.pcmFormat({ type: 's16', channels: 1, views: new Array(9).fill('mono') }).frameBytes);
      out.bad.push(em.pcmFormat({ type: 's16', channels: 2, views: [[1, NaN]] }).frameBytes);
      for (const ch of [1, 2, 3, 6, 8]) {
        const names = ch >= 2 ? ['left', 'right', 'mid', 'side', 'mono'] : ['left', 'mono'];
        out.views[ch] = Array.from(new Uint32Array(em.pcmFormat({ type: 'f32', channels: ch, views: names }).mix.buffer));
      }
      console.log(JSON.stringify(out));
    """)
    if res is None:
        pytest.skip("node or the addon is not available")
    per = {"s16": 2, "s24": 3, "s32": 4, "f32": 4}
    for t, b in per.items():
        for ch in range(1, 9):
            assert res["bytes"][f"{t}{ch}"] == b * ch
    assert res["bad"] == [-1, -1, -1, -1]
    for ch in (1, 2, 3, 6, 8):
        names = ["left", "right", "mid", "side", "mono"] if ch >= 2 else ["left", "mono"]
        py = emspec.PcmFormat.make("f32", ch, views=names).matrix
        assert res["views"][str(ch)] == py.view(np.uint32).reshape(-1).tolist()
