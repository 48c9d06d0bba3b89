"""CPU: the stereo image (include/emspec.h: emspec_stereo_*) without a GPU.  The host twin emspec_stereo_host
(plain C++ in the product library) and a stand-alone program over the same HIP-free header
(em-spec_amd/csrc/emspec_stereo_plan.h, tests/cdriver/stereo_plan_driver.cpp - built with the host compiler under ASan and
UBSan; nothing is preloaded, nothing is loaded into Python under a sanitizer) are held, byte for byte, against the numpy
restatement tests/stereo_ref.py: on a constructed array of every special case of the law, and on the bit models' dB of the test
signal the GPU tests use.  Then the palette builder, every refusal of the host twin, the struct's size, and that the signal
exercises the law - without that a kernel that writes one constant could pass the GPU tests."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import emspec
import oracle as O
import stereo_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32
ROWS = 64
MAPS = {"default": T.DEFAULT_MAP, "view": T.VIEW_MAP}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stereo_plan")
    exe = str(tmp / "stereo_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "stereo_plan_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (args[:2], r.returncode, r.stderr[-2000:])
        return r.stdout
    run.tmp = tmp
    return run


def _hex(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _driver_compose(driver, db, views, a, b, map):
    """The stand-alone program's four outputs for db [pairs * views][cells]."""
    db = np.ascontiguousarray(db, F).reshape(db.shape[0], -1)
    pairs, cells = db.shape[0] // views, db.shape[1]
    src, dst = driver.tmp / "in.bin", driver.tmp / "out.bin"
    db.tofile(src)
    driver("compose", src, dst, pairs, views, a, b, cells, *[_hex(x) for x in map])
    raw = np.fromfile(dst, np.uint8)
    n = pairs * cells
    assert raw.size == 10 * n
    return {"level": raw[:4 * n].view(F).reshape(pairs, cells), "index": raw[4 * n:5 * n].reshape(pairs, cells),
            "pan": raw[5 * n:6 * n].reshape(pairs, cells), "rgba": raw[6 * n:].reshape(pairs, cells, 4)}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


def _equal(got, want, what):
    assert _same_bits(got["level"].reshape(want["level"].shape), want["level"]), what
    for k in ("index", "pan", "rgba"):
        if want[k] is not None and got[k] is not None:
            assert np.array_equal(got[k].reshape(want[k].shape), want[k]), (what, k)


@functools.lru_cache(maxsize=None)
def _model_db(exact):
    """The bit model's dB of the decoded test signal: [8][27][64], streams L R M S of two sources.  Computed once, read-only."""
    pcm = T.decoded_signal(4)
    cfg = O.make_cfg(T.N, T.HOP, True, rows=ROWS)
    db = (O.batch_exact(cfg, pcm, want=("db",)) if exact else O.batch_f32(cfg, pcm, want=("db",)))[0]
    assert db.shape == (8, T.FRAMES, ROWS)
    db.setflags(write=False)
    return db


def _streams(db, views):
    """views = 2: the L R streams of both sources; 4: all of them."""
    return db if views == 4 else np.ascontiguousarray(db.reshape(2, 4, *db.shape[1:])[:, :2].reshape(4, *db.shape[1:]))


# ---- 1. the host twin and the stand-alone program against the restatement ----
@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("pan_range", [16.0, 12.0])
def test_special_cases_byte_for_byte(driver, name, pan_range):
    map = MAPS[name][:4] + (pan_range,)
    db = T.special_cases(map)
    pal = emspec.make_stereo_colormap(0.5)
    want = T.compose(db, 2, 0, 1, map, pal)
    # the restatement itself does what the issue says of the special cases
    xa, xb = db
    lv, pan, idx = want["level"][0], want["pan"][0], want["index"][0]
    assert np.isnan(lv[2]) and not np.isnan(lv[0]) and not np.isnan(lv[1])          # NaN only when both are
    assert lv[0] == F(-20) and lv[1] == F(-20) and (pan[0], pan[1], pan[2]) == (16, 16, 16) and idx[2] == 0
    assert lv.view(U)[3] == xb.view(U)[3] and lv.view(U)[4] == 0x7FC12345             # both NaN: B's own bits
    assert list(pan[5:9]) == [0, 32, 32, 0] and list(pan[9:11]) == [16, 16] and list(pan[11:13]) == [0, 32]
    assert idx[5] == 255 and idx[10] == 0
    assert list(lv.view(U)[13:17]) == list(xa.view(U)[13:17])                        # -0 / +0: neither is greater, A's bits
    gate = slice(17, 23)
    assert list(pan[gate]) == [0, 32, 16, 16, 16, 16] and not want["gated"][0][17:20].any() and want["gated"][0][20:23].all()
    assert (idx[20:23] == 0).all()
    assert list(pan[23:31]) == ([32, 32, 32, 32, 0, 0, 0, 0] if pan_range == 12.0 else [28, 28, 32, 32, 4, 4, 0, 0])
    if pan_range == 16.0:      # half to even: k + 0.5 -> the even neighbour, on both constructions
        ties = pan[31:31 + 64].reshape(32, 2).astype(int) - 16
        for k, (p0, p1) in zip(range(-16, 16), ties):
            even = k if k % 2 == 0 else k + 1
            assert p0 == p1 == even, (k, p0, p1)
    for got, who in ((emspec.stereo_host(db, 2, 0, 1, map, pal, want=("level", "index", "pan", "rgba")), "host twin"),
                     (_driver_compose(driver, db, 2, 0, 1, map), "driver")):
        _equal(got, want, (who, name, pan_range))
    # channels swapped: the other stream order through (a, b) = (1, 0)
    swapped = T.compose(db, 2, 1, 0, map, pal)
    _equal(emspec.stereo_host(db, 2, 1, 0, map, pal, want=("level", "index", "pan", "rgba")), swapped, "swapped")
    assert np.array_equal(swapped["pan"][0][23:31], 32 - want["pan"][0][23:31])


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_bit_model_db_byte_for_byte_and_the_signal_exercises_the_law(driver, exact, name):
    """The four (views, a, b) on the bit model's dB under both maps; per case at least 24 balance values among ungated cells
    with both ends and the centre, more than 8 palette indices, at least 400 ungated cells (measured when this was written:
    at least 30 of 33 balance values and 170 indices per case; mid / side centres more than 40 % of its cells)."""
    db = _model_db(exact)
    pal = emspec.make_stereo_colormap(0.5)
    for views, a, b in T.CASES:
        x = _streams(db, views)
        want = T.compose(x, views, a, b, MAPS[name], pal)
        assert want["level"].shape == (2, T.FRAMES, ROWS)
        got = emspec.stereo_host(x, views, a, b, MAPS[name], pal, want=("level", "index", "pan", "rgba"))
        _equal(got, want, ("host twin", views, a, b))
        _equal(_driver_compose(driver, x, views, a, b, MAPS[name]), want, ("driver", views, a, b))
        pans, indices, cells = T.exercised(want)
        print(name, "exact" if exact else "fast", (views, a, b), "balance values", pans, "indices", indices, "ungated cells", cells,
              "centred %.2f" % float(np.mean(want["pan"] == 16)))
    # each output asked for alone gives the same bytes
    x = _streams(db, 4)
    full = emspec.stereo_host(x, 4, 2, 3, MAPS[name], pal, want=("level", "index", "pan", "rgba"))
    for k in ("level", "index", "pan", "rgba"):
        only = emspec.stereo_host(x, 4, 2, 3, MAPS[name], pal if k == "rgba" else None, want=(k,))
        assert all(only[o] is None for o in only if o != k) and np.array_equal(only[k].view(np.uint8), full[k].view(np.uint8)), k


# ---- 2. the palette ----
def test_palette_builder(driver):
    for brightness in (0.5, 0.7, 1.0, 0.05):
        base = emspec.make_colormap(brightness)
        want = T.palette(base)
        got = emspec.make_stereo_colormap(brightness)
        assert got.shape == (33, 256, 4) and np.array_equal(got, want), brightness
        out = driver.tmp / "pal.bin"
        driver("palette", out, _hex(brightness))
        assert np.array_equal(np.fromfile(out, np.uint8).reshape(33, 256, 4), want), brightness
        assert np.array_equal(got[16], base)
        assert not np.array_equal(got[0], base) and not np.array_equal(got[32], base) and not np.array_equal(got[0], got[32])
        assert np.array_equal(got[:, :, 3], np.broadcast_to(base[:, 3], (33, 256)))
    pal = emspec.make_stereo_colormap(0.5)
    assert np.array_equal(pal[16], O.default_lut())                     # the engine's default colour map
    assert pal[0, 255].tolist() == [255, 96, 32, 255] and pal[32, 255].tolist() == [32, 160, 255, 255]
    with pytest.raises(emspec.EmspecError):
        emspec.make_stereo_colormap(-1.0)


# ---- 3. refusals ----
def test_every_refusal_of_the_host_twin(driver):
    db = np.zeros((4, 8), F)
    ok = T.DEFAULT_MAP
    nan = float("nan")

    def refused(needle, *args, **kw):
        with pytest.raises(emspec.EmspecError) as ei:
            emspec.stereo_host(*args, **kw)
        assert ei.value.code == emspec.ERR_INVALID_ARG and needle in str(ei.value), str(ei.value)
    refused("views >= 2", db, 1, 0, 0, ok)
    refused("0 .. views - 1", db, 2, 0, 2, ok)
    refused("0 .. views - 1", db, 2, -1, 1, ok)
    refused("must differ", db, 2, 1, 1, ok)
    refused("negative", np.zeros((3, 8), F), 2, 0, 1, ok)                      # (the binding passes -1 pairs for 3 streams of 2 views)
    refused("cells % 4", np.zeros((4, 6), F), 2, 0, 1, ok)
    refused("db_range > 0", db, 2, 0, 1, (0.0, 0.0, -80.0, 0.0, 12.0))
    refused("db_range > 0", db, 2, 0, 1, (0.0, nan, -80.0, 0.0, 12.0))
    refused("pan_range_db > 0", db, 2, 0, 1, (0.0, 80.0, -80.0, 0.0, 0.0))
    refused("pan_range_db > 0", db, 2, 0, 1, (0.0, 80.0, -80.0, 0.0, -3.0))
    refused("pan_range_db > 0", db, 2, 0, 1, (0.0, 80.0, -80.0, 0.0, nan))
    for i in (0, 2, 3):
        m = list(ok)
        m[i] = nan
        refused("NaN", db, 2, 0, 1, tuple(m))
    refused("null map", db, 2, 0, 1, None)
    refused("at least one output", db, 2, 0, 1, ok, want=())
    refused("palette", db, 2, 0, 1, ok, want=("rgba",))
    lib = emspec.load()
    m = emspec.StereoMap(*ok)
    out = np.empty((2, 8), np.uint8)
    import ctypes as C
    assert lib.emspec_stereo_host(None, 2, 2, 0, 1, 8, C.byref(m), None, None, out.ctypes.data, None, None) == emspec.ERR_INVALID_ARG
    assert lib.emspec_stereo_host(db.ctypes.data + 2, 2, 2, 0, 1, 8, C.byref(m), None, None, out.ctypes.data, None, None) == emspec.ERR_INVALID_ARG
    assert b"aligned" in lib.emspec_last_error(None)
    assert lib.emspec_stereo_host(None, 0, 2, 0, 1, 8, C.byref(m), None, None, out.ctypes.data, None, None) == emspec.OK   # no pairs: a no-op
    # and a call that is accepted afterwards
    assert emspec.stereo_host(db, 2, 0, 1, ok)["pan"].tolist() == [[16] * 8] * 2
    # the stand-alone program names the same rules
    assert "views >= 2" in driver("check", 1, 0, 0, *[_hex(x) for x in ok])
    assert "must differ" in driver("check", 4, 3, 3, *[_hex(x) for x in ok])
    assert "pan_range_db" in driver("check", 2, 0, 1, *[_hex(x) for x in ok[:4] + (0.0,)])
    assert driver("check", 4, 2, 3, *[_hex(x) for x in ok]).strip() == "ok"


# ---- 4. the struct ----
def test_struct_size_and_abi_version(driver):
    import ctypes as C
    assert driver("abi").split() == ["20", "2", "16", "33"]
    assert C.sizeof(emspec.StereoMap) == 20 and emspec.ABI_VERSION == 2
    assert (emspec.STEREO_PAN_CENTRE, emspec.STEREO_PAN_LEVELS) == (T.CENTRE, T.LEVELS) == (16, 33)
    assert set(emspec.STEREO_SYMBOLS) <= set(emspec.SYMBOLS)
