"""CPU: the level meters (include/emspec.h: emspec_level_host, emspec_cross_host and the pure helpers) without
a device - the host forms against tests/level_ref.py byte for byte on the envelope's cases and on the worst-case signals, the
quantiser's edges, the factor law, known answers through the helpers, the refusals, the plan header through its stand-alone
driver (tests/cdriver/window_plan_driver.cpp), and the Node binding's levelsOf / crossOf."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec
import level_ref as LR
import worst_signals as WS
from window_cases import PRECEDENCE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
IDS = dict(ids=lambda c: "n%d-hop%d-L%d-f%d" % c)


@pytest.fixture(scope="module")
def refs():
    """case -> (signal, reference level records, reference cross records of streams (0, 1) of the 3), computed once"""
    out = {}
    for case in LR.CASES:
        n, hop, L, f = case
        x = LR.case_signal(case)
        out[case] = (x, LR.levels(x, n, hop, f), LR.crosses(x, 3, 0, 1, n, hop, f))
    return out


def test_reference_quantiser_forms_agree():
    """The vectorised quantiser of the reference is its scalar definition, on the edges and on random bits."""
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(U),
                        np.array([0, 1, 0x80000000, 0x007FFFFF, 0x32800000, 0x32800001, 0x33000000, 0x33400000, 0x33C00000, 0x34200000,
                                  0x42FFFFFF, 0x43000000, 0xC3000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001], U)])
    k, odd = LR.quantise_all(u)
    for ui, ki, oi in zip(u, k, odd):
        assert LR.quantise(ui) == (int(ki), int(oi)), hex(int(ui))


@pytest.mark.parametrize("case", LR.CASES, **IDS)
def test_level_and_cross_host_are_the_reference(refs, case):
    n, hop, L, f = case
    x, want, cwant = refs[case]
    assert LR.same(emspec.level_host(x, n, hop, f), want)
    assert LR.same(emspec.cross_host(x, 3, 0, 1, n, hop, f), cwant)
    # a stream against itself: the cross limbs are the level's sums; views 1 is every stream its own pair
    self = emspec.cross_host(x, 1, 0, 0, n, hop, f)
    assert np.array_equal(self["lo"], want["sq_lo"]) and np.array_equal(self["hi"].astype(np.uint64), want["sq_hi"])


def test_reference_array_form_is_the_integer_form(refs):
    """levels / crosses (numpy, int64 sums) against level_of / cross_of (Python integers) on windows of a case with odd samples."""
    case = (1024, 255, 1024 + 255 * 9 + 100, 4)
    n, hop, L, f = case
    x, lv, cr = refs[case]
    u = x.view(U)
    C = LR.num_columns(L, n, hop)
    for g in range(lv.shape[1]):
        i0, i1 = LR.window(g, C, n, hop, f)
        for s in range(3):
            assert tuple(int(v) for v in lv[s, g]) == LR.level_of(u[s, i0:i1])
        assert tuple(int(v) for v in cr[0, g]) == LR.cross_of(u[0, i0:i1], u[1, i0:i1])


def test_cases_hold_what_they_plant(refs):
    """Over the case list the references show the odd samples (a window of NaN only counts every sample and sums nothing; the
    infinities and +-1e30 saturate) and records whose high limb is used."""
    lv = np.concatenate([r.ravel() for _, r, _ in refs.values()])
    assert (lv["odd"] > 0).any() and ((lv["odd"] > 0) & (lv["sq_lo"] == 0) & (lv["sq_hi"] == 0) & (lv["peak"] == 0)).any()
    assert (lv["peak"] == LR.KMAX).any() and (lv["sq_hi"] > 0).any() and ((lv["peak"] == 0) & (lv["odd"] == 0)).any()
    cr = np.concatenate([r.ravel() for _, _, r in refs.values()])
    assert (cr["hi"] < 0).any() and (cr["hi"] > 0).any()


@pytest.mark.parametrize("kind", WS.KINDS)
def test_worst_signals(kind):
    n, hop = 1024, 256
    x = np.stack([WS.signal(kind, n, hop, 12), WS.signal("chirp_reach", n, hop, 12)])
    for f in (1, 5):
        assert LR.same(emspec.level_host(x, n, hop, f), LR.levels(x, n, hop, f))
        assert LR.same(emspec.cross_host(x, 2, 1, 0, n, hop, f), LR.crosses(x, 2, 1, 0, n, hop, f))


def _one_window(values):
    """the level record of a stream whose single window (n = hop = 256) holds `values` and zeros"""
    x = np.zeros((1, 256), F)
    bits = values if isinstance(values, np.ndarray) and values.dtype == U else np.asarray(values, F).view(U)
    x.view(U)[0, :len(bits)] = bits
    return emspec.level_host(x, 256, 256)[0, 0], x


def test_quantiser_edges():
    e25 = F(2.0 ** -25)
    up = np.nextafter(e25, F(1))
    for v, k in [(e25, 0), (-e25, 0), (up, 1), (-up, 1), (F(1.5 * 2.0 ** -24), 2), (F(2.5 * 2.0 ** -24), 2), (F(-2.5 * 2.0 ** -24), 2),
                 (F(3.5 * 2.0 ** -24), 4), (F(1.0), 2 ** 24), (F(-1.0), 2 ** 24), (F(1e-40), 0), (F(-0.0), 0)]:
        r, _ = _one_window([v])
        assert (int(r["peak"]), int(r["odd"])) == (k, 0), (v, r)
        assert LR.sum_sq(r) == k * k
    below = np.nextafter(F(128), F(0))
    r, _ = _one_window([below])
    assert int(r["odd"]) == 0 and int(r["peak"]) == 2 ** 31 - 128
    for v in (F(128), F(-128), F(np.inf), F(-np.inf), F(1e30)):
        r, _ = _one_window([v])
        assert (int(r["peak"]), int(r["odd"])) == (LR.KMAX, 1) and LR.sum_sq(r) == LR.KMAX ** 2, (v, r)
    # NaN with either sign and with payloads: counted, taken as 0
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FABCDEF], U)
    r, x = _one_window(nans)
    assert (int(r["peak"]), int(r["odd"]), LR.sum_sq(r)) == (0, 5, 0)
    # the sign goes into the cross record only: (-3)(+5) 2^-48
    y = np.zeros((2, 256), F)
    y[0, 0], y[1, 0] = F(-3 * 2.0 ** -24), F(5 * 2.0 ** -24)
    c = emspec.cross_host(y, 2, 0, 1, 256, 256)[0, 0]
    assert LR.sum_ab(c) == -15 and int(c["hi"]) == -1 and int(c["lo"]) == 2 ** 32 - 15
    # a NaN against anything contributes nothing
    y.view(U)[0, 0] = 0x7FC00000
    assert LR.sum_ab(emspec.cross_host(y, 2, 0, 1, 256, 256)[0, 0]) == 0


@pytest.mark.parametrize("case", [c for c in LR.CASES if c[3] > 1], **IDS)
def test_factor_law(refs, case):
    n, hop, L, f = case
    x, _, _ = refs[case]
    assert LR.same(emspec.level_host(x, n, hop, f), LR.regroup(emspec.level_host(x, n, hop, 1), f))
    assert LR.same(emspec.cross_host(x, 3, 2, 1, n, hop, f), LR.regroup(emspec.cross_host(x, 3, 2, 1, n, hop, 1), f))


def test_known_answers_through_the_helpers():
    n = hop = 1024
    L, per = 8 * 1024, 64                                    # 128 whole periods in the one window at f = 8
    t = np.arange(L)
    sine = np.sin(2 * np.pi * t / per).astype(F)
    quad = np.cos(2 * np.pi * t / per).astype(F)
    x = np.stack([sine, sine, -sine, quad, np.zeros(L, F)])
    lv = emspec.level_host(x, n, hop, 8)[:, 0]
    samples = emspec.level_window(L, n, hop, 8, 0)
    assert samples == L and emspec.level_window(L, n, hop, 8, 1) == 0 and emspec.level_window(L, n, hop, 3, 2) == 2 * 1024
    rms, peak = emspec.level_values(lv[0], samples)
    # from the integer sums: 10 log10(sum k^2 / N) - 20 log10(2^24), in binary64 from Python's exact integers
    want = 10 * math.log10(LR.sum_sq(lv[0]) / samples) - 20 * math.log10(2 ** 24)
    assert abs(rms - want) < 1e-9 and round(rms, 4) == -3.0103 and abs(rms - 10 * math.log10(0.5)) < 1e-6
    assert peak == 0.0 and int(lv[0]["peak"]) == 2 ** 24 and int(lv[0]["odd"]) == 0
    cross = lambda a, b: emspec.cross_host(x, 5, a, b, n, hop, 8)[0, 0]
    assert emspec.cross_correlation(lv[0], lv[1], cross(0, 1)) == 1.0
    assert emspec.cross_correlation(lv[0], lv[2], cross(0, 2)) == -1.0
    assert abs(emspec.cross_correlation(lv[0], lv[3], cross(0, 3))) < 1e-6
    # silence: -inf and rho = 0
    assert emspec.level_values(lv[4], samples) == (-math.inf, -math.inf)
    assert emspec.cross_correlation(lv[4], lv[0], cross(4, 0)) == 0.0 and emspec.cross_correlation(lv[4], lv[4], cross(4, 4)) == 0.0
    # half scale: -6.02 dB peak
    half = emspec.level_host((sine * F(0.5))[None], n, hop, 8)[0, 0]
    assert abs(emspec.level_values(half, samples)[1] - 20 * math.log10(0.5)) < 1e-12
    lib = emspec.load()
    assert lib.emspec_level_values(None, 1, None, None) == emspec.ERR_INVALID_ARG
    one = emspec.Level(1, 0, 1, 0)
    assert lib.emspec_level_values(C.byref(one), 0, None, None) == emspec.ERR_INVALID_ARG
    assert lib.emspec_cross_correlation(C.byref(one), C.byref(one), None, None) == emspec.ERR_INVALID_ARG


def test_sizes_and_header():
    assert C.sizeof(emspec.Level) == 24 and C.sizeof(emspec.Cross) == 16
    assert emspec.LEVEL_DTYPE.itemsize == 24 and emspec.CROSS_DTYPE.itemsize == 16
    assert emspec.LEVEL_DTYPE == LR.LEVEL and emspec.CROSS_DTYPE == LR.CROSS
    lib = emspec.load()
    header = open(os.path.join(ROOT, "include", "emspec.h")).read()
    for sym in emspec.LEVEL_SYMBOLS:
        assert hasattr(lib, sym) and sym in emspec.SYMBOLS and sym in header
    assert len(emspec.LEVEL_SYMBOLS) == 9
    assert "typedef struct emspec_level { uint64_t sq_lo; uint64_t sq_hi; uint32_t peak; uint32_t odd; } emspec_level;" in header
    assert "typedef struct emspec_cross { uint64_t lo; int64_t hi; } emspec_cross;" in header
    assert "#define EMSPEC_ABI_VERSION 2" in header and "No RMS or other sum" not in header


def test_refusals():
    lib = emspec.load()
    x = np.zeros((4, 1000), F)
    out = np.full((4, 8, 3), 7, np.uint64)
    p, o = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(fn, *a):
        rc = fn(*a)
        msg = lib.emspec_last_error(None).decode()
        assert rc == emspec.ERR_INVALID_ARG and msg, (rc, msg)
        return msg

    lv, cr = lib.emspec_level_host, lib.emspec_cross_host
    assert "factor" in refused(lv, p, 2, 1000, 256, 100, 0, o) and "factor" in refused(lv, p, 2, 1000, 256, 100, 65537, o)
    assert "hop" in refused(lv, p, 2, 1000, 256, 0, 1, o) and "hop" in refused(lv, p, 2, 1000, 256, 257, 1, o)
    assert "fft size" in refused(lv, p, 2, 1000, 300, 100, 1, o) and "fft size" in refused(lv, p, 2, 1000, 32768, 100, 1, o)
    assert "streams" in refused(lv, p, -1, 1000, 256, 100, 1, o) and "streams" in refused(lv, p, 65536, 1000, 256, 100, 1, o)
    assert "length" in refused(lv, p, 2, -1, 256, 100, 1, o)
    assert "null" in refused(lv, None, 2, 1000, 256, 100, 1, o) and "null" in refused(lv, p, 2, 1000, 256, 100, 1, None)
    assert "4-byte" in refused(lv, C.c_void_p(x.ctypes.data + 2), 1, 998, 256, 100, 1, o)
    assert "8-byte" in refused(lv, p, 2, 1000, 256, 100, 1, C.c_void_p(out.ctypes.data + 4))
    assert "views" in refused(cr, p, 1, 0, 0, 0, 1000, 256, 100, 1, o) and "views" in refused(cr, p, 1, 65, 0, 0, 1000, 256, 100, 1, o)
    assert "a and b" in refused(cr, p, 2, 2, 2, 0, 1000, 256, 100, 1, o) and "a and b" in refused(cr, p, 2, 2, 0, -1, 1000, 256, 100, 1, o)
    assert "pairs x views" in refused(cr, p, 1024, 64, 0, 1, 1000, 256, 100, 1, o) and "pairs x views" in refused(cr, p, -1, 2, 0, 1, 1000, 256, 100, 1, o)
    assert "factor" in refused(cr, p, 2, 2, 0, 1, 1000, 256, 100, 0, o) and "hop" in refused(cr, p, 2, 2, 0, 1, 1000, 256, 0, 1, o)
    assert "fft size" in refused(cr, p, 2, 2, 0, 1, 1000, 300, 100, 1, o)
    assert "null" in refused(cr, None, 2, 2, 0, 1, 1000, 256, 100, 1, o) and "null" in refused(cr, p, 2, 2, 0, 1, 1000, 256, 100, 1, None)
    assert "8-byte" in refused(cr, p, 2, 2, 0, 1, 1000, 256, 100, 1, C.c_void_p(out.ctypes.data + 4))
    assert np.all(out == 7)
    # L < n: no column, nothing to write - a no-op even without an output; so are S = 0 and pairs = 0
    assert lv(p, 2, 255, 256, 100, 1, None) == 0 and lv(None, 0, 1000, 256, 100, 1, None) == 0
    assert cr(p, 2, 2, 0, 1, 255, 256, 100, 1, None) == 0 and cr(None, 0, 2, 0, 1, 1000, 256, 100, 1, None) == 0
    # and the bindings raise with the library's message
    with pytest.raises(emspec.EmspecError, match="factor"):
        emspec.level_host(x, 256, 100, 0)
    with pytest.raises(emspec.EmspecError, match="a and b"):
        emspec.cross_host(x, 2, 0, 2, 256, 100)


def test_host_forms_report_the_first_broken_rule():
    lib = emspec.load()
    x = np.zeros((4, 1000), F)
    out = np.full((4, 8, 3), 7, np.uint64)
    p, o = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for (S, L, n, hop, f), word in PRECEDENCE:
        for call in (lambda: lib.emspec_wave_host(p, S, L, n, hop, f, o), lambda: lib.emspec_level_host(p, S, L, n, hop, f, o),
                     lambda: lib.emspec_cross_host(p, S, 1, 0, 0, L, n, hop, f, o)):
            msg = (call(), lib.emspec_last_error(None).decode())
            assert msg[0] == emspec.ERR_INVALID_ARG and word in msg[1], ((S, L, n, hop, f), msg)
    # the choice of streams comes first
    assert lib.emspec_cross_host(p, -1, 0, 0, 0, -1, 300, 0, 0, o) == emspec.ERR_INVALID_ARG and "views" in lib.emspec_last_error(None).decode()
    assert lib.emspec_cross_host(p, 1024, 64, 0, 1, -1, 300, 0, 0, o) == emspec.ERR_INVALID_ARG and "pairs x views" in lib.emspec_last_error(None).decode()
    assert np.all(out == 7)


def test_level_plan_driver(tmp_path):
    """The stand-alone driver over the plan headers, built with the host compiler under ASan and UBSan (a program of its own:
    nothing is preloaded): the quantiser against the integer form, limb bounds at 2^30 saturated samples, combine associativity on
    random splits, the pipeline table's offsets and coverage with the new rows set and cleared - and the kernels' own scan for the
    envelope, level and cross reducers: every lane of every team size against the plain loop on heap blocks that end with the
    window, the pieces of long windows, the team rule."""
    exe = str(tmp_path / "window_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "window_plan_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr and r.stdout.startswith("ok "), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    quantised, splits, plans, scans, pieces = (int(v) for v in r.stdout.split()[1:6])
    assert quantised >= 2000000 and splits == 300 and plans >= 1000
    # 76 lengths x 4 alignments of A (x 4 of B for the cross reducer) x 2 kinds of window x 8 team sizes; 13 pieces per reducer
    assert scans == 76 * 4 * 2 * 8 * (1 + 1 + 4) and pieces == 3 * 13


def test_node_levels_of_is_the_reference(refs):
    node = shutil.which("node") or shutil.which("nodejs")
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not node or not os.path.exists(os.path.join(js, "emspec.node")):
        return                                                   # (compared where the addon is built)
    for case in [c for c in LR.CASES if c[0] <= 1024]:
        n, hop, L, f = case
        x, want, cwant = refs[case]
        code = ("const em = require('./index.js'); const fs = require('fs');"
                "const b = fs.readFileSync(0); const x = new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length));"
                f"const lv = em.levelsOf(x, {x.shape[0]}, {L}, {n}, {hop}, {f});"
                f"const cr = em.crossOf(x, 1, 3, 0, 1, {L}, {n}, {hop}, {f});"
                "process.stdout.write(Buffer.from(lv.bytes.buffer, 0, lv.bytes.byteLength));"
                "process.stdout.write(Buffer.from(cr.bytes.buffer, 0, cr.bytes.byteLength));")
        r = subprocess.run([node, "-e", code], cwd=js, input=x.tobytes(), capture_output=True, check=True, timeout=60)
        nb = want.nbytes
        assert r.stdout[:nb] == want.tobytes() and r.stdout[nb:] == cwant.tobytes(), case
