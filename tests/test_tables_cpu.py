"""CPU: what the kernels take as given - the twiddle and row-edge tables in float32 and binary64, the specified ratio^x, the
palettes and the per-shape scalars of PlanDev / ExactPlanDev / DbMap / ExactDbMap (em-spec_amd/csrc/emspec_tables.h; DESIGN.md
§3.1, §3.7) - against the bit models of oracle/ and against numpy restatements, bit for bit, without a GPU.

tests/cdriver/tables_driver.cpp is a program of its own that includes only that header, built with the host compiler under ASan
and UBSan (nothing is preloaded, nothing is loaded into Python under a sanitizer):

    g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
        tests/cdriver/tables_driver.cpp -o tables_driver

Every run must exit with status 0 and an empty stderr."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import axis_cases as A
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384)
ROWS = (64, 1024, 4096)
# (sample_rate, fmin, fmax): the default axis, a narrower one at another rate, and one whose unclamped binary64 top edge rounds
# above N / 2 (tests/axis_cases.py: tel)
AXES = ((48000.0, 20.0, 24000.0), (44100.0, 30.0, 20000.0), (8000.0, 30.0, 4000.0))
WARPED = (1024, 20.0, 24000.0, 2.0, 1.6)   # the custom axis of the GPU tests (test_gpu_exact.py, test_gpu_sizes.py)


def f32(x):
    return "%08x" % int(np.array(x, F).view(np.uint32))


def f64(x):
    return "%016x" % int(np.array(x, np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tables") / "tables_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "tables_driver.cpp"), "-o", exe])

    def run(*args):
        """One case in a child process -> {name: [tokens]} of the lines it printed."""
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (args, r.returncode, r.stderr[-2000:])
        return {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] if " " in ln else "" for ln in r.stdout.splitlines()}
    return run


def bits(tokens, dtype):
    """Hex bit patterns -> an array of that unsigned type (compare these: NaNs and signed zeros count)."""
    return np.array([int(t, 16) for t in tokens.split()], dtype)


def as_f32(tokens):
    return bits(tokens, np.uint32).view(F)


def as_f64(tokens):
    return bits(tokens, np.uint64).view(np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


@pytest.fixture(scope="module")
def warped(driver):
    """The custom axis, by the header's own law (test_colormap_and_warped_edges_are_the_library_s ties it to the library's)."""
    return as_f32(driver("warped", WARPED[0], *map(f32, WARPED[1:]))["hz"])


def test_twiddles_are_the_bit_models(driver):
    """float32: oracle.tables; binary64: eo_twiddle64; and the properties the kernels rely on, in binary64 too."""
    for n in SIZES:
        out = driver("twiddles", n)
        tw32, tw64 = as_f32(out["tw32"]), as_f64(out["tw64"])
        assert same_bits(tw32, O.tables(O.make_cfg(n, 256))[0]), n
        assert same_bits(tw64, O.twiddle64(n)), n
        re, im = tw64[0::2], tw64[1::2]
        q = n // 4
        assert np.array_equal(re[q:], im[:q]) and np.array_equal(im[q:], -re[:q]), n   # tw[q + N/4] == (tw[q].im, -tw[q].re)
        assert same_bits(re[q + 1:], im[1:q]) and same_bits(im[q + 1:], -re[1:q]), n   # (in every bit but for the exact entry)
        assert re[q] == 0.0 and not np.signbit(re[q]) and im[q] == -1.0 and re[0] == 1.0, n


def _edge_cases(warped):
    for n in SIZES:
        for (sr, lo, hi), rows in itertools.product(AXES, ROWS):
            yield n, rows, sr, lo, hi, None
        yield n, WARPED[0], 48000.0, WARPED[1], WARPED[2], warped


def test_edges_are_the_bit_models(driver, warped, tmp_path):
    """float32 edges: oracle.tables; binary64 edges: oracle.edges64; the Hz value of every edge and the 6 % axis test of the EXACT
    mode's no-parking kernel restated here.  70 cases: every N, three row counts on three log axes, and the custom axis.  The
    top edge is min(e[R], N / 2): the Hz value of the last edge is fmax itself, its bin value never exceeds N / 2."""
    path = tmp_path / "warped.f32"
    warped.tofile(path)
    count = 0
    for n, rows, sr, lo, hi, custom in _edge_cases(warped):
        cfg = O.make_cfg(n, 256, rows=rows, sample_rate=sr, fmin_hz=lo, fmax_hz=hi)
        O.set_custom_edges_hz(custom)
        try:
            want32, want64 = O.tables(cfg)[1], O.edges64(cfg)
        finally:
            O.set_custom_edges_hz(None)
        out = driver("edges", n, rows, f32(sr), f32(lo), f32(hi), *([path] if custom is not None else []))
        case = (n, rows, sr, custom is not None)
        assert same_bits(as_f32(out["e32"]), want32), case
        assert same_bits(as_f64(out["e64"]), want64), case
        assert out["error32"] == "-" and out["error64"] == "-", case
        if custom is None:
            ratio = float(F(hi)) / float(F(lo))
            hz = np.array([float(F(lo)) * _spec_pow(ratio, r / rows) for r in range(rows + 1)])
        else:
            hz = custom.astype(np.float64)
        assert same_bits(as_f64(out["hz"]), hz), case
        assert out["low_share_ok"].split() == ["1" if h / (float(F(sr)) * 0.5) <= 0.06 else "0" for h in hz], case
        raw = hz * float(n) / float(F(sr))
        assert same_bits(want64[:-1], raw[:-1]) and want64[-1] == min(raw[-1], n / 2), case
        if custom is None and hi == sr / 2:
            assert want64[-1] == n / 2 and want32[-1] == F(n / 2), case
        count += 1
    assert count == 70
    assert A.raw_top_edge("tel", 4096) > 2048.0      # the clamp decides on that axis


def _spec_pow(ratio, x):
    lib = O.lib()
    lib.eo_spec_pow.restype = C.c_double
    lib.eo_spec_pow.argtypes = [C.c_double, C.c_double]
    return lib.eo_spec_pow(ratio, x)


def test_spec_pow_is_the_bit_model_s(driver):
    for ratio, R in itertools.product((1200.0, 666.67, 2.0), ROWS):
        got = as_f64(driver("pow", f64(ratio), R)["pow"])
        assert same_bits(got, np.array([_spec_pow(ratio, r / R) for r in range(R + 1)])), (ratio, R)
        assert got[R] == ratio and got[0] == 1.0   # x == 1 returns the ratio itself


def test_default_palette_is_the_bit_model_s(driver):
    assert np.array_equal(bits(driver("palette")["lut"], np.uint8).reshape(256, 4), O.default_lut())


def test_colormap_and_warped_edges_are_the_library_s(driver, warped):
    """emspec_make_colormap and emspec_warped_edges_hz need no device: the library must give what the header gives."""
    try:
        import emspec
        emspec.load()
    except Exception as e:   # (no HIP runtime on this machine, or the library was not built)
        pytest.skip(f"libemspec cannot be loaded here: {e}")
    for b in (0.5, 0.7, 1.0):
        assert np.array_equal(bits(driver("colormap", f32(b))["lut"], np.uint8).reshape(256, 4), emspec.make_colormap(b)), b
    assert same_bits(warped, emspec.warped_edges_hz(*WARPED))
    assert same_bits(as_f32(driver("warped", 512, f32(30.0), f32(20000.0), f32(2.0), f32(1.5))["hz"]),
                     emspec.warped_edges_hz(512, 30.0, 20000.0, 2.0, 1.5))


CONFIGS = (dict(gain=1.0, db_top=0.0, db_range=80.0, gate_db=-80.0, power_floor=1e-14),
           dict(gain=0.5, db_top=-6.0, db_range=60.0, gate_db=-70.0, power_floor=1e-8))


def test_scalars_are_one_rounded_operation_each(driver):
    """Every scalar of the four constant sets, restated as the IEEE operations the header performs (Python floats are binary64,
    numpy float32 scalars are binary32: one rounding per operation), and equal in every bit.  l2e0 and rscale go through the C
    library's float log2 and are hints whose last bit does not decide a row: those two are bounded."""
    for n, cfg, reassign in itertools.product((256, 4096, 16384), CONFIGS, (1, 0)):
        for hop in (1, 256, n):
            rows, sr, lo, hi = 1024, 48000.0, 20.0, 24000.0
            out = driver("scalars", n, hop, reassign, rows, f32(sr), f32(lo), f32(hi), f32(cfg["gain"]), f32(cfg["db_top"]),
                         f32(cfg["db_range"]), f32(cfg["gate_db"]), f32(cfg["power_floor"]))
            case = (n, hop, reassign, cfg["gain"])
            D = (n + 2 * hop - 1) // (2 * hop) if reassign else 0
            assert [int(t) for t in out["ints"].split()] == [rows, 1, D, reassign, hop, D], case
            nn, g = float(n), float(F(cfg["gain"]))
            top, rng = F(cfg["db_top"]), F(cfg["db_range"])
            tscale = nn / 2.0 / float(hop)
            pk = nn / 4.0
            pfloor = float(F(cfg["power_floor"])) * pk * pk
            qscale = math.ldexp(1.0, 52 - (2 * int(math.log2(n)) - 4))
            pmax = math.ldexp(1.0, 61) / qscale
            scale = 32.0 / (3.0 * nn * nn) * g * g
            e = O.edges64(O.make_cfg(n, hop, rows=rows, sample_rate=sr, fmin_hz=lo, fmax_hz=hi))
            want64 = dict(tscale=tscale, pfloor=pfloor, pmax=pmax, qscale=qscale, pfloor64=64.0 * pfloor, pmax64=64.0 * pmax,
                          qscale64=qscale / 64.0, e0=e[0], eR=e[rows])
            for name, want in want64.items():
                assert out[name] == f64(want), (case, name, out[name], f64(want))
            assert math.frexp(qscale)[0] == 0.5   # a power of two: the fixed-point scaling is exact
            assert out["tscale32"] == f32(F(tscale)) and out["pfloor_abs"] == f32(F(pfloor)), case
            assert out["db"].split() == [f32(F(scale)), f32(top - rng), f32(F(1.0 / float(rng))), f32(cfg["gate_db"])], case
            assert out["exact_db"].split() == [f32(F(scale * (1.0 / qscale))), f32(F(float(top) - float(rng))),
                                               f32(F(1.0 / float(rng))), f32(cfg["gate_db"])], case
            l2e0, rscale = float(as_f32(out["l2e0"])[0]), float(as_f32(out["rscale"])[0])
            ref = math.log2(float(F(e[0])))
            assert math.isfinite(l2e0) and math.isfinite(rscale), case
            assert abs(l2e0 - ref) <= float(np.spacing(F(abs(ref)))), (case, l2e0, ref)
            assert abs(rscale * (math.log2(float(F(e[rows]))) - l2e0) - rows) <= 4 * float(np.spacing(F(rows))), (case, rscale)


def test_collapsed_edges_are_reported_not_crashed_on(driver, tmp_path):
    """4096 rows on a strongly warped axis: the low edges collapse in float32.  The header says so as a value (the engine turns it
    into EMSPEC_ERR_INVALID_ARG), in the precision that fails; the binary64 table of the same axis still increases."""
    rows = 4096
    hz = as_f32(driver("warped", rows, f32(20.0), f32(24000.0), f32(3.0), f32(1.0))["hz"])
    path = tmp_path / "collapsed.f32"
    hz.tofile(path)
    out = driver("edges", 4096, rows, f32(48000.0), f32(20.0), f32(24000.0), path)
    e32 = as_f32(out["e32"])
    assert not np.all(np.diff(e32) > 0)
    assert "not strictly increasing in float32" in out["error32"]
    want64 = "-" if np.all(np.diff(as_f64(out["e64"])) > 0) else "row edges are not strictly increasing"
    assert out["error64"] == want64


# ---- the row hint of the FAST kernels: hint_rows_ok (emspec_tables.h) ----------------------------------------------------------

def _hint(driver, n, rows, axis):
    out = driver("hint", n, rows, *map(f32, axis))
    return int(out["ok"]), float(as_f64(out["e0"])[0]), float(as_f64(out["eR"])[0]), out["error32"]


@pytest.fixture(scope="module")
def narrowest(driver):
    """n -> the largest float32 fmin for which 4096 rows up to 24 kHz at 48 kHz keep the hint, by bisection on the predicate."""
    found = {}
    for n in A.PROBE_SIZES:
        lo, hi = F(1000.0), F(23990.0)
        assert _hint(driver, n, A.NARROW_ROWS, (48000.0, lo, 24000.0))[0] == 1 and _hint(driver, n, A.NARROW_ROWS, (48000.0, hi, 24000.0))[0] == 0
        while np.nextafter(lo, F(np.inf)) < hi:
            mid = F(0.5 * (float(lo) + float(hi)))
            if _hint(driver, n, A.NARROW_ROWS, (48000.0, mid, 24000.0))[0]:
                lo = mid
            else:
                hi = mid
        found[n] = (float(lo), float(hi))
    return found


def test_hint_predicate_on_both_sides_of_its_bound(driver, narrowest):
    """The predicate is its formula (restated in axis_cases.hint_value with libm's log2) away from the bound, and monotone up to
    it: the last hinted float32 fmin and its neighbour lie within 1e-6 of the bound on either side."""
    for n, (last, first_not) in narrowest.items():
        for fmin, want in ((last, 1), (first_not, 0)):
            ok, e0, eR, err = _hint(driver, n, A.NARROW_ROWS, (48000.0, fmin, 24000.0))
            v = A.hint_value(e0, eR, A.NARROW_ROWS) / A.HINT_BOUND
            assert ok == want and err == "-" and abs(v - 1.0) < 1e-6 and (v <= 1.0) == bool(want), (n, fmin, v)
        # the axes the GPU probe uses: within 1 % of the bound on the hinted side, and past it
        ok, e0, eR, err = _hint(driver, n, A.NARROW_ROWS, A.NARROW_HINTED[n])
        assert ok == 1 and err == "-" and 0.99 < A.hint_value(e0, eR, A.NARROW_ROWS) / A.HINT_BOUND < 1.0, n
        for axis, rows in A.NARROW_SEARCHED:
            ok, e0, eR, err = _hint(driver, n, rows, axis)
            assert ok == 0 and err == "-" and A.hint_value(e0, eR, rows) > 1.1 * A.HINT_BOUND, (n, axis)   # emspec_create takes it: searched


def test_ordinary_axes_stay_hinted(driver):
    """The default axis, the six axes of tests/axis_cases.py and one octave below Nyquist, at 64 .. 4096 rows and every N: the
    plan's log_rows is 1 as before, with a margin of at least 4 below the bound."""
    axes = [(48000.0, 20.0, 24000.0), (48000.0, 12000.0, 24000.0), *A.AXES.values()]
    for axis in axes:
        for n in (256, 1024, 4096, 16384):
            for rows in (64, 68, 1024, 4092, 4096):
                ok, e0, eR, err = _hint(driver, n, rows, axis)
                assert ok == 1 and err == "-" and A.hint_value(e0, eR, rows) < 0.25 * A.HINT_BOUND, (axis, n, rows)


def test_hint_model_equals_bisection_on_the_narrowest_hinted_axis(driver, narrowest):
    """A numpy float32 model of HintLookup::row_signed_log with the logarithm moved by up to +-4 float32 ulp (the bound budgets
    1 for v_log_f32), on the narrowest hinted axis of each n: every edge, its neighbours at 1 and 2 ulp and the row midpoints
    land in bisection's row.  The same model on the axes past the bound does give wrong rows: the probe can fail."""
    for n, (fmin, _) in narrowest.items():
        eb = as_f32(driver("edges", n, A.NARROW_ROWS, f32(48000.0), f32(fmin), f32(24000.0))["e32"])
        kh = A.probe_values(eb)
        want = A.bisect_rows(eb, kh)
        assert want.min() == -1 and want.max() == A.NARROW_ROWS
        for ulps in range(-4, 5):
            got = A.lookup_model(eb, kh, ulps)
            assert np.array_equal(got, want), (n, fmin, ulps, int(np.sum(got != want)))
    axis, rows = A.NARROW_SEARCHED[0]
    eb = as_f32(driver("edges", 16384, rows, *map(f32, axis))["e32"])
    kh = A.probe_values(eb)
    assert any(not np.array_equal(A.lookup_model(eb, kh, u), A.bisect_rows(eb, kh)) for u in (-1, 0, 1))
