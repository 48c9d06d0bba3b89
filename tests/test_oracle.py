"""CPU: the oracle itself.  Pins the C oracle (float64 textbook method and float32 bit model)
against (i) the committed golden fixtures made by the independent numpy formulation,
(ii) that formulation run live, (iii) analytic known-answer tests.
The reference's own outputs are not available (private source): parity is UNPINNED with
respect to the reference, and these tests say so by construction."""
import glob
import os

import numpy as np
import pytest

import oracle as O
import ref_numpy as RN
from emspec import synth

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
FS = 48000.0


def test_golden_files_present():
    assert len(GOLD) >= 4


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_f64_oracle_matches_golden(path):
    g = np.load(path)
    n, hop, f0, fr, re = int(g["n"]), int(g["hop"]), int(g["frame0"]), int(g["frames"]), bool(g["reassign"])
    cfg = O.make_cfg(n, hop, re)
    p, that, khat, col, row = O.frames_f64(cfg, g["pcm"], f0, fr)
    assert np.allclose(p, g["power"], rtol=1e-9, atol=1e-18)
    assert np.max(np.abs(that - g["that"])) < 1e-4
    assert np.max(np.abs(khat - g["khat"])) < 1e-6
    assert np.mean(col != g["col"]) < 1e-4 and np.mean(row != g["row"]) < 1e-4


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_f32_bit_model_matches_golden(path):
    """The float32 bit model (what the kernels compute) against the float64 vectors:
    power within 1e-4 for bins within 60 dB of the frame maximum, indices equal except
    for rare bins that sit on a cell edge."""
    g = np.load(path)
    n, hop, f0, fr, re = int(g["n"]), int(g["hop"]), int(g["frame0"]), int(g["frames"]), bool(g["reassign"])
    cfg = O.make_cfg(n, hop, re)
    p, col, row = O.frames_f32(cfg, g["pcm"], f0, fr)
    strong = g["power"] >= g["power"].max(axis=1, keepdims=True) * 1e-6
    rel = np.abs(p - g["power"]) / np.maximum(g["power"], 1e-300)
    assert rel[strong].max() < 1e-4
    valid = g["row"] >= 0
    assert np.mean(row[valid] != g["row"][valid]) < 2e-3
    assert np.mean(col[valid] != g["col"][valid]) < 2e-3


@pytest.mark.parametrize("n,hop", [(256, 64), (1024, 256), (2048, 512), (4096, 256), (8192, 1024)])
def test_f64_oracle_matches_numpy_live(n, hop):
    pcm = synth.stream(40 + n % 7, n + hop * 9)
    cfg = O.make_cfg(n, hop, True)
    p, that, khat, col, row = O.frames_f64(cfg, pcm, 2, 5)
    r = RN.reassign_frames(pcm, n, hop, 2, 5)
    assert np.allclose(p, r["power"], rtol=1e-9, atol=1e-18)
    assert np.max(np.abs(khat - r["khat"])) < 1e-6
    assert np.mean(row != r["row"]) < 1e-4


def test_kat_stationary_sine():
    n, hop = 4096, 256
    t = np.arange(n + hop * 4)
    x = np.cos(2 * np.pi * 1234.567 * t / FS + 0.3).astype(np.float32)
    cfg = O.make_cfg(n, hop, True)
    p, that, khat, col, row = O.frames_f64(cfg, x, 0, 2)
    kp = int(round(1234.567 * n / FS))
    assert np.max(np.abs(khat[:, kp - 2:kp + 3] * FS / n - 1234.567)) < 5e-3     # f-hat at the true frequency
    assert np.max(np.abs(that[0, kp - 2:kp + 3] - n / 2)) < 1e-3                 # t-hat at the frame centre
    tw, eb = O.tables(cfg)
    expect_row = np.searchsorted(eb, np.float32(1234.567 * n / FS), side="right") - 1
    p32, c32, r32 = O.frames_f32(cfg, x, 0, 2)
    assert np.all(r32[:, kp - 2:kp + 3] == expect_row) and np.all(c32[0, kp - 2:kp + 3] == 0)


def test_kat_impulse():
    n, hop = 4096, 256
    x = np.zeros(n + hop * 4, np.float32)
    x[2500] = 1.0
    cfg = O.make_cfg(n, hop, True, power_floor=0.0)
    p, that, khat, col, row = O.frames_f64(cfg, x, 0, 1)
    assert np.max(np.abs(that - 2500.0)) < 1e-6
    expect = int(np.floor((2500 - n / 2) / hop + 0.5))
    assert col.min() == col.max() == expect
    p32, c32, r32 = O.frames_f32(cfg, x, 0, 1)
    assert c32.min() == c32.max() == expect


def test_kat_linear_chirp():
    n, hop = 4096, 256
    t = np.arange(n + hop) / FS
    f0, rate = 2000.0, 4.0e4
    x = np.sin(2 * np.pi * (f0 * t + 0.5 * rate * t * t)).astype(np.float32)
    cfg = O.make_cfg(n, hop, True)
    p, that, khat, col, row = O.frames_f64(cfg, x, 0, 1)
    strong = p[0] > p[0].max() * 1e-3
    fhat = khat[0][strong] * FS / n
    line = f0 + rate * that[0][strong] / FS
    assert np.max(np.abs(fhat - line)) < 0.05      # (t-hat, f-hat) lies on the chirp's line


def test_packed_fft_identity():
    """x + j*ramp*x in one complex FFT == two real FFTs; spectral Hann identity == time-domain Hann."""
    n = 1024
    rng = np.random.default_rng(5)
    x = rng.standard_normal(n)
    i = np.arange(n)
    ramp = (i - n / 2) / (n / 2)
    Z = np.fft.fft(x + 1j * ramp * x)
    Zm = np.conj(np.roll(Z[::-1], 1))
    Y = (Z + Zm) / 2
    T = (Z - Zm) / 2j
    assert np.allclose(Y, np.fft.fft(x), atol=1e-9) and np.allclose(T, np.fft.fft(ramp * x), atol=1e-9)
    h = 0.5 - 0.5 * np.cos(2 * np.pi * i / n)
    Xh = 0.5 * Y - 0.25 * (np.roll(Y, 1) + np.roll(Y, -1))
    assert np.allclose(Xh, np.fft.fft(x * h), atol=1e-9)
    Xdh = (np.pi / n) * (np.roll(Y, 1) - np.roll(Y, -1)) / 2j
    assert np.allclose(Xdh, np.fft.fft(x * (np.pi / n) * np.sin(2 * np.pi * i / n)), atol=1e-9)


def test_tables_and_lut():
    cfg = O.make_cfg(4096, 256, True)
    tw, eb = O.tables(cfg)
    assert np.all(np.diff(eb) > 0) and eb.size == 1025
    assert np.isclose(eb[0], 20.0 * 4096 / FS) and np.isclose(eb[-1], 2048.0)
    assert tw[0] == 1.0 and tw[2 * 1024] == 0.0 and tw[2 * 1024 + 1] == -1.0
    lut = O.default_lut()
    assert tuple(lut[0]) == (0, 0, 0, 255) and tuple(lut[255]) == (255, 255, 200, 255)
    assert tuple(lut[64][:3]) == (80, 0, 80) or abs(int(lut[64][0]) - 80) <= 1


@pytest.mark.parametrize("n", [256, 1024, 4096, 16384])
def test_twiddle_table_is_what_libm_gives_and_quarter_turn_symmetric(n):
    """tw[q] = (cos, -sin)(2 pi q / N) evaluated in double and rounded once; the second quarter is
    written by symmetry (tw[q + N/4] = (tw[q].im, -tw[q].re)), which must be an identity on the libm values so that the
    golden vectors and every earlier result stay bit-identical."""
    tw, _ = O.tables(O.make_cfg(n, 64, True))
    q = np.arange(n // 2)
    a = 2.0 * np.pi * q.astype(np.float64) / n
    direct = np.stack([np.cos(a), -np.sin(a)], axis=1).astype(np.float32)
    direct[n // 4] = (0.0, -1.0)
    assert np.array_equal(tw.reshape(-1, 2), direct)
    c, s = tw[0::2], tw[1::2]
    assert np.array_equal(c[n // 4:], s[:n // 4]) and np.array_equal(s[n // 4 + 1:], -c[1:n // 4])
    # the kernels' last pass carries these two entries as literals (emspec_device.h fft_stages, kC8)
    c8 = np.float32(0.70710677)
    assert c8.view(np.uint32) == 0x3F3504F3
    assert (c[n // 8], s[n // 8]) == (c8, -c8) and (c[3 * n // 8], s[3 * n // 8]) == (-c8, -c8)


@pytest.mark.parametrize("n,hop,reassign", [(4096, 256, True), (1024, 256, False), (16384, 512, True), (2048, 128, True),
                                            (8192, 1024, True)])
def test_cpu_fast_port_agrees_with_bit_model(n, hop, reassign):
    """bench.py's cpu_baseline port (emspec_cpu_fast.c: Stockham radix-4 FFT, ring histogram, polynomial log2) runs the
    same pipeline as the bit model.  It is not bit-identical (other butterfly grouping), so a bin whose coordinate sits on
    a cell edge may land next door (rare), and cells near the display floor carry either FFT's rounding noise."""
    frames = 60
    pcm = synth.streams(2, n + hop * (frames - 1) + 13)
    cfg = O.make_cfg(n, hop, reassign)
    odb, _, oidx = O.batch_f32(cfg, pcm, want=("db", "index"))
    fdb, fidx = O.fast_batch(cfg, pcm, threads=2)
    d = np.abs(fdb - odb)
    strong = odb > -60.0          # 20 dB above the display floor: float32 rounding of either FFT is far below these cells
    shown = odb > -80.0           # the displayed range (gate = -80 dB); a bin on a cell edge may land next door
    assert np.percentile(d[strong], 99) < 1e-4 and np.mean(d[strong] > 1e-3) < 5e-3
    assert np.mean(d[shown] > 1e-3) < 1e-2
    assert np.mean(fidx != oidx) < 1e-3


def test_batch_pipeline_consistency():
    """eo_batch_f32 == scatter of eo_frames_f32 + dB map, including edge drops and empty cells."""
    n, hop, frames = 1024, 256, 20
    pcm = synth.streams(2, n + hop * (frames - 1))
    cfg = O.make_cfg(n, hop, True)
    db, rgba, idx = O.batch_f32(cfg, pcm)
    hist = O.hist_f32(cfg, pcm)
    for s in range(2):
        p, col, row = O.frames_f32(cfg, pcm[s], 0, frames)
        h = np.zeros((frames, 1024), np.float64)
        ok = (row >= 0) & (col >= 0) & (col < frames)
        np.add.at(h, (col[ok], row[ok]), p[ok].astype(np.float64))
        assert np.allclose(hist[s], h, rtol=1e-5, atol=1e-12)
    scale = 32.0 / (3.0 * n * n)
    assert np.allclose(db, 10 * np.log10(hist.astype(np.float64) * scale + 1e-20), atol=1e-3)
    assert db.min() == pytest.approx(-200.0, abs=1e-3)
    assert np.array_equal(rgba, O.default_lut()[idx])


def test_ragged_and_degenerate_inputs():
    n, hop = 1024, 256
    cfg = O.make_cfg(n, hop, True)
    z = np.zeros((1, n + hop * 3), np.float32)           # silence: everything gated, empty columns
    db, _, idx = O.batch_f32(cfg, z)
    assert np.all(db == db.flat[0]) and np.all(idx == 0)
    one = synth.streams(1, n)                             # exactly one frame
    db1, _, _ = O.batch_f32(cfg, one)
    assert db1.shape == (1, 1, 1024)
    assert O.num_columns(n - 1, n, hop) == 0


@pytest.mark.skipif(__import__("shutil").which("node") is None, reason="node not installed")
@pytest.mark.parametrize("path", GOLD[:3], ids=[os.path.basename(p)[:-4] for p in GOLD[:3]])
def test_plain_js_restatement_matches_golden(path, tmp_path):
    """A third independent implementation (ordinary JS under node, oracle/js/reassign_ref.js)
    reproduces the golden vectors: the closest stand-in for a 'JS CPU path' that can exist here."""
    import subprocess
    g = np.load(path)
    n, hop, f0, fr, re = int(g["n"]), int(g["hop"]), int(g["frame0"]), int(g["frames"]), bool(g["reassign"])
    pcm_file = tmp_path / "pcm.f32"
    g["pcm"].astype(np.float32).tofile(pcm_file)
    js = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "js", "reassign_ref.js")
    subprocess.check_call(["node", js, "check", str(pcm_file), str(n), str(hop), str(f0), str(fr), str(int(re)), str(tmp_path / "o")])
    K = n // 2 + 1
    p = np.fromfile(tmp_path / "o.power", np.float64).reshape(fr, K)
    khat = np.fromfile(tmp_path / "o.khat", np.float64).reshape(fr, K)
    row = np.fromfile(tmp_path / "o.row", np.int32).reshape(fr, K)
    col = np.fromfile(tmp_path / "o.col", np.int32).reshape(fr, K)
    assert np.allclose(p, g["power"], rtol=1e-8, atol=1e-16)
    assert np.max(np.abs(khat - g["khat"])) < 1e-5
    assert np.mean(row != g["row"]) < 1e-4 and np.mean(col != g["col"]) < 1e-4


def test_js_synthetic_generator_matches_python():
    """the synthetic input is a counter-based generator defined once and implemented in Python
    (emspec/synth.py) and JavaScript (js/synth.js); both must produce the same stream."""
    import json, shutil, subprocess, sys
    node = shutil.which("node") or shutil.which("nodejs")
    if not node:
        pytest.skip("no node")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "em-spec_amd"))
    from emspec import synth
    for s, L in ((0, 30000), (41, 5000)):
        out = subprocess.run([node, os.path.join(root, "em-spec_amd", "js", "synth.js"), str(s), str(L)],
                             capture_output=True, text=True, check=True, timeout=120).stdout
        js = np.array(json.loads(out), np.float32)
        py = synth.stream(s, L)
        assert js.shape == py.shape
        assert np.max(np.abs(js - py)) <= 1.2e-7      # sin/log may differ in the last double bit between libms
        assert np.mean(js != py) < 1e-3


# ---- EXACT mode bit model (oracle/emspec_exact.c) ----------------------------------------------

@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_exact_model_matches_golden(path):
    """The binary64 bit model against the numpy float64 goldens: EVERY (column,row) equal (the float32 model is allowed
    2e-3 of mismatches above), power to 1e-9."""
    g = np.load(path)
    n, hop, f0, fr, re = int(g["n"]), int(g["hop"]), int(g["frame0"]), int(g["frames"]), bool(g["reassign"])
    p, col, row, q = O.frames_exact(O.make_cfg(n, hop, re), g["pcm"], f0, fr)
    valid = g["row"] >= 0
    assert np.array_equal(row >= 0, valid)
    assert np.array_equal(row[valid], g["row"][valid]) and np.array_equal(col[valid], g["col"][valid])
    strong = g["power"] >= g["power"].max(axis=1, keepdims=True) * 1e-12
    assert (np.abs(p - g["power"]) / np.maximum(g["power"], 1e-300))[strong].max() < 1e-9
    assert np.all(q[~valid] == 0) and np.all(q[valid] > 0)


@pytest.mark.parametrize("n,hop,frames", [(256, 64, 200), (1024, 256, 120), (2048, 128, 100), (4096, 256, 80), (8192, 512, 30),
                                          (16384, 512, 16)])
def test_exact_model_indices_equal_float64_method(n, hop, frames):
    """Against the independent float64 three-window method (explicitly windowed FFTs; shares no code): the mismatch
    rate of the integer (column,row) is asserted <= 1e-6 (north_star: 'exactly on reassigned integer (time,freq) bin
    indices'); measured 0 on ~1.6 M bins."""
    bad = tot = 0
    for seed in (3, 4):
        pcm = synth.stream(seed, n + hop * (frames - 1))
        cfg = O.make_cfg(n, hop, True)
        _, col, row, _ = O.frames_exact(cfg, pcm, 0, frames)
        _, _, _, c64, r64 = O.frames_f64(cfg, pcm, 0, frames)
        bad += int(np.sum(col != c64) + np.sum(row != r64))
        tot += 2 * col.size
    assert bad <= 1e-6 * tot, (bad, tot)


def test_exact_db_polynomial():
    """The specified binary32 10 log10 evaluation (no libm; round 5: binary32 instead of binary64 - the outputs are a float32
    dB and a palette byte) against numpy over the whole range a cell can take: within 3e-5 dB, i.e. a few binary32 ulp of the
    result; known answers pin the bits."""
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.exp(rng.uniform(np.log(1e-20), np.log(1e6), 20000)), [1e-20, 1.0, 2.0, 0.5, 1.4142135623730951]]).astype(np.float32)
    err = max(abs(O.exact_db(float(x)) - 10.0 * np.log10(np.float64(x))) for x in xs)
    assert err < 3e-5, err
    assert O.exact_db(1.0) == 0.0 and O.exact_db(2.0) == float(np.float32(3.01029992)) and O.exact_db(0.5) == -float(np.float32(3.01029992))
    kat = {1e-20: None, 3.0: None, 1234.5: None}
    for x in kat:
        d = O.exact_db(x)
        assert d == float(np.float32(d))                 # a binary32 value
    # the evaluation restated in numpy float32 (each fmaf = one rounding of the exact product-sum, which binary64 holds):
    # mantissa folded into (sqrt 1/2, sqrt 2], f = m - 1, log2 m = f P(f), degree 8 - no division (round 5, last form)
    coef = [0.123109683, -0.205861881, 0.216078222, -0.239169881, 0.287903249, -0.360693276, 0.480910748, -0.721347451, 1.44269502]
    x32 = xs[:4000]
    u = x32.view(np.uint32)
    e = ((u >> 23) & 0xff).astype(np.int32) - 127
    m = ((u & 0x007fffff) | 0x3f800000).view(np.float32)
    big = m > np.float32(1.41421354)
    m = np.where(big, m * np.float32(0.5), m).astype(np.float32)
    e = e + big
    f = (m - np.float32(1.0)).astype(np.float32)
    p = np.full_like(f, np.float32(coef[0]))
    for c in coef[1:]:
        p = (p.astype(np.float64) * f.astype(np.float64) + np.float64(np.float32(c))).astype(np.float32)
    l2 = (f * p).astype(np.float32)
    want = ((e.astype(np.float32) + l2).astype(np.float32) * np.float32(3.01029992)).astype(np.float32)
    got = np.array([O.exact_db(float(v)) for v in x32], np.float32)
    assert np.array_equal(got, want)
    l2err = np.max(np.abs(l2.astype(np.float64) - np.log2(m.astype(np.float64))))
    assert l2err < 6.5e-8, l2err


def test_exact_sum32_is_two_conversions_and_one_fma():
    """The int64 cell sum enters the dB stage as fmaf((float)hi32, 2^32, (float)lo32): within 1.5 binary32 ulp of the sum,
    exact below 2^24, and the same bits as the numpy restatement."""
    rng = np.random.default_rng(3)
    vals = np.concatenate([rng.integers(0, 1 << 62, 3000), rng.integers(0, 1 << 33, 2000), [0, 1, (1 << 24) - 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1]])
    for v in vals:
        v = int(v)
        hi, lo = np.float32(v >> 32), np.float32(v & 0xffffffff)
        want = np.float32(np.float64(hi) * 4294967296.0 + np.float64(lo))    # exact in binary64, one rounding to binary32
        got = O.exact_sum32(v)
        assert got == float(want), v
        assert abs(got - v) <= 1.5 * 2.0 ** -23 * max(v, 1)
        if v < (1 << 24):
            assert got == float(v)


def test_exact_batch_is_order_independent_fixed_point():
    """eo_batch_exact's int64 histogram equals a numpy scatter of the per-bin fixed-point energies done in REVERSED order
    (integer adds commute), and its dB / index follow from those sums alone."""
    n, hop, frames = 1024, 256, 60
    pcm = synth.streams(2, n + hop * (frames - 1))
    cfg = O.make_cfg(n, hop, True)
    db, rgba, idx, hist = O.batch_exact(cfg, pcm, want=("db", "rgba", "index", "hist"))
    for s in range(2):
        _, col, row, q = O.frames_exact(cfg, pcm[s], 0, frames)
        ok = (row >= 0) & (col >= 0) & (col < frames)
        h = np.zeros((frames, cfg.rows), np.int64)
        np.add.at(h, (col[ok][::-1], row[ok][::-1]), q[ok][::-1])
        assert np.array_equal(h, hist[s])
    scale = 32.0 / (3.0 * n * n)
    ref = 10.0 * np.log10(hist.astype(np.float64) * 2.0 ** -(52 - (2 * 10 - 4)) * scale + 1e-20)
    assert np.max(np.abs(db - ref)) < 2e-5          # float32 output format
    assert np.array_equal(rgba, O.default_lut()[idx])
    # and the exact model agrees with the float32 bit model to the float32 model's accuracy
    db32, _, _ = O.batch_f32(cfg, pcm, want=("db",))
    loud = ref > -60.0
    assert np.mean(np.abs(db32 - db)[loud] < 1e-2) > 0.99


@pytest.mark.parametrize("n,hop", [(1024, 256), (4096, 256), (16384, 512)])
def test_power_against_scipy_stft(n, hop):
    """An EXTERNAL implementation for the rows 'Frame gather', 'Windows', 'STFT', 'Power' of SURVEY.md §8(a): scipy.signal.stft
    (periodic Hann, no padding) against |X_h|^2 of the float64 method, the binary64 bit model and - within float32 accuracy -
    the float32 bit model.  (scipy has no reassignment; (t-hat, f-hat) stay pinned by the numpy formulation and the KATs.)"""
    ss = pytest.importorskip("scipy.signal")
    frames = 10
    pcm = synth.stream(5, n + hop * (frames - 1))
    w = ss.get_window("hann", n, fftbins=True)
    _, _, Z = ss.stft(pcm.astype(np.float64), fs=FS, window=w, nperseg=n, noverlap=n - hop, boundary=None, padded=False,
                      return_onesided=True, scaling="spectrum")
    ref = ((np.abs(Z) * w.sum()) ** 2).T                      # [frames][K]
    cfg = O.make_cfg(n, hop, True)
    p64 = O.frames_f64(cfg, pcm, 0, frames)[0]
    pex = O.frames_exact(cfg, pcm, 0, frames)[0]
    p32 = O.frames_f32(cfg, pcm, 0, frames)[0]
    strong = ref >= ref.max(axis=1, keepdims=True) * 1e-12
    assert (np.abs(p64 - ref) / np.maximum(ref, 1e-300))[strong].max() < 1e-9
    assert (np.abs(pex - ref) / np.maximum(ref, 1e-300))[strong].max() < 1e-9
    strong32 = ref >= ref.max(axis=1, keepdims=True) * 1e-6
    assert (np.abs(p32 - ref) / np.maximum(ref, 1e-300))[strong32].max() < 1e-4


def test_reassignment_equals_phase_derivatives():
    """north_star names the method by its definition: 'per-bin phase-derivative reassignment of energy to (t-hat, f-hat)'.
    The three-window formulas the oracle (and the kernels) evaluate are the closed form of those derivatives; this test
    evaluates the DEFINITION numerically - f-hat = (1/2pi) d(phase)/dt by a central difference of the Hann STFT over +-1
    sample, t-hat = -d(phase)/d(omega) by a central difference on a 256x zero-padded frequency grid - and compares, using
    nothing but numpy FFTs of Hann-windowed frames.  Signal: two sinusoids, a chirp and two clicks."""
    n, hop, j = 4096, 256, 4
    L = n + hop * 8 + 4
    t = np.arange(L) / FS
    x = 0.6 * np.cos(2 * np.pi * 1234.567 * t + 0.3) + 0.3 * np.cos(2 * np.pi * (3000 * t + 0.5 * 2.0e4 * t * t)) + \
        0.2 * np.cos(2 * np.pi * 9876.5 * t)
    x[3000] += 0.8
    x[2100] += 0.5
    x = x.astype(np.float32)
    p = j * hop
    h = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    cfg = O.make_cfg(n, hop, True)
    p64, that, khat, c64, r64 = O.frames_f64(cfg, x, j, 1)
    strong = p64[0] > p64[0].max() * 1e-4
    k = np.arange(n // 2 + 1)
    # instantaneous frequency: phase advance per sample at a fixed bin, unwrapped around the bin's own frequency
    Xm = np.fft.rfft(x[p - 1:p - 1 + n].astype(np.float64) * h)
    Xp = np.fft.rfft(x[p + 1:p + 1 + n].astype(np.float64) * h)
    dphi = np.angle(Xp * np.conj(Xm) * np.exp(-1j * 4 * np.pi * k / n)) / 2 + 2 * np.pi * k / n
    assert np.max(np.abs(khat[0] - dphi * n / (2 * np.pi))[strong]) < 1e-4          # bins (measured 2e-5)
    # group delay: -d(phase)/d(omega) on a fine grid, time origin at the frame centre
    Z = 256
    Xf = np.fft.rfft(x[p:p + n].astype(np.float64) * h, Z * n)
    Xr = Xf * np.exp(1j * np.pi * np.arange(Xf.size) / Z)
    kk = np.arange(1, n // 2)
    d = np.angle(Xr[Z * kk + 1] * np.conj(Xr[Z * kk - 1])) / 2
    t_fd = p + n / 2 - d * (Z * n) / (2 * np.pi)
    err = np.abs(that[0][1:n // 2] - t_fd)[strong[1:n // 2]]
    assert err.max() < 0.5 and np.median(err) < 1e-3, (err.max(), np.median(err))   # samples (measured 0.13 / 7e-5; O(1/Z^2))
    # and the exact mode's integer indices are the float64 method's on this frame
    _, col, row, _ = O.frames_exact(cfg, x, j, 1)
    assert np.array_equal(col, c64) and np.array_equal(row, r64)


def test_row_edges_come_from_a_specified_evaluation():
    """The log-spaced row edges are fmin * ratio^(r/R) with ratio^x evaluated by eo_spec_pow - plain IEEE operations in a
    fixed order (atanh-series log2, Taylor exp2), no libm pow, so the table does not depend on the host's C library
    (ADVICE r03 / VERDICT r04 item 9; the library builds its tables with the same operations, emspec_tables.h:spec_pow,
    and tests/test_gpu_parity.py compares the two tables bit for bit on the GPU box).  Known answers pin the bits; the
    value stays within a few ulp of the real power."""
    import ctypes as C
    import math
    lib = O.lib()
    lib.eo_spec_pow.restype = C.c_double
    lib.eo_spec_pow.argtypes = [C.c_double, C.c_double]
    kat = {(1200.0, 0.5): "0x1.1520cd1372febp+5", (1200.0, 1 / 1024): "0x1.01c756e6f3f26p+0",
           (1200.0, 777 / 1024): "0x1.b1fd445e89ca8p+7", (1000.0, 1.0): "0x1.f400000000000p+9",
           (2.0, 0.25): "0x1.306fe0a31b715p+0", (999.5, 1023 / 1024): "0x1.f063edc702c02p+9"}
    for (ratio, x), want in kat.items():
        assert lib.eo_spec_pow(ratio, x) == float.fromhex(want), (ratio, x)
    rng = np.random.default_rng(3)
    for ratio, x in zip(10.0 ** rng.uniform(0.01, 4.0, 20000), rng.uniform(0.0, 1.0, 20000)):
        got, ref = lib.eo_spec_pow(float(ratio), float(x)), math.pow(float(ratio), float(x))
        assert abs(got - ref) <= 16 * math.ulp(ref)
    assert lib.eo_spec_pow(1200.0, 0.0) == 1.0
    e = O.edges64(O.make_cfg(4096, 256, True))
    assert np.all(np.diff(e) > 0) and e[0] == 20.0 * 4096 / FS


def test_exact_palette_bytes_vs_a_binary64_db_stage():
    """the EXACT mode's dB + colour stage is a specified binary32 evaluation of the int64 cell sums.
    Held here against an independent binary64 one (numpy log10 of the same sums, the same map in float64): dB within 3e-5,
    and the share of cells whose PALETTE BYTE differs - a cell whose 255 v sits within ~1e-5 of a half - stays below 1e-3
    (measured: a few 1e-5)."""
    n, hop = 4096, 256
    pcm = synth.streams(3, n + hop * 99)
    cfg = O.make_cfg(n, hop, True)
    db, _, idx, hist = O.batch_exact(cfg, pcm, want=("db", "index", "hist"))
    scale = 32.0 / (3.0 * n * n) * float(cfg.gain) ** 2
    qscale = 2.0 ** 52 / (n / 4.0) ** 2
    d64 = 10.0 * np.log10(hist.astype(np.float64) * (scale / qscale) + 1e-20)
    assert np.max(np.abs(db.astype(np.float64) - d64)) < 3e-5
    lo, rng_ = float(cfg.db_top) - float(cfg.db_range), float(cfg.db_range)
    v = np.clip((d64 - lo) / rng_, 0.0, 1.0)
    v[d64 < float(cfg.gate_db)] = 0.0
    i64 = np.floor(v * 255.0 + 0.5).astype(np.int32)
    diff = i64 != idx.astype(np.int32)
    assert np.max(np.abs(i64 - idx.astype(np.int32))) <= 1
    share = float(np.mean(diff))
    print(f"palette bytes that differ from a binary64 dB stage: {share:.2e} of {diff.size} cells")
    assert share < 1e-3, share
