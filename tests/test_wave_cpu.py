"""CPU: the waveform envelope (include/emspec.h: emspec_wave_host, emspec_set_wave_out) without a device - the
host twin against tests/wave_ref.py byte for byte, the peak-hold rule between factors, the refusals, the envelope's part of the
host pipeline's plan (tests/cdriver/wave_plan_driver.cpp over emspec_pipe_plan.h), and the Node binding's waveOf."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec
import wave_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint32


@pytest.fixture(scope="module")
def refs():
    """case -> (signal, reference envelope), computed once"""
    out = {}
    for case in W.CASES:
        x = W.case_signal(case)
        out[case] = (x, W.envelope(x, case[0], case[1], case[3]))
    return out


def test_cases_hold_what_they_plant(refs):
    """Over the case list the references show every planted pattern: an empty window, the two zeros told apart, both
    infinities, a negative denormal as lo - and the reference's key is the total order the definition names."""
    probe = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    k = W.keys(probe.view(U)).astype(np.int64)
    assert np.all(np.diff(k) > 0) and np.array_equal(W.unkeys(W.keys(probe.view(U))), probe.view(U))
    u = np.concatenate([r.view(U).reshape(-1, 2) for _, r in refs.values()])
    lo, hi = u[:, 0], u[:, 1]
    assert ((lo == 0x7F800000) & (hi == 0xFF800000)).any()       # a window of NaN only
    assert ((lo == 0x80000000) & (hi == 0)).any()                # a window of -0.0 and +0.0 only
    assert (hi == 0x7F800000).any() and (lo == 0xFF800000).any() and (lo == 0x80000007).any()
    assert not W.is_nan_bits(u).any()
    assert len(W.CASES) == 18 and all(L % 2 == 1 for n, hop, L, f in W.CASES if (n, hop) not in ((256, 1), (256, 3), (4096, 257)))


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: "n%d-hop%d-L%d-f%d" % c)
def test_wave_host_is_the_reference(refs, case):
    n, hop, L, f = case
    x, want = refs[case]
    got = emspec.wave_host(x, n, hop, f)
    assert W.same(got, want)
    # the boundary plants of stream 0: 2000 + i is the first sample of its window and shows there only
    if f == 1 and want.shape[1] > 2:
        hi = want[0, :, 1]
        assert (hi >= 2000).sum() == len({1, want.shape[1] // 2, want.shape[1] - 1}) and not (np.abs(want[0]) > 1e29).any()


@pytest.mark.parametrize("case", [c for c in W.CASES if c[3] > 1], ids=lambda c: "n%d-hop%d-L%d-f%d" % c)
def test_factor_is_peak_hold_of_the_full_rate_pairs(refs, case):
    n, hop, L, f = case
    x, _ = refs[case]
    assert W.same(emspec.wave_host(x, n, hop, f), W.regroup(emspec.wave_host(x, n, hop, 1), f))


def test_wave_host_refusals():
    lib = emspec.load()
    x = np.zeros((2, 1000), np.float32)
    out = np.full((2, 8, 2), 7.0, np.float32)
    p, o = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(*a):
        rc = lib.emspec_wave_host(*a)
        msg = lib.emspec_last_error(None).decode()
        assert rc == emspec.ERR_INVALID_ARG and msg, (rc, msg)
        return msg

    assert "factor" in refused(p, 2, 1000, 256, 100, 0, o) and "factor" in refused(p, 2, 1000, 256, 100, 65537, o)
    assert "hop" in refused(p, 2, 1000, 256, 0, 1, o) and "hop" in refused(p, 2, 1000, 256, 257, 1, o)
    assert "fft size" in refused(p, 2, 1000, 300, 100, 1, o) and "fft size" in refused(p, 2, 1000, 32768, 100, 1, o)
    assert "streams" in refused(p, -1, 1000, 256, 100, 1, o) and "streams" in refused(p, 65536, 1000, 256, 100, 1, o)
    assert "null" in refused(None, 2, 1000, 256, 100, 1, o) and "null" in refused(p, 2, 1000, 256, 100, 1, None)
    assert "aligned" in refused(C.c_void_p(x.ctypes.data + 2), 1, 998, 256, 100, 1, o)
    assert np.all(out == 7.0)
    # L < n: no column, nothing to write - a no-op even without an output; so is S = 0
    assert lib.emspec_wave_host(p, 2, 255, 256, 100, 1, None) == 0 and lib.emspec_wave_host(None, 0, 1000, 256, 100, 1, None) == 0
    # and the binding raises with the library's message
    with pytest.raises(emspec.EmspecError, match="factor"):
        emspec.wave_host(x, 256, 100, 0)
    # an output that is 4-byte aligned only is served
    raw = np.zeros(2 * 8 * 2 + 1, np.float32)
    assert lib.emspec_wave_host(p, 2, 1000, 256, 100, 1, C.c_void_p(raw.ctypes.data + 4)) == 0
    assert W.same(raw[1:].reshape(2, 8, 2), W.envelope(x, 256, 100, 1))


def test_wave_plan_covers_every_pair_once(tmp_path):
    """The stand-alone driver over the plan header, built with the host compiler under ASan and UBSan (a program of its own:
    nothing is preloaded): for S, V in {1, 4}, L, f and forced unit counts - whole streams and runs of columns - the wave pieces
    of all units cover [0, S V Cr) exactly once and come from inside the unit's pair array; a set without the row keeps its
    layout."""
    exe = str(tmp_path / "wave_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "wave_plan_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr and r.stdout.startswith("ok "), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    cases, units, runs = (int(v) for v in r.stdout.split()[1:4])
    assert cases >= 1000 and units > cases and runs > 0


def test_abi_carries_the_envelope():
    lib = emspec.load()
    header = open(os.path.join(ROOT, "include", "emspec.h")).read()
    for sym in ("emspec_wave_device", "emspec_wave_host", "emspec_set_wave_out"):
        assert hasattr(lib, sym) and sym in emspec.SYMBOLS and sym in header
    assert tuple(emspec.WAVE_SYMBOLS) == ("emspec_wave_device", "emspec_wave_host", "emspec_set_wave_out")
    assert "typedef struct emspec_wave { float lo; float hi; } emspec_wave;" in header and "#define EMSPEC_ABI_VERSION 2" in header


def test_node_wave_of_is_the_reference(refs):
    node = shutil.which("node") or shutil.which("nodejs")
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not node or not os.path.exists(os.path.join(js, "emspec.node")):
        return                                                   # (compared where the addon is built)
    for case in [c for c in W.CASES if c[0] <= 1024]:
        n, hop, L, f = case
        x, want = refs[case]
        code = ("const em = require('./index.js'); const fs = require('fs');"
                "const b = fs.readFileSync(0); const x = new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length));"
                f"const w = em.waveOf(x, {x.shape[0]}, {L}, {n}, {hop}, {f});"
                "process.stdout.write(Buffer.from(w.buffer, w.byteOffset, w.byteLength));")
        r = subprocess.run([node, "-e", code], cwd=js, input=x.tobytes(), capture_output=True, check=True, timeout=60)
        got = np.frombuffer(r.stdout, np.float32).reshape(want.shape)
        assert W.same(got, want), case
