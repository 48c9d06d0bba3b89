"""The N = 4096 product kernel (fused4096_pp_kernel, hop 256 / 512 / 1024) issues the stores of its FFT passes B, C and D pair
by pair behind the butterflies that produce them (f8::pass8_store_as_you_go); the form that stores after the whole pass is
kept in libemspec_diag.so as A/B variant `pp4`.  Only the order of independent instructions differs, so

 - the product kernel must still match the oracle (dB within 8.7e-4, palette index within one step: the comparison and the
   tolerances of tests/test_gpu_golden.py and test_fused_segments_match_oracle), and
 - it must agree with the kept variant on the same input as every A/B variant had to (the bounds of the retired
   test_fused_ab_variants_match_the_product, docs/HISTORY.md "Retired kernel forms":
   live dB within 1e-3 - the float32 histogram sums in arrival order -, index within one step on at most 1e-3 of the cells),
   with a clean emspec_device_status.

Shapes: the smallest at which the schedule can go wrong.  S = 3 streams; C = 2D + 5 columns, shorter than the ring (2D + 2
slots) plus the pipeline fill, so every frame is a first, a last or a ring-wrapping one; C = 131, odd, which the shared-device
plan cuts into segments (the plan of a GPU shared with a collective, EMSPEC_SHARED=1 in the diagnostic build).  For hop 256
also one stream whose samples end inside the frame after the last one (the kernel prefetches that frame: zero fill), and a
stream of zeros (no bin passes the power floor: every column is the floor).  Both reassign settings (off: D = 0, C = 5).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import emspec
import oracle as O
from palette import palette_close
from emspec import synth

pytestmark = pytest.mark.gpu

N = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    out = []
    for hop in (256, 512, 1024):
        for reassign in (True, False):
            out.append((f"h{hop}_{'re' if reassign else 'off'}_2Dplus5", hop, reassign, "short"))
            out.append((f"h{hop}_{'re' if reassign else 'off'}_c131", hop, reassign, "c131"))
    for reassign in (True, False):
        out.append((f"h256_{'re' if reassign else 'off'}_tail", 256, reassign, "tail"))
        out.append((f"h256_{'re' if reassign else 'off'}_zeros", 256, reassign, "zeros"))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]
_inputs = {}


def _input(case):
    """The case's samples [S][L] (deterministic, made once)."""
    name, hop, reassign, kind = case
    if name not in _inputs:
        D = emspec.latency_columns(N, hop, reassign)
        if kind == "short":
            pcm = synth.streams(3, N + hop * (2 * D + 5 - 1))
        elif kind == "c131":
            pcm = synth.streams(3, N + hop * 130)
        elif kind == "tail":     # 2D + 6 columns; the samples end 100 short of one more frame
            pcm = synth.streams(1, N + hop * (2 * D + 6) - 100)
        else:
            pcm = np.zeros((1, N + hop * (2 * D + 5 - 1)), np.float32)
        _inputs[name] = np.ascontiguousarray(pcm, np.float32)
    return _inputs[name]


def _columns(case):
    return emspec.num_columns(_input(case).shape[1], N, case[1])


def test_shapes_are_what_the_docstring_says():
    for case in CASES:
        name, hop, reassign, kind = case
        D = emspec.latency_columns(N, hop, reassign)
        want = {"short": 2 * D + 5, "c131": 131, "tail": 2 * D + 6, "zeros": 2 * D + 5}[kind]
        assert _columns(case) == want, name
        if kind == "tail":
            L = _input(case).shape[1]
            assert (want - 1) * hop + N < L < want * hop + N


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_matches_oracle(case, engine, monkeypatch):
    name, hop, reassign, kind = case
    pcm = _input(case)
    assert engine.fused(N, hop, reassign)
    if kind == "c131":       # the shared-device plan: a switch of the diagnostic build (same kernel sources)
        monkeypatch.setenv("EMSPEC_SHARED", "1")
        eng = emspec.Engine(diag=True)
    else:
        eng = engine
    try:
        out = eng.batch(pcm, N, hop, reassign, want=("db", "index"))
        eng.device_status()
    finally:
        if eng is not engine:
            eng.close()
    odb, _, oidx = O.batch_f32(O.make_cfg(N, hop, reassign), pcm, want=("db", "index"))
    assert out["db"].shape == odb.shape == (pcm.shape[0], _columns(case), 1024)
    err = float(np.max(np.abs(out["db"] - odb)))
    print(f"MEASURED {name}: max |dB - oracle| {err:.2e}")
    assert err < 8.7e-4
    palette_close(out["index"], oidx)
    if kind == "zeros":
        assert np.all(out["db"] == out["db"].flat[0]) and np.all(out["index"] == out["index"].flat[0])


_OLD_CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "em-spec_amd")]
import emspec
inp = np.load(sys.argv[1])
res = {}
with emspec.Engine(diag=True) as e:
    for key in inp.files:
        name, hop, reassign = key.rsplit("|", 2)
        out = e.batch(inp[key], 4096, int(hop), bool(int(reassign)), want=("db", "index"))
        e.device_status()
        res[name + "|db"], res[name + "|index"] = out["db"], out["index"]
np.savez(sys.argv[2], **res)
"""


@pytest.fixture(scope="module")
def old_variant(tmp_path_factory):
    """Every case through the kept old kernel body: one child process (the variant switch is read once per process)."""
    d = tmp_path_factory.mktemp("pp4")
    fin, fout = str(d / "in.npz"), str(d / "out.npz")
    np.savez(fin, **{f"{c[0]}|{c[1]}|{int(c[2])}": _input(c) for c in CASES})
    r = subprocess.run([sys.executable, "-c", _OLD_CHILD % dict(root=ROOT), fin, fout],
                       env=dict(os.environ, EMSPEC_FUSED_VARIANT="pp4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(fout)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_matches_kept_old_variant(case, engine, old_variant):
    name, hop, reassign, kind = case
    new = engine.batch(_input(case), N, hop, reassign, want=("db", "index"))
    engine.device_status()
    odb, oidx = old_variant[name + "|db"], old_variant[name + "|index"]
    assert new["db"].shape == odb.shape
    live = new["db"] > -100
    err = float(np.max(np.abs(new["db"][live] - odb[live]))) if live.any() else 0.0
    diff = new["index"].astype(np.int16) - oidx.astype(np.int16)
    print(f"MEASURED {name}: max |dB new - old| {err:.2e}, {np.count_nonzero(diff)} of {diff.size} palette indices differ")
    assert err < 1e-3
    assert np.max(np.abs(diff)) <= 1
    assert np.count_nonzero(diff) <= 1e-3 * diff.size
