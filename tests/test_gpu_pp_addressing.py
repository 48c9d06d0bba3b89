"""The N = 4096 product kernel (fused4096_pp_kernel, hop 256 / 512 / 1024) keeps its column bookkeeping in 32 bits relative
to the segment's first frame: the half-iteration index against per-segment int limits, the sample prefetch as a row pointer
with a remaining-samples count, the finalize's output offset carried from pair to pair.  (The same work also formed the LDS
addresses of pass D, of the pass-A write and of the twelve spectrum reads from hoisted bases and constants; that measured
slower and is kept as tools/experiments/pp_lds_address_bases.patch - docs/HISTORY.md section 22.)  None of that is arithmetic, so

 - the product kernel must still match the oracle (dB within 8.7e-4, palette index within one step: the comparison and the
   tolerances of tests/test_gpu_golden.py), and
 - it must agree with the kept old body (variant `pp4` of libemspec_diag.so, which keeps the old addressing and the 64-bit
   bookkeeping) on the same input: live dB within 1e-3 - the float32 histogram sums in arrival order -, index within one step
   on at most 1e-3 of the cells, with a clean emspec_device_status (the bounds of tests/test_gpu_pp_store_order.py).

Shapes: those of tests/test_gpu_pp_store_order.py - S = 3 streams; C = 2D + 5 columns; C = 131 under the shared-device plan
(EMSPEC_SHARED=1 in the diagnostic build); for hop 256 a stream that ends 100 samples short of the frame after the last and a
stream of zeros; both reassign settings - and, for the bookkeeping:

 - `edge0`: one stream of exactly N + hop (C - 1) samples, C = 2D + 8: the last frame's last sample is the stream's last, so
   the prefetch's remaining count reaches exactly zero at a register boundary; `edge1`: one sample fewer (C = 2D + 7, the
   frame after the last is one sample short);
 - `seg33`: C = 131 cut with EMSPEC_SEGLEN=33 in the diagnostic build.  The planner rounds a segment length up to even, so
   the segments are 34 columns: c0 = 34 g is no multiple of the ring length or of D, j0 = c0 - D and the last c1 = 131 is odd.
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
            tag = f"h{hop}_{'re' if reassign else 'off'}"
            out.append((f"{tag}_2Dplus5", hop, reassign, "short"))
            out.append((f"{tag}_c131", hop, reassign, "c131"))
            out.append((f"{tag}_edge0", hop, reassign, "edge0"))
            out.append((f"{tag}_edge1", hop, reassign, "edge1"))
            out.append((f"{tag}_seg33", hop, reassign, "seg33"))
    for reassign in (True, False):
        out.append((f"h256_{'re' if reassign else 'off'}_tail", 256, reassign, "tail"))
        out.append((f"h256_{'re' if reassign else 'off'}_zeros", 256, reassign, "zeros"))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]
ENV = {"c131": {"EMSPEC_SHARED": "1"}, "seg33": {"EMSPEC_SEGLEN": "33"}}   # switches of the diagnostic build, read per launch
_inputs = {}


def _input(case):
    """The case's samples [S][L] (deterministic, made once)."""
    name, hop, reassign, kind = case
    if name not in _inputs:
        D = emspec.latency_columns(N, hop, reassign)
        if kind == "short":
            pcm = synth.streams(3, N + hop * (2 * D + 5 - 1))
        elif kind in ("c131", "seg33"):
            pcm = synth.streams(3, N + hop * 130)
        elif kind == "tail":     # 2D + 6 columns; the samples end 100 short of one more frame
            pcm = synth.streams(1, N + hop * (2 * D + 6) - 100)
        elif kind == "edge0":
            pcm = synth.streams(1, N + hop * (2 * D + 7))
        elif kind == "edge1":
            pcm = synth.streams(1, N + hop * (2 * D + 7) - 1)
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
        want = {"short": 2 * D + 5, "c131": 131, "seg33": 131, "tail": 2 * D + 6, "zeros": 2 * D + 5, "edge0": 2 * D + 8,
                "edge1": 2 * D + 7}[kind]
        assert _columns(case) == want, name
        L = _input(case).shape[1]
        if kind == "tail":
            assert (want - 1) * hop + N < L < want * hop + N
        if kind == "edge0":
            assert L == (want - 1) * hop + N
        if kind == "edge1":
            assert L == want * hop + N - 1


def _product(case, engine, monkeypatch):
    """The case through the product kernel: libemspec.so, or - where the case needs one of its switches - the same kernel
    sources in the diagnostic build."""
    name, hop, reassign, kind = case
    assert engine.fused(N, hop, reassign)
    eng = engine
    if kind in ENV:
        for k, v in ENV[kind].items():
            monkeypatch.setenv(k, v)
        eng = emspec.Engine(diag=True)
    try:
        out = eng.batch(_input(case), N, hop, reassign, want=("db", "index"))
        eng.device_status()
    finally:
        if eng is not engine:
            eng.close()
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_matches_oracle(case, engine, monkeypatch):
    name, hop, reassign, kind = case
    pcm = _input(case)
    out = _product(case, engine, monkeypatch)
    odb, _, oidx = O.batch_f32(O.make_cfg(N, hop, reassign), pcm, want=("db", "index"))
    assert out["db"].shape == odb.shape == (pcm.shape[0], _columns(case), 1024)
    err = float(np.max(np.abs(out["db"] - odb)))
    print(f"MEASURED {name}: max |dB - oracle| {err:.2e}")
    assert err < 8.7e-4
    palette_close(out["index"], oidx)
    if kind == "zeros":
        assert np.all(out["db"] == out["db"].flat[0]) and np.all(out["index"] == out["index"].flat[0])


_OLD_CHILD = r"""
import json, os, sys
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "em-spec_amd")]
import emspec
inp = np.load(sys.argv[1])
envs = json.loads(sys.argv[3])
res = {}
with emspec.Engine(diag=True) as e:
    for key in inp.files:
        name, hop, reassign, kind = key.rsplit("|", 3)
        for k, v in envs.get(kind, {}).items():
            os.environ[k] = v
        out = e.batch(inp[key], 4096, int(hop), bool(int(reassign)), want=("db", "index"))
        e.device_status()
        for k in envs.get(kind, {}):
            del os.environ[k]
        res[name + "|db"], res[name + "|index"] = out["db"], out["index"]
np.savez(sys.argv[2], **res)
"""


@pytest.fixture(scope="module")
def old_variant(tmp_path_factory):
    """Every case through the kept old kernel body: one child process (the variant switch is read once per process)."""
    import json
    d = tmp_path_factory.mktemp("pp4")
    fin, fout = str(d / "in.npz"), str(d / "out.npz")
    np.savez(fin, **{f"{c[0]}|{c[1]}|{int(c[2])}|{c[3]}": _input(c) for c in CASES})
    r = subprocess.run([sys.executable, "-c", _OLD_CHILD % dict(root=ROOT), fin, fout, json.dumps(ENV)],
                       env=dict(os.environ, EMSPEC_FUSED_VARIANT="pp4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(fout)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_matches_kept_old_variant(case, engine, old_variant, monkeypatch):
    name, hop, reassign, kind = case
    new = _product(case, engine, monkeypatch)
    odb, oidx = old_variant[name + "|db"], old_variant[name + "|index"]
    assert new["db"].shape == odb.shape
    live = new["db"] > -100
    err = float(np.max(np.abs(new["db"][live] - odb[live]))) if live.any() else 0.0
    diff = new["index"].astype(np.int16) - oidx.astype(np.int16)
    print(f"MEASURED {name}: max |dB new - old| {err:.2e}, {np.count_nonzero(diff)} of {diff.size} palette indices differ")
    assert err < 1e-3
    assert np.max(np.abs(diff)) <= 1
    assert np.count_nonzero(diff) <= 1e-3 * diff.size
