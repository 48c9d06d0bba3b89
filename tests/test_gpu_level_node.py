"""GPU: the level meters through the Node addon (em-spec_amd/js/test_level.js: engine.setLevelOut / setCrossOut with
computeColumnsPcmPacked, levelsOf, crossOf, levelValues, crossCorrelation) against the records of tests/level_ref.py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec
import level_ref as LR
import pcm_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_level_meters_match_the_reference(tmp_path):
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_level.js", str(tmp_path)], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sources, frames, n, hop, f = res["sources"], res["frames"], res["fftSize"], res["hop"], res["factor"]
    raw = np.fromfile(str(tmp_path / "src.i16"), np.int16).reshape(sources, frames * 2)
    fmt = emspec.PcmFormat.make("s16", 2, ("left", "right", "mid", "side"))
    assert np.array_equal(fmt.matrix.ravel(), np.array(res["mix"], F))
    dec = PR.decode(raw.view(np.uint8), PR.S16, 2, fmt.matrix)
    Cr = emspec.reduced_columns(res["columns"], f)
    level = np.fromfile(str(tmp_path / "level.bin"), emspec.LEVEL_DTYPE).reshape(sources * 4, Cr)
    cross = np.fromfile(str(tmp_path / "cross.bin"), emspec.CROSS_DTYPE).reshape(sources, Cr)
    assert LR.same(level, LR.levels(dec, n, hop, f)) and LR.same(cross, LR.crosses(dec, 4, 0, 1, n, hop, f))
    L = res["L"]
    pcm = np.fromfile(str(tmp_path / "pcm.f32"), F).reshape(4, L)
    got = np.fromfile(str(tmp_path / "levels_of.bin"), emspec.LEVEL_DTYPE).reshape(4, -1)
    assert LR.same(got, LR.levels(pcm, 1024, 255, 4)) and (got["odd"] > 0).sum() == 3
    assert LR.same(np.fromfile(str(tmp_path / "cross_of.bin"), emspec.CROSS_DTYPE).reshape(2, -1), LR.crosses(pcm, 2, 1, 0, 1024, 255, 4))
