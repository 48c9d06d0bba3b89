"""GPU: the live level meters through the Node addon (em-spec_amd/js: engine.setLiveLevel, engine.setLiveCross, em.levelSum,
em.crossSum): 8 streams as 4 pairs x 20 hops; after every call engine.columnsLevel and engine.columnsCross are levelsOf / crossOf
of the samples fed, byte for byte, and the summed records of an inverted pair correlate at exactly -1 (js/test_live_level.js
makes the comparison and throws on the first difference).  Run and skipped by the rule of the other addon tests."""
import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_live_level():
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_live_level.js"], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["S"] == 8 and res["pairs"] == 4 and res["hops"] == 20
    assert res["emitted"] == 8 * 20 and res["empty"] > 0 and res["odd"] >= 3 and res["rho"] == -1
