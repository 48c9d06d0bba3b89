"""GPU: the live calls' overlays through the Node addon (em-spec_amd/js: engine.setLivePeaks, engine.setLiveWave): 64 streams x
20 hops; after every call engine.columnsPeaks and engine.columnsWave are peaksOf of the delivered dB and waveOf of the samples
fed, bit for bit (js/test_live_overlay.js makes the comparison and throws on the first difference).  Run and skipped by the
rule of the other addon tests."""
import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_live_overlays():
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    r = subprocess.run(["node", "test_live_overlay.js"], cwd=js, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["S"] == 64 and res["hops"] == 20 and res["k"] == 8
    assert res["emitted"] == 64 * 20 and res["empty"] > 0 and res["withPeaks"] > 0
