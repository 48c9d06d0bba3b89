"""GPU: the live audio history through the Node addon (em-spec_amd/js: engine.setLiveAudio, liveAudio, audioView, reanalyse):
one EXACT session of three streams fed hop by hop from a file this test writes; js/test_audio.js checks liveAudio after every
call, that the view of everything held is the samples fed and that reanalyse equals computeColumns of them, and writes the
view's, the re-analysis' dB and index bytes - which must equal the samples and the Python binding's re-analysis of the same
feed, byte for byte.  Run and skipped by the rule of the other addon tests."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N, HOP, R, W, FRAMES = 3, 1024, 256, 64, 2500, 12


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_audio_view_and_reanalysis_equal_the_python_bindings(tmp_path):
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    L = N + HOP * (FRAMES - 1)
    pcm = (np.random.default_rng(21).standard_normal((S, L)) * 0.2).astype(np.float32)
    feed, out = tmp_path / "feed.f32", tmp_path / "audio.bin"
    pcm.tofile(feed)
    r = subprocess.run(["node", "test_audio.js", str(feed), str(out)] + [str(v) for v in (S, L, N, HOP, R, W)], cwd=js,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["S"] == S and res["hops"] == FRAMES and (res["end"], res["first"]) == (L, L - W)
    # the same feed through the Python binding
    with emspec.Engine(mode=emspec.MODE_EXACT, rows=R) as e:
        e.set_live_audio(W)
        for j in range(FRAMES):
            e.columns(pcm[:, j * HOP:j * HOP + N], HOP, True)
        assert e.live_audio(0) == (L, L - W)
        view = e.audio_view(L - W, W)
        re = e.audio_batch(L - W, W, 256, 128, False, want=("db", "index"))
    assert np.array_equal(view.view(np.uint32), pcm[:, L - W:].view(np.uint32))
    assert re["db"].shape[1] == res["columns"] == emspec.num_columns(W, 256, 128)
    want = [view.tobytes(), re["db"].tobytes(), re["index"].tobytes()]
    got = out.read_bytes()
    assert len(got) == sum(len(w) for w in want)
    at = 0
    for name, w in zip(("view", "db", "index"), want):
        assert got[at:at + len(w)] == w, name
        at += len(w)
    assert len(np.unique(np.frombuffer(want[2], np.uint8))) > 4
