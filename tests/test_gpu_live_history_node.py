"""GPU: the live history through the Node addon (em-spec_amd/js: engine.setLiveHistory, liveHistory, historyView): one EXACT
session of three streams fed hop by hop from a file this test writes; js/test_history.js checks liveHistory after every call and
writes the bytes of four views - dB, index and RGBA each; the default law and a map; a sub-range of streams; one group of
everything held - which must equal the Python binding's views of the same feed, byte for byte.  Run and skipped by the rule of
the other addon tests."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec
import history_ref as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, N, HOP, R, W, FRAMES = 3, 1024, 256, 64, 5, 27


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_history_views_equal_the_python_bindings(tmp_path):
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not os.path.exists(os.path.join(js, "emspec.node")):
        pytest.skip("addon not built")
    L = N + HOP * (FRAMES - 1)
    pcm = H.signal(S, L)
    feed, out = tmp_path / "feed.f32", tmp_path / "views.bin"
    pcm.tofile(feed)
    r = subprocess.run(["node", "test_history.js", str(feed), str(out)] + [str(v) for v in (S, L, N, HOP, R, W)], cwd=js,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["S"] == S and res["hops"] == FRAMES and res["emitted"] == FRAMES and res["views"] == 4
    # the same feed through the Python binding
    want = []
    with emspec.Engine(mode=emspec.MODE_EXACT, rows=R) as e:
        e.set_live_history(W)
        for j in range(FRAMES):
            e.columns(pcm[:, j * HOP:j * HOP + N], HOP, True)
        for _ in range(emspec.latency_columns(N, HOP, True)):
            e.columns_flush()
        assert e.live_history(0) == (FRAMES, FRAMES - W)
        first = FRAMES - W
        assert res["first"] == first
        all3 = ("db", "index", "rgba")
        for v in (e.history_view(first, 1, W, want=all3), e.history_view(first, 2, 3, map=H.VIEW_MAP, want=all3),
                  e.history_view(first + 1, 3, 2, stream0=1, streams=S - 1, map=H.VIEW_MAP, want=all3),
                  e.history_view(first, 65536, 1, want=all3)):
            want += [v["db"].tobytes(), v["index"].tobytes(), v["rgba"].tobytes()]
    got = out.read_bytes()
    assert len(got) == sum(len(w) for w in want)
    at = 0
    for i, w in enumerate(want):
        assert got[at:at + len(w)] == w, ("view", i // 3, ("db", "index", "rgba")[i % 3])
        at += len(w)
    assert len(np.unique(np.frombuffer(want[1], np.uint8))) > 4
