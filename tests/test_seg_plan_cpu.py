"""CPU: the segment plans of the walking kernels (em-spec_amd/csrc/emspec_seg_plan.h) - how the fused float32 kernels, the two
EXACT fused kernels and the float32 and EXACT scatters cut a stream into segments, the grid that follows, the low-row scratch
and the stream split - are the ones recorded in tests/golden/seg_plans.json.  That file was written once by the arithmetic as
it stood inside the five launchers before the header took it over, which tests/cdriver/seg_plan_verbatim.h keeps unchanged for
this purpose:

    g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -DSEG_PLAN_VERBATIM \
        -I em-spec_amd/csrc tests/cdriver/seg_plan_driver.cpp -o seg_plan_verbatim
    ./seg_plan_verbatim > tests/golden/seg_plans.json

It is never written by the library's own header (the same command without -DSEG_PLAN_VERBATIM): a change of a plan shows up
here, without a GPU."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "seg_plans.json")


def build_driver(tmp_path, name, *defines, sanitize=True):
    """The stand-alone driver, built with the host compiler - here under ASan and UBSan (a program of its own: nothing is
    preloaded); sanitize=False for a caller that holds a GPU and only wants the driver's numbers."""
    exe = str(tmp_path / name)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", *san, *defines, "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "seg_plan_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _seg_of_block(sp, C, bx, by, ny):
    """seg_of_block (emspec_device.h) for arrays of blockIdx.x / blockIdx.y and gridDim.y = ny: stream, segment, c0, c1, valid."""
    bx, by = np.broadcast_arrays(bx, by)
    if not sp["short_last"]:
        c0 = bx * sp["seglen"]
        return by, bx, c0, np.minimum(c0 + sp["seglen"], C), c0 < C
    s, y = bx, by
    nl = min(sp["nlong"], ny)
    g = np.where(y < nl, (y + s) % nl, nl + ((y - nl) + s) % (ny - nl))
    ln = np.where(g < sp["nlong"], sp["seglen"], sp["tail"])
    c0 = np.where(g < sp["nlong"], g * sp["seglen"], sp["nlong"] * sp["seglen"] + (g - sp["nlong"]) * sp["tail"])
    return s, g, c0, np.minimum(c0 + ln, C), c0 < C


def _covers_every_stream_once(sp, C, S, nseg):
    """The whole grid of a launch: every stream's workgroups take each segment once (the rotated order of the shared-device plan
    is a permutation) and their column ranges are [0, C) cut at increasing points."""
    if sp["short_last"]:
        gx, gy = S, nseg            # grid = (streams, segments)
    else:
        gx, gy = nseg, S            # grid = (segments, streams)
    per = max(1, (1 << 20) // nseg)   # streams per slice of the grid
    streams = range(0, S, per)
    # (uniform plan: c0 and c1 are functions of blockIdx.x alone and the stream is blockIdx.y itself, so a grid of more than
    # 2^24 workgroups is walked for its first and last slice of streams only)
    if not sp["short_last"] and S * nseg > 1 << 24:
        streams = [0, max(0, S - per)]
    for s0 in streams:
        sv = np.arange(s0, min(S, s0 + per), dtype=np.int64)[:, None]
        gv = np.arange(nseg, dtype=np.int64)[None, :]
        bx, by = (sv, gv) if sp["short_last"] else (gv, sv)
        s, g, c0, c1, valid = _seg_of_block(sp, C, bx, by, gy)
        assert np.array_equal(s, np.broadcast_to(sv, s.shape)) and valid.all()
        assert np.array_equal(np.sort(g, axis=1), np.broadcast_to(gv, g.shape))
        order = np.argsort(c0, axis=1)
        c0, c1 = np.take_along_axis(c0, order, 1), np.take_along_axis(c1, order, 1)
        assert (c0[:, 0] == 0).all() and (c1[:, -1] == C).all() and np.array_equal(c1[:, :-1], c0[:, 1:]) and (c1 > c0).all()
    assert gx >= 1 and gy <= 65535


def _uniform(seg):
    return {"seglen": seg, "nlong": 1 << 30, "tail": seg, "short_last": 0}


def _round_candidates(ncu, S, C, seg_min):
    """Segment lengths that r = 1..4 rounds of workgroups propose (the integer part of the rounds-by-efficiency choice)."""
    out = []
    for r in (1, 2, 3, 4):
        ns = min(max(1, r * ncu // S), max(1, (C + seg_min - 1) // seg_min))
        out.append((C + ns - 1) // ns)
    return out


def test_seg_plans_match_the_recorded_plans(tmp_path):
    """The header's plans equal the fixture field by field; the case list reaches every branch; every recorded plan has the
    properties the kernels and the host layer rely on."""
    got = json.loads(run_driver(build_driver(tmp_path, "seg_plan_driver")))
    want = json.load(open(FIXTURE))
    assert len(got) == len(want) >= 300
    for g, w in zip(got, want):
        assert g["kind"] == w["kind"] and g["case"] == w["case"], (g["case"], w["case"])
        for key in w:
            assert g[key] == w[key], (w["kind"], w["case"], key, g[key], w[key])
    kinds = {k: [w for w in want if w["kind"] == k] for k in ("fused", "exact_fused", "exact_lr", "scatter", "exact_scatter")}
    assert all(kinds.values()) and sum(map(len, kinds.values())) == len(want)

    # ---- the list reaches every branch ----
    fused = kinds["fused"]
    asked_shared = lambda c: c["force"] == 1 or (c["force"] < 0 and c["shared"] == 1)
    assert any(w["short_last"] and w["streams_first"] and w["nlong"] < w["nseg"] for w in fused)
    assert any(asked_shared(w["case"]) and not w["short_last"] and w["nseg"] < 2 for w in fused)        # the tail cut refused: one segment
    assert any(asked_shared(w["case"]) and not w["short_last"] and w["nseg"] >= 2 for w in fused)       # ... and a tail below seg_min
    assert any(not w["ok"] and w["nseg"] > 65535 for w in fused)
    assert any(not w["ok"] for w in kinds["exact_fused"]) and any(not w["ok"] for w in kinds["exact_lr"])
    alone = {json.dumps(w["case"], sort_keys=True): w for w in fused if w["case"]["shared"] == 0}
    twin = lambda w: alone.get(json.dumps(dict(w["case"], shared=0), sort_keys=True))
    assert any(w["case"]["shared"] == 2 and w["seglen"] == 1024 and twin(w) and twin(w)["seglen"] > 1024 for w in fused)   # the cap bites
    assert any(w["case"]["shared"] == 1 and w["case"]["force"] == 0 and not w["short_last"] and w["seglen"] > 1024 for w in fused)
    assert any(w["case"]["ovr"] == 33 and w["seglen"] == 34 for w in fused) and any(w["case"]["ovr"] == 64 and w["seglen"] == 64 for w in fused)
    assert any(w["case"]["ovr"] == 1 and w["seglen"] != 2 for w in fused)                              # an override below 2 is ignored
    assert {w["case"]["kind"] for w in fused} == {0, 1, 2} and {w["case"]["shared"] for w in fused} == {0, 1, 2}
    assert {w["case"]["ncu"] for w in fused} == {256, 304, 64, 1} == {w["case"]["ncu"] for w in kinds["exact_fused"]}
    assert {w["case"]["D"] for w in fused} == {0, 1, 2, 8, 16, 32, 64, 1024}
    assert {w["case"]["S"] for w in fused} == {1, 2, 3, 5, 16, 34, 36, 64, 70, 257, 65535} == {w["case"]["S"] for w in kinds["exact_fused"]}
    assert {w["case"]["C"] for w in fused} == {1, 15, 16, 17, 130, 700, 4081, 16369, 262144, 8388593} == {w["case"]["C"] for w in kinds["exact_fused"]}
    # each number of rounds wins somewhere (the winner: the first r that proposes the recorded length)
    winners = set()
    for w in kinds["exact_fused"]:
        c = w["case"]
        if not c["ovr"]:
            cand = _round_candidates(c["ncu"], c["S"], c["C"], max(64, 4 * c["D"]))
            assert w["seg"] in cand
            winners.add(cand.index(w["seg"]) + 1)
    assert winners == {1, 2, 3, 4}
    for w in kinds["exact_lr"]:
        c = w["case"]
        assert c["ovr"] or w["seg"] in _round_candidates(c["ncu"], c["S"], c["C"], max(16, 2 * c["D"]))
    assert {w["case"]["n"] for w in kinds["exact_lr"]} == {4096, 2048, 1024}
    assert any(w["accept"] and w["case"]["rl"] and w["s_per"] < w["case"]["S"] for w in kinds["exact_lr"])   # a stream split
    assert any(w["accept"] and w["case"]["rl"] and w["s_per"] == w["case"]["S"] > 1 for w in kinds["exact_lr"])
    assert any(w["groups"] == 2048 for w in kinds["exact_lr"]) and any(w["groups"] == w["nseg"] > 2048 for w in kinds["exact_lr"])
    sc = kinds["scatter"]
    assert any(w["walk"] for w in sc) and any(not w["walk"] and w["ok"] for w in sc) and any(not w["ok"] for w in sc)
    assert any(not w["walk"] and w["case"]["D"] >= 16 and w["case"]["use_walk"] and w["walk_lds"] > 156 * 1024 for w in sc)
    assert any(not w["walk"] and w["case"]["D"] >= 16 and not w["case"]["use_walk"] for w in sc)
    assert {w["ch"] for w in sc} == {4, 8, 32} and {w["seg"] for w in sc if w["walk"]} >= {128, 1024} and any(w["tile"] == 32 for w in sc)
    assert any(w["walk"] and 128 < w["seg"] < 1024 for w in sc)
    xs = kinds["exact_scatter"]
    assert any(w["F"] and not w["rl"] and w["launched_F"] for w in xs)                                  # the whole ring walks
    assert any(w["F"] == 6 and w["rl"] and w["launched_F"] for w in xs)                                 # the row split
    assert any(w["F"] == 6 and w["rl"] and not w["launched_F"] and w["tile"] and w["ok"] for w in xs)   # ... without its scratch: tiles
    assert any(not w["F"] and w["ok"] and w["tile"] for w in xs) and any(not w["ok"] for w in xs)       # the tile fallback
    split = {json.dumps(dict(w["case"], axis=0), sort_keys=True) for w in xs if w["case"]["axis"] == 1 and w["rl"]}
    assert any(w["case"]["axis"] == 2 and not w["F"] and json.dumps(dict(w["case"], axis=0), sort_keys=True) in split for w in xs)   # past 6 %
    assert any(w["case"]["axis"] == 0 and not w["F"] and json.dumps(w["case"], sort_keys=True) in split for w in xs)                 # no table
    assert any(w["launched_F"] and w["rl"] and w["s_per"] < w["case"]["S"] for w in xs)                 # a stream split
    assert {w["case"]["rows"] for w in xs} >= {64, 1024}

    # ---- properties of every recorded plan ----
    for w in fused:
        c = w["case"]
        assert w["seglen"] % 2 == 0 and w["tail"] % 2 == 0 and w["seglen"] >= 2
        assert w["ok"] == (w["nseg"] <= 65535) and w["streams_first"] == w["short_last"]
        if w["ok"]:
            _covers_every_stream_once({k: w[k] for k in ("seglen", "nlong", "tail", "short_last")}, c["C"], c["S"], w["nseg"])
    for w in kinds["exact_fused"] + kinds["exact_lr"]:
        c = w["case"]
        assert w["seg"] >= 1 and w["nseg"] == -(-c["C"] // w["seg"]) and w["ok"] == (w["nseg"] <= 65535 and w["seg"] <= 0x3fffffff)
        if w["ok"]:
            _covers_every_stream_once(_uniform(w["seg"]), c["C"], c["S"], w["nseg"])
    for w in kinds["exact_lr"]:
        c = w["case"]
        assert w["per_group"] == c["slots"] * c["rl"] * 8 and not w["accept_less"]
        if c["rl"]:
            assert w["groups"] >= w["nseg"] and w["groups"] * w["per_group"] == w["scratch_bytes"] >= w["per_group"] * w["nseg"]
        # what was sized for S streams is accepted by the launch for the same S, and a launch's streams fit it
        assert w["accept"] == w["ok"]
        if w["accept"]:
            assert 1 <= w["s_per"] <= c["S"] and (not c["rl"] or w["s_per"] * w["nseg"] <= w["groups"])
    for w in sc:
        c = w["case"]
        if w["walk"]:
            assert w["seg"] % w["F"] == 0 and 128 <= w["seg"] <= 1024 + w["F"] and w["nseg"] == -(-c["C"] // w["seg"]) <= 65535
            assert w["walk_lds"] == (2 * c["D"] + w["F"]) * c["rows"] * 4 + 1024 <= 156 * 1024
            _covers_every_stream_once(_uniform(w["seg"]), c["C"], c["S"], w["nseg"])
        elif w["ok"]:
            assert 1 <= w["tile"] <= 32 and w["tile_lds"] <= 151 * 1024 and w["ntiles"] == -(-c["C"] // w["tile"])
    for w in xs:
        c = w["case"]
        if w["F"]:
            assert w["seg"] % w["F"] == 0 and w["nseg"] == -(-c["C"] // w["seg"]) and w["lds"] <= 158 * 1024
            assert w["per_group"] == (2 * c["D"] + w["F"]) * w["rl"] * 8
            assert w["groups"] * w["per_group"] == w["scratch_bytes"] >= w["per_group"] * w["nseg"]
        if w["F"] and w["rl"]:
            assert w["groups"] >= w["nseg"] and w["launched_F"] == (w["F"] if c["low"] else 0)   # the sized scratch is accepted
        if w["launched_F"]:
            assert 1 <= w["s_per"] <= c["S"] and (not w["rl"] or w["s_per"] * w["nseg"] <= w["groups"])
            if w["nseg"] <= 65535:
                _covers_every_stream_once(_uniform(w["seg"]), c["C"], c["S"], w["nseg"])
        elif w["ok"]:
            assert 1 <= w["tile"] <= 16 and w["tile_lds"] <= 151 * 1024 and w["ntiles"] == -(-c["C"] // w["tile"])


def test_recorded_plans_are_the_earlier_arithmetic(tmp_path):
    """The fixture is, byte for byte, what the launchers' own arithmetic from before the header prints (the generator command of
    the module's docstring): its provenance can be checked, and it cannot drift with the library's header."""
    assert run_driver(build_driver(tmp_path, "seg_plan_verbatim", "-DSEG_PLAN_VERBATIM")) == open(FIXTURE).read()
