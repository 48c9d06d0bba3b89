"""CPU: the streaming session's host arithmetic (em-spec_amd/csrc/emspec_live_plan.h) - the geometry of a
session, every buffer size, the per-stream accounting of every call (what a launch's descriptors say, which column each
output slot holds), the kernels each launch runs and the rule that refuses a call which does not fit the open session - against
the pure-Python restatement tests/live_ref.py and against closed forms, without a GPU.  (The bands of a multi-band session:
tests/test_live_band_plan_cpu.py, on the same driver.)

tests/cdriver/live_plan_driver.cpp is a program of its own that includes only that header and runs the calls of emspec_live.cpp
with the HIP calls left out, built with the host compiler under ASan and UBSan (nothing is preloaded, nothing is loaded into
Python under a sanitizer):

    g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
        tests/cdriver/live_plan_driver.cpp -o live_plan_driver

Every run must exit with status 0 and an empty stderr."""
import json
import os
import random
import subprocess

import pytest

import live_ref as L
from test_live_multires_cpu import shape_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384)
STREAMS = (1, 3, 64, 2048, 65535)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("live_plan")
    exe = str(tmp / "live_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "live_plan_driver.cpp"), "-o", exe])
    count = [0]

    def run(cmd, lines):
        """The lines as the driver's input file, one child process -> what it printed, parsed."""
        count[0] += 1
        path = tmp / ("in%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, cmd, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (cmd, lines[:3], r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)
    return run


# ---- geometry ----
def _geometry_cases():
    """(S, n, hop, reassign, form, n_high, split, R, cell, views, frame_bytes, cols)"""
    extra = ((1024, 4, 1, 4, 7), (1024, 8, 2, 6, 3), (4096, 8, 1, 24, 64))   # (R, cell, views, frame_bytes, cols), in turn
    i = 0
    for n in SIZES:
        for hop in sorted({1, 64, 256, 300, n // 2, n}):
            if hop > n:
                continue
            for S in STREAMS:
                for form in (1, 2):
                    for reassign in (1, 0):
                        i += 1
                        yield (S, n, hop, reassign, form, 0, 0) + extra[i % 3]
    for n_low in (8192, 16384):
        for n_high in (1024, 2048, 4096):
            for hop in range(64, 513):
                if shape_ok(n_low, n_high, hop):
                    for S in (1, 64, 65535):
                        for form in (1, 2):
                            for reassign in (1, 0):
                                i += 1
                                R = extra[i % 3][0]
                                yield (S, n_low, hop, reassign, form, n_high, (R * (1 + i % 5)) // 7) + extra[i % 3]


def test_geometry_and_sizes_equal_the_restatement(driver):
    cases = list(_geometry_cases())
    multi = [c for c in cases if c[5]]
    assert len(cases) - len(multi) == 7 * 6 * 5 * 2 * 2 - 5 * 2 * 2 * 3   # (hop 300 > N = 256; hop 256 is N / 2 or N at N = 512 / 256)
    assert len(multi) >= 12 * 39 and {c[2] for c in multi} >= {64, 128, 256, 512}
    got = driver("geometry", [_shape(*c[:8], views=c[9], fb=c[10]) + " %d %d" % (c[8], c[11]) for c in cases])
    assert len(got) == len(cases)
    for c, have in zip(cases, got):
        g = L.geometry(*c[:7])
        want = dict(g, **L.sizes(g, *c[7:]))
        assert have == want, (c, {k: (have.get(k), want[k]) for k in want if have.get(k) != want[k]})
        # closed forms
        ring = have["ring_mask"] + 1
        assert ring & (ring - 1) == 0 and ring >= have["n"] + have["cap"] > ring // 2, c
        assert have["cap"] == (have["n"] if have["form"] == 1 else have["mmax"] * have["hop"]) and have["cap"] <= max(have["n"], 1 << 17), c
        assert 1 <= have["mmax"] <= 64 and have["slots"] == 2 * have["D"] + have["mmax"], c
        if c[5]:
            assert have["slots_high"] == have["mmax"] + have["shift"] + have["D"] + have["D_high"], c
            assert 2 * have["shift"] * have["hop"] == have["n"] - have["n_high"], c
            if have["reassign"]:
                assert have["D"] == have["D_high"] + have["shift"], c
        else:
            assert have["slots_high"] == have["ring_high_bytes"] == have["split"] == 0, c


# ---- traces ----
def _shape(S, n, hop, reassign, form, n_high=0, split=0, R=1024, views=0, fb=1):
    """A single-resolution or (n_high != 0) two-band session as the driver reads it."""
    return L.open_line(2 if n_high else 1, S, hop, reassign, form, R, [n, n_high][:2 if n_high else 1], [split] if n_high else [], views, fb)[5:]


def _open(*a, **kw):
    return "open " + _shape(*a, **kw)


CAP = 64 * 256   # 3 streams at hop 256: 64 frames per launch
SCRIPTS = {
    # one frame per call; a reset of one stream mid-session; flushes until nothing is pending, some streams empty before others;
    # a refused feed; reset and feed again
    "frames": [_open(3, 1024, 256, 1, 1)] + ["frame"] * 5 + ["reset 1", "frame"] + ["flush"] * 4 + ["frame", "reset 0", "frame",
              "reset 1", "reset 2", "predict 1024"] + ["frame"] * 4,
    "frames_plain": [_open(2, 512, 300, 0, 1)] + ["frame"] * 3 + ["flush", "frame"],
    # blocks of 1 sample, 128 samples, exactly one hop, exactly cap, cap + 1, several times cap - staged and in place
    "push": [_open(3, 1024, 256, 1, 2), "predict 1", "push 1 0", "push 128 0"] + ["push 128 1"] * 7 + ["predict 256", "push 256 0", "push 256 1",
             "predict %d" % CAP, "push %d 0" % CAP, "push %d 1" % (CAP + 1), "predict %d" % (3 * CAP + 5), "push %d 1" % (3 * CAP + 5),
             "push %d 0" % (2 * CAP), "push 0 0", "reset 2", "predict 2000", "push 2000 1", "push %d 1" % (2 * CAP + 77), "flush", "flush", "flush",
             "push 5 0", "reset 0", "reset 1", "reset 2", "push 1500 0", "flush", "flush"],
    # a staging block smaller than a frame (64 streams at hop 64: 32 frames = 2,048 samples): blocks that complete no frame launch
    # nothing until the staging block is full, and then only move samples
    "worklet": [_open(64, 16384, 64, 1, 2)] + ["push 128 0"] * 40 + ["push 16384 0", "reset 7", "push 100 1", "push 64 0"],
    # a PCM-style session: raw frames per source, every stream equally full; a drain in front of a stream's reset
    "pcm": [_open(4, 1024, 256, 1, 2, views=2, fb=6), "push 100 0", "push 2000 0", "push 77 0", "reset 1", "push 300 0", "push 40000 1", "reset 3",
            "push 9 0", "flush"],
    # multi-resolution sessions: a stream's first frame primes the short band
    "multires_push": [_open(2, 16384, 256, 1, 2, 4096, 300), "push 16000 0", "push 384 0", "push 256 0", "reset 1", "push 20000 1"],
    "multires_frames": [_open(2, 8192, 512, 0, 1, 2048, 100), "frame", "frame", "reset 0", "frame", "flush"],
    # ... its staging block smaller than a frame, as "worklet": a launch that only moves samples runs the long band alone
    "multires_worklet": [_open(64, 16384, 64, 1, 2, 4096, 300)] + ["push 128 0"] * 40 + ["push 16384 0", "push 64 1", "flush"],
    # ... 16384 / 1024 at hop 512: a frame per call finalises the long band in place while the short band (n < 2048) defers
    "multires_mixed": [_open(2, 16384, 512, 1, 1, 1024, 512)] + ["frame"] * 3 + ["flush"],
}


def _launches(trace):
    return [(k, l) for k in trace for l in k["launches"]]


def test_traces_equal_the_restatement_and_reach_every_branch(driver):
    traces = {}
    for name, script in SCRIPTS.items():
        got, want = driver("trace", script), L.run(script)
        assert len(got) == len(want) == len(script) - 1, name
        for i, (have, ref) in enumerate(zip(got, want)):
            assert have == ref, (name, i, script[i + 1], {k: (have.get(k), ref[k]) for k in ref if have.get(k) != ref[k]})
        traces[name] = got
    every = [kl for t in traces.values() for kl in _launches(t)]
    pushes = [(k, l) for k, l in every if k["op"] == "push"]
    # the branches, by what only they leave behind
    assert any(not l["launched"] for _, l in pushes)                                               # a block that only joins the staging block
    assert any(l["launched"] and l["mx"] == 0 for _, l in pushes)                                  # ... until it is full: samples only
    assert any(len(k["launches"]) >= 3 and all(l["launched"] for l in k["launches"]) for k, _ in pushes)   # several rounds in one call
    assert any(l["take"] == CAP and l["maxpend"] == 0 for _, l in pushes) and any(l["take"] == 1 for _, l in pushes)
    assert any(l["maxpend"] > 0 and l["launched"] for _, l in pushes)                              # a round on top of staged samples
    assert any(d[4] > 0 for _, l in pushes for d in l["desc"])                                     # in place: later rounds further in
    assert any(l["launched"] and not l["uniform"] for k, l in every if k["op"] == "push")          # streams in different states
    assert any(not l["uniform"] for k, l in every if k["op"] == "frame")
    assert any(l["uniform"] for _, l in every)
    flushes = [k for t in traces.values() for k in t if k["op"] == "flush"]
    assert any(-1 in k["first"] and max(k["first"]) >= 0 for k in flushes)                         # "column -1" beside a real one
    assert any(k["refused"] == "no pending column" for k in flushes)
    feeds = [k for t in traces.values() for k in t if k["op"] in ("frame", "push")]
    assert any("was flushed" in k["refused"] for k in feeds if k["op"] == "frame") and any("was flushed" in k["refused"] for k in feeds if k["op"] == "push")
    assert any(k["op"] == "reset" and k["launches"] for k in traces["pcm"])                        # the drain
    assert any(k["op"] == "reset" and not k["launches"] for k in traces["pcm"])                    # nothing staged: none
    assert all(len(set(k["pend"])) == 1 for k in traces["pcm"] if k["op"] == "push")
    for name in ("multires_push", "multires_frames"):
        prim = [l["priming"] for _, l in _launches(traces[name]) if l["launched"]]
        assert prim[0] == 1 and 0 in prim and 1 in prim[1:], name                                 # first frame; steady; after a reset
    assert not any(l["priming"] for k, l in every if k["op"] == "flush")
    # the kernels of every launch equalled the restatement's above; between them the scripts reach every branch of that rule, for
    # both kinds.  (A frame step: [FRAMES, band, workgroups, 0, defers, ingest]; a finalize: [FINALIZE, band, 0, columns, 0, 0].)
    reached = set()
    for name, t in traces.items():
        kind, small = ("two-band", None) if name.startswith("multires") else ("single", int(SCRIPTS[name][0].split()[10]) < 2048)
        for k, l in _launches(t):
            assert len(l["steps"]) <= 4 and all(st[0] != L.FINALIZE_BANDS for st in l["steps"]), (name, l)
            if not l["launched"]:
                assert l["steps"] == []
                reached.add((kind, "staged only"))
                continue
            frames = {st[1]: st for st in l["steps"] if st[0] == L.FRAMES}
            fins = {st[1]: st for st in l["steps"] if st[0] == L.FINALIZE}
            if l["flush"]:
                assert not frames and [st[3] for st in l["steps"]] == [1] * (2 if kind == "two-band" else 1), (name, l)
                reached.add((kind, "flush"))
                continue
            assert frames[0][5] == 1 and all(st[5] == 0 for b, st in frames.items() if b), (name, l)   # one ingest, the first band's
            assert set(fins) == ({b for b, st in frames.items() if st[4]} if l["mlaunch"] else set()), (name, l)
            assert all(st[3] == l["mlaunch"] for st in fins.values()), (name, l)
            if l["mlaunch"] == 0:
                assert list(frames) == [0] and frames[0][2] == 0, (name, l)
                reached.add((kind, "samples only"))
                continue
            if l["priming"]:
                reached.add((kind, "priming"))
            if l["mlaunch"] > L.INLINE:
                assert all(st[4] for st in frames.values()), (name, l)
                reached.add((kind, "defers: many columns"))
            elif kind == "single":
                reached.add((kind, "defers: small transform" if small else "in place"))
                assert frames[0][4] == int(small), (name, l)
            else:
                reached.add((kind, {(0, 0): "in place", (0, 1): "only the short band defers"}[(frames[0][4], frames[1][4])]))
    assert reached >= {(kind, what) for kind in ("single", "two-band") for what in
                       ("staged only", "samples only", "priming", "defers: many columns", "in place", "flush")}, reached
    assert reached >= {("single", "defers: small transform"), ("two-band", "only the short band defers")}, reached


# ---- closed forms, on the driver's output alone ----
def _check_session(trace, g, total_by_stream=None):
    """What must hold for any session of the block form, whatever the blocks."""
    S, D, n, hop = g["S"], g["D"], g["n"], g["hop"]
    seen = [0] * S
    for k in trace:
        assert k["pending"] == [int(f > e) for f, e in zip(k["fed"], k["emitted"])]
        assert k["any_pending"] == int(any(k["pending"]))
        assert all(0 <= p <= g["cap"] for p in k["pend"])
        assert [a + b for a, b in zip(k["newbase"], k["pend"])] == k["seen"]
        if k["op"] == "reset":
            seen[k["arg"]] = 0
        if k["op"] != "push" or k["refused"]:
            continue
        for l in k["launches"]:
            seen = [x + l["take"] for x in seen]
            for s, d in enumerate(l["desc"]):
                assert d[1] + d[3] == seen[s] and 0 <= d[3] <= g["cap"]      # newbase + pend == seen, before the launch
                assert 0 <= d[2] <= g["mmax"] and d[2] <= l["mx"]            # frames per launch
        assert seen == k["seen"]
        assert max(k["counts"]) == k["predict"]                              # the call's prediction is what it produced
        assert all(sum(l["nc"][s] for l in k["launches"] if l["launched"]) == k["counts"][s] for s in range(S))


def test_any_split_of_the_same_samples_gives_the_same_columns(driver):
    rng = random.Random(20260101)
    for (S, n, hop, reassign), total in (((3, 1024, 256, 1), 60000), ((1, 4096, 256, 1), 40000), ((5, 512, 300, 0), 9000),
                                         ((64, 16384, 64, 1), 30000), ((2, 2048, 2048, 1), 300000)):
        g = L.geometry(S, n, hop, reassign, 2)
        cap = g["cap"]
        want = max(L.whole_frames(total, n, hop) - g["D"], 0)
        splits = [[total], [hop] * (total // hop) + [total % hop], [cap + 1] * (total // (cap + 1)) + [total % (cap + 1)]]
        for _ in range(3):
            blocks, left = [], total
            while left:
                b = min(left, rng.choice((1, 127, 128, hop, rng.randrange(1, 3 * hop + 2), rng.randrange(1, 2 * cap + 2))))
                blocks.append(b)
                left -= b
            splits.append(blocks)
        for blocks in splits:
            blocks = [b for b in blocks if b]
            assert sum(blocks) == total
            script = [_open(S, n, hop, reassign, 2)]
            for b in blocks:
                script += ["predict %d" % b, "push %d %d" % (b, rng.randrange(2))]
            trace = driver("trace", script)
            _check_session(trace, g)
            pushes = [k for k in trace if k["op"] == "push"]
            for s in range(S):
                assert sum(k["counts"][s] for k in pushes) == want, (S, n, hop, blocks[:8])
                firsts = [k["first"][s] for k in pushes if k["counts"][s]]
                assert firsts.count(0) == (1 if want else 0) and all(k["first"][s] == -1 for k in pushes if not k["counts"][s])
                nxt = 0
                for k in pushes:                               # the columns come in order, none twice, none left out
                    if k["counts"][s]:
                        assert k["first"][s] == nxt
                        nxt += k["counts"][s]
            for pre, k in zip(trace[0::2], trace[1::2]):       # the prediction asked beforehand, too
                assert pre["op"] == "predict" and pre["predict"] == k["predict"] == max(k["counts"])


def test_invariants_hold_on_the_scripted_sessions(driver):
    for name in ("push", "worklet", "pcm", "multires_push"):
        o = L.parse_open(SCRIPTS[name][0])
        _check_session(driver("trace", SCRIPTS[name]), L.geometry(o["S"], o["n"][0], o["hop"], o["reassign"], o["form"], *(o["n"][1:] + o["split"])))


# ---- the rule that refuses a call which does not fit the open session ----
# (the messages: copied from live_check of em-spec_amd/csrc/emspec_live.cpp as it stood before the rule moved into the header)
IS_BANDS = "the live session is a multi-band one (emspec_columns_multiband / emspec_push_samples_multiband); call emspec_reset() first"
NOT_BANDS = "the live session is not a multi-band one; call emspec_reset() before a multi-band call"
IS_TWO = "the live session is a multi-resolution one (emspec_columns_multires / emspec_push_samples_multires); call emspec_reset() first"
IS_SINGLE = "the live session is a single-resolution one; call emspec_reset() before a multi-resolution call"
CHANGED = {1: "streams / fft size / hop / reassign / feeding mode changed mid-stream; call emspec_reset() first",
           2: "streams / fft sizes / hop / split row / reassign / feeding mode changed mid-stream; call emspec_reset() first",
           3: "streams / bands / fft sizes / split rows / hop / reassign / feeding mode changed mid-stream; call emspec_reset() first"}
# kind, S, hop, reassign, form, R, sizes, split rows.  The two-band session and the K = 2 multi-band one: the same bands
KINDS = {"single": (1, 3, 256, 1, 2, 1024, [16384], []), "two-band": (2, 3, 256, 1, 2, 1024, [16384, 4096], [512]),
         "bands2": (3, 3, 256, 1, 2, 1024, [16384, 4096], [512]), "bands3": (3, 3, 256, 1, 2, 1024, [16384, 4096, 2048], [256, 512])}


def test_a_call_that_does_not_fit_the_open_session_is_refused_in_the_same_words(driver):
    def line(a, b):
        return L.open_line(*a)[5:] + " | " + L.open_line(*b)[5:]

    pairs, want = [], []
    for a, have in KINDS.items():
        for b, ask in KINDS.items():
            pairs.append(line(have, ask))
            if have[0] == ask[0] == 3:
                want.append("" if a == b else CHANGED[3])          # K = 2 against K = 3: the bands changed
            elif have[0] == 3:
                want.append(IS_BANDS)
            elif ask[0] == 3:
                want.append(NOT_BANDS)
            else:
                want.append("" if a == b else IS_TWO if have[0] == 2 else IS_SINGLE)
    assert len(pairs) == 16 and want.count("") == 4
    # one field changed, every other as opened: streams, hop, reassign, the feeding form, a size, a split row - and the band count
    for name, have in KINDS.items():
        kind, S, hop, reassign, form, R, n, split = have
        changes = [(kind, S + 1, hop, reassign, form, R, n, split), (kind, S, hop // 2, reassign, form, R, n, split),
                   (kind, S, hop, 0, form, R, n, split), (kind, S, hop, reassign, 1, R, n, split),
                   (kind, S, hop, reassign, form, R, [8192] + n[1:], split)]
        if len(n) > 1:
            changes += [(kind, S, hop, reassign, form, R, n[:-1] + [1024], split), (kind, S, hop, reassign, form, R, n, [split[0] - 4] + split[1:]),
                        (kind, S, hop, reassign, form, R, n, split[:-1] + [split[-1] + 64])]
        for ask in changes:
            pairs.append(line(have, ask))
            want.append(CHANGED[kind])
    got = driver("compat", pairs)
    assert [x["why"] for x in got] == want, [(p, x["why"], w) for p, x, w in zip(pairs, got, want) if x["why"] != w]
