"""CPU: the host arithmetic of the live calls' overlays (em-spec_amd/csrc/emspec_live_plan.h: live_out_slot, live_overlay_pair,
live_overlay_fits, live_wave_slots) without a GPU: which slot of the caller's arrays every peak list and
envelope pair of a call goes to, the capacity rule, and the envelope's pair ring - that every emitted column finds its own pair
in its slot, that no pair is overwritten before its column is emitted or its stream reset, and that the ring has the size the
header's comment derives.

tests/cdriver/live_overlay_plan_driver.cpp is a program of its own that includes only that header, runs the calls of
emspec_live.cpp with the HIP calls left out and models what the overlay kernel's waves do to the ring, built with the host
compiler under ASan and UBSan (nothing is preloaded, nothing is loaded into Python under a sanitizer).  The descriptors of
every launch come from the pure-Python restatement tests/live_ref.py; the slot rule is restated below."""
import json
import os
import random
import subprocess

import pytest

import live_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, hop, reassign, n_high, split): the issue's four geometries and one multi-resolution session
GEOMETRIES = ((1024, 256, 1, 0, 0), (4096, 256, 1, 0, 0), (4096, 4096, 0, 0, 0), (16384, 128, 1, 0, 0), (8192, 256, 1, 2048, 128))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("live_overlay_plan")
    exe = str(tmp / "live_overlay_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "live_overlay_plan_driver.cpp"), "-o", exe])
    count = [0]

    def run(lines):
        count[0] += 1
        path = tmp / ("in%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (lines[:3], r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)
    return run


# ---- the restatement: the columns a launch writes for one stream, as (i, slot, column) ----
def written(j0, frames, out_at, flush, D, empty_col):
    out = []
    for i in range(flush or frames):
        c = j0 - D + i
        if c < 0 and not empty_col:
            continue
        out.append((i, out_at + (i if empty_col else len(out)), c))
    return out


def expected_events(call, g, cols):
    """What the driver must print for one call of live_ref's trace: [s, i, slot, column, source, pair index]."""
    ev, produced = [], [0] * g["S"]
    per_frame = call["op"] in ("frame", "flush")
    for l in call["launches"]:
        if not l["launched"] or (call["op"] == "push" and l["mx"] == 0):
            continue
        for s, (j0, _newbase, frames, _newcount, out_at, flush) in enumerate(l["desc"]):
            for i, slot, c in written(j0, frames, out_at, flush, g["D"], per_frame):
                src = 0 if c < 0 else (1 if flush or c < j0 else 2)
                base = 0 if (per_frame or out_at or call["direct"]) else produced[s]
                ev.append([s, i, slot, c, src, s * cols + base + slot])
        if call["op"] == "push":
            produced = [p + n for p, n in zip(produced, l["nc"])]
    return ev


def run_both(driver, head, ops):
    """ops: 'frame' | 'flush' | ('push', count, direct) | ('reset', s).  A push gets max_columns = what it completes."""
    S, n, hop, reassign, form, n_high, split = head
    ref = L.Session(S, n, hop, reassign, form, n_high, split)
    g = L.geometry(*head)
    lines, want = ["open %d %d %d %d %d %d %d" % head], []
    for op in ops:
        if op == "frame":
            call, cols = ref.frame(), 1
            lines.append("frame")
        elif op == "flush":
            call, cols = ref.flush(), 1
            lines.append("flush")
        elif op[0] == "push":
            cols = ref.predict(op[1])
            call = ref.push(op[1], op[2])
            lines.append("push %d %d %d" % (op[1], op[2], cols))
        else:
            call, cols = ref.reset(op[1]), 1
            lines.append("reset %d" % op[1])
        call["direct"] = op[2] if op[0] == "push" else 0
        want.append((call, cols))
    got = driver(lines)
    assert len(got) == len(want)
    for k, (have, (call, cols)) in enumerate(zip(got, want)):
        if call["refused"]:
            assert have["refused"] == 1 and have["events"] == [], (head, k)
            continue
        # the driver runs its waves writes first, reads second: the order of the events is (s, i) ascending, as here
        assert have["events"] == expected_events(call, g, cols), (head, k, ops[k])
        assert have["fed"] == call["fed"] and have["emitted"] == call["emitted"], (head, k)
        assert have["stale"] == 0 and have["lost"] == 0, (head, k, ops[k], have["stale"], have["lost"])
    return got, g


def test_ring_size_is_the_derived_one(driver):
    for n, hop, reassign, n_high, split in GEOMETRIES:
        for form in (1, 2):
            for S in (1, 5, 64):
                head = (S, n, hop, reassign, form, n_high, split)
                g = L.geometry(*head)
                got = driver(["open %d %d %d %d %d %d %d" % head, "fits 1 1 1 1"])[0]
                # D slots still to be emitted + the most frames one launch writes
                assert got["wslots"] == g["D"] + g["mmax"] and got["ring_bytes"] == S * got["wslots"] * 8, head
                assert got["off"] == n // 2 - hop // 2 and got["off"] + hop <= n, head


def test_per_frame_sessions_with_staggered_streams(driver):
    for n, hop, reassign, n_high, split in GEOMETRIES:
        D = L.latency(n, hop, reassign)
        ops = ["frame"] * (D + 3) + [("reset", 2), "frame", "frame"] + ["flush"] * (D + 1) + [("reset", 0), ("reset", 1), ("reset", 2),
                                                                                              ("reset", 3), ("reset", 4)] + ["frame"] * (2 * D + 2) + ["flush"]
        got, g = run_both(driver, (5, n, hop, reassign, 1, n_high, split), ops)
        ev = [e for k in got for e in k["events"]]
        assert {e[4] for e in ev} == ({0, 1} if D else {2}), (n, hop)       # empty columns and the ring; D = 0: the launch's own frame
        assert any(e[3] == -1 for e in ev) or D == 0


def test_block_sessions_scripted_and_random(driver):
    rng = random.Random(20261019)
    for n, hop, reassign, n_high, split in GEOMETRIES:
        for S in (1, 4):
            head = (S, n, hop, reassign, 2, n_high, split)
            g = L.geometry(*head)
            cap = g["cap"]
            sizes = [1, 128, hop, hop + 1, n, cap, cap + 1, 3 * cap + 5, 128, hop]
            ops = [("push", b, i % 2) for i, b in enumerate(sizes)]
            if S > 1:
                ops += [("reset", 2), ("push", n + 3 * hop, 0), ("push", 2 * cap + 77, 1)]
            ops += ["flush"] * 2 + [("reset", s) for s in range(S)] + [("push", n + (g["D"] + 2) * hop, 1)]
            for _ in range(12):
                ops.append(("push", rng.choice((1, 127, 128, hop, rng.randrange(1, 3 * hop + 2), rng.randrange(1, 2 * cap + 2))), rng.randrange(2)))
                if S > 1 and rng.randrange(4) == 0:
                    ops.append(("reset", rng.randrange(S)))
            got, _ = run_both(driver, head, ops)
            ev = [e for k in got for e in k["events"]]
            # columns from the ring and - where a launch can bring more frames than the latency - from the launch's own samples
            assert {e[4] for e in ev} == ({1, 2} if 0 < g["D"] < g["mmax"] else {1} if g["D"] else {2}), head
            assert any(len(k["events"]) > S * g["D"] for k in got), head     # a launch that completes more columns than it reads from the ring
            assert not any(e[3] < 0 for e in ev)                             # the block form emits no empty column


def test_capacity_rule(driver):
    cases = [(1, 1, 1, 1), (1, 1, 1, 0), (64, 1, 8, 512), (64, 1, 8, 511), (3, 7, 32, 3 * 7 * 32), (3, 7, 32, 3 * 7 * 32 - 1), (5, 0, 8, 0),
             (65535, 2 ** 62, 32, 2 ** 63 - 1), (65535, 2 ** 31, 1, 65535 * 2 ** 31), (65535, 2 ** 31, 1, 65535 * 2 ** 31 - 1), (2, 3, 1, 6), (2, 3, 1, 5)]
    got = driver(["open 1 1024 256 1 1 0 0"] + ["fits %d %d %d %d" % c for c in cases])
    for (S, cols, per, capacity), have in zip(cases, got):
        assert have["refused"] == (0 if S * cols * per <= capacity else 1), (S, cols, per, capacity)
    # a push whose block completes more columns than max_columns is refused before anything is fed
    g = L.geometry(2, 1024, 256, 1, 2)
    total = 1024 + (g["D"] + 3) * 256
    got = driver(["open 2 1024 256 1 2 0 0", "push %d 0 3" % total, "push %d 0 4" % total])
    assert got[0]["refused"] == 1 and got[0]["events"] == [] and got[0]["fed"] == [0, 0]
    assert got[1]["refused"] == 0 and len(got[1]["events"]) == 2 * 4 and [e[5] for e in got[1]["events"]] == list(range(8))
