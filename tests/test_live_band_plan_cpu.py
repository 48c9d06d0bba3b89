"""CPU: the live multi-band session's host arithmetic (the bands of em-spec_amd/csrc/emspec_live_plan.h) -
every band's shift, latency, ring slots and byte sizes, the priming rule, the finalize rule and the launches of every call - against
the pure-Python restatement tests/live_band_ref.py, against the two-band geometry, and against closed forms, without a GPU.

tests/cdriver/live_plan_driver.cpp is a program of its own that includes only that header (and what it includes), built with
the host compiler under ASan and UBSan (nothing is preloaded, nothing is loaded into Python under a sanitizer):

    g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
        tests/cdriver/live_plan_driver.cpp -o live_plan_driver

Every run must exit with status 0 and an empty stderr."""
import json
import os
import subprocess

import pytest

import live_band_ref as B
import live_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the ladders of tests/test_gpu_live_multiband.py: (sizes, hop)
LADDERS = {"A": ((4096, 2048, 1024), 256), "B": ((16384, 4096, 1024), 256), "C": ((8192, 4096, 2048), 128),
           "D": ((16384, 8192, 4096, 2048), 512)}
STREAMS = (1, 3, 64, 512)
R = 1024


def _splits(K, rows=R):
    return [rows * (k + 1) // K // 4 * 4 for k in range(K - 1)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("live_band_plan")
    exe = str(tmp / "live_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "live_plan_driver.cpp"), "-o", exe])
    count = [0]

    def run(cmd, lines):
        count[0] += 1
        path = tmp / ("in%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, cmd, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (cmd, lines[:3], r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)
    return run


def _line(S, hop, reassign, form, rows, cell, n, split):
    return L.open_line(3, S, hop, reassign, form, rows, n, split)[5:] + " %d 1" % cell


def _two_band_shapes():
    """Every two-band shape both rules accept at a few hops: (n_low, n_high, hop)."""
    for n_low in (8192, 16384):
        for n_high in (1024, 2048, 4096):
            for hop in (64, 128, 256, 384, 512, 1024):
                if hop <= n_high and (n_low - n_high) % (2 * hop) == 0:
                    yield n_low, n_high, hop


def test_geometry_and_sizes_equal_the_restatement(driver):
    cases = []
    for sizes, hop in LADDERS.values():
        for S in STREAMS:
            for form in (1, 2):
                for reassign in (1, 0):
                    for cell in (4, 8):
                        cases.append((S, hop, reassign, form, R, cell, sizes, _splits(len(sizes))))
    for n_low, n_high, hop in _two_band_shapes():
        for S in STREAMS:
            for form in (1, 2):
                cases.append((S, hop, 1, form, R, 4 + 4 * (S & 1), (n_low, n_high), [300 if S == 3 else 512]))
    cases.append((3, 256, 1, 2, 4096, 8, (16384, 8192, 2048, 1024), [64, 128, 4032]))   # the thinnest bands, 4096 rows
    got = driver("geometry", [_line(*c) for c in cases])
    assert len(got) == len(cases) >= 4 * 4 * 2 * 2 * 2 + 20
    for c, have in zip(cases, got):
        S, hop, reassign, form, rows, cell, n, split = c
        assert have.pop("error") == "", c
        two = have.pop("two", None)
        want = B.geometry(S, hop, reassign, form, rows, cell, list(n), list(split))
        assert have == want, (c, {k: (have.get(k), want[k]) for k in want if have.get(k) != want[k]})
        K, D = len(n), have["D"]
        # closed forms
        assert have["lo"][0] == 0 and have["hi"][-1] == rows and have["lo"][1:] == have["hi"][:-1] == list(split), c
        assert have["slots"][0] == 2 * D + have["mmax"] and have["shift"][0] == have["lat_extra"][0] == 0, c
        for k in range(K):
            assert 2 * have["shift"][k] * hop == n[0] - n[k], c
            assert have["slots"][k] == have["mmax"] + have["shift"][k] + D + have["band_D"][k], c
            assert have["lat_extra"][k] == D - have["band_D"][k] >= 0, c
            if reassign:
                assert have["band_D"][k] + have["shift"][k] == D, c      # every band's frames end on the long band's
            assert have["ring_bytes"][k] == have["slots"][k] * (have["hi"][k] - have["lo"][k]) * cell, c
        assert have["done_bytes"] == S * 4 * K, c
        # K = 2: every derived number is what live_geometry(n_high, split) gives today
        assert (two is not None) == (K == 2), c
        if two:
            same = {"D": have["D"], "mmax": have["mmax"], "cap": have["cap"], "ring_mask": have["ring_mask"], "slots": have["slots"][0],
                    "slots_high": have["slots"][1], "shift": have["shift"][1], "D_high": have["band_D"][1], "split": split[0],
                    "ring_bytes": have["ring_bytes"][0], "ring_high_bytes": have["ring_bytes"][1],
                    "rings_bytes": have["rings_bytes"][0], "rings_high_bytes": have["rings_bytes"][1],
                    "sring_bytes": have["sring_bytes"], "desc_bytes": have["desc_bytes"], "fresh_bytes": have["fresh_bytes"],
                    "done_bytes": have["done_bytes"]}
            assert {k: two[k] for k in same} == same, (c, two, same)
            g = L.geometry(S, n[0], hop, reassign, form, n[1], split[0])          # ... and the restatement's
            assert all(two[k] == g[k] for k in ("D", "mmax", "cap", "ring_mask", "slots", "slots_high", "shift", "D_high", "split")), c
    assert sum(1 for c in cases if len(c[6]) == 2) >= 4 * 2 * 10


@pytest.mark.parametrize("n, hop, split, rows, why", [
    ((4096,), 256, [], 1024, "bands must be in 2..4"),
    ((16384, 8192, 4096, 2048, 1024), 256, [64, 128, 192, 256], 1024, "bands must be in 2..4"),
    ((4096, 512), 256, [512], 1024, "every fft size must be 1024, 2048, 4096, 8192 or 16384"),
    ((2048, 4096), 256, [512], 1024, "fft sizes must be strictly decreasing"),
    ((4096, 4096), 256, [512], 1024, "fft sizes must be strictly decreasing"),
    ((4096, 1024), 2048, [512], 1024, "hop must be in [1, n[bands - 1]]"),
    ((4096, 1024), 0, [512], 1024, "hop must be in [1, n[bands - 1]]"),
    ((4096, 1024), 1000, [512], 1024, "every (n[0] - n[k]) / (2 hop) must be an integer"),
    ((4096, 2048, 1024), 256, [510, 768], 1024, "every split row must be a multiple of 4"),
    ((4096, 2048, 1024), 256, [512, 512], 1024, "split rows must be strictly increasing"),
    ((4096, 2048, 1024), 256, [60, 512], 1024, "every band must be at least 64 rows high"),
    ((4096, 2048, 1024), 256, [512, 964], 1024, "every band must be at least 64 rows high"),
])
def test_rejected_shapes_name_the_rule(driver, n, hop, split, rows, why):
    got = driver("geometry", [_line(3, hop, 1, 2, rows, 4, n, split)])
    assert got == [{"error": why}]
    assert (B.shape_error(list(n), hop) or B.split_error(len(n), list(split), rows)) == why


def _open(S, hop, reassign, form, n, split):
    return L.open_line(3, S, hop, reassign, form, R, n, split)


def _scripts():
    a, hop = LADDERS["A"]
    b, _ = LADDERS["B"]
    c, hop_c = LADDERS["C"]
    d, hop_d = LADDERS["D"]
    cap = 64 * hop
    return {
        # per-frame form: a reset mid-session, flushes until nothing is pending, a refused feed
        "frames_A": [_open(2, hop, 1, 1, a, _splits(3))] + ["frame"] * 10 + ["reset 1", "frame"] + ["flush"] * 9 + ["frame", "flush"],
        "frames_C": [_open(3, hop_c, 1, 1, c, _splits(3))] + ["frame"] * 3 + ["reset 0", "frame", "flush"],
        # uneven blocks: less than a hop, a hop, several staging blocks, in place and staged, a reset, a flush and a refused push
        "push_B": [_open(3, hop, 1, 2, b, _splits(3)), "predict 128", "push 128 0", "push 16256 1", "push 256 0", "push 256 1", "push 1000 0",
                   "predict %d" % (2 * cap + 77), "push %d 1" % (2 * cap + 77), "reset 2", "push 20000 0", "push 255 1", "push 1 1",
                   "flush", "push 5 0"],
        "push_C": [_open(3, hop_c, 0, 2, c, _splits(3)), "push 8191 0", "push 1 0", "push 128 1", "push 256 1", "push 384 0", "reset 1",
                   "push 9000 0"],
        # a staging block smaller than a frame (64 streams at hop 64): it fills without a frame, and the launch only moves samples
        "worklet_B": [_open(64, 64, 1, 2, b, _splits(3))] + ["push 128 0"] * 40 + ["push 16384 0"],
        "push_D": [_open(64, hop_d, 1, 2, d, _splits(4)), "push 16384 0", "push 512 0", "push 1024 1", "push 1536 1", "reset 63",
                   "push 40000 0", "flush"],
    }


def test_sessions_report_the_columns_of_the_single_resolution_session_at_n0(driver):
    branches = set()
    for name, script in _scripts().items():
        got, want = driver("trace", script), B.run(script)
        assert len(got) == len(want) == len(script) - 1, name
        for i, (have, ref) in enumerate(zip(got, want)):
            assert have == ref, (name, i, script[i + 1], {k: (have.get(k), ref[k]) for k in ref if have.get(k) != ref[k]})
        # the columns of every call: tests/live_ref.py's session at n[0], on its own
        o = L.parse_open(script[0])
        S, hop, reassign, form, n, K = o["S"], o["hop"], o["reassign"], o["form"], o["n"], len(o["n"])
        one = L.run([L.open_line(1, S, hop, reassign, form, R, n[:1], [])] + script[1:])
        for have, ref in zip(got, one):
            assert (have["counts"], have["first"], have["predict"], have["refused"]) == (ref["counts"], ref["first"], ref["predict"], ref["refused"]), name
            assert (have["fed"], have["emitted"], have["seen"]) == (ref["fed"], ref["emitted"], ref["seen"]), name
        for k in got:
            for l in k["launches"]:
                if not l["launched"]:
                    branches.add("staged only")
                    continue
                # of the launch's steps: per band the workgroups per stream of its frame launch (-1: none), the kernels in all,
                # whether the frame launches only scatter
                frames = {st[1]: st for st in l["steps"] if st[0] == L.FRAMES}
                l = dict(l, mx=l["mlaunch"], groups=[frames[b][2] if b in frames else -1 for b in range(K)], kernels=len(l["steps"]),
                         defer=max([st[4] for st in frames.values()] + [0]))
                assert len({st[4] for st in frames.values()}) <= 1 and all(st[0] != L.FINALIZE for st in l["steps"]), (name, l)
                assert l["kernels"] <= K + 1, (name, l)              # the bound the bands kernel is there for
                if l["flush"]:
                    assert l["kernels"] == 1 and l["groups"] == [-1] * K
                    branches.add("flush")
                    continue
                assert l["groups"][0] == l["mx"]
                if l["mx"] == 0:
                    assert l["groups"][1:] == [-1] * (K - 1) and l["kernels"] == 1     # only the ingest: no other band is launched
                    branches.add("samples only")
                    continue
                extra = [(n[0] - v) // hop if l["priming"] else 0 for v in n]
                assert l["groups"] == [l["mx"] + x for x in extra], (name, l)
                assert l["kernels"] == K + l["defer"]
                branches.add(("priming" if l["priming"] else "steady", "deferred" if l["defer"] else "in place"))
            if k["op"] == "reset":
                assert all(z >= 1 for z in k["cleared"]), name       # every band's ring of the stream
    assert branches >= {"staged only", "flush", "samples only", ("priming", "deferred"), ("steady", "deferred"), ("priming", "in place"),
                        ("steady", "in place")}, branches
