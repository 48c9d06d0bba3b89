"""CPU: what the multi-band batch accepts and how it lays out its workspace (em-spec_amd/csrc/emspec_band_plan.h; DESIGN.md §3.13,
§4.14).  A stand-alone program (tests/cdriver/band_plan_driver.cpp, built with the host compiler under ASan and UBSan) prints the
header's answers for a list of cases; they are checked here against a numpy restatement of the rules written from the definition:
the shifts, every rejection with the rule named in its message, band row ranges that tile [0, rows), workspace planes of
(C + 2 shift[k]) * rows_k * 4 bytes per stream that do not overlap."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1024, 2048, 4096, 8192, 16384)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("band_plan") / "band_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "band_plan_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout)


def rule_broken(n, hop, split, rows):
    """The definition's rules in the order the header checks them: a word of the rule broken, or None."""
    K = len(n)
    if not 2 <= K <= 4:
        return "bands"
    if any(v not in SIZES for v in n):
        return "fft size"
    if any(b >= a for a, b in zip(n, n[1:])):
        return "decreasing"
    if not 1 <= hop <= n[-1]:
        return "hop"
    if any((n[0] - v) % (2 * hop) for v in n):
        return "integer"
    if any(s % 4 for s in split):
        return "multiple of 4"
    if any(b <= a for a, b in zip(split, split[1:])):
        return "increasing"
    if np.diff([0, *split, rows]).min() < 64:
        return "64 rows"
    return None


def _find(cases, **kw):
    hit = [w for w in cases if all(w[k] == v for k, v in kw.items())]
    assert hit, kw
    return hit[0]


def test_shifts_of_the_ladders(cases):
    assert _find(cases, n=[16384, 4096, 1024], hop=256, error=None)["shift"] == [0, 24, 30]
    assert _find(cases, n=[16384, 8192, 4096, 2048], hop=128, error=None)["shift"] == [0, 32, 48, 56]
    assert _find(cases, n=[8192, 2048, 1024], hop=512, error=None)["shift"] == [0, 6, 7]
    assert _find(cases, n=[16384, 1024], hop=1, error=None)["shift"] == [0, 7680]


def test_every_rejection_names_its_rule(cases):
    bad = {(tuple(w["n"]), w["hop"], tuple(w["split"])): w for w in cases if w["error"] is not None}
    want = {
        ((16384,), 256, ()): "bands",                                          # K = 1
        ((16384, 8192, 4096, 2048, 1024), 128, (200, 400, 600, 800)): "bands",  # K = 5
        ((4096, 16384, 1024), 256, (368, 668)): "decreasing",
        ((16384, 4096, 4096), 256, (368, 668)): "decreasing",
        ((16384, 4096, 512), 256, (368, 668)): "fft size",
        ((32768, 4096, 1024), 256, (368, 668)): "fft size",
        ((16384, 4096, 2048), 1000, (368, 668)): "integer",
        ((16384, 4096, 1024), 2048, (368, 668)): "hop",
        ((16384, 4096, 1024), 0, (368, 668)): "hop",
        ((16384, 4096, 1024), 256, (366, 668)): "multiple of 4",
        ((16384, 4096, 1024), 256, (368, 428)): "64 rows",
        ((16384, 4096, 1024), 256, (60, 668)): "64 rows",
        ((16384, 4096, 1024), 256, (368, 964)): "64 rows",
        ((16384, 4096, 1024), 256, (668, 368)): "increasing",
        ((16384, 4096, 1024), 256, (368, 368)): "increasing",
    }
    assert set(bad) == set(want)
    for key, rule in want.items():
        w = bad[key]
        assert rule in w["error"], (key, w["error"])
        assert w["stage"] == ("shape" if rule in ("bands", "decreasing", "fft size", "integer", "hop") else "split")


def test_every_case_follows_the_restated_rules(cases):
    """Accepted exactly when the restatement finds no rule broken; band row ranges tile [0, rows); the planes have the definition's
    sizes, start on 256-byte boundaries, do not overlap and fit what the chunk rule is asked for."""
    assert sum(w["error"] is None for w in cases) >= 30
    assert {len(w["n"]) for w in cases if w["error"] is None} == {2, 3, 4}
    assert {w["post"] for w in cases if w["error"] is None} == {0, 1} and {w["chunk"] for w in cases} >= {1, 3, 64}
    for w in cases:
        n, hop, split, rows, L, chunk = w["n"], w["hop"], w["split"], w["rows"], w["L"], w["chunk"]
        rule = rule_broken(n, hop, split, rows)
        if rule is not None:
            assert w["error"] is not None and rule in w["error"], (w, rule)
            continue
        assert w["error"] is None, w
        K = len(n)
        C = (L - n[0]) // hop + 1 if L >= n[0] else 0
        assert w["columns"] == C
        assert w["shift"] == [(n[0] - v) // (2 * hop) for v in n]
        # each band's own batch has exactly C + 2 shift columns: composed column c has its column c + shift in every band
        if C:
            assert [(L - v) // hop + 1 for v in n] == [C + 2 * d for d in w["shift"]]
        assert w["lo"] == [0, *split] and w["hi"] == [*split, rows]
        assert w["lo"][0] == 0 and w["hi"][-1] == rows and w["lo"][1:] == w["hi"][:-1]
        assert all(h - l >= 64 and l % 4 == 0 for l, h in zip(w["lo"], w["hi"]))
        assert w["plane"] == [(C + 2 * d) * (h - l) * 4 for d, l, h in zip(w["shift"], w["lo"], w["hi"])]
        assert w["raw_plane"] == (C * rows * 4 if w["post"] else 0)
        assert w["per_stream"] == sum(w["plane"]) + w["raw_plane"]
        spans = [(o, o + p * chunk) for o, p in zip(w["offset"] + [w["raw_offset"]], w["plane"] + [w["raw_plane"]])]
        assert spans[0][0] == 0 and all(a % 256 == 0 for a, _ in spans)
        for (_, end), (start, _) in zip(spans, spans[1:]):
            assert end <= start < end + 256
        assert w["chunk_bytes"] == spans[-1][1] <= w["per_stream"] * chunk + w["pad"]
        assert len(spans) == K + 1
