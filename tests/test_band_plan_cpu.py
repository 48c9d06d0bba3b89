"""CPU: what the multi-band batch accepts and how it lays out its workspace (em-spec_amd/csrc/emspec_band_plan.h; DESIGN.md §3.13,
§4.14).  A stand-alone program (tests/cdriver/band_plan_driver.cpp, built with the host compiler under ASan and UBSan) prints the
header's answers for a list of cases; they are checked here against a numpy restatement of the rules written from the definition:
the shifts, every rejection with the rule named in its message, band row ranges that tile [0, rows), workspace planes of
(C + 2 shift[k]) * rows_k * 4 bytes per stream that do not overlap.  The two-band entries (emspec_batch_multires*) check a call by
rules of their own and then go through band_plan at K = 2: whatever those rules accept the multi-band rules accept too, with the
two-band batch's shift, row ranges and workspace bytes, and every refusal keeps its message."""
import json
import os
import subprocess

import numpy as np
import pytest

import chunk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1024, 2048, 4096, 8192, 16384)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("band_plan") / "band_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "band_plan_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)
    return run


@pytest.fixture(scope="module")
def cases(driver):
    return driver()


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


# ---- the two-band entries: rules of their own in front of band_plan(2, ...) ----
# the messages of the two-band batch and session as they stood when the batch had a run function of its own
TWO_BAND_MESSAGES = {
    "n_low": "n_low must be 8192 or 16384",
    "n_high": "n_high must be 1024, 2048 or 4096",
    "hop": "hop must be in [1, n_high]",
    "shift": "(n_low - n_high) / (2 hop) must be an integer",
    "split": "split_row must be a multiple of 4 in [64, rows - 64]",
}
TWO_BAND_HOPS = (1, 64, 128, 256, 512, 1024, 4096, 4097)
TWO_BAND_ROWS = (128, 256, 1024, 1000)


def two_band_shape_message(n_low, n_high, hop):
    """The two-band shape rules in their order of precedence: the message of the first one broken, or None."""
    if n_low not in (8192, 16384):
        return TWO_BAND_MESSAGES["n_low"]
    if n_high not in (1024, 2048, 4096):
        return TWO_BAND_MESSAGES["n_high"]
    if not 1 <= hop <= n_high:
        return TWO_BAND_MESSAGES["hop"]
    if (n_low - n_high) % (2 * hop):
        return TWO_BAND_MESSAGES["shift"]
    return None


def test_what_the_two_band_rules_accept_the_multi_band_rules_accept(driver):
    """Over every (n_low, n_high) of the five sizes, eight hops, four row counts and every split row in [0, rows] that is a multiple of 4
    (and some that are not): the two-band messages are the recorded ones; an accepted call passes band_shape_error(2, ...) and
    band_split_error(2, ...), and band_plan(2, ...) / band_layout give the two-band batch's shift, row ranges and workspace bytes
    (chunk_ref.multires_bytes) without and with the raw plane."""
    out = driver("two")
    C, shapes = out["C"], out["shapes"]
    assert [(w["n_low"], w["n_high"], w["hop"]) for w in shapes] == [(a, b, h) for a in SIZES for b in SIZES for h in TWO_BAND_HOPS]
    seen, accepted_shapes, accepted_cells = set(), 0, 0
    for w in shapes:
        n_low, n_high, hop = w["n_low"], w["n_high"], w["hop"]
        want = two_band_shape_message(n_low, n_high, hop)
        assert w["two"] == want, w
        seen.add(want)
        if want is not None:
            assert not w["cells"]
            continue
        accepted_shapes += 1
        assert w["band"] is None, (n_low, n_high, hop, w["band"])
        splits = {rows: [c[1] for c in w["cells"] if c[0] == rows] for rows in TWO_BAND_ROWS}
        assert sum(len(v) for v in splits.values()) == len(w["cells"])
        for rows, got in splits.items():
            assert set(range(0, rows + 1, 4)) < set(got) and any(s % 4 for s in got), (rows, got)
        for cell in w["cells"]:
            rows, split, two, band = cell[:4]
            ok = split % 4 == 0 and 64 <= split <= rows - 64
            assert two == (None if ok else TWO_BAND_MESSAGES["split"]), cell
            if not ok:
                assert len(cell) == 4
                continue
            accepted_cells += 1
            assert band is None, (n_low, n_high, hop, cell)
            shift = (n_low - n_high) // (2 * hop)
            assert cell[4:10] == [0, shift, 0, split, split, rows], (n_low, n_high, hop, cell)
            assert cell[10:] == [chunk_ref.multires_bytes(C, n_low, n_high, hop, rows, split, post) for post in (False, True)], cell
        assert {c[1] for c in w["cells"] if c[2] is None and c[0] == 1000} >= {64, 936}     # the limits themselves, rows % 64 != 0
    assert seen == {None, *(v for k, v in TWO_BAND_MESSAGES.items() if k != "split")}
    assert accepted_shapes >= 30 and accepted_cells >= 10000, (accepted_shapes, accepted_cells)
