"""CPU: tests/chunk_ref.py - the restatement of the stream-chunk rule that tests/test_gpu_chunks.py prints its expected chunk lists
from - says what the HIP-free headers say (em-spec_amd/csrc/emspec_kernel_plan.h, emspec_band_plan.h).  A stand-alone program
(tests/cdriver/chunk_plan_driver.cpp, built with the host compiler under ASan and UBSan) answers one line per question:
f32_record_bytes, exact_record_bytes, first_chunk / next_chunk, second_array_offset, kChunkPad, band_plan + band_layout + kBandPad -
for a few dozen argument sets of its own and for every workspace of every case of the GPU file (the two-band batch's: band_layout
at K = 2).  The two per-stream sizes that live in .cpp files (time reduction, peaks) cannot be reached this way: chunk_ref cites
their lines, and the GPU cases' budgets keep 10 % of margin around them, which is checked here."""
import json
import os
import subprocess

import pytest

import chunk_ref as K
import test_gpu_chunks as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chunk_plan") / "chunk_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "chunk_plan_driver.cpp"), "-o", exe])

    def run(lines):
        text = "".join(" ".join(str(int(v)) if not isinstance(v, str) else v for v in line) + "\n" for line in lines)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        out = [json.loads(row) for row in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384)
COLUMNS = (1, 25, 31, 373, 8185, 522304)


def test_pads_and_record_bytes(ask):
    assert ask([("pads",)])[0] == {"kind": "pads", "args": [], "chunk_pad": K.CHUNK_PAD, "band_pad": K.BAND_PAD, "max_bands": 4}
    sets = [(n, C) for n in SIZES for C in COLUMNS]
    for (n, C), w in zip(sets, ask([("f32", n, C) for n, C in sets])):
        assert w["per_stream"] == K.f32_record_bytes(n, C), (n, C)
    for (n, C), w in zip(sets, ask([("exact", n, C) for n, C in sets])):
        assert (w["q"], w["key"], w["per_stream"]) == K.exact_record_bytes(n, C), (n, C)
    # the table of the issue that the old test was measured against: 70 x 8196 x 12 bytes
    assert K.exact_record_bytes(16384, 70)[2] == 70 * 8196 * 12 and K.f32_record_bytes(4096, 25) == 25 * 2050 * 8


def test_first_chunk_and_the_halvings(ask):
    MiB = 1 << 20
    sets = []
    # (64 bytes: one index column of 64 rows, the least an entry asks for.  first_chunk narrows budget / per_stream to int before
    # its clamp: at 64 bytes the largest cap gives 2^27, far from a wrap)
    for per in (64, 62 * 1024, 384000, MiB - 1, MiB, MiB + 1, 6 * MiB + 12345, 300 * MiB, 5 << 30):
        for S in (1, 2, 5, 9, 64, 65535):
            for budget in (-1, 0, 1, 2, 6, 64, 4096):
                sets.append((0, 0, per, K.CHUNK_PAD, 4 << 30, S, budget))
    # the unbudgeted rule: a quarter of free + held, floor 256 MiB, cap
    for free, have in ((0, 0), (100 * MiB, 0), (2 << 30, 1 << 30), (280 << 30, 0), (1 << 30, 3 * MiB)):
        for cap in (4 << 30, 8 << 30):
            sets.append((free, have, 6 * MiB, 0, cap, 4000, -1))
    for a, w in zip(sets, ask([("chunk", *a) for a in sets])):
        free, have, per, extra, cap, S, budget = a
        chunk = K.first_chunk(None if budget < 0 else budget, per, S, free, have, cap)
        assert w["chunk"] == chunk and w["bytes"] == per * chunk + extra, (a, w)
        assert [h[0] for h in w["halvings"]] == K.halvings(chunk) and all(h[1] == per * h[0] + extra for h in w["halvings"])
        assert 1 <= chunk <= S
    assert K.chunks(1, 384000, 5) == (2, 2, 1) and K.chunks(0, 384000, 5) == (1,) * 5 and K.chunks(None, 384000, 5) == (5,)
    assert K.chunks(64, 70 * 8196 * 12, 5) == (5,)          # the old records test: one chunk
    assert K.halvings(5) == [3, 2, 1] and K.halvings(1) == []


def test_second_array_offset(ask):
    sets = [(first, chunk) for first in (0, 1, 255, 256, 257, 25 * 8196 * 8, 75 * 1024 * 4, (1 << 32) + 3) for chunk in (1, 2, 3, 5, 64)]
    for (first, chunk), w in zip(sets, ask([("second", first, chunk) for first, chunk in sets])):
        assert w["offset"] == K.second_array_offset(first, chunk) >= first * chunk and w["offset"] % 256 == 0


def _band_line(n, splits, hop, rows, C, post, chunk):
    return ("band", len(n), *n, *splits, hop, rows, C, int(post), chunk)


def test_band_layout(ask):
    sets = []
    for n, hop, splits in (*G.LADDERS.values(), ((16384, 4096, 1024), 256, (368, 668)), ((16384, 4096), 512, (368,)), ((2048, 1024), 512, (64,))):
        for C in (1, 25, 58, 85, 449):
            for post in (0, 1):
                for chunk in (1, 2, 5):
                    sets.append((n, splits, hop, 1024 if n[0] > 2048 else 128, C, post, chunk))
    for a, w in zip(sets, ask([_band_line(*a) for a in sets])):
        n, splits, hop, rows, C, post, chunk = a
        planes = K.band_planes(n, splits, hop, C, rows, post)
        assert w["planes"][:len(planes)] == planes and w["per_stream"] == sum(planes) == K.band_bytes(n, splits, hop, C, rows, post), a
        off = K.band_offsets(planes, chunk)
        assert w["offsets"] == off, a
        assert w["chunk_bytes"] == off[-1] + planes[-1] * chunk <= w["per_stream"] * chunk + K.BAND_PAD, a


def test_every_gpu_case_meets_the_budget_rule_and_the_headers(ask):
    """For each case of tests/test_gpu_chunks.py: an integer budget holds 2.25 .. 2.75 streams of the outermost workspace, so five
    streams run as (2, 2, 1) - and still do when that workspace's per-stream size drifts by 10 % either way; budget 0 gives one
    stream per chunk.  Every workspace on the case's path that a header sizes has the header's bytes."""
    assert len(G.CASES) >= 40
    lines, want = [], []
    for key, (c, _) in G.CASES.items():
        columns, b = K.columns_and_budget(c)
        assert columns >= 25 and b >= 1, key
        path = K.path(c, columns)
        per = path[0][1]
        assert 2.25 <= (b << 20) / per <= 2.75, key
        for drift in (0.9, 1.0, 1.1):
            assert K.chunks(b, int(per * drift), G.S) == (2, 2, 1), (key, drift)
        assert K.chunks(0, per, G.S) == (1,) * 5 and K.chunks(None, per, G.S) == (5,), key
        assert K.outer_chunks(c, columns, b, G.S) == (2, 2, 1)
        text = K.expected(c, columns, b, G.S)
        assert len(text) == len(path) and "(2, 2, 1)" in text[0], key
        R = c.get("rows", 1024)
        n0, hop = G._n0_hop(c)
        for name, nbytes in path:
            if name.startswith("d_hist"):
                n = int(name.rstrip(")").split("= ")[1])
                lines.append(("exact" if c["exact"] else "f32", n, columns + (n0 - n) // hop))
                want.append((key, name, nbytes))
            elif name.startswith("d_mres (multi-band)"):
                sizes, hop, splits = c["shape"]
                lines.append(_band_line(sizes, splits, hop, R, columns, bool(c.get("display")), 2))
                want.append((key, name, nbytes))
            elif name.startswith("d_mres (two-band)"):   # K = 2 of the multi-band layout has the two-band batch's planes
                n_low, n_high, hop, split = c["shape"]
                lines.append(_band_line((n_low, n_high), (split,), hop, R, columns, bool(c.get("display")), 2))
                want.append((key, name, nbytes))
            else:
                assert name.startswith("d_full"), name
    assert len(lines) >= 30
    for (key, name, nbytes), w in zip(want, ask(lines)):
        assert w["per_stream"] == nbytes, (key, name, w)
