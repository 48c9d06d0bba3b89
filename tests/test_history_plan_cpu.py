"""CPU: the arithmetic of the live history (em-spec_amd/csrc/emspec_history_plan.h) without a GPU, pinned to
the numpy model tests/history_ref.py: the slot of a column, the range a ring holds after a launch, which of a launch's columns
are stored when it emits more than W (and that no slot is written twice in one launch), whether a view fits, and the columns
its groups read - through the slot runs across the wrap and through the kernel's incremental slot.

tests/cdriver/history_plan_driver.cpp is a program of its own that includes only that header and models what the store and
view kernels' workgroups do to a ring of exactly W entries, built with the host compiler under ASan and UBSan (nothing is
preloaded, nothing is loaded into Python under a sanitizer)."""
import json
import os
import subprocess

import numpy as np
import pytest

import history_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = tuple(range(1, 10)) + (64,)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("history_plan")
    exe = str(tmp / "history_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "history_plan_driver.cpp"), "-o", exe])
    count = [0]

    def run(lines):
        count[0] += 1
        path = tmp / ("in%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (lines[:3], r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)
    return run


def model_launch(ring, count):
    """Feed the model `count` columns whose every cell is the column's number; -> the columns it stored."""
    before = ring.end
    ring.launch(np.repeat(np.arange(before, before + count, dtype=np.float32)[:, None], ring.rows, axis=1))
    return sorted(c for c in ring.holds if c >= before)


def test_launches_store_the_last_w_columns_each_in_its_own_slot(driver):
    """Every W in 1 .. 9 and 64, from several fill states, launches of 0 .. 2 W + 1 columns: the stored columns, the ring's
    content, the held range, and at most one write per slot and launch."""
    lines, expect = [], []
    for W in WIDTHS:
        for lead in (0, 1, W - 1, W + 3):
            for count in range(0, 2 * W + 2):
                ring = H.Ring(W, 1)
                lines.append("ring %d" % W)
                expect.append(None)
                if lead:
                    lines.append("launch %d" % lead)
                    model_launch(ring, lead)
                    expect.append(None)
                lines.append("launch %d" % count)
                stored = model_launch(ring, count)
                expect.append((W, lead, count, stored, list(ring.holds), ring.held()))
    out = driver(lines)
    assert len(out) == len(expect)
    checked = 0
    for got, want in zip(out, expect):
        if want is None:
            continue
        W, lead, count, stored, holds, (end, first) = want
        key = (W, lead, count)
        assert sorted(got["stored"]) == stored and len(stored) == min(count, W), key
        assert got["ring"] == holds, key
        assert (got["end"], got["first"]) == (end, first) == (lead + count, max(0, lead + count - W)), key
        assert got["most_writes"] == (1 if count else 0), key
        assert got["keep_from"] == lead + max(0, count - W), key
        # what the header promises: after any call the ring holds exactly [max(0, end - W), end)
        assert sorted(c for c in got["ring"] if c >= 0) == list(range(first, end)), key
        checked += 1
    assert checked == sum(4 * (2 * W + 2) for W in WIDTHS)


def view_cases(W, end):
    """Every (first, f, groups) that fits a ring of W after `end` columns, and the nearest that do not."""
    first_held = max(0, end - W)
    fit, unfit = [], []
    for first in range(first_held, end):
        for f in range(1, W + 2):
            most = -(-(end - first) // f)
            fit += [(first, f, g) for g in range(1, most + 1)]
            unfit.append((first, f, most + 1))
    for f in (1, 2, W):
        unfit += [(first_held - 1, f, 1), (end, f, 1), (end + 1, f, 1), (first_held, f, 0), (first_held, f, -1)]
    unfit += [(first_held, 0, 1), (first_held, -1, 1), (first_held, 65537, 1)]
    return fit, unfit


@pytest.mark.parametrize("W", WIDTHS)
def test_views_fit_and_read_their_columns_across_the_wrap(driver, W):
    """Every (first, f, groups) that fits, at fill states before, at and after the wrap: each group reads exactly its columns,
    in order, through the slot runs and through the incremental slot; the nearest views that do not fit are refused."""
    ends = (1, W - 1, W, W + 1, 2 * W + 3) if W < 64 else (W - 1, 2 * W + 3)
    for end in sorted({e for e in ends if e > 0}):
        ring = H.Ring(W, 1)
        model_launch(ring, min(end, 3))
        if end > 3:
            model_launch(ring, end - 3)
        lines = ["ring %d" % W, "launch %d" % min(end, 3)] + (["launch %d" % (end - 3)] if end > 3 else [])
        fit, unfit = view_cases(W, end)
        lines += ["view %d %d %d" % v for v in fit + unfit]
        out = driver(lines)[len(lines) - len(fit) - len(unfit):]
        for (first, f, groups), got in zip(fit, out):
            key = (W, end, first, f, groups)
            assert ring.fits(first, f, groups) and got["rc"] == 0 and len(got["groups"]) == groups, key
            for g, grp in enumerate(got["groups"]):
                c0 = first + g * f
                c1 = min(c0 + f, end)
                want = list(range(c0, c1))
                assert grp["c"] == [c0, c1] and grp["by_runs"] == want and grp["by_walk"] == want, (key, g, grp)
                slot0, n0, n1 = grp["runs"]
                assert slot0 == c0 % W and n0 >= 1 and n1 >= 0 and n0 + n1 == c1 - c0 and slot0 + n0 <= W and n1 <= slot0, (key, g, grp)
                assert (n1 > 0) == (c0 % W + (c1 - c0) > W), (key, g, grp)
            # the model reads the same columns through its own slots
            assert np.array_equal(ring.view_db(first, f, groups)[:, 0],
                                  np.array([max(range(first + g * f, min(first + (g + 1) * f, end))) for g in range(groups)], np.float32)), key
        for (first, f, groups), got in zip(unfit, out[len(fit):]):
            assert not ring.fits(first, f, groups) and got["rc"] != 0 and got["groups"] == [], (W, end, first, f, groups, got["rc"])


def test_ring_bytes_and_limits(driver):
    out = driver(["ring 1", "bytes 64 2048 1024", "bytes 3 5 68", "bytes 65535 1048576 4096"])
    assert out[1]["bytes"] == 64 * 2048 * 1024 * 4 and out[1]["cells"] == 64 * 2048 * 1024
    assert out[2]["bytes"] == 3 * 5 * 68 * 4
    assert out[3]["bytes"] == 65535 * 1048576 * 4096 * 4            # (no 32-bit product anywhere)
    hdr = open(os.path.join(ROOT, "em-spec_amd", "csrc", "emspec_history_plan.h")).read()
    assert "kHistoryMaxColumns = 1 << 20" in hdr and "kHistoryMaxFactor = 65536" in hdr


def test_model_view_is_the_time_reduction_of_the_stored_columns():
    """history_ref itself: a view's dB is overview_ref.reduce_db of the held columns, the index the law on dB + shift."""
    import overview_ref as V
    import post_ref as P
    rng = np.random.default_rng(5)
    cols = (rng.random((23, 8)) * 90 - 100).astype(np.float32)
    h = H.History(1, 5, 8)
    for a, b in ((0, 1), (1, 4), (4, 16), (16, 23)):
        h.launch([cols[a:b]])
    assert h.held(0) == (23, 18)
    for f in (1, 2, 3, 5, 7):
        for first in range(18, 23):
            groups = -(-(23 - first) // f)
            v = h.view(first, f, groups, map=(-3.0, 70.0, -75.0, 6.0))
            assert np.array_equal(v["db"][0].view(np.uint32), V.reduce_db(cols[None, first:23], f)[0].view(np.uint32))
            assert np.array_equal(v["index"], P.cell_index_f32((v["db"] + np.float32(6.0)).astype(np.float32), -3.0, 70.0, -75.0))
    with pytest.raises(AssertionError):
        h.view(17, 1, 1)
    with pytest.raises(AssertionError):
        h.view(22, 1, 2)
