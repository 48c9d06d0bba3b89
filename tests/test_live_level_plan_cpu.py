"""CPU: the host arithmetic of the live level meters (em-spec_amd/csrc/emspec_live_plan.h: live_level_ring_bytes,
live_cross_ring_bytes, live_level_bytes, live_cross_bytes, live_cross_error) without a GPU - the rings' byte
counts, the capacity rule for pairs, the refusal of a stream count that is no multiple of `views`, and that every 24-byte and
16-byte record a scripted session writes at slot j % slots of a ring of exactly that many bytes stays in bounds, is found by
the column that needs it and is not overwritten before - and the two pure sums of the C ABI (emspec_level_sum,
emspec_cross_sum) against tests/level_ref.py.

tests/cdriver/live_level_plan_driver.cpp is a program of its own that includes only that header, built with the host compiler
under ASan and UBSan (nothing is preloaded, nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import emspec
import level_ref as LR
import live_ref as L
from test_live_overlay_plan_cpu import GEOMETRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("live_level_plan")
    exe = str(tmp / "live_level_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "live_level_plan_driver.cpp"), "-o", exe])
    count = [0]

    def run(lines):
        count[0] += 1
        path = tmp / ("in%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (lines[:3], r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)
    return run


def _open(S, n, hop, reassign, form, n_high, split, views):
    return "open %d %d %d %d %d %d %d %d" % (S, n, hop, reassign, form, n_high, split, views)


def test_ring_and_output_sizes(driver):
    for n, hop, reassign, n_high, split in GEOMETRIES:
        for form in (1, 2):
            for S in (1, 5, 64):
                g = L.geometry(S, n, hop, reassign, form, n_high, split)
                slots = g["D"] + g["mmax"]          # the envelope's ring, by the same argument
                for views in (1, 2, 5):
                    got = driver([_open(S, n, hop, reassign, form, n_high, split, views), "fits 1 1 1 1"])[0]
                    pairs = S // views if S % views == 0 else 0
                    assert got["slots"] == slots and got["level_ring"] == S * slots * 24, (S, n, hop, form)
                    assert got["pairs"] == pairs and got["cross_ring"] == pairs * slots * 16, (S, views)
                    assert got["level_out"] == S * 7 * 24 and got["cross_out"] == pairs * 7 * 16


def test_capacity_rule_for_pairs_and_streams_that_are_no_multiple(driver):
    # (S, views, cols, capacity) -> 0 fits, 1 too small, 2 no pairs
    cases = [(6, 2, 1, 3), (6, 2, 1, 2), (8, 4, 7, 14), (8, 4, 7, 13), (64, 2, 64, 2048), (64, 2, 64, 2047), (4, 1, 3, 12), (4, 1, 3, 11),
             (5, 2, 1, 100), (1, 2, 1, 100), (6, 4, 1, 100), (65535, 1, 2 ** 31, 65535 * 2 ** 31), (65535, 1, 2 ** 31, 65535 * 2 ** 31 - 1),
             (6, 2, 0, 0), (6, 2, 1, -1), (6, 0, 1, 100)]
    got = driver([_open(1, 1024, 256, 1, 1, 0, 0, 1)] + ["fits %d %d %d %d" % c for c in cases])
    for (S, views, cols, capacity), have in zip(cases, got):
        want = 2 if views < 1 or S % views else (0 if (S // views) * cols <= capacity and (capacity >= 0 or cols <= 0) else 1)
        assert have["refused"] == want, (S, views, cols, capacity)


def test_records_stay_in_bounds_over_scripted_sessions(driver):
    """Pushes of 1, hop, cap + 1 and 3 cap + 5 samples and a flush, per-frame sessions with a reset: every record is written and
    read inside rings of exactly the plan's bytes (ASan), none is lost or stale, and each emitted column reads one."""
    for n, hop, reassign, n_high, split in GEOMETRIES:
        for S, views in ((1, 1), (4, 2), (5, 1), (64, 2)):
            g = L.geometry(S, n, hop, reassign, 2, n_high, split)
            cap = g["cap"]
            ops = ["push 1", "push %d" % hop, "push %d" % (cap + 1), "push %d" % (3 * cap + 5), "push %d" % n] + ["flush"] * (g["D"] + 1)
            last = driver([_open(S, n, hop, reassign, 2, n_high, split, views)] + ops)[-1]
            assert last["stale"] == 0 and last["lost"] == 0, (n, hop, S, views, last)
            assert last["reads"] == sum(last["emitted"]) and last["writes"] == sum(last["fed"]) >= last["reads"] > S * g["D"], (n, hop, S)
            assert (last["own"] > 0) == (g["mmax"] > g["D"]), (n, hop, S)     # columns of a launch's own frames: only where one brings more than D
            if views == 1 and S > 1:    # a stream restarts: its records do, the others' stay
                more = ["reset 2", "push %d" % (n + 3 * hop), "push %d" % (2 * cap + 77), "flush"]
                last = driver([_open(S, n, hop, reassign, 2, n_high, split, views)] + ops[:5] + more)[-1]
                assert last["stale"] == 0 and last["lost"] == 0, (n, hop, S, last)
            if views > 1:
                assert driver([_open(S, n, hop, reassign, 2, n_high, split, views), "push %d" % n, "reset 1"])[-1]["refused"] == 1
        D = L.latency(n, hop, reassign)
        ops = ["frame"] * (D + 3) + ["reset 2", "frame", "frame"] + ["flush"] * (D + 1)
        last = driver([_open(5, n, hop, reassign, 1, n_high, split, 1)] + ops)[-1]
        assert last["stale"] == 0 and last["lost"] == 0 and last["reads"] > 0


# ---- emspec_level_sum / emspec_cross_sum: pure, no engine, no device ----
def _records():
    n, hop, frames = 1024, 256, 23
    rng = np.random.default_rng(7)
    pcm = (rng.standard_normal((4, n + hop * (frames - 1))) * 0.5).astype(np.float32)
    pcm[1, 3000] = np.nan
    pcm[2, 2000:2100] = 1.0          # k^2 = 2^48: the high limb counts
    pcm[3, 4000] = 1e9
    return LR.levels(pcm, n, hop), LR.crosses(pcm, 2, 0, 1, n, hop)


def test_sums_are_the_factor_law():
    lv, cr = _records()
    for rec, fn in ((lv, emspec.level_sum), (cr, emspec.cross_sum)):
        C_ = rec.shape[1]
        for f in (1, 2, 7, C_):
            want = LR.regroup(rec, f)
            for s in range(rec.shape[0]):
                for g in range(want.shape[1]):
                    got = fn(rec[s, g * f:(g + 1) * f])
                    assert got.tobytes() == want[s, g].tobytes(), (f, s, g)
        assert fn(rec[0, 3:4]).tobytes() == rec[0, 3].tobytes()          # a single record comes back unchanged
    assert lv["sq_hi"].max() > 0 and lv["odd"].sum() == 2 and cr["hi"].min() < 0


def test_sums_refuse_wraps_nulls_and_no_record():
    lib = emspec.load()
    top = 2 ** 64 - 1

    def refused(fn, recs, count=None, out=True):
        dtype = recs.dtype
        res = np.full((), 0x5A, np.uint8).repeat(dtype.itemsize).view(dtype)
        rc = fn(recs.ctypes.data if recs.size else None, recs.size if count is None else count, res.ctypes.data if out else None)
        assert rc == emspec.ERR_INVALID_ARG and len(lib.emspec_last_error(None)) > 20
        assert np.all(res.view(np.uint8) == 0x5A), "a refused sum wrote its output"

    one = np.zeros(2, LR.LEVEL)
    for field, a, b in (("sq_lo", top, 1), ("sq_hi", top, 1), ("odd", 2 ** 32 - 1, 1), ("sq_lo", 2 ** 63, 2 ** 63)):
        one[:] = 0
        one[field] = (a, b)
        refused(lib.emspec_level_sum, one)
        one[field][1] = b - 1                       # one less fits
        assert emspec.level_sum(one)[field] == a + b - 1
    x = np.zeros(2, LR.CROSS)
    for field, a, b in (("lo", top, 1), ("hi", 2 ** 63 - 1, 1), ("hi", -2 ** 63, -1)):
        x[:] = 0
        x[field] = (a, b)
        refused(lib.emspec_cross_sum, x)
        x[field][1] = 0
        assert emspec.cross_sum(x)[field] == a
    one[:] = 0
    x[:] = 0
    refused(lib.emspec_level_sum, one, count=0)
    refused(lib.emspec_level_sum, one, count=-1)
    refused(lib.emspec_cross_sum, x, count=0)
    refused(lib.emspec_level_sum, one, out=False)
    refused(lib.emspec_cross_sum, x, out=False)
    res = np.zeros((), LR.LEVEL)
    assert lib.emspec_level_sum(None, 1, res.ctypes.data) == emspec.ERR_INVALID_ARG
    assert lib.emspec_cross_sum(None, 1, res.ctypes.data) == emspec.ERR_INVALID_ARG
    with pytest.raises(emspec.EmspecError):
        emspec.level_sum(np.zeros(0, LR.LEVEL))
    # the peak is a maximum, not a sum
    one["peak"] = (5, 2 ** 32 - 1)
    assert emspec.level_sum(one)["peak"] == 2 ** 32 - 1
    assert C.sizeof(emspec.Level) == 24 and C.sizeof(emspec.Cross) == 16
