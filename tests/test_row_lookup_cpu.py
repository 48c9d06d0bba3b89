"""CPU: the decision of the FAST kernels' hinted row lookup - one compare against the nearest edge, one table read per bin
(em-spec_amd/csrc/emspec_row_hint.h: row_hint_offset, row_hint, row_from_hint, the functions HintLookup calls on the device) -
equals the binary search of the float32 table, without a GPU.

tests/cdriver/row_lookup_driver.cpp is a program of its own that includes only that header and emspec_tables.h, built with the
host compiler under ASan and UBSan (nothing is preloaded, nothing is loaded into Python under a sanitizer):

    g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
        tests/cdriver/row_lookup_driver.cpp -o row_lookup_driver

The table is read in a heap block of exactly rows + 1 floats, so a hint that left the table would be ASan's to report.  Every run
must exit with status 0 and an empty stderr.

hint_rows_ok bounds the hint's own error below a quarter of a row; one compare decides while the error stays below half a row.
Each probe value therefore runs with the hint displaced by -1/4, 0 and +1/4 row (the rest of the budget, spent on purpose) and
with the logarithm, correctly rounded here, moved by -1, 0 and +1 float32 ulp (v_log_f32 is documented to 1 ulp): nine lookups per
value, each of which must give bisection's row."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DEFAULT = (48000.0, 20.0, 24000.0)
# (n, rows) on the default axis: every FFT size with a fused kernel at 1024 rows, and the headline size at a small row count and
# at one that is no power of two
AXES = [(1024, 1024), (4096, 1024), (16384, 1024), (4096, 64), (4096, 1000)]
# the densest axis hint_rows_ok still admits, found by the driver by bisection on the predicate: 4096 rows up to 24 kHz at 48 kHz
DENSEST = [(1024, 4096), (4096, 4096), (16384, 4096)]


def f32(x):
    return "%08x" % int(np.array(x, F).view(np.uint32))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("row_lookup") / "row_lookup_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "row_lookup_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (args, r.returncode, r.stderr[-2000:])
        return {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] if " " in ln else "" for ln in r.stdout.splitlines()}
    return run


def check_sweep(out, rows, what):
    values = (rows + 1) * 9 + rows + 12
    assert int(out["cases"]) == 9 * values, (what, out["cases"])
    assert "mismatch" not in out and int(out["mismatches"]) == 0, (what, out.get("mismatch"), out["mismatches"])
    assert int(out["range_bad"]) == 0, (what, out["range_bad"])       # (unsigned)row < R exactly for the in-range values
    # the sweep did reach all three outcomes: below the axis, on it, at or above its end
    assert int(out["below"]) >= 9 * 9 and int(out["above"]) >= 9 * 11 and int(out["in_range"]) >= 9 * (10 * rows - 8), (what, out)
    assert out["error32"] == "-", (what, out["error32"])


@pytest.mark.parametrize("n,rows", AXES)
def test_nearest_edge_equals_bisection(driver, n, rows):
    out = driver("sweep", n, rows, *map(f32, DEFAULT))
    assert int(out["hint_ok"]) == 1 and float(out["bound_ratio"]) < 0.25
    check_sweep(out, rows, (n, rows))


@pytest.mark.parametrize("n,rows", DENSEST)
def test_nearest_edge_equals_bisection_on_the_densest_hinted_axis(driver, n, rows):
    """The last float32 fmin the predicate admits: the hint's own error is at its bound there."""
    out = driver("densest", n, rows, f32(48000.0), f32(24000.0))
    assert int(out["hint_ok"]) == 1 and 0.999999 < float(out["bound_ratio"]) <= 1.0, out["bound_ratio"]
    check_sweep(out, rows, (n, rows, out["fmin"]))


@pytest.mark.parametrize("n,rows", [(4096, 1024), (4096, 1000)])
def test_driver_rows_equal_numpy_bisection(driver, n, rows):
    """The driver's reference is its own bisection; this ties the lookup's rows to numpy's on the table the driver printed."""
    out = driver("rows", n, rows, *map(f32, DEFAULT))
    eb = np.array([int(t, 16) for t in out["e32"].split()], np.uint32).view(F)
    kh = np.array([int(t, 16) for t in out["kh"].split()], np.uint32).view(F)
    got = np.array(out["row"].split(), np.int64)
    assert eb.size == rows + 1 and np.all(np.diff(eb) > 0) and eb[-1] == F(n / 2)
    want = np.where(np.isnan(kh), -1, np.searchsorted(eb, kh, side="right").astype(np.int64) - 1)
    assert np.array_equal(got, want)
    assert want.min() == -1 and want.max() == rows and np.isnan(kh).sum() == 1
