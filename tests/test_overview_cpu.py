"""CPU: the time reduction's numpy restatement (tests/overview_ref.py) against a plain double loop over the definition
(DESIGN.md §3.10), emspec_reduced_columns through ctypes, and the three new names in the header, the linker map and the
ctypes binding."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import emspec
import overview_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("emspec_set_time_reduce", "emspec_time_reduce", "emspec_reduced_columns")


def loop_reduce(db, index, lut, f):
    """The definition, cell by cell."""
    S, Cn, R = index.shape
    Cr = (Cn + f - 1) // f
    odb = np.empty((S, Cr, R), np.float32)
    oidx = np.empty((S, Cr, R), np.uint8)
    for s in range(S):
        for g in range(Cr):
            for r in range(R):
                m = db[s, g * f, r]
                i = index[s, g * f, r]
                for c in range(g * f + 1, min((g + 1) * f, Cn)):
                    if db[s, c, r] > m:
                        m = db[s, c, r]
                    if index[s, c, r] > i:
                        i = index[s, c, r]
                odb[s, g, r] = m
                oidx[s, g, r] = i
    return odb, lut[oidx], oidx


@pytest.mark.parametrize("Cn,f", [(12, 1), (12, 2), (12, 3), (13, 4), (17, 16), (5, 7), (1, 3), (9, 9), (10, 65536)])
def test_restatement_equals_the_double_loop(Cn, f):
    rng = np.random.default_rng(Cn * 1000 + f)
    S, R = 2, 8
    db = (rng.standard_normal((S, Cn, R)) * 20 - 40).astype(np.float32)
    db[rng.random(db.shape) < 0.1] = 0.0
    db[rng.random(db.shape) < 0.1] = -0.0
    db[0, 0, 0] = np.nan                       # at the head of a group: it holds
    if Cn > 1:
        db[1, Cn - 1, 3] = np.nan              # behind the head (or the head of the last group)
        db[0, 1, 5] = np.nan
    index = rng.integers(0, 256, (S, Cn, R), dtype=np.uint8)
    lut = rng.integers(0, 256, (256, 4), dtype=np.uint8)
    full = {"db": db, "index": index, "rgba": lut[index]}
    got = V.reduce(full, f, lut)
    wdb, wrgba, widx = loop_reduce(db, index, lut, f)
    assert got["db"].shape == (S, V.reduced_columns(Cn, f), R)
    assert np.array_equal(got["db"].view(np.uint32), wdb.view(np.uint32))      # NaNs and signed zeros bit for bit
    assert np.array_equal(got["index"], widx) and np.array_equal(got["rgba"], wrgba)
    if f == 1:
        assert np.array_equal(got["db"].view(np.uint32), db.view(np.uint32)) and np.array_equal(got["index"], index)


def test_a_nan_holds_only_at_the_head_of_its_group():
    db = np.array([[[np.nan], [1.0], [2.0], [3.0], [np.nan], [-5.0]]], np.float32)   # [1][6][1]
    got = V.reduce_db(db, 3)[0, :, 0]
    assert np.isnan(got[0]) and got[1] == 3.0
    got = V.reduce_db(db, 4)[0, :, 0]
    assert np.isnan(got[0]) and np.isnan(got[1])


def test_reduced_columns_through_ctypes():
    lib = emspec.load()
    for cols, f in [(0, 1), (1, 1), (16369, 1), (16369, 64), (16369, 16369), (16369, 65536), (12, 3), (13, 3), (675000, 338),
                    (1 << 40, 65536), ((1 << 62) + 1, 2)]:
        assert emspec.reduced_columns(cols, f) == V.reduced_columns(cols, f) == -(-cols // f), (cols, f)
    for cols, f in [(-1, 1), (10, 0), (10, -1), (10, 65537), (-5, 0)]:
        assert emspec.reduced_columns(cols, f) == -1, (cols, f)
    assert lib.emspec_time_reduce(None) == -1
    assert lib.emspec_set_time_reduce(None, 2) == emspec.ERR_INVALID_ARG


def test_header_map_and_binding_agree_on_the_new_names():
    header = open(os.path.join(ROOT, "include", "emspec.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {n: re.search(r"([a-z0-9_]+)\s+" + n + r"\s*\(([^)]*)\)\s*;", code) for n in NAMES}
    assert all(decl.values()), decl
    assert decl["emspec_set_time_reduce"].group(1) == "int" and "int32_t factor" in decl["emspec_set_time_reduce"].group(2)
    assert decl["emspec_time_reduce"].group(1) == "int32_t" and "const emspec_engine" in decl["emspec_time_reduce"].group(2)
    assert decl["emspec_reduced_columns"].group(1) == "int64_t" and \
        re.sub(r"\s+", " ", decl["emspec_reduced_columns"].group(2)) == "int64_t columns, int32_t factor"
    assert "#define EMSPEC_ABI_VERSION 2" in header                      # no struct changed
    # the linker map exports them (its global patterns) and nothing hides them first
    vmap = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "em-spec_amd", "csrc", "emspec.map")).read(), flags=re.S)
    globs = re.search(r"global:(.*?)local:", vmap, flags=re.S).group(1).replace(";", " ").split()
    for n in NAMES:
        assert any(fnmatch.fnmatchcase(n, g) for g in globs), (n, globs)
    # the binding lists them, types them, and both libraries export them
    assert set(NAMES) <= set(emspec.SYMBOLS) and tuple(emspec.REDUCE_SYMBOLS) == NAMES
    for diag in (False, True):
        lib = emspec.load(diag)
        for n in NAMES:
            assert hasattr(lib, n), (n, diag)
        assert lib.emspec_reduced_columns.restype is C.c_int64 and lib.emspec_time_reduce.restype is C.c_int32
        assert lib.emspec_reduced_columns.argtypes == [C.c_int64, C.c_int32]
        assert lib.emspec_set_time_reduce.argtypes == [C.c_void_p, C.c_int32]
    for name in ("set_time_reduce", "time_reduce"):
        assert hasattr(emspec.Engine, name)
