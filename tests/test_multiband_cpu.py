"""CPU: the multi-band batch's pure functions and argument checks through ctypes (no engine, no device), and the reference
composition (tests/multiband_ref.py) on the bit model: for two bands it is tests/multires_ref.py's, and a click lands in the column
the shared grid gives it in every band."""
import ctypes as C

import numpy as np
import pytest

import emspec
import multiband_ref as B
import multires_ref as M
from emspec import synth


@pytest.mark.parametrize("n,hop,shifts", [
    ((16384, 4096, 1024), 256, (0, 24, 30)),
    ((16384, 8192, 4096, 2048), 128, (0, 32, 48, 56)),
    ((8192, 2048, 1024), 512, (0, 6, 7)),
    ((16384, 4096), 256, (0, 24)),
    ((4096, 1024), 128, (0, 12)),          # sizes the two-band entry does not take
])
def test_shifts_and_columns_of_accepted_shapes(n, hop, shifts):
    assert emspec.multiband_shifts(n, hop) == shifts == tuple(B.shifts(n, hop))
    L = 1 << 22
    Cm = emspec.multiband_columns(L, n, hop)
    assert Cm == emspec.num_columns(L, n[0], hop)
    # band k's own batch has exactly 2 shift[k] more columns: every composed column has its column c + shift[k]
    assert [emspec.num_columns(L, v, hop) for v in n] == [Cm + 2 * d for d in shifts]
    assert emspec.multiband_columns(n[0] - 1, n, hop) == 0
    # shifts_out may be NULL
    arr = (C.c_int32 * len(n))(*n)
    assert emspec.load().emspec_multiband_shifts(len(n), arr, hop, None) == 0


def test_two_band_shapes_agree_with_the_two_band_functions():
    for n_low, n_high, hop in ((16384, 4096, 256), (8192, 2048, 128), (16384, 1024, 512), (8192, 4096, 64)):
        assert emspec.multiband_shifts((n_low, n_high), hop) == (0, emspec.multires_shift(n_low, n_high, hop))
        assert emspec.multiband_columns(1 << 20, (n_low, n_high), hop) == emspec.multires_columns(1 << 20, n_low, n_high, hop)


@pytest.mark.parametrize("n,hop", [
    ((16384,), 256),                           # K = 1
    ((16384, 8192, 4096, 2048, 1024), 128),    # K = 5
    ((4096, 16384, 1024), 256),                # not decreasing
    ((16384, 4096, 4096), 256),
    ((16384, 4096, 512), 256),                 # a size of 512
    ((16384, 4096, 2048), 1000),               # shifts 6.144 and 7.168
    ((16384, 4096, 1024), 2048),               # hop above n[K-1]
    ((16384, 4096, 1024), 0),
])
def test_rejected_shapes(n, hop):
    assert emspec.multiband_shifts(n, hop) is None
    assert emspec.multiband_columns(1 << 22, n, hop) == -1


def test_null_arguments_are_invalid():
    lib = emspec.load()
    assert lib.emspec_multiband_shifts(3, None, 256, None) == -1
    assert lib.emspec_multiband_columns(1 << 20, 3, None, 256) == -1
    pcm = np.zeros(1 << 15, np.float32)
    n = (C.c_int32 * 3)(16384, 4096, 1024)
    split = (C.c_int32 * 2)(368, 668)
    out = emspec.Out(None, None, None)
    assert lib.emspec_batch_multiband(None, C.c_void_p(pcm.ctypes.data), 1, pcm.size, 3, n, split, 256, 1,
                                      C.byref(out)) == emspec.ERR_INVALID_ARG
    assert lib.emspec_batch_multiband_device(None, C.c_void_p(pcm.ctypes.data), 1, pcm.size, 3, n, split, 256, 1,
                                             None, None, None, None) == emspec.ERR_INVALID_ARG


def test_split_rows_of_the_ladders_on_the_default_axis():
    e = M.default_edges_hz()
    assert [M.split_row_for_hz(e, hz) for hz in (250.0, 2000.0)] == [368, 668]
    assert [M.split_row_for_hz(e, hz) for hz in (120.0, 500.0, 2000.0)] == [260, 468, 668]
    assert B.bands((260, 468, 668), 1024) == [(0, 260), (260, 468), (468, 668), (668, 1024)]


def test_reference_for_two_bands_is_the_two_band_reference():
    n_low, n_high, hop, split = 8192, 2048, 128, 368
    pcm = synth.streams(2, 1 << 14)
    for exact in (True, False):
        a = B.compose(pcm, (n_low, n_high), (split,), hop, True, exact=exact)
        b = M.compose(pcm, n_low, n_high, hop, split, True, exact=exact)
        for k in ("db", "rgba", "index"):
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (exact, k)


def test_reference_click_lands_in_the_same_column_in_every_band():
    """A click at sample t0 = c0 * hop + n[0] / 2 is column c0's centre: after the stitch (band k shifted by shift[k] columns)
    the reassigned click sits in column c0 in every band's rows."""
    n, hop, split, L = (8192, 2048, 1024), 512, (368, 668), 1 << 15
    C0 = (L - n[0]) // hop + 1
    c0 = C0 // 2 + 3
    pcm = np.zeros((1, L), np.float32)
    pcm[0, c0 * hop + n[0] // 2] = 1.0
    img = B.compose(pcm, n, split, hop, reassign=True, exact=True, want=("db",))["db"][0]
    assert img.shape == (C0, 1024)
    p = 10.0 ** (img.astype(np.float64) / 10.0)
    for lo, hi in B.bands(split, 1024):
        assert int(np.argmax(p[:, lo:hi].sum(axis=1))) == c0, (lo, hi)
