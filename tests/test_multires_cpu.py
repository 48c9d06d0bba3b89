"""CPU: the multi-resolution batch's pure functions and argument checks (no device needed), and the reference composition
(tests/multires_ref.py) on the bit model: a click lands where the definition's shared column grid puts it."""
import ctypes as C

import numpy as np
import pytest

import emspec
import multires_ref as M


@pytest.mark.parametrize("n_low,n_high,hop,shift", [
    (16384, 4096, 256, 24), (16384, 4096, 128, 48), (16384, 4096, 512, 12), (16384, 4096, 1024, 6),
    (8192, 2048, 128, 24), (8192, 2048, 256, 12), (16384, 1024, 512, 15), (8192, 4096, 64, 32),
])
def test_shift_and_columns_of_accepted_shapes(n_low, n_high, hop, shift):
    assert emspec.multires_shift(n_low, n_high, hop) == shift
    L = 1 << 22
    assert emspec.multires_columns(L, n_low, n_high, hop) == emspec.num_columns(L, n_low, hop)
    # the short FFT has exactly 2 shift more columns: every composed column has its high-band column c + shift
    assert emspec.num_columns(L, n_high, hop) == emspec.num_columns(L, n_low, hop) + 2 * shift
    assert emspec.multires_columns(n_low - 1, n_low, n_high, hop) == 0


@pytest.mark.parametrize("n_low,n_high,hop", [
    (16384, 2048, 1000),    # shift 7.168
    (16384, 4096, 3000),    # not an integer either
    (4096, 2048, 256),      # n_low = 4096
    (8192, 8192, 256),      # n_low <= n_high
    (4096, 8192, 256),
    (16384, 512, 256),      # n_high not in {1024, 2048, 4096}
    (32768, 4096, 256),     # n_low not in {8192, 16384}
    (16384, 4096, 0),       # hop < 1
    (16384, 1024, 2048),    # hop > n_high
])
def test_rejected_shapes(n_low, n_high, hop):
    assert emspec.multires_shift(n_low, n_high, hop) == -1
    assert emspec.multires_columns(1 << 22, n_low, n_high, hop) == -1


def test_null_engine_is_an_invalid_argument():
    lib = emspec.load()
    pcm = np.zeros(1 << 15, np.float32)
    out = emspec.Out(None, None, None)
    assert lib.emspec_batch_multires(None, C.c_void_p(pcm.ctypes.data), 1, pcm.size, 16384, 4096, 256, 368, 1,
                                     C.byref(out)) == emspec.ERR_INVALID_ARG
    assert lib.emspec_batch_multires_device(None, C.c_void_p(pcm.ctypes.data), 1, pcm.size, 16384, 4096, 256, 368, 1,
                                            None, None, None, None) == emspec.ERR_INVALID_ARG


def test_split_row_for_250_hz_on_the_default_axis():
    e = M.default_edges_hz()
    assert M.split_row_for_hz(e, 250.0) == 368
    assert e[364] < 250.0 <= e[368]          # (the first multiple of 4 whose lower edge is >= 250 Hz)


@pytest.mark.parametrize("n_low,n_high,hop", [(16384, 4096, 256), (8192, 2048, 128)])
def test_reference_click_lands_in_the_same_column_in_both_bands(n_low, n_high, hop):
    """A click at sample t0 = c0 * hop + n_low / 2 is column c0's centre: after the stitch (the high band shifted by
    `shift` columns) the reassigned click sits in column c0 in the low rows and in the high rows alike."""
    L = 1 << 16
    C0 = (L - n_low) // hop + 1
    c0 = C0 // 2 + 3
    pcm = np.zeros((1, L), np.float32)
    pcm[0, c0 * hop + n_low // 2] = 1.0
    split = M.split_row_for_hz(M.default_edges_hz(), 250.0)
    img = M.compose(pcm, n_low, n_high, hop, split, reassign=True, exact=True, want=("db",))["db"][0]
    assert img.shape == (C0, 1024)
    p = 10.0 ** (img.astype(np.float64) / 10.0)
    assert int(np.argmax(p[:, :split].sum(axis=1))) == c0
    assert int(np.argmax(p[:, split:].sum(axis=1))) == c0
