"""GPU: the hinted row lookup of the FAST kernels (one compare against the nearest edge, one LDS read per bin:
emspec_device.h: HintLookup, emspec_row_hint.h) inside every kernel family that uses it, on a signal made for it.

The lookup is per bin, so short inputs suffice: 2 streams of n + hop (2 D + 8) samples.  One shape per FAST family at 1024
rows - 4096/256, 4096/512, 4096/1024 (fused_pp), 4096/300 and 1024/256 (fused_small), 8192/512, 16384/512 - plus 64 and 1000
rows at 4096/256.  Stream 0 is a logarithmic sweep over the whole axis (every row is visited by a strong bin) plus steady
tones placed exactly on row edges (k-hat falls on either side of an edge from frame to frame); stream 1 is the same sweep
backwards plus tones on other edges.

The per-bin dump's (column, row) - and the power - must equal the float32 bit model's exactly, as tests/test_gpu_parity.py compares
them, and the batch output must agree with the oracle within 8.7e-4 dB (1e-4 relative on magnitude), the tolerance these shapes
have in tests/test_gpu_parity.py and tests/test_gpu_golden.py.  tests/test_row_lookup_cpu.py runs the decision itself on the CPU."""
import numpy as np
import pytest

import emspec
import oracle as O

pytestmark = pytest.mark.gpu

FS, FMIN, FMAX = 48000.0, 20.0, 24000.0
# (family, n, hop, rows)
CASES = [("fused_pp", 4096, 256, 1024), ("fused_pp", 4096, 512, 1024), ("fused_pp", 4096, 1024, 1024),
         ("fused_small", 4096, 300, 1024), ("fused_small", 1024, 256, 1024), ("fused_8192", 8192, 512, 1024),
         ("fused_16384", 16384, 512, 1024), ("fused_pp", 4096, 256, 64), ("fused_pp", 4096, 256, 1000)]


def edge_hz(r, rows):
    return FMIN * (FMAX / FMIN) ** (r / rows)


def signal(n, hop, rows):
    """float32 [2][n + hop (2 D + 8)]: a log sweep from below the axis to Nyquist (stream 1: downwards) plus six tones on row edges."""
    D = emspec.latency_columns(n, hop, True)
    L = n + hop * (2 * D + 8)
    t = np.arange(L, dtype=np.float64)
    lo, hi = 0.5 * FMIN, 0.4999 * FS
    k = np.log(hi / lo) / L
    up = 2.0 * np.pi * lo * (np.exp(k * t) - 1.0) / (k * FS)            # phase of a frequency lo * exp(k t)
    down = 2.0 * np.pi * hi * (1.0 - np.exp(-k * t)) / (k * FS)
    x = np.stack([0.4 * np.sin(up), 0.4 * np.sin(down)])
    for s, offset in ((0, 0), (1, rows // 13)):
        for i in range(6):
            r = (rows // 7) * (i + 1) + offset
            x[s] += 0.07 * np.sin(2.0 * np.pi * edge_hz(r, rows) * t / FS + i)
    return x.astype(np.float32)


@pytest.mark.parametrize("family,n,hop,rows", CASES, ids=[f"{n}-{hop}-{rows}" for _, n, hop, rows in CASES])
def test_rows_equal_the_bit_model_in_every_fast_family(family, n, hop, rows):
    D = emspec.latency_columns(n, hop, True)
    frames = 2 * D + 9
    pcm = signal(n, hop, rows)
    assert pcm.shape[1] == n + hop * (frames - 1)
    cfg = O.make_cfg(n, hop, True, rows=rows)
    with emspec.Engine(rows=rows) as e:
        assert e.fused(n, hop, True), family
        pw, col, row = e.parity_dump(pcm, n, hop, True, 0, frames)
        out = e.batch(pcm, n, hop, True, want=("db",))
    hit = set()
    for s in range(pcm.shape[0]):
        opw, ocol, orow = O.frames_f32(cfg, pcm[s], 0, frames)
        assert np.array_equal(col[s], ocol), f"column indices differ: {np.sum(col[s] != ocol)}"
        assert np.array_equal(row[s], orow), f"row indices differ: {np.sum(row[s] != orow)}"
        assert np.array_equal(pw[s], opw), f"power differs in {np.sum(pw[s] != opw)} bins"
        hit |= set(np.unique(orow[orow >= 0]).tolist())
        assert (orow < 0).any()
    # the signal did its work: the bins that landed cover the axis from its first rows to its last
    assert min(hit) < rows // 8 and max(hit) == rows - 1 and len(hit) > rows // 2, (min(hit), max(hit), len(hit))
    odb, _, _ = O.batch_f32(cfg, pcm, want=("db",))
    assert out["db"].shape == odb.shape == (2, frames, rows)
    assert np.max(np.abs(out["db"] - odb)) < 8.7e-4
