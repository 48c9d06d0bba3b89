"""Reference composition of the multi-resolution batch from the CPU bit models.

The composed image is DEFINED as a stitch of two single-resolution images on the same row table:
    image[s][c][r] = single(n_low)[s][c][r]           r <  split_row
    image[s][c][r] = single(n_high)[s][c + shift][r]  r >= split_row,   shift = (n_low - n_high) / (2 hop)
so the reference needs no oracle of its own: single(n) is oracle.batch_f32 (FAST) or oracle.batch_exact (EXACT) with the
engine's full edge table (oracle.set_custom_edges_hz for a custom axis).
"""
import numpy as np

import oracle as O


def shift(n_low, n_high, hop):
    assert (n_low - n_high) % (2 * hop) == 0
    return (n_low - n_high) // (2 * hop)


def single(n, hop, reassign, pcm, exact, edges_hz=None, want=("db", "rgba", "index")):
    """One single-resolution image of the bit model: {"db", "rgba", "index"} (entries not wanted are None)."""
    cfg = O.make_cfg(n, hop, reassign)
    if edges_hz is not None:
        O.set_custom_edges_hz(edges_hz)
    try:
        if exact:
            db, rgba, idx, _ = O.batch_exact(cfg, pcm, want=want)
        else:
            db, rgba, idx = O.batch_f32(cfg, pcm, want=want)
    finally:
        if edges_hz is not None:
            O.set_custom_edges_hz(None)
    return {"db": db, "rgba": rgba, "index": idx}


def stitch(low, high, split_row, d, C):
    """low [S][>=C][R...] of n_low, high [S][>=C + 2d][R...] of n_high -> the composed [S][C][R...]."""
    return np.ascontiguousarray(np.concatenate([low[:, :C, :split_row], high[:, d:d + C, split_row:]], axis=2))


def compose(pcm, n_low, n_high, hop, split_row, reassign=True, exact=True, edges_hz=None, want=("db", "rgba", "index")):
    """The composed image by the definition, from the bit model."""
    pcm = np.ascontiguousarray(pcm, np.float32)
    if pcm.ndim == 1:
        pcm = pcm[None]
    C = O.num_columns(pcm.shape[1], n_low, hop)
    d = shift(n_low, n_high, hop)
    lo = single(n_low, hop, reassign, pcm, exact, edges_hz, want)
    hi = single(n_high, hop, reassign, pcm, exact, edges_hz, want)
    return {k: (stitch(lo[k], hi[k], split_row, d, C) if lo[k] is not None else None) for k in ("db", "rgba", "index")}


def split_row_for_hz(edges_hz, hz):
    """The smallest admissible split row (multiple of 4 in [64, rows - 64]) whose lower edge is >= hz."""
    R = len(edges_hz) - 1
    for r in range(64, R - 63, 4):
        if edges_hz[r] >= np.float32(hz):
            return r
    raise ValueError(hz)


def default_edges_hz(rows=1024, fmin=20.0, fmax=24000.0):
    """The default log axis in Hz as float32 (what Engine.row_edges_hz() returns on a default engine, up to the last bit)."""
    return (fmin * (fmax / fmin) ** (np.arange(rows + 1) / rows)).astype(np.float32)
