"""Reference composition of the multi-band batch from the CPU bit models: tests/multires_ref.py's stitch
generalised to K bands.

The composed image is DEFINED as a stitch of K single-resolution images on the same row table:
    image[s][c][r] = single(n[k])[s][c + shift[k]][r]   lo_k <= r < hi_k,   shift[k] = (n[0] - n[k]) / (2 hop)
with lo_0 = 0, lo_k = split_rows[k - 1], hi_k = split_rows[k], hi_{K-1} = rows; single(n) is multires_ref.single.
"""
import numpy as np

import multires_ref as M
import oracle as O


def shifts(n, hop):
    assert all((n[0] - v) % (2 * hop) == 0 for v in n)
    return [(n[0] - v) // (2 * hop) for v in n]


def bands(split_rows, rows):
    """[(lo_k, hi_k)] of the K = len(split_rows) + 1 bands."""
    cuts = [0, *split_rows, rows]
    return list(zip(cuts[:-1], cuts[1:]))


def stitch(images, n, split_rows, hop, C):
    """images[k] [S][>= C + 2 shift[k]][R...] of n[k] -> the composed [S][C][R...]."""
    R = images[0].shape[2]
    parts = [img[:, d:d + C, lo:hi] for img, d, (lo, hi) in zip(images, shifts(n, hop), bands(split_rows, R))]
    return np.ascontiguousarray(np.concatenate(parts, axis=2))


def compose(pcm, n, split_rows, hop, reassign=True, exact=True, edges_hz=None, want=("db", "rgba", "index")):
    """The composed image by the definition, from the bit model."""
    pcm = np.ascontiguousarray(pcm, np.float32)
    if pcm.ndim == 1:
        pcm = pcm[None]
    assert 2 <= len(n) <= 4 and len(split_rows) == len(n) - 1
    C = O.num_columns(pcm.shape[1], n[0], hop)
    singles = [M.single(v, hop, reassign, pcm, exact, edges_hz, want) for v in n]
    return {k: (stitch([s[k] for s in singles], n, split_rows, hop, C) if singles[0][k] is not None else None)
            for k in ("db", "rgba", "index")}
