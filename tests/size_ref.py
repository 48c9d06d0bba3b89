"""Inputs and column choices for the size tests (tests/test_gpu_sizes.py): batches of up to 4.4e9 samples that never exist on
the host whole.  The host keeps a small base; the batch is built from it on the device with torch, and any slice of any stream
is regenerated here, bit for bit, without materialising the stream.  tests/test_size_ref.py checks the two against each other.

Many-streams batch [S][L] from a base [B][L] (emspec.synth.streams):
    stream s = roll(base[s % B], s * prime) * gain(s),   gain(s) = 0.5 + 0.125 * ((7 s) mod 5)
    (roll as numpy / torch: out[i] = in[(i - s * prime) mod L]; the five gains are exact in binary32, so the product is one
    binary32 rounding wherever it is computed)

One long stream [L] from a base [P] (P a multiple of 2^20):
    x[i] = base[i mod P] * lgain(i),   lgain(i) = 0.5 + ((i >> 20) mod 17) / 32
    (a gain that steps every 2^20 samples through 17 values exact in binary32: period 17 * 2^20 samples, coprime with the
    base's period in blocks, so no two stretches of the stream repeat within 17 * P samples)
"""
import numpy as np

PRIME = 1237
LBLOCK = 20          # log2 of the long stream's gain step


def gain(s):
    return np.float32(0.5 + 0.125 * ((7 * int(s)) % 5))


def stream_slice(base, s, a, b, prime=PRIME):
    """Samples [a, b) of stream s of the many-streams batch, float32, on the host."""
    B, L = base.shape
    assert 0 <= a <= b <= L
    i = (np.arange(a, b, dtype=np.int64) - int(s) * prime) % L
    return (base[s % B][i] * gain(s)).astype(np.float32)


def build_batch(base_t, S, prime=PRIME, rows=None):
    """The batch [S][L] (or the streams listed in `rows`) as a torch tensor on base_t's device; base_t: float32 [B][L]."""
    import torch
    B, L = base_t.shape
    rows = list(range(S)) if rows is None else list(rows)
    x = torch.empty((len(rows), L), dtype=torch.float32, device=base_t.device)
    for k, s in enumerate(rows):
        sh = (s * prime) % L
        g = float(gain(s))
        torch.mul(base_t[s % B][:L - sh], g, out=x[k, sh:])
        if sh:
            torch.mul(base_t[s % B][L - sh:], g, out=x[k, :sh])
    return x


def lgain(i):
    i = np.asarray(i, np.int64)
    return (0.5 + ((i >> LBLOCK) % 17) / 32.0).astype(np.float32)


def long_slice(base, a, b):
    """Samples [a, b) of the long stream, float32, on the host; base: float32 [P]."""
    P = base.shape[0]
    i = np.arange(a, b, dtype=np.int64)
    return (base[i % P] * lgain(i)).astype(np.float32)


def build_long(base_t, L, S=1, out=None, first=0):
    """S consecutive windows of L samples of the long stream, [S][L] on base_t's device: row k holds samples
    [first + k L, first + (k + 1) L).  base_t: float32 [P]."""
    import torch
    P = base_t.shape[0]
    blk = 1 << LBLOCK
    assert P % blk == 0
    x = out if out is not None else torch.empty((S, L), dtype=torch.float32, device=base_t.device)
    flat = x.view(-1)
    total = S * L
    pos = 0
    while pos < total:                      # block by block of the gain (the first and last may be partial)
        i = first + pos
        take = min(blk - i % blk, total - pos)
        # whole periods of 17 * P samples would allow bigger steps; a block is 4 MB and the loop a few thousand launches
        torch.mul(base_t[i % P:i % P + take], float(lgain(i)), out=flat[pos:pos + take])
        pos += take
    return x


# ---- which columns to check ---------------------------------------------------------------------------------------------

def boundaries(S, Cn, R, itemsize):
    """The 32-bit boundaries inside an output array [S][Cn][R] of `itemsize` bytes per cell: {name: cell offset} for the cell
    offsets 2^31 and 2^32 and the byte offsets 2^32, 2^33, 2^34 that lie strictly inside the array."""
    total = S * Cn * R
    out = {}
    for name, cell in (("cell 2^31", 1 << 31), ("cell 2^32", 1 << 32), ("byte 2^32", (1 << 32) // itemsize),
                       ("byte 2^33", (1 << 33) // itemsize), ("byte 2^34", (1 << 34) // itemsize)):
        if 0 < cell < total:
            out[name] = cell
    return out


def cell_to_column(cell, Cn, R):
    lin = cell // R
    return int(lin // Cn), int(lin % Cn)


def segment_lengths(S, Cn, cus=256, seg_min=16):
    """Candidate segment lengths of the FAST fused launchers' exclusive-device plan (launch_fused: r = 1..4 rounds of `cus`
    workgroups), rounded up to even as the launcher does; the tests put columns on both sides of the first boundary of each.
    This is a model, not the launcher: it assumes 256 compute units and the smallest floor (16 columns; the launcher's is 2 D or
    4 D), and it says nothing about the EXACT kernels' plans or the record paths' scatter tiles.  Where it misses, those two
    columns are two more ordinary columns; the seams themselves are covered by the whole-stream comparison, whose one-stream
    launch is cut into different segments, so a column wrong at a seam of either launch differs there."""
    out = set()
    for r in range(1, 5):
        ns = max(1, r * cus // S)
        ns = min(ns, max(1, -(-Cn // seg_min)))
        sl = -(-Cn // ns)
        sl = (max(sl, seg_min) + 1) & ~1
        if sl < Cn:
            out.add(sl)
    return sorted(out)


def chosen_columns(S, Cn, R, itemsizes, seed, nrandom=8):
    """(stream, column) pairs of a case: the column holding each crossed boundary and its two neighbours (in linear column
    order, so a neighbour may be the previous stream's last column), the first and last column of the first and last stream,
    both sides of the candidate segment boundaries in the last stream (which lies past every boundary), and `nrandom` seeded
    picks past the lowest boundary.  Returns (pairs, {boundary name: (stream, column)})."""
    rng = np.random.default_rng(seed)
    crossed = {}
    for it in itemsizes:
        for name, cell in boundaries(S, Cn, R, it).items():
            crossed[f"{name} of a {it}-byte array"] = cell
    pairs = []
    where = {}
    for name, cell in crossed.items():
        lin = cell // R
        where[name] = cell_to_column(cell, Cn, R)
        for d in (-1, 0, 1):
            if 0 <= lin + d < S * Cn:
                pairs.append(((lin + d) // Cn, (lin + d) % Cn))
    pairs += [(0, 0), (0, Cn - 1), (S - 1, 0), (S - 1, Cn - 1)]
    for sl in segment_lengths(S, Cn):
        pairs += [(S - 1, sl - 1), (S - 1, sl)]
    if crossed:
        lo = min(crossed.values()) // R
        for _ in range(nrandom):
            lin = int(rng.integers(lo + 1, S * Cn))
            pairs.append((lin // Cn, lin % Cn))
    seen, uniq = set(), []
    for p in pairs:
        p = (int(p[0]), int(p[1]))
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq, where
