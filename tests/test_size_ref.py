"""tests/size_ref.py on the CPU: the slices it regenerates equal the full construction done with torch, bit for bit, and the
column chooser puts columns on every 32-bit boundary of a shape."""
import numpy as np
import pytest

import size_ref as Z

torch = pytest.importorskip("torch")


def _base(B, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, L)) * 0.3).astype(np.float32)


@pytest.mark.parametrize("B,L,S,prime", [(3, 1000, 11, 1237), (4, 4096, 9, 1237), (2, 777, 7, 101), (1, 64, 5, 64)])
def test_stream_slices_equal_the_full_construction(B, L, S, prime):
    base = _base(B, L, 5)
    bt = torch.from_numpy(base)
    # the construction as the issue states it, literally
    full = torch.stack([torch.roll(bt[s % B], s * prime) * float(Z.gain(s)) for s in range(S)]).numpy()
    built = Z.build_batch(bt, S, prime).numpy()
    assert np.array_equal(full.view(np.uint32), built.view(np.uint32))
    ref = np.stack([np.roll(base[s % B], s * prime) * Z.gain(s) for s in range(S)]).astype(np.float32)
    assert np.array_equal(full.view(np.uint32), ref.view(np.uint32))
    rng = np.random.default_rng(1)
    for s in range(S):
        sh = (s * prime) % L
        # whole stream, slices on both sides of the roll's wrap point and across it, empty and one-sample slices, random ones
        cuts = [(0, L), (0, 0), (L - 1, L), (max(0, sh - 5), min(L, sh + 5)), (0, min(L, sh + 1)), (max(0, sh - 1), L)]
        cuts += [tuple(sorted(int(v) for v in rng.integers(0, L + 1, 2))) for _ in range(6)]
        for a, b in cuts:
            got = Z.stream_slice(base, s, a, b, prime)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), full[s, a:b].view(np.uint32)), (s, a, b)
    some = Z.build_batch(bt, S, prime, rows=[S - 1, 0, 2]).numpy()
    assert np.array_equal(some.view(np.uint32), full[[S - 1, 0, 2]].view(np.uint32))


def test_long_stream_slices_equal_the_full_construction(monkeypatch):
    monkeypatch.setattr(Z, "LBLOCK", 6)          # gain steps every 64 samples: a small stream sees many steps and periods
    P, L, S = 256, 3001, 3
    base = _base(1, P, 9)[0]
    i = np.arange(S * L + 50, dtype=np.int64)
    full = (base[i % P] * (0.5 + ((i >> 6) % 17) / 32.0).astype(np.float32)).astype(np.float32)
    for first in (0, 50):
        built = Z.build_long(torch.from_numpy(base), L, S, first=first).numpy()
        assert np.array_equal(built.view(np.uint32), full[first:first + S * L].reshape(S, L).view(np.uint32))
    rng = np.random.default_rng(2)
    for a, b in [(0, S * L), (63, 65), (P - 1, P + 1), (17 * 64 - 1, 17 * 64 + 1), (L - 3, L + 3)] + \
            [tuple(sorted(int(v) for v in rng.integers(0, S * L, 2))) for _ in range(8)]:
        assert np.array_equal(Z.long_slice(base, a, b).view(np.uint32), full[a:b].view(np.uint32)), (a, b)
    assert len({float(g) for g in Z.lgain(np.arange(0, 17 * 64, 64))}) == 17


def test_boundaries_and_chosen_columns():
    # the headline many-streams shape: 160 x 16,369 x 1,024
    S, Cn, R = 160, 16369, 1024
    b4, b1 = Z.boundaries(S, Cn, R, 4), Z.boundaries(S, Cn, R, 1)
    assert set(b4) == {"cell 2^31", "byte 2^32", "byte 2^33"} and set(b1) == {"cell 2^31"}
    assert Z.cell_to_column(b4["byte 2^32"], Cn, R)[0] == 64 and Z.cell_to_column(b4["byte 2^33"], Cn, R)[0] == 128
    assert Z.cell_to_column(b1["cell 2^31"], Cn, R)[0] == 128
    assert Z.cell_to_column(Z.boundaries(264, Cn, R, 1)["cell 2^32"], Cn, R)[0] == 256
    assert Z.boundaries(64, Cn, R, 4) == {} and Z.boundaries(64, Cn, R, 1) == {}     # the bench shape crosses nothing
    pairs, where = Z.chosen_columns(S, Cn, R, (4, 1), seed=3)
    assert len(pairs) == len(set(pairs)) and all(0 <= s < S and 0 <= c < Cn for s, c in pairs)
    for name, (s, c) in where.items():
        lin = s * Cn + c
        for d in (-1, 0, 1):
            assert ((lin + d) // Cn, (lin + d) % Cn) in pairs, name
    # the boundary's cell really lies in the column named for it
    for it in (4, 1):
        for name, cell in Z.boundaries(S, Cn, R, it).items():
            s, c = where[f"{name} of a {it}-byte array"]
            assert (s * Cn + c) * R <= cell < (s * Cn + c + 1) * R
    for p in [(0, 0), (0, Cn - 1), (S - 1, 0), (S - 1, Cn - 1)]:
        assert p in pairs
    lo = min(Z.boundaries(S, Cn, R, 4).values()) // R
    assert sum(1 for s, c in pairs if s * Cn + c > lo) >= 8
    # 64 streams on 256 compute units: the launcher's one-round plan is four segments per stream
    assert ((-(-Cn // 4) + 1) & ~1) in Z.segment_lengths(64, Cn)
