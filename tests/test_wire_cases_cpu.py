"""CPU: the structured wire-image sets of tests/wire_cases.py hold what they claim (so that the GPU tests on them cannot be
vacuous), round-trip through the numpy restatement oracle/wire_ref.py, and expand on the host (emspec_wire_unpack_host: plain C,
no device) to the same columns."""
import numpy as np
import pytest

import emspec
import wire_cases as WC
import wire_ref as W


def _round_trips(cols):
    columns, rows = cols.shape
    w = W.pack(cols)
    assert w.size <= W.bound(columns, rows)
    assert w.size == W.fixed_bytes(columns, rows) + ((int((cols != 0).sum()) + 15) // 16) * 16
    assert np.array_equal(W.unpack(w, columns, rows), cols)
    out = np.full((columns, rows), 0xCD, np.uint8)
    assert np.array_equal(emspec.wire_unpack_host(w, columns, rows, out=out), cols)


def test_set_a_holds_every_lane_mask_once_in_staged_columns():
    cols = WC.set_a(256)
    assert cols.shape == (4096, 256)
    masks = WC.lane_masks(cols)
    assert np.array_equal(np.sort(masks.reshape(-1)), np.arange(1 << 16))            # each of the 65,536 masks exactly once
    st = WC.staged(cols)
    tot, _ = WC.totals_and_offsets(cols)
    assert np.all(tot[st] + 3 <= WC.STAGE_BYTES)
    in_staged = np.unique(masks[st].reshape(-1))
    assert in_staged.size >= 60000
    # every (p1 >= 4, p2 >= 8, p3 >= 12) combination that a 16-bit mask can give occurs in a staged column
    possible = set(zip(*(a.tolist() for a in WC.window_selects(np.arange(1 << 16)))))
    present = set(zip(*(a.tolist() for a in WC.window_selects(in_staged))))
    assert possible == present == {(False, False, False), (True, False, False), (True, True, False), (True, True, True)}
    # every nibble value at each of the four positions: the whole selector table, from every output dword
    for j in range(4):
        assert np.unique((in_staged >> (4 * j)) & 15).size == 16
    # the same cells as 1,024-row columns: 64 lanes a column, every column past the staged switch
    wide = WC.set_a(1024)
    assert wide.shape == (1024, 1024) and np.array_equal(wide.reshape(-1), cols.reshape(-1))
    assert not WC.staged(wide).any()


def test_set_b_covers_the_staged_switch():
    cols, info = WC.set_b(1024)
    tot, off = WC.totals_and_offsets(cols)
    pairs = set()
    for i, it in enumerate(info):
        if it is None:
            assert tot[i] <= 3
            continue
        t, pl, res = it
        assert tot[i] == t and (off[i] & 3) == res
        pairs.add((res, t))
        nzr = np.flatnonzero(cols[i])
        if pl == "from_row_0":
            assert nzr[0] == 0 and nzr[-1] == t - 1
        elif pl == "to_last_row":
            assert nzr[-1] == 1023 and nzr[0] == 1024 - t
    assert pairs == {(r, t) for r in range(4) for t in WC.B_TOTALS} and len(pairs) == 44
    assert sum(it is not None for it in info) == 44 * len(WC.B_PLACEMENTS)
    st = WC.staged(cols)
    # the switch itself: 256 bytes from the aligned start are staged, 257 are not
    for i, it in enumerate(info):
        if it is not None:
            assert st[i] == (it[0] + it[2] <= 256)
    groups = st[:len(st) // WC.WAVE_COLUMNS * WC.WAVE_COLUMNS].reshape(-1, WC.WAVE_COLUMNS)
    mixed = int(np.sum(groups.any(axis=1) & ~groups.all(axis=1)))
    tcols = np.array([it is not None for it in info])[:groups.size].reshape(-1, WC.WAVE_COLUMNS)
    both_t = int(np.sum([len({bool(s) for s, t in zip(g, tc) if t}) == 2 for g, tc in zip(groups, tcols)]))
    assert mixed >= 20 and both_t >= 10      # waves with both kinds; waves whose two t-columns fall on different sides


@pytest.mark.parametrize("rows", [256, 1024])
def test_set_a_round_trips(rows):
    _round_trips(WC.set_a(rows))


def test_set_b_round_trips():
    _round_trips(WC.set_b(1024)[0])


@pytest.mark.parametrize("rows", WC.C_FAST_ROWS)
def test_set_c_round_trips(rows):
    for columns in WC.C_COUNTS:
        _round_trips(WC.set_c(columns, rows))


@pytest.mark.parametrize("rows", WC.C_FAST_ROWS + WC.C_GENERIC_ROWS)
def test_edge_columns_round_trip(rows):
    _round_trips(WC.edge_columns(rows))
    if rows == 1024:       # totals around the staged switch among the C columns as well
        tot, _ = WC.totals_and_offsets(WC.set_c(1025, rows))
        assert np.any((tot > 230) & (tot <= 253)) and np.any((tot > 256) & (tot < 330))
