"""GPU: the pack / expand kernels of the gather's wire image (pack.hip.inc) on the structured columns of tests/wire_cases.py -
every lane mask, column totals on both sides of the staged switch inside one wave, edge counts and rows - byte for byte against
the numpy restatement oracle/wire_ref.py.  tests/test_wire_cases_cpu.py asserts that the sets hold what they claim."""
import numpy as np
import pytest
import torch

import emspec
import wire_cases as WC
import wire_ref as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    torch.cuda.init()
    made = {}

    def get(rows):
        if rows not in made:
            made[rows] = emspec.Engine(rows=rows)
        return made[rows]
    yield get
    for e in made.values():
        e.close()


def _check(e, cols):
    """GPU pack == numpy pack, every byte and the pad, over a buffer that held 0xAB; GPU expand of it == the columns, over 0xCD."""
    columns, rows = cols.shape
    assert rows == e.rows
    ref = W.pack(cols)
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(cols).to(dev)
    wire = torch.full((emspec.wire_bound(columns, rows),), 0xAB, dtype=torch.uint8, device=dev)
    nbytes = e.wire_pack(t, wire)
    assert nbytes == ref.size
    got = wire[:nbytes].cpu().numpy()
    assert np.array_equal(got, ref), f"{columns} x {rows}: {int(np.sum(got != ref))} bytes of the image differ, first at {int(np.flatnonzero(got != ref)[0])}"
    back = torch.full_like(t, 0xCD)
    e.wire_unpack(wire, nbytes, back)
    torch.cuda.synchronize()
    back = back.cpu().numpy()
    bad = np.argwhere(back != cols)
    assert bad.size == 0, f"{columns} x {rows}: {len(bad)} cells differ, first (column, row) {tuple(bad[0])}: {back[tuple(bad[0])]} != {cols[tuple(bad[0])]}"


@pytest.mark.parametrize("rows", [256, 1024])
def test_every_lane_mask(engines, rows):
    """Set A: each of the 65,536 lane masks once; rows = 256: every column staged (the window selects and the selector table),
    rows = 1024: the same cells, every column read straight from the image."""
    _check(engines(rows), WC.set_a(rows))


def test_staged_switch(engines):
    """Set B: totals 250..260 at every payload offset residue, three placements; staged and unstaged columns share waves."""
    _check(engines(1024), WC.set_b(1024)[0])


@pytest.mark.parametrize("rows", [r for r in WC.C_FAST_ROWS if r >= WC.ENGINE_MIN_ROWS])
def test_edge_counts_fast_kernels(engines, rows):
    """Set C on the 16-rows-per-lane kernels: 1..17, 1023, 1024, 1025, 4097 columns (ragged waves and workgroups, the two levels
    of the offset scan).  (rows = 32 is below what an engine accepts: that image exists on the host side only, CPU tests.)"""
    e = engines(rows)
    for columns in WC.C_COUNTS:
        _check(e, WC.set_c(columns, rows))
    _check(e, WC.edge_columns(rows))


@pytest.mark.parametrize("rows", [r for r in WC.C_GENERIC_ROWS if r >= WC.ENGINE_MIN_ROWS])
def test_edge_columns_generic_kernels(engines, rows):
    """The one-wave-per-column kernels (rows % 32 != 0 or rows > 1024): all-zero, all-255, alternating and single-cell columns,
    a single cell at row 0 and at row R - 1.  (rows = 4: host side only.)"""
    e = engines(rows)
    _check(e, WC.edge_columns(rows))
    _check(e, WC.set_c(5, rows))
