"""Structured columns for the gather's wire image (em-spec_amd/csrc/pack.hip.inc; numpy restatement: oracle/wire_ref.py).

Uniform random columns at a density of 5 - 7 % (tests/test_gather.py) never reach the selection logic of
wire_expand16_kernel: a lane whose first four, eight or twelve cells are ALL non-zero (the p1 >= 4 / p2 >= 8 / p3 >= 12
window selects), most of the 65,536 lane masks (the 16-entry v_perm selector table is indexed with every nibble of them),
and column totals on both sides of the staged switch `tot + (off & 3) <= 256` inside one wave (four consecutive columns).
The sets below build exactly those.  Cell values are non-zero bytes from emspec.synth.uniform; nothing else is random.

Plain numpy: shared by the CPU tests (tests/test_wire_cases_cpu.py) and the GPU tests (tests/test_gpu_wire_cases.py)."""
import numpy as np

from emspec import synth

STAGE_BYTES = 256        # wire_expand16_kernel stages one dword per lane: runs of tot + (off & 3) <= 256 bytes
WAVE_COLUMNS = 4         # columns one wave expands together (kWireNC)


def values(seed, count):
    """count non-zero bytes (1..255)."""
    return (1 + np.floor(synth.uniform(seed, count) * 255.0)).astype(np.uint8)


def fill(nz, seed):
    """bool [columns][rows] -> uint8 columns with a non-zero byte wherever nz."""
    out = np.zeros(nz.shape, np.uint8)
    out[nz] = values(seed, int(nz.sum()))
    return out


def totals_and_offsets(cols):
    tot = (cols != 0).sum(axis=1).astype(np.int64)
    return tot, np.cumsum(tot) - tot


def staged(cols):
    """Which columns take the staged branch of wire_expand16_kernel (only meaningful for rows % 32 == 0, rows <= 1024)."""
    tot, off = totals_and_offsets(cols)
    return tot + (off & 3) <= STAGE_BYTES


def lane_masks(cols):
    """The 16-bit mask of every lane: uint32 [columns][rows / 16], bit b = cell 16 lane + b is non-zero."""
    c, r = cols.shape
    bits = (cols != 0).reshape(c, r // 16, 16).astype(np.uint32)
    return (bits << np.arange(16, dtype=np.uint32)).sum(axis=2).astype(np.uint32)


def popc(m):
    m = np.asarray(m, np.uint32)
    return sum(((m >> np.uint32(b)) & np.uint32(1)).astype(np.int64) for b in range(16))


def window_selects(masks):
    """(p1 >= 4, p2 >= 8, p3 >= 12) of every lane mask: the three selects of the staged branch."""
    m = np.asarray(masks, np.uint32)
    return popc(m & 0xF) >= 4, popc(m & 0xFF) >= 8, popc(m & 0xFFF) >= 12


# ---- A: every lane mask exactly once ------------------------------------------------------------------------------------------
def set_a(rows=256):
    """All 65,536 lane masks, each exactly once, in a fixed pseudo-random order: 4,096 columns of 256 rows (16 lanes a column,
    totals near 128: every column staged).  A column whose total would exceed 253 swaps lanes with the next column until
    tot + 3 <= 256.  rows = 1024: the same cells as 1,024 columns of 64 lanes (totals near 512: every column unstaged)."""
    order = np.argsort(synth.splitmix64(0xA11, 1 << 16), kind="stable").astype(np.uint32)
    lanes = order.reshape(4096, 16)
    cnt = popc(lanes)
    for c in range(4096):
        nxt = (c + 1) % 4096
        while cnt[c].sum() > STAGE_BYTES - 3:
            i, j = int(np.argmax(cnt[c])), int(np.argmin(cnt[nxt]))
            if cnt[c, i] <= cnt[nxt, j]:
                break
            lanes[c, i], lanes[nxt, j] = lanes[nxt, j], lanes[c, i]
            cnt[c, i], cnt[nxt, j] = cnt[nxt, j], cnt[c, i]
    nz = ((lanes[:, :, None] >> np.arange(16, dtype=np.uint32)) & 1).astype(bool).reshape(4096, 256)
    cols = fill(nz, 0xA12)
    return np.ascontiguousarray(cols.reshape(-1, rows))


# ---- B: column totals around the staged switch ---------------------------------------------------------------------------------
B_TOTALS = tuple(range(250, 261))
B_PLACEMENTS = ("from_row_0", "to_last_row", "scattered")


def set_b(rows=1024):
    """For each total t in 250..260, each of three placements and each residue off & 3 in 0..3: a column of exactly t non-zero
    cells, preceded by a column of 0..3 cells that brings the payload offset to the residue.  The totals alternate between the
    two ends of the range, so that the waves (four consecutive columns) hold staged and unstaged columns side by side.
    Returns (columns, info): info[i] = (t, placement, off & 3) for the t-columns, None for the fillers."""
    ts = []
    lo, hi = 0, len(B_TOTALS) - 1
    while lo <= hi:                       # 250, 260, 251, 259, ...
        ts.append(B_TOTALS[lo]); lo += 1
        if lo <= hi:
            ts.append(B_TOTALS[hi]); hi -= 1
    cols, info, off, k = [], [], 0, 0
    for res in range(4):
        for pl in B_PLACEMENTS:
            for t in ts:
                f = (res - off) & 3
                filler = np.zeros(rows, bool)
                filler[(np.argsort(synth.splitmix64(0xB00 + k, rows), kind="stable"))[:f]] = True
                col = np.zeros(rows, bool)
                if pl == "from_row_0":
                    col[:t] = True
                elif pl == "to_last_row":
                    col[rows - t:] = True
                else:
                    col[np.argsort(synth.splitmix64(0xB80 + k, rows), kind="stable")[:t]] = True
                cols += [filler, col]
                info += [None, (t, pl, (off + f) & 3)]
                off += f + t
                k += 1
    return fill(np.stack(cols), 0xB13), info


# ---- C: edge counts and rows ----------------------------------------------------------------------------------------------------
C_COUNTS = tuple(range(1, 18)) + (1023, 1024, 1025, 4097)
C_FAST_ROWS = (32, 64, 1024)                  # the 16-rows-per-lane kernels (rows % 32 == 0, rows <= 1024)
C_GENERIC_ROWS = (4, 68, 100, 2048, 4096)     # one wave per column, a dword per lane and iteration
ENGINE_MIN_ROWS = 64                          # emspec_create accepts rows in [64, 4096]: smaller images exist on the host side only


def set_c(columns, rows):
    """`columns` columns whose density cycles through 0, 5 %, 24 % (at rows = 1024: totals around the staged switch), 30 % and 100 %."""
    dens = np.array([0.0, 0.05, 0.24, 0.30, 1.0])[np.arange(columns) % 5]
    u = synth.uniform(0xC00 + rows, columns * rows).reshape(columns, rows)
    return fill(u < dens[:, None], 0xC14 + columns)


def edge_columns(rows):
    """All-zero, all-255, both alternations, a single cell at row 0, at row R - 1, both: 7 columns (two waves, the second ragged)."""
    c = np.zeros((7, rows), np.uint8)
    c[1] = 255
    c[2, 0::2] = 255
    c[3, 1::2] = 255
    c[4, 0] = 7
    c[5, rows - 1] = 9
    c[6, 0], c[6, rows - 1] = 1, 255
    return c
