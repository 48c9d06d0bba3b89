"""numpy model of the live history (include/emspec.h: emspec_set_live_history, emspec_history_view): a ring of
W delivered dB columns per stream, and views of it.

    column c of a stream lives in slot c mod W; after `end` columns the ring holds [max(0, end - W), end)
    a launch that emits more than W columns of a stream stores its last W
    view(first, f, groups): group g covers first + g f .. min(first + (g + 1) f, end) - 1;
        db    = overview_ref.reduce_db of the stored columns (the ordered comparison of DESIGN.md §3.10)
        index = post_ref.cell_index_f32(db + shift) under the view's law
        rgba  = LUT[index]

The model keeps the slots, not a list of columns, so that a wrong slot rule shows as wrong bytes.  Lives under tests/ (like
overview_ref.py); the product never imports it."""
import numpy as np

import overview_ref as V
import post_ref as P

F = np.float32

# ---- what the GPU tests and the CPU check of their colour case share ----
# a map that differs from the default configuration (db_top 0, db_range 80, gate_db -80) in every field, and a shift
VIEW_MAP = (-6.0, 55.0, -58.5, 4.25)          # (db_top, db_range, gate_db, shift_db)
HOLD_HOP = 16                             # post_ref.signals holds a level for 97 x this many samples: ~6 columns at hop 256


def signal(S, L):
    """S streams of L samples whose levels jump every ~6 columns of hop 256 (post_ref.signals at a short hold), exact zeros
    included: a ring of a few columns sees loud, silent and quiet columns side by side."""
    return P.signals(S, L, hop=HOLD_HOP)


def colour_map(seed=11):
    """An uploaded colour map: 256 distinct random RGBA entries."""
    lut = np.random.default_rng(seed).integers(0, 256, size=(256, 4)).astype(np.uint8)
    lut[:, 0] = np.arange(256, dtype=np.uint8)  # (distinct entries: a wrong index shows)
    return lut


class Ring:
    """One stream's ring."""

    def __init__(self, W, rows):
        self.W, self.rows = int(W), int(rows)
        self.reset()

    def reset(self):
        self.end = 0
        self.slots = np.full((self.W, self.rows), np.nan, F)
        self.holds = [-1] * self.W                       # the column each slot holds

    @property
    def first(self):
        return max(0, self.end - self.W)

    def held(self):
        """(end, first), as emspec_live_history reports them."""
        return self.end, self.first

    def launch(self, columns):
        """One launch emits these columns ([count][rows], in order): the last W of them are stored."""
        columns = np.asarray(columns, F).reshape(-1, self.rows)
        count = columns.shape[0]
        keep_from = self.end + max(0, count - self.W)
        for i in range(count):
            c = self.end + i
            if c >= keep_from:
                self.slots[c % self.W] = columns[i]
                self.holds[c % self.W] = c
        self.end += count

    def fits(self, first, f, groups):
        if f < 1 or f > 65536 or groups < 1:
            return False
        return self.first <= first < self.end and first + (groups - 1) * f < self.end

    def columns(self, c0, c1):
        """The stored columns [c0, c1) in order, read through their slots."""
        for c in range(c0, c1):
            assert self.holds[c % self.W] == c, (c, self.holds)
        return np.stack([self.slots[c % self.W] for c in range(c0, c1)])

    def view_db(self, first, f, groups):
        assert self.fits(first, f, groups), (first, f, groups, self.held())
        out = np.empty((groups, self.rows), F)
        for g in range(groups):
            c0 = first + g * f
            out[g] = V.reduce_db(self.columns(c0, min(c0 + f, self.end))[None], f)[0, 0]
        return out


class History:
    """The rings of a session's S streams, fed with what its calls deliver."""

    def __init__(self, S, W, rows):
        self.rings = [Ring(W, rows) for _ in range(S)]

    def launch(self, per_stream):
        """per_stream[s]: the columns [count_s][rows] stream s emits in this launch (count_s may be 0)."""
        for ring, cols in zip(self.rings, per_stream):
            ring.launch(cols)

    def reset_stream(self, s):
        self.rings[s].reset()

    def held(self, s):
        return self.rings[s].held()

    def view(self, first, f, groups, stream0=0, streams=None, map=None, lut=None):
        """map: (db_top, db_range, gate_db, shift_db).  -> {"db", "index", "rgba" (with a lut)}; index needs a map."""
        rings = self.rings[stream0:] if streams is None else self.rings[stream0:stream0 + streams]
        db = np.stack([r.view_db(first, f, groups) for r in rings])
        out = {"db": db, "index": None, "rgba": None}
        if map is not None:
            top, rng, gate, shift = map
            out["shifted"] = (db + F(shift)).astype(F)
            out["index"] = P.cell_index_f32(out["shifted"], top, rng, gate)
            if lut is not None:
                out["rgba"] = np.asarray(lut, np.uint8).reshape(256, 4)[out["index"]]
        return out
