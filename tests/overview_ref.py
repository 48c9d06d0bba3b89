"""numpy restatement of the time reduction (include/emspec.h: emspec_set_time_reduce): groups of f
consecutive finished columns of a stream collapse into one by maximum, the last group may be short.

    db   [s][g][r] = m,  m = full_db[s][g f][r];  then for c = g f + 1 .. in order:  if (full_db[s][c][r] > m) m = full_db[s][c][r]
    index[s][g][r] = max over the group of full_index[s][c][r]          (unsigned bytes)
    rgba [s][g][r] = LUT[index[s][g][r]]

The reduced image is a function of the full-rate one, so the reference needs no oracle of its own: it is applied to what the
CPU bit models (oracle.batch_exact / oracle.batch_f32), tests/multires_ref.py or the engine itself at factor 1 produce.
The palette index is np.maximum.reduceat along the column axis.  The dB takes the ordered comparison of the definition instead:
np.maximum lets a NaN anywhere in a group through, the definition only one at the head of the group (x > m is false for a NaN),
and keeps the sign of the first of several zeros.  Lives under tests/ (like multires_ref.py); the product never imports it."""
import numpy as np


def reduced_columns(C, f):
    return -(-C // f)


def reduce_index(index, f, axis=1):
    """uint8 [..][C][..] -> [..][ceil(C / f)][..] along `axis`."""
    index = np.asarray(index)
    assert index.dtype == np.uint8 and f >= 1
    return np.ascontiguousarray(np.maximum.reduceat(index, np.arange(0, index.shape[axis], f), axis=axis))


def reduce_db(db, f, axis=1):
    """float32 [..][C][..] -> [..][ceil(C / f)][..] along `axis`, by the ordered comparison of the definition."""
    db = np.moveaxis(np.asarray(db), axis, 0)
    assert db.dtype == np.float32 and f >= 1
    C = db.shape[0]
    m = db[0::f].copy()
    for j in range(1, min(f, C)):
        x = db[j::f]                      # column g f + j of every group that has one
        k = x.shape[0]
        with np.errstate(invalid="ignore"):
            m[:k] = np.where(x > m[:k], x, m[:k])
    return np.ascontiguousarray(np.moveaxis(m, 0, axis))


def reduce(full, f, lut):
    """full: {"db", "rgba", "index"} arrays [S][C][R] (+[4]) or None, as the batch entries return them at factor 1 ->
    the same at factor f.  RGBA comes from the reduced index (full["index"] is needed for it)."""
    out = {"db": None, "rgba": None, "index": None}
    if full.get("db") is not None:
        out["db"] = reduce_db(full["db"], f)
    if full.get("index") is not None:
        out["index"] = reduce_index(full["index"], f)
        if full.get("rgba") is not None:
            out["rgba"] = np.ascontiguousarray(np.asarray(lut, np.uint8).reshape(256, 4)[out["index"]])
    return out
