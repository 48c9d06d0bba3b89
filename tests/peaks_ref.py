"""numpy restatement of the spectral peaks (include/emspec.h: emspec_peaks_device) and the columns the peak
tests share.

The peaks of a column are a function of its dB values x[0 .. R), of k and of min_db, in binary32 with one rounding per operation:

    candidate r:  x[r] >= min_db and x[r] > x[r-1] and x[r] >= x[r+1]          (-inf beyond either end)
    db  = x[r]                                                                 (the cell's own bits)
    pos = r + 0.5 at r = 0 and r = R-1, else (r + 0.5) + d with
          t = a - c;  u = (a - b) + (c - b);  d = (0.5 t) / u;  d > 0.5 -> 0.5;  d < -0.5 -> -0.5;  NaN -> 0
    the k first by dB descending, ties by ascending row; unused slots (-1, -inf)

The peaks are a function of the dB image, so the reference needs no oracle of its own: it is applied to what the CPU bit models
(oracle.batch_exact / oracle.batch_f32), tests/multires_ref.py or the engine itself deliver.  Every array operation below is a
float32 numpy operation (numpy does not promote float32 arrays, and 0.5 is given as np.float32).  Lives under tests/ (like
overview_ref.py); the product never imports it."""
import numpy as np

F = np.float32
NINF = F(-np.inf)


def parts(db, min_db):
    """db float32 [columns, R] -> (candidate mask, pos, d, u), each [columns, R]: steps 1 and 3 of the definition for every row."""
    x = np.ascontiguousarray(db, F)
    assert x.ndim == 2
    cols, R = x.shape
    edge = np.full((cols, 1), NINF, F)
    a = np.concatenate([edge, x[:, :-1]], axis=1)
    c = np.concatenate([x[:, 1:], edge], axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cand = (x >= F(min_db)) & (x > a) & (x >= c)
        t = a - c
        u = (a - x) + (c - x)
        d = (F(0.5) * t) / u
        d = np.where(d > F(0.5), F(0.5), d)
        d = np.where(d < F(-0.5), F(-0.5), d)
        d = np.where(d != d, F(0.0), d).astype(F)
    d[:, 0] = 0
    d[:, R - 1] = 0
    centre = np.arange(R, dtype=F) + F(0.5)
    pos = (centre[None, :] + d).astype(F)
    assert t.dtype == F and u.dtype == F and d.dtype == F and pos.dtype == F
    return cand, pos, d, u


def peaks(db, k, min_db):
    """db float32 [..., R] -> float32 [..., k, 2] of (pos, dB): what emspec_peaks_device / emspec_peaks_host deliver."""
    db = np.ascontiguousarray(db, F)
    R = db.shape[-1]
    x = db.reshape(-1, R)
    cand, pos, _, _ = parts(x, min_db)
    out = np.empty((x.shape[0], k, 2), F)
    out[:, :, 0] = F(-1.0)
    out[:, :, 1] = NINF
    for col in range(x.shape[0]):
        rows = np.nonzero(cand[col])[0]
        if rows.size == 0:
            continue
        vals = x[col, rows]
        order = np.lexsort((rows, -vals))[:k]          # dB descending by float comparison (-0.0 == +0.0), ties by row
        sel = rows[order]
        out[col, :sel.size, 0] = pos[col, sel]
        out[col, :sel.size, 1] = x[col, sel]           # (a float32 copy keeps the bits, the sign of a zero included)
    return out.reshape(db.shape[:-1] + (k, 2))


def bits(p):
    return np.ascontiguousarray(p, F).view(np.uint32)


def cases(R, seed=0):
    """[(name, db float32 [columns, R], min_db)]: the columns of the issue's list that exist at R rows."""
    rng = np.random.default_rng(1000 + R + seed)
    out = []
    floor = np.full(R, -80.0, F)

    def add(name, cols, min_db=-60.0):
        out.append((name, np.ascontiguousarray(np.atleast_2d(np.asarray(cols, F))), float(min_db)))

    # no cell at or above min_db (bumps below it)
    x = floor.copy(); x[1::2] = -70.0
    add("below_min_db", x)
    # a sawtooth with R/2 peaks, of seven different heights
    x = floor.copy(); x[0::2] = -10.0 - (np.arange(R // 2) % 7).astype(F)
    add("sawtooth", x)
    # exactly k peaks, k = 1, 8, 32, with distinct heights in a shuffled order
    for k in (1, 8, 32):
        if 2 * k <= R:
            x = floor.copy()
            at = np.sort(rng.choice(R // 2, k, replace=False)) * 2 + (1 if R > 4 else 0)
            x[np.minimum(at, R - 1)] = -5.0 - rng.permutation(k).astype(F)
            add(f"exactly_{k}", x)
    # peaks drawn from a four-value set: dB ties broken by row
    x = floor.copy(); x[0::2] = rng.choice(np.array([-10.0, -20.0, -30.0, -40.0], F), R // 2)
    add("four_values", x)
    # plateaus: a flat top, and one that rises afterwards (its first row still reports: x[r] >= x[r+1] holds on the flat part)
    if R >= 16:
        x = floor.copy(); x[3:6] = -20.0; x[9:11] = -30.0; x[11] = -10.0
        add("plateaus", x)
    x = np.full(R, -20.0, F)
    add("flat_above", x)
    # peaks at row 0 and row R-1
    x = floor.copy(); x[0] = -10.0; x[R - 1] = -12.0
    add("ends", x)
    x = floor.copy(); x[0] = -10.0; x[1] = -10.0; x[R - 2] = -30.0; x[R - 1] = -12.0
    add("ends_sloped", x)
    # peaks on both sides of the quad, lane-round and wave-round boundaries
    for lo in (3, 255, 1023):
        if lo + 2 < R:
            for at in (lo, lo + 1):
                x = floor.copy(); x[at] = -10.0; x[at - 1] = -40.0; x[at + 1] = -25.0
                add(f"boundary_{at}", x)
            x = floor.copy(); x[lo] = -10.0; x[lo + 1] = -10.0     # a plateau across the boundary
            add(f"boundary_plateau_{lo}", x)
    # a column at the engine's floor: nothing at min_db = -60, row 0 alone at min_db = -200
    add("floor_200", np.full(R, -200.0, F))
    add("floor_200_all_pass", np.full(R, -200.0, F), -200.0)
    # -0.0 ties with +0.0: row order decides, the bits are kept
    x = np.full(R, -5.0, F); x[0] = -0.0; x[2] = 0.0
    y = np.full(R, -5.0, F); y[0] = 0.0; y[2] = -0.0
    add("signed_zeros", np.stack([x, y]), -1.0)
    if R >= 16:
        x = np.full(R, -5.0, F); x[R - 3] = 0.0; x[5] = -0.0; x[9] = 0.0
        add("signed_zeros_far", x, -1.0)
    # one NaN, one +inf, one -inf among random values
    if R >= 16:
        cols = rng.uniform(-90.0, 0.0, (4, R)).astype(F)
        for c in range(4):
            at = rng.choice(R, 3, replace=False)
            cols[c, at[0]] = np.nan; cols[c, at[1]] = np.inf; cols[c, at[2]] = -np.inf
        cols[3, 0] = np.nan; cols[3, R - 1] = np.inf
        add("nan_inf", cols, -60.0)
        add("nan_inf_min_ninf", cols, -np.inf)
    x = floor.copy(); x[1] = np.nan; x[2] = -10.0        # a NaN neighbour: -10 > NaN is false, no peak
    add("nan_neighbour", x)
    # q = b - c one ulp above zero: t and u round to the same magnitude and |d| reaches the clamp's bound, 0.5
    if R >= 8:
        cols = []
        for a, b in ((-50.0, -10.0), (-10.5, -10.0), (-199.0, -3.25), (-11.0, -1.0e-3)):
            x = floor.copy(); x[2] = a; x[3] = b; x[4] = np.nextafter(F(b), NINF)
            cols.append(x)
            x = floor.copy(); x[4] = a; x[3] = b; x[2] = np.nextafter(F(b), NINF)
            cols.append(x)
        add("one_ulp", np.stack(cols))
    # 20 random columns: ten continuous, ten quantised to 3 dB (plateaus and ties)
    cols = rng.uniform(-100.0, 0.0, (20, R)).astype(F)
    cols[10:] = np.round(cols[10:] / 3.0) * 3.0
    add("random", cols)
    return out


def all_columns(R, seed=0):
    """Every case's columns, stacked per min_db: {min_db: db [n, R]} (one call of the code under test per min_db)."""
    groups = {}
    for _, db, m in cases(R, seed):
        groups.setdefault(m, []).append(db)
    return {m: np.concatenate(v) for m, v in groups.items()}
