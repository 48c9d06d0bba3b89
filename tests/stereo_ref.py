"""numpy float32 restatement of the stereo image (include/emspec.h: emspec_stereo_*): level and balance of a
channel pair in one picture, as a function of the two channels' dB values.

    lo = db_top - db_range (binary32), inv = (float)(1 / (double)db_range), inv_pan = (float)(1 / (double)pan_range_db)
    level:   m = (x_b > x_a || x_a != x_a) ? x_b : x_a                  the cell's own bits; NaN only when both are
    shifted: s = m + shift_db;  gated = s < gate_db
    index:   0 if s is NaN, else post_ref.cell_index_f32 of s
    balance: d = x_b - x_a; u = d * inv_pan, clamped to [-1, 1]; pan = 16 + rint(u * 16) (half to even);
             pan = 16 if gated or d is NaN
    rgba:    PAL[pan][index]

and the integer builder of the [33][256][4] palette.  Also what the CPU and the GPU tests share: the constructed array of the
law's special cases, and the test signal (two stereo S16 sources decoded to L R M S).  Lives under tests/ (like history_ref.py);
the product never imports it."""
import numpy as np

import history_ref as H
import pcm_ref
import post_ref as P

F, U = np.float32, np.uint32
CENTRE, LEVELS = 16, 33
WARM, COLD = (255, 96, 32), (32, 160, 255)
CASES = ((2, 0, 1), (4, 0, 1), (4, 2, 3), (4, 1, 0))      # (views, a, b)
N, HOP, FRAMES = 1024, 256, 27
DEFAULT_MAP = (0.0, 80.0, -80.0, 0.0, 12.0)               # the default configuration's law, shift 0, 12 dB to a side
VIEW_MAP = H.VIEW_MAP + (12.0,)                           # history_ref's map (every field differs, a shift), the same range


def compose(db, views, a, b, map, palette=None):
    """db [pairs * views][...] float32; map (db_top, db_range, gate_db, shift_db, pan_range_db) ->
    {"level", "index", "pan", "rgba" (with a palette)} of shape [pairs][...]."""
    db = np.ascontiguousarray(db, F)
    top, rng, gate, shift, pan_range = (F(x) for x in map)
    x = db.reshape((-1, views) + db.shape[1:])
    xa, xb = x[:, a], x[:, b]
    with np.errstate(invalid="ignore", over="ignore"):
        take_b = (xb > xa) | np.isnan(xa)
        level = np.where(take_b, xb.view(U), xa.view(U)).view(F)   # (the bits, not the value)
        s = (level + shift).astype(F)
        nan_s = np.isnan(s)
        gated = s < gate
        index = P.cell_index_f32(np.where(nan_s, F(gate), s).astype(F), top, rng, gate)
        index[nan_s] = 0
        d = (xb - xa).astype(F)
        inv_pan = F(1.0 / float(pan_range))
        u = (d * inv_pan).astype(F)
        u = np.where(u > F(1), F(1), u)
        u = np.where(u < F(-1), F(-1), u).astype(F)
        t = (u * F(16.0)).astype(F)
        centre = gated | np.isnan(t)
        pan = (CENTRE + np.rint(np.where(centre, F(0), t)).astype(np.int32)).astype(np.uint8)   # (np.rint: half to even)
        pan[centre] = CENTRE
    out = {"level": np.ascontiguousarray(level), "index": index, "pan": pan, "rgba": None, "gated": gated | nan_s}
    if palette is not None:
        out["rgba"] = np.asarray(palette, np.uint8).reshape(LEVELS, 256, 4)[pan, index]
    return out


def palette(base):
    """The [33][256][4] palette of a [256][4] colour map, in integers."""
    base = np.asarray(base, np.uint8).reshape(256, 4).astype(np.int64)
    out = np.empty((LEVELS, 256, 4), np.uint8)
    v = base[:, :3].max(axis=1)
    for pan in range(LEVELS):
        t = pan - CENTRE
        w = abs(t)
        K = np.array(WARM if t < 0 else COLD, np.int64)
        tint = (K[None, :] * v[:, None] + 127) // 255
        out[pan, :, :3] = (base[:, :3] * (16 - w) + tint * w + 8) // 16
        out[pan, :, 3] = base[:, 3]
    return out


def random_palette(seed=12):
    """An uploaded palette: 33 x 256 distinct random entries (a wrong pan or index shows)."""
    pal = np.random.default_rng(seed).integers(0, 256, size=(LEVELS, 256, 4)).astype(np.uint8)
    pal[:, :, 0] = np.arange(256, dtype=np.uint8)[None, :]
    pal[:, :, 1] = np.arange(LEVELS, dtype=np.uint8)[:, None]
    return pal


def _below(x):
    return np.nextafter(F(x), F(-np.inf))


def special_cases(map, cells=None):
    """(db [2][cells], pan_range) for views = 2, a = 0, b = 1: every special case of the law under `map`'s level fields.
    The ties need pan_range_db = 16: d = k + 0.5 for k in -16 .. 15 makes u * 16 exactly k + 0.5.  Padded with a plain pair to
    a multiple of 4 (or to `cells`)."""
    top, rng, gate, shift = (F(x) for x in map[:4])
    nan, inf = F(np.nan), F(np.inf)
    a, b = [], []

    def add(xa, xb):
        a.append(F(xa))
        b.append(F(xb))
    add(nan, -20.0), add(-20.0, nan), add(nan, nan)                      # NaN in A only, in B only, in both
    payload = np.array([0x7FC12345], U).view(F)[0]
    add(payload, nan), add(nan, payload)                                   # both NaN: the level is B's bits
    add(inf, -20.0), add(-20.0, inf), add(-inf, -20.0), add(-20.0, -inf)
    add(inf, inf), add(-inf, -inf), add(inf, -inf), add(-inf, inf)         # the same infinity in both: d is NaN -> centre
    add(-0.0, 0.0), add(0.0, -0.0), add(0.0, 0.0), add(-0.0, -0.0)
    # s exactly at the gate (not gated) and one ulp below (gated: pan 16, index 0), from either channel, off centre
    at = F(gate - shift)
    assert F(at + shift) == gate, "the map's gate must be reachable exactly"
    lower = at
    while not F(lower + shift) < gate:
        lower = _below(lower)
    for x in (at, lower):
        add(x, F(x - F(30.0))), add(F(x - F(30.0)), x), add(x, x)
    for dd in (12.0, 12.5, 40.0, 1e30, -12.0, -12.5, -40.0, -1e30):        # |d| at and beyond the range on both sides
        add(-30.0, F(-30.0) + F(dd))
    for k in range(-16, 16):                                               # exact ties at pan_range_db = 16
        add(-40.0, F(-40.0) + F(k + 0.5))
        add(F(-8.0) - F(k + 0.5), -8.0)
    for k in range(-17, 18):                                               # and whole steps
        add(-25.0, F(-25.0) + F(k))
    n = len(a)
    total = cells if cells is not None else -(-n // 4) * 4
    assert total >= n and total % 4 == 0
    while len(a) < total:
        add(-33.0 - len(a) % 7, -31.0)
    return np.stack([np.array(a, F), np.array(b, F)])


def raw_signal(frames=FRAMES, n=N, hop=HOP, sources=2):
    """`sources` stereo S16 sources from history_ref.signal(2 sources, L): int16 [sources][L * 2], interleaved."""
    L = n + hop * (frames - 1)
    x = H.signal(2 * sources, L)
    return np.stack([np.round(np.stack([x[2 * i], x[2 * i + 1]], -1).reshape(-1) * 32767).astype("<i2") for i in range(sources)])


LRMS = [[1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [0.5, -0.5]]


def decoded_signal(views=4, **kw):
    """The streams the PCM front end makes of raw_signal: [sources * views][L] float32 (views = 2: L R; 4: L R M S)."""
    raw = raw_signal(**kw)
    return pcm_ref.decode(raw.view(np.uint8), pcm_ref.S16, 2, LRMS[:views])


def exercised(out, min_pans=24, min_indices=9, min_cells=400):
    """The law is exercised by a case's result: enough balance values among ungated cells, both ends and the centre among
    them, more than 8 palette indices, enough ungated cells.  -> (pans, indices, ungated cells)."""
    live = ~out["gated"]
    pans = np.unique(out["pan"][live])
    idx = np.unique(out["index"][live])
    n = int(np.count_nonzero(live))
    assert len(pans) >= min_pans and 0 in pans and CENTRE in pans and LEVELS - 1 in pans, pans
    assert len(idx) >= min_indices, len(idx)
    assert n >= min_cells, n
    return len(pans), len(idx), n
