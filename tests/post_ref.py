"""The display post-process law (header comment of em-spec_amd/csrc/post.hip.inc) for the tests:

  reference   the law evaluated sequentially in binary64 on float32 raw columns;
  model_f32   a float32 numpy model of the chunked batch kernels with their constants as parameters - for the CPU
              checks of tests/test_post_cpu.py only: the GPU tests never compare against it;
  bound       the worst-case float32 rounding error of a correct implementation against `reference`, as an expression;
  signals     deterministic streams whose loudness holds a level for 97 columns and then jumps.

Nothing here is taken from oracle.postprocess (a float32 restatement in the kernels' order; it is one of the things
tests/test_post_cpu.py checks against `reference`).
"""
import numpy as np

from emspec import synth

F = np.float32
U = 2.0 ** -24                       # unit roundoff of binary32, round to nearest

# The law's constants are the binary32 numbers the API and the kernels carry (0.02 is not a binary fraction: the law's "0.02"
# is the binary32 number nearest to it, as `smoothing` and `agc_strength` are the binary32 numbers emspec_set_display receives).
AGC_UP, AGC_DOWN, AGC_MAX_GAIN = float(F(0.25)), float(F(0.02)), 40.0
POST_CHUNK, POST_WARM = 1024, 512
SMOOTHING_MAX = 0.95                 # emspec_set_display accepts [0, 0.95]

HOLD = 97                            # columns a level holds (see signals)
LEVELS = (0.9, 0.0, 1e-3, 0.3)


def _per_column(v, C):
    """A setting as binary64 [C] holding binary32 values: a scalar, or one value per column."""
    v = np.asarray(v, F).astype(np.float64)
    return np.full(C, float(v)) if v.ndim == 0 else v.reshape(C)


def level(raw):
    """The AGC level p [S][C] in binary64: p_c = p_{c-1} + k (m_c - p_{c-1}), k = 0.25 rising / 0.02 falling, p_{-1} = m_0."""
    m = np.asarray(raw, F).max(axis=2).astype(np.float64)
    p = np.empty_like(m)
    cur = m[:, 0].copy()
    for c in range(m.shape[1]):
        d = m[:, c] - cur
        cur = cur + np.where(d > 0.0, AGC_UP, AGC_DOWN) * d
        p[:, c] = cur
    return p


def reference(raw, sm, agc, db_top):
    """The law in binary64, sequentially, on float32 raw dB columns raw [S][C][R]:
        m_c = max_r raw[c][r];  p_c as `level`;  g_c = clamp(agc_c (db_top - p_c), -40, 40) (0 where agc_c = 0);
        y_c = sm_c y_{c-1} + (1 - sm_c) (raw_c + g_c),  y_0 = raw_0 + g_0.
    sm / agc: scalars, or one value per column (a change of settings mid-session).  -> (y [S][C][R], g [S][C]), binary64."""
    raw = np.asarray(raw, F)
    S, C, R = raw.shape
    sm, agc = _per_column(sm, C), _per_column(agc, C)
    top = float(F(db_top))
    p = level(raw)
    g = np.clip(agc[None, :] * (top - p), -AGC_MAX_GAIN, AGC_MAX_GAIN)
    g[:, agc <= 0.0] = 0.0
    y = np.empty((S, C, R), np.float64)
    cur = None
    for c in range(C):
        x = raw[:, c, :].astype(np.float64) + g[:, c, None]
        cur = x if c == 0 else sm[c] * cur + (1.0 - sm[c]) * x
        y[:, c, :] = cur
    return y, g


def model_f32(raw, sm, agc, db_top, chunk=POST_CHUNK, warm=POST_WARM, up=0.25, down=0.02, gmax=40, fused=False,
              chunk_start="first"):
    """float32 model of the batch kernels (column_max_kernel, agc_scan_kernel, smooth_apply_kernel): the IIR cut into chunks
    of `chunk` columns, each warmed up over the `warm` columns before it.  fused=True rounds sm*y + a*x once (computed in
    binary64 - both products are exact there - then cast): the compiler is free to contract that expression.
    chunk_start: "first" = a chunk's state starts as its first warm-up column (the kernel); "zero" = it starts from y = 0.
    -> y float32 [S][C][R]."""
    raw = np.asarray(raw, F)
    S, C, R = raw.shape
    sm, ag, top = F(sm), F(agc), F(db_top)
    up, down, gmax = F(up), F(down), F(gmax)
    gain = np.zeros((S, C), F)
    if ag > 0:
        m = raw.max(axis=2)
        p = m[:, 0].copy()
        for c in range(C):
            d = (m[:, c] - p).astype(F)
            p = (p + (np.where(d > 0, up, down).astype(F) * d).astype(F)).astype(F)
            gain[:, c] = np.clip((ag * (top - p).astype(F)).astype(F), -gmax, gmax)
    a = F(F(1.0) - sm)
    out = np.empty_like(raw)
    for c_out in range(0, C, chunk):
        c_end = min(c_out + chunk, C)
        c_beg = (c_out - warm if c_out > warm else 0) if sm > 0 else c_out
        y = None
        for c in range(c_beg, c_end):
            x = (raw[:, c, :] + gain[:, c, None]).astype(F)
            if y is None:
                y = np.zeros_like(x) if chunk_start == "zero" else x
            if c > c_beg or c_beg > 0 or chunk_start == "zero":
                if fused:
                    y = (np.float64(sm) * y.astype(np.float64) + np.float64(a) * x.astype(np.float64)).astype(F)
                else:
                    y = ((sm * y).astype(F) + (a * x).astype(F)).astype(F)
            else:
                y = x
            if c >= c_out:
                out[:, c, :] = y
    return out


def bound(sm, agc, M):
    """Worst-case |float32 implementation - reference| in dB, to first order in u = 2^-24 (second-order terms are below
    2^-20 of it; the roundings-up below are far larger).  M bounds every magnitude that gets rounded: the raw dB, the AGC
    level p (between the smallest and the largest raw peak), x = raw + g and y (a convex combination of x).

    AGC level.  float32: d = fl(m - p), p' = fl(p + fl(k d)); the column peak m is exact (a maximum of float32 numbers).
    With e = p_f32 - p_ref and three roundings d1, d2, d3 (|di| <= u):
        e' = (1 - k) e + k (m - p)(d1 + d2) + d3 p',     |m - p| <= 2 M
        |e'| <= (1 - k) |e| + (4 k + 1) u M.
    If |e| <= B then |e'| <= B as long as B >= (4 + 1/k) u M; the larger demand is k = 0.02: B = 54 u M.
    A `d > 0` decision that differs between the two: fl(m - p) has the sign of m - p, so the decisions differ only if p_ref
    and p_f32 lie on either side of m, i.e. m - p_ref = t e with t in [0, 1].  Then (k_f, k_r the constants each side picked)
        e' = e + k_f (m - p_f32) - k_r (m - p_ref) = e (1 - k_f + (k_f - k_r) t),
    a factor between 1 - k_f and 1 - k_r, so <= 0.98: the step still contracts and the induction above holds unchanged.
    A differing decision costs nothing beyond B.

    Gain.  g = clamp(fl(agc fl(top - p))): clamp is 1-Lipschitz, so the level's error enters scaled by agc, and the two
    roundings act on a number that is at most 40 where it is not clamped anyway: |g_f32 - g_ref| <= agc 54 u M + 2 u 40.

    IIR.  x = fl(raw + g), a = fl(1 - sm), y' = fl(fl(sm y) + fl(a x)): five roundings, of x (<= u M, scaled by 1 - sm),
    of a (<= u (1 - sm) M), of the two products (<= u sm M and u (1 - sm) M) and of the sum (<= u M):
        |e_y'| <= sm |e_y| + (1 - sm) |g_f32 - g_ref| + (4 - 2 sm) u M <= sm |e_y| + (1 - sm) |e_g| + 4 u M,
    hence |e_y| <= 4 u M / (1 - sm) + max |e_g|.  The first column (y = x) and a contracted sm y + a x (one rounding fewer)
    are below the same figure.

    Chunks.  The batch form may restart the recurrence from x at a column 512 before its first output: what is left of the
    difference to the true state, at most 2 M, is 2 M sm^512 - 4e-12 x 2 M at sm = 0.95, the largest accepted smoothing and
    the one POST_WARM = 512 is sized for (1.3e-4 u M; at a warm-up of 128 columns it would be 2.8e-3 M).  The only term that
    is not a rounding error.

    sm / agc: scalars or per-column arrays (the largest is taken)."""
    sm = float(np.max(np.asarray(sm, F)))
    agc = float(np.max(np.asarray(agc, F)))
    M = float(M)
    e_level = (4.0 + 1.0 / AGC_DOWN) * U * M
    e_gain = (agc * e_level + 2.0 * U * AGC_MAX_GAIN) if agc > 0.0 else 0.0
    return 4.0 * U * M / (1.0 - sm) + e_gain + 2.0 * M * sm ** POST_WARM


def signals(S, L, hop=256, fs=48000.0):
    """S deterministic float32 streams of L samples: three tones (frequencies and phases from emspec.synth's counter-based
    uniforms, stream s: seed 2000 + s) and a little noise, under an amplitude that holds a level for HOLD = 97 columns'
    worth of samples (97 hop) and then jumps.  The levels cycle through 0.9, exact zeros, 1e-3 and 0.3; stream s starts s
    places into the cycle and scales the non-zero levels by 1 / (1 + 0.13 (s // 4)), so no two streams agree and a stream
    mix-up shows.  97 is prime to the chunk arithmetic: steps fall 27 columns before column 512 and 81 before 1536, where
    the warm-ups of the batch kernel's second and third chunk start, and at column 1067, 43 after the second chunk begins.
    Every sample depends on its index alone: signals(S, L1) is a prefix of signals(S, L2)."""
    t = np.arange(L, dtype=np.float64)
    seg = (np.arange(L) // (HOLD * hop)).astype(np.int64)
    out = np.empty((S, L), F)
    for s in range(S):
        u = synth.uniform(2000 + s, 8)
        x = np.zeros(L)
        for i, amp in enumerate((1.0, 0.1, 0.01)):
            f = 100.0 * 100.0 ** u[i]                                  # 100 Hz .. 10 kHz
            x += amp * np.sin(2 * np.pi * (f / fs) * t + 2 * np.pi * u[3 + i])
        x += 2e-3 * (synth.uniform(3000 + s, L) - 0.5)
        lv = np.array(LEVELS) / (1.0 + 0.13 * (s // 4))
        out[s] = (0.9 * x * lv[(seg + s) % len(LEVELS)]).astype(F)
    return out


def cell_index_f32(db, db_top, db_range=80.0, gate_db=-80.0):
    """float32 restatement of cell_index (emspec_device.h) on dB values: the palette index, uint8."""
    db = np.asarray(db, F)
    lo = F(F(db_top) - F(db_range))
    inv = F(1.0 / float(F(db_range)))
    v = ((db - lo).astype(F) * inv).astype(F)
    v = np.clip(v, F(0), F(1))
    v[db < F(gate_db)] = 0
    return ((v * F(255.0)).astype(F) + F(0.5)).astype(F).astype(np.int32).astype(np.uint8)


def index_borderline(db, db_top, db_range=80.0, gate_db=-80.0):
    """Cells where the binary64 value of v 255 + 0.5 lies within 2^-14 of an integer: there a float32 evaluation may land
    on either side, and the palette index may differ by one."""
    db = np.asarray(db, np.float64)
    lo = float(F(db_top)) - float(F(db_range))
    v = np.clip((db - lo) * float(F(1.0 / float(F(db_range)))), 0.0, 1.0)
    v[db < float(F(gate_db))] = 0.0
    t = v * 255.0 + 0.5
    return np.abs(t - np.rint(t)) <= 2.0 ** -14
