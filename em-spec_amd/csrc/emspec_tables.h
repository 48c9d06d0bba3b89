// emspec_tables.h — internal: everything the kernels take as given, computed on the host: the twiddle and
// row-edge tables in float32 and binary64, the specified ratio^x and cos/sin evaluations, the palettes and the per-shape scalars of
// PlanDev / ExactPlanDev / DbMap / ExactDbMap.  The order of the floating-point operations is the specification.  No HIP, nothing
// of the engine: tests/test_tables_cpu.py compares every bit with the bit models.
#pragma once
#include "../../include/emspec.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace emspec {

// (oracle/emspec_exact.c:ex_cos_sin states the same operations)
/* cos and sin of a in [0, pi/4] by their Taylor series in Horner form, plain binary64 operations in this order (no
 * libm call: glibc's sincos(), which gcc substitutes for a cos()/sin() pair, and its separate cos()/sin() differ in the
 * last bit for some arguments, so a table built from libm depends on the compiler).  Truncation < 3e-18; result
 * within about one ulp. */
inline void cos_sin_octant(double a, double* c, double* s) {
    const double z = a * a;
    double ps = -1.0 / 121645100408832000.0;       /* -1/19! */
    ps = ps * z + 1.0 / 355687428096000.0;         /* +1/17! */
    ps = ps * z - 1.0 / 1307674368000.0;           /* -1/15! */
    ps = ps * z + 1.0 / 6227020800.0;              /* +1/13! */
    ps = ps * z - 1.0 / 39916800.0;                /* -1/11! */
    ps = ps * z + 1.0 / 362880.0;                  /* +1/9! */
    ps = ps * z - 1.0 / 5040.0;                    /* -1/7! */
    ps = ps * z + 1.0 / 120.0;                     /* +1/5! */
    ps = ps * z - 1.0 / 6.0;                       /* -1/3! */
    *s = a + a * (ps * z);
    double pc = 1.0 / 6402373705728000.0;          /* +1/18! */
    pc = pc * z - 1.0 / 20922789888000.0;          /* -1/16! */
    pc = pc * z + 1.0 / 87178291200.0;             /* +1/14! */
    pc = pc * z - 1.0 / 479001600.0;               /* -1/12! */
    pc = pc * z + 1.0 / 3628800.0;                 /* +1/10! */
    pc = pc * z - 1.0 / 40320.0;                   /* -1/8! */
    pc = pc * z + 1.0 / 720.0;                     /* +1/6! */
    pc = pc * z - 1.0 / 24.0;                      /* -1/4! */
    pc = pc * z + 0.5;                             /* +1/2! */
    *c = 1.0 - pc * z;
}

// (oracle/emspec_oracle.c: eo_spec_pow states the same operations)
/* ratio^x by a SPECIFIED evaluation: exp2(x * log2(ratio)) from plain IEEE binary64 operations in this
 * order - no libm, whose pow() is not correctly rounded and differs between C libraries, so a table built from it would
 * depend on the host.  log2 by the atanh series on the mantissa folded into [1/sqrt2, sqrt2]; 2^f, |f| <= 1/2,
 * by the Taylor series of e^(f ln 2) in Horner form (truncation < 4e-18); scaling by 2^i is exact.  Within ~3 ulp of the
 * real value; what matters is that every build produces the same bits. */
inline double spec_log2(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    int e = (int)((u >> 52) & 0x7ff) - 1023;
    u = (u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;
    double m;
    memcpy(&m, &u, 8);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double pz = 1.0 / 21.0;
    pz = pz * z + 1.0 / 19.0;
    pz = pz * z + 1.0 / 17.0;
    pz = pz * z + 1.0 / 15.0;
    pz = pz * z + 1.0 / 13.0;
    pz = pz * z + 1.0 / 11.0;
    pz = pz * z + 1.0 / 9.0;
    pz = pz * z + 1.0 / 7.0;
    pz = pz * z + 1.0 / 5.0;
    pz = pz * z + 1.0 / 3.0;
    pz = pz * z + 1.0;
    return (double)e + (s * pz) * 2.8853900817779268; /* 2 / ln 2 */
}
inline double spec_exp2(double x) {
    const double i = (double)(long long)(x < 0.0 ? x - 0.5 : x + 0.5); /* nearest integer (halves away from zero) */
    const double t = (x - i) * 0.6931471805599453;                    /* x - i is exact; |t| <= 0.3466 */
    double p = 1.0 / 87178291200.0;      /* 1/14! */
    p = p * t + 1.0 / 6227020800.0;      /* 1/13! */
    p = p * t + 1.0 / 479001600.0;       /* 1/12! */
    p = p * t + 1.0 / 39916800.0;        /* 1/11! */
    p = p * t + 1.0 / 3628800.0;         /* 1/10! */
    p = p * t + 1.0 / 362880.0;          /* 1/9! */
    p = p * t + 1.0 / 40320.0;           /* 1/8! */
    p = p * t + 1.0 / 5040.0;            /* 1/7! */
    p = p * t + 1.0 / 720.0;             /* 1/6! */
    p = p * t + 1.0 / 120.0;             /* 1/5! */
    p = p * t + 1.0 / 24.0;              /* 1/4! */
    p = p * t + 1.0 / 6.0;               /* 1/3! */
    p = p * t + 0.5;                     /* 1/2! */
    p = p * t + 1.0;
    p = p * t + 1.0;
    const uint64_t su = (uint64_t)(1023 + (long long)i) << 52;        /* 2^i, |i| < 1000 */
    double sd;
    memcpy(&sd, &su, 8);
    return p * sd;
}
inline double spec_pow(double ratio, double x) {
    if (x == 1.0) return ratio; /* the axis ends exactly at fmax (as pow(ratio, 1) would) */
    return spec_exp2(x * spec_log2(ratio));
}

inline int latency(int n, int hop, int reassign) { return reassign ? (n + 2 * hop - 1) / (2 * hop) : 0; }

// The frequency axis: `rows` rows between rows + 1 edges - log-spaced from fmin to fmax, or the table custom_hz (rows + 1 entries
// in Hz, emspec_set_row_edges_hz) when that is not null.
struct Axis {
    int rows;
    float sample_rate, fmin_hz, fmax_hz;
    const float* custom_hz;
};
inline Axis axis_of(const emspec_config& c, const std::vector<float>& custom_hz) {
    return Axis{c.rows, c.sample_rate, c.fmin_hz, c.fmax_hz, custom_hz.empty() ? nullptr : custom_hz.data()};
}
inline double edge_hz(const Axis& a, int r) {
    return a.custom_hz ? (double)a.custom_hz[r]
                       : (double)a.fmin_hz * spec_pow((double)a.fmax_hz / (double)a.fmin_hz, (double)r / (double)a.rows);
}
// Row edges in DFT-bin units (DESIGN.md §3 "Tables"): binary64, and the float32 table is that one rounded once per entry.
// The axis ends at Nyquist by construction: e[R] = min(e[R], n / 2).  fmax <= sample_rate / 2 is enforced by emspec_create, but
// fmin * (fmax / fmin) * n / fs rounds twice and can come out an ulp above n / 2 (8 kHz from 30 Hz to 4 kHz: + 4.5e-13 at
// n = 4096); the Nyquist bin, whose k-hat is exactly n / 2, would then belong to row R - 1 in binary64 and to no row in float32.
// With the clamp k-hat = n / 2 >= e[R] in both precisions, so no route of either mode accumulates that bin.  (Custom edges satisfy
// it already: hz <= 0.5f * fs is checked, hz * n is exact in double and the division is monotone.)
inline std::vector<double> edges_bin64(const Axis& a, int n) {
    std::vector<double> e((size_t)a.rows + 1);
    for (int r = 0; r <= a.rows; ++r) e[r] = edge_hz(a, r) * (double)n / (double)a.sample_rate;
    e[a.rows] = std::min(e[a.rows], (double)n * 0.5);
    return e;
}
inline std::vector<float> edges_bin32(const std::vector<double>& e64) { return std::vector<float>(e64.begin(), e64.end()); }
// null, or why a table of edges cannot serve: the row lookup needs strictly increasing edges in the precision it compares in
template <class T> bool strictly_increasing(const std::vector<T>& e) {
    for (size_t r = 0; r + 1 < e.size(); ++r)
        if (!(e[r] < e[r + 1])) return false;
    return true;
}
inline const char* edges_error(const std::vector<float>& e) {
    return strictly_increasing(e) ? nullptr : "row edges are not strictly increasing in float32 (too many rows for this range)";
}
inline const char* edges_error(const std::vector<double>& e) { return strictly_increasing(e) ? nullptr : "row edges are not strictly increasing"; }
// EXACT mode, the no-parking kernel's axis test: at most 6 % of a frame's bins (of the band up to sample_rate / 2) lie below `row`
inline bool low_share_ok(const Axis& a, int row) {
    const double share = edge_hz(a, row) / ((double)a.sample_rate * 0.5);
    return share <= 0.06;
}

// May the FAST kernels' log2 row hint (emspec_device.h: HintLookup) serve a log axis from e0 to eR bins in `rows` rows?  The hint
// f = fma(v_log_f32(k), rscale, c0), l2e0 = log2f(e0), rscale = rows / (log2f(eR) - l2e0), c0 = fma(-l2e0, rscale, 1/2)
// (emspec_row_hint.h), is k's position on the axis in rows plus one half; its integer part names the NEAREST edge, and one
// compare against that edge decides the row.  That is right while the position's error stays below HALF a row (the integer
// part is then one of the two edges around k).  With u = 2^-23 (one float32 ulp is at most u |x|),
// L = max(1, |log2 e0|, |log2 eR|) the largest |log2| of a k on the axis, W = log2(eR / e0) <= 2 L and rho = rows / W rows per
// unit of log2, the error in rows is at most
//     rho * (u L      v_log_f32: 1 ulp, the ISA documentation's figure
//          + u L      l2e0: log2f is within 1 ulp
//          + u L      c0, rounded once: u (rho L + 1/2) / 2 - half of this line; the other half is spare
//          + 2 u L    rscale's denominator: two logarithms and a rounding, relative to W, on a hint of at most `rows` rows (the
//                     SAME rscale multiplies the logarithm and l2e0, so its error scales their difference, as it did the product's)
//          + 2 u)     e0 and eR are the float32 table's ends, and an edge sits half an ulp from its log-spaced place: 1.44 u / 2 each
//     + 2 u rows      the quotient rscale and the fma's one rounding of a value of at most `rows` + 1: u / 2 each, doubled
//   <= u (8 rho L + 2 rows),
// which must stay below 1 / 4: a safety factor of 2 against the half row, since the instruction's figure is documented, not
// measured here.  (The earlier two-edge form, h = (log - l2e0) * rscale corrected by one row either way against eb[r0] and
// eb[r0 + 1], needed only "within one row" and had the same terms: the difference's rounding where c0's stands now, and two
// roundings of at most `rows`.  The bound, and so the set of hinted axes, did not change.)  k off the
// axis by d in log2 adds d u to the error and d rho to the distance, so the clamped hint still ends on the first or last edge.
// The default axis has 8 rho L + 2 rows = 1.3e4 at 1024 rows, one octave in 4096 rows 4.3e5; the bound, 2^21, is reached near
// 20,000 rows per unit of log2 (a row 5e-5 wide, 290 float32 ulp at 8192 bins).  Narrower axes are searched (PlanDev::log_rows
// = 0, the generic per-bin core): the same rows, slower.  spec_log2: the same answer on every host.
inline bool hint_rows_ok(double e0, double eR, int rows) {
    if (!(e0 > 0.0) || !(eR > e0) || rows < 1) return false;
    const double l0 = spec_log2(e0), lR = spec_log2(eR);
    const double L = std::max(1.0, std::max(std::fabs(l0), std::fabs(lR)));
    const double rho = (double)rows / (lR - l0);
    return 8.0 * rho * L + 2.0 * (double)rows <= 2097152.0;   // 2^23 / 4
}

// Twiddles tw[q] = (cos, -sin)(2 pi q / n), q < n / 2, interleaved.  The first quarter is the caller's; this writes the second by
// symmetry: tw[q + N/4] = -j tw[q] = (tw[q].im, -tw[q].re).  With a correctly rounded libm this is what cos/sin give anyway
// (checked for every N here); writing it down makes it a property of the table that the kernels may rely on (fused_n16384.hip.inc
// loads 8 pass-1 twiddles instead of 15).  The bit models do the same.
template <class T> void twiddle_second_quarter(std::vector<T>& tw, int n) {
    for (int q = 0; q < n / 4; ++q) {
        tw[2 * (q + n / 4)] = tw[2 * q + 1];
        tw[2 * (q + n / 4) + 1] = -tw[2 * q];
    }
    tw[2 * (n / 4)] = (T)0.0;       // quarter turn is exact: (0,-1)
    tw[2 * (n / 4) + 1] = (T)-1.0;
}
// float32: evaluated in double, rounded once to float
inline std::vector<float> twiddles32(int n) {
    std::vector<float> tw((size_t)n);
    const double pi = 3.14159265358979323846;
    for (int q = 0; q < n / 2; ++q) {
        const double a = 2.0 * pi * (double)q / (double)n;
        tw[2 * q] = (float)std::cos(a);
        tw[2 * q + 1] = (float)(-std::sin(a));
    }
    twiddle_second_quarter(tw, n);
    return tw;
}
// binary64 (oracle/emspec_exact.c: ex_twiddle): first octant by the specified series, second by cos(pi/2 - x) = sin x
inline std::vector<double> twiddles64(int n) {
    std::vector<double> tw((size_t)n);
    const double pi = 3.14159265358979323846;
    for (int q = 0; q <= n / 8; ++q) {
        double c, sn;
        cos_sin_octant(2.0 * pi * (double)q / (double)n, &c, &sn);
        tw[2 * q] = c;
        tw[2 * q + 1] = -sn;
        if (q > 0) {
            tw[2 * (n / 4 - q)] = sn;
            tw[2 * (n / 4 - q) + 1] = -c;
        }
    }
    twiddle_second_quarter(tw, n);
    return tw;
}

// The per-shape scalars the kernels are handed (emspec_device.h: PlanDev, ExactPlanDev), without the device pointers.  tscale and
// pfloor are the binary64 plan's; the float32 plan's are those rounded once.
struct PlanScalars {
    int rows, log_rows, D, reassign, hop;
    double tscale;   // (N/2)/hop
    double pfloor;   // gate on |X_h|^2
    float tscale32, pfloor_abs;
};
inline PlanScalars plan_scalars(const emspec_config& c, int rows, bool log_rows, int n, int hop, int reassign) {
    PlanScalars d;
    d.rows = rows;
    d.log_rows = log_rows ? 1 : 0;
    d.D = latency(n, hop, reassign);
    d.reassign = reassign ? 1 : 0;
    d.hop = hop;
    d.tscale = (double)n / 2.0 / (double)hop;
    const double pk = (double)n / 4.0;   // |X_h| of a full-scale sine
    d.pfloor = (double)c.power_floor * pk * pk;
    d.tscale32 = (float)d.tscale;
    d.pfloor_abs = (float)d.pfloor;
    return d;
}
// EXACT mode: the fixed point of the histogram, and the float32 log2 hint of the row lookup from the ends e0 / eR of the plan's
// binary64 edge table (oracle/emspec_exact.c: explan_init)
struct ExactScalars {
    double pmax, qscale, pfloor64, pmax64, qscale64;
    float l2e0, rscale;
};
inline ExactScalars exact_scalars(int n, int rows, double pfloor, double e0, double eR) {
    ExactScalars d;
    int log2n = 0;
    while ((1 << log2n) < n) ++log2n;
    d.qscale = std::ldexp(1.0, 52 - (2 * log2n - 4));
    d.pmax = std::ldexp(1.0, 61) / d.qscale;
    d.pfloor64 = 64.0 * pfloor;
    d.pmax64 = 64.0 * d.pmax;
    d.qscale64 = d.qscale / 64.0;
    d.l2e0 = std::log2((float)e0);
    d.rscale = (float)rows / (std::log2((float)eR) - d.l2e0);
    return d;
}
// stage "dB + colour" (DbMap; ExactDbMap, whose `scale` is its sc): every constant rounded once to binary32
struct DbScalars { float scale, lo, inv_range, gate; };
inline DbScalars db_scalars(const emspec_config& c, int n) {
    DbScalars m;
    const double nn = (double)n;
    m.scale = (float)(32.0 / (3.0 * nn * nn) * (double)c.gain * (double)c.gain);
    m.lo = c.db_top - c.db_range;
    m.inv_range = (float)(1.0 / (double)c.db_range);
    m.gate = c.gate_db;
    return m;
}
// (oracle/emspec_exact.c: eo_batch_exact states the same operations)
inline DbScalars exact_db_scalars(const emspec_config& c, int n, double qscale) {
    DbScalars m;
    const double nn = (double)n;
    const double scale = 32.0 / (3.0 * nn * nn) * (double)c.gain * (double)c.gain;
    m.scale = (float)(scale * (1.0 / qscale));
    m.lo = (float)((double)c.db_top - (double)c.db_range);
    m.inv_range = (float)(1.0 / (double)c.db_range);
    m.gate = c.gate_db;
    return m;
}

// 5-stop gradient measured from the reference's settings screenshot (assets/settings.png): 0/25/50/75/100 %.
constexpr int kPaletteStops[5][3] = {{0, 0, 0}, {80, 0, 80}, {200, 50, 50}, {255, 150, 0}, {255, 255, 200}};
// the default palette: integer interpolation, 256 RGBA entries
inline void default_lut(uint8_t* lut) {
    for (int i = 0; i < 256; ++i) {
        const int pos = 4 * i;
        const int seg = pos >= 3 * 255 ? 3 : pos / 255;
        const int w1 = pos - seg * 255, w0 = 255 - w1;
        for (int c = 0; c < 3; ++c) lut[4 * i + c] = (uint8_t)((kPaletteStops[seg][c] * w0 + kPaletteStops[seg + 1][c] * w1 + 127) / 255);
        lut[4 * i + 3] = 255;
    }
}
// emspec_make_colormap's law: the same stops stretched by brightness / 0.5 and clipped
inline void make_colormap(float brightness, uint8_t* out) {
    for (int i = 0; i < 256; ++i) {
        const double v = std::min(1.0, ((double)i / 255.0) * ((double)brightness / 0.5));
        const double t = v * 4.0;
        const int s = std::min(3, (int)std::floor(t));
        const double f = t - (double)s;
        for (int c = 0; c < 3; ++c) {
            const double a = (double)kPaletteStops[s][c], b = (double)kPaletteStops[s + 1][c];
            out[4 * i + c] = (uint8_t)std::floor(a + f * (b - a) + 0.5);
        }
        out[4 * i + 3] = 255;
    }
}
// emspec_warped_edges_hz's law: rows + 1 edges in Hz
inline void warped_edges_hz(int rows, float fmin_hz, float fmax_hz, float low_end_boost, float freq_scale, float* out) {
    const double span = std::log((double)fmax_hz / (double)fmin_hz) / (double)freq_scale;
    for (int r = 0; r <= rows; ++r)
        out[r] = (float)((double)fmin_hz * std::exp(span * std::pow((double)r / (double)rows, (double)low_end_boost)));
}

}  // namespace emspec
