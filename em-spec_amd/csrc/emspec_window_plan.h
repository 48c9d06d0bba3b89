// emspec_window_plan.h — internal: the walk over the samples under each delivered column and the three reductions it carries
// (include/emspec.h: emspec_wave_*, emspec_level_*, emspec_cross_*, emspec_set_wave_out, _level_out, _cross_out; DESIGN.md
// §3.12, §3.17, §4.13, §4.19): which samples the window of a group of columns holds, how a launch cuts its windows into teams
// of lanes or pieces over workgroups, what the entries' arguments must obey, the arithmetic of the envelope (keys in the total
// order of the floats) and of the level meters (integers in units of 2^-24), and the scan of one lane's share of a window.
// Integer minima, maxima and sums only: a result is a function of the window's bits, whatever the order, the split of the
// work or the engine's mode.  No HIP, nothing of the engine: tests/test_level_cpu.py runs it through a stand-alone program
// (tests/cdriver/window_plan_driver.cpp) without a GPU.  The kernels (window.hip.inc) and the host forms (emspec_window.cpp)
// call the SAME functions.  Which windows a unit of the host pipeline serves: emspec_pipe_plan.h (wave_run_of, wave_span_of).
#pragma once
#include "../../include/emspec.h"
#include <cstddef>
#include <cstdint>

#ifndef EMSPEC_HD
#ifdef __HIPCC__
#define EMSPEC_HD __host__ __device__
#else
#define EMSPEC_HD
#endif
#endif

namespace emspec {

// ---- geometry.  Group g of f columns of hop samples, `cols` columns in all from `first` samples into the stream on: its
// window is the samples [a, b) of the stream.
struct WindowSpan { int64_t a, b; };
EMSPEC_HD inline WindowSpan window_of(int64_t g, int64_t f, int64_t cols, int64_t hop, int64_t first) {
    const int64_t c0 = g * f, c1 = c0 + f < cols ? c0 + f : cols;
    return WindowSpan{c0 * hop + first, c1 * hop + first};
}
EMSPEC_HD inline int64_t window_longest(int64_t f, int64_t cols, int64_t hop) { return (f < cols ? f : cols) * hop; }

constexpr int kWindowBlock = 256;           // threads of a workgroup
constexpr int64_t kWindowSplit = 16384;     // windows longer than this are cut into pieces over workgroups
constexpr int64_t kWindowPiece = 65536;     // samples of a long window that one workgroup reduces (256 KB)
constexpr int64_t kWindowGridCap = 8 * 256 * 8;   // workgroups: a few per CU, then the grid strides

// Up to kWindowSplit samples: a team of T lanes per window, a power of two with about 16 samples or more per lane
EMSPEC_HD inline int window_team(int64_t longest) {
    int T = 1;
    while (T < 64 && (int64_t)T * 32 <= longest) T *= 2;
    return T;
}
// Longer: `ppw` pieces per window; item `it` of windows x ppw is piece it % ppw of window it / ppw, empty [b, b) where it
// lies past a short last window's end
EMSPEC_HD inline int64_t window_pieces(int64_t longest) { return (longest + kWindowPiece - 1) / kWindowPiece; }
EMSPEC_HD inline WindowSpan window_piece(const WindowSpan& w, int64_t p) {
    const int64_t a = w.a + p * kWindowPiece;
    if (a >= w.b) return WindowSpan{w.b, w.b};
    return WindowSpan{a, a + kWindowPiece < w.b ? a + kWindowPiece : w.b};
}

// ---- what the entries' arguments must obey: null, or the rule they break.  fft_ok: the caller's verdict on n (the FFT-size
// rule lives with the kernels); factor_rule: the message of the entry's own factor rule.
inline const char* window_arg_error(int64_t S, int64_t L, int64_t n, int64_t hop, int64_t factor, bool fft_ok, const char* factor_rule) {
    if (S < 0 || S > 65535) return "need 0..65535 streams";
    if (L < 0) return "the stream length must not be negative";
    if (!fft_ok) return "fft size must be a power of two in [256,16384]";
    if (hop < 1 || hop > n) return "hop must be in [1, fft size]";
    if (factor < 1 || factor > 65536) return factor_rule;
    return nullptr;
}
constexpr const char* kWaveFactorRule = "the envelope's factor must be in [1, 65536]";
constexpr const char* kLevelFactorRule = "the level's factor must be in [1, 65536]";
// ... of a choice of streams: pair p reads streams p views + a and p views + b (a == b is allowed: the stream against itself)
inline const char* cross_pair_error(int64_t pairs, int64_t views, int64_t a, int64_t b) {
    if (views < 1 || views > 64) return "a cross record needs views in 1 .. 64";
    if (a < 0 || a >= views || b < 0 || b >= views) return "a cross record's channels a and b must be in 0 .. views - 1";
    if (pairs < 0 || pairs * views > 65535) return "need pairs x views in 0..65535 streams";
    return nullptr;
}

// ---- the envelope's arithmetic.  u: a sample's 32 bits.
//   key(u) = (u & 0x80000000) ? ~u : (u | 0x80000000)      the total order of the floats, -0.0 < +0.0
//   lo = the sample with the smallest key, hi = the one with the largest, each with its own bits; NaN samples are skipped
// The keys of the samples that are not NaN lie in [key(-inf), key(+inf)].  A NaN counts as key(+inf) for the minimum and as
// key(-inf) for the maximum, which are also the values a reduction starts from: it changes nothing, and a window without a
// sample decodes to (+inf, -inf).
constexpr uint32_t kWaveLoNone = 0xff800000u, kWaveHiNone = 0x007fffffu;
EMSPEC_HD inline void wave_take(uint32_t u, uint32_t& lo, uint32_t& hi) {
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    const bool nan = (u & 0x7fffffffu) > 0x7f800000u;
    const uint32_t kl = nan ? kWaveLoNone : key, kh = nan ? kWaveHiNone : key;
    lo = kl < lo ? kl : lo;
    hi = kh > hi ? kh : hi;
}
EMSPEC_HD inline uint32_t wave_bits(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// ---- the level meters' arithmetic: the quantiser that turns a sample's bits into an integer in units of
// 2^-24, the limb split of a square and of a cross product, the field-wise combine of two records.
constexpr uint32_t kLevelMax = 0x7fffffffu;        // |k| of a saturated sample
constexpr uint32_t kLevelSatBits = 0x43000000u;    // the bits of 128.0f: |x| >= 128, the infinities and every NaN lie at or above
constexpr int64_t kLevelWindowMax = (int64_t)1 << 30;   // samples of the longest window: factor 65536 x hop 16384

// |k| of the sample with bits u, and `odd` one more for a NaN (k = 0) or a saturated sample (|k| = 2^31 - 1).  Below 128 the
// product x 2^24 is exact in binary32 (a power of two; no overflow, and a denormal x gives a normal product or, where denormals
// are flushed, 0 - both round to 0), rint rounds it to nearest, ties to even, and the result is below 2^31.
EMSPEC_HD inline uint32_t level_magnitude(uint32_t u, uint32_t& odd) {
    const uint32_t a = u & 0x7fffffffu;
    if (a >= kLevelSatBits) {
        odd += 1;
        return a > 0x7f800000u ? 0u : kLevelMax;
    }
    float x;
    __builtin_memcpy(&x, &a, 4);
    return (uint32_t)(int32_t)__builtin_rintf(x * 16777216.0f);
}
// k itself
EMSPEC_HD inline int32_t level_quantise(uint32_t u, uint32_t& odd) {
    const int32_t m = (int32_t)level_magnitude(u, odd);
    return (u & 0x80000000u) ? -m : m;
}

// one more sample into a level record: q = k^2 < 2^62 in two 32-bit limbs, each summed in 64 bits (not normalised)
EMSPEC_HD inline void level_take(emspec_level& r, uint32_t u) {
    const uint32_t m = level_magnitude(u, r.odd);
    const uint64_t q = (uint64_t)m * (uint64_t)m;
    r.sq_lo += q & 0xffffffffu;
    r.sq_hi += q >> 32;
    r.peak = m > r.peak ? m : r.peak;
}
// one more pair of samples into a cross record: p = k_A k_B, its low limb unsigned, its high limb with the sign
EMSPEC_HD inline void cross_take(emspec_cross& r, uint32_t ua, uint32_t ub) {
    uint32_t odd = 0;
    const int64_t p = (int64_t)level_quantise(ua, odd) * (int64_t)level_quantise(ub, odd);
    r.lo += (uint64_t)p & 0xffffffffu;
    r.hi += p >> 32;
}
// field-wise: sums add, the peak is the larger.  Associative and commutative, and the record of no sample is all zero.
EMSPEC_HD inline void level_combine(emspec_level& r, const emspec_level& o) {
    r.sq_lo += o.sq_lo;
    r.sq_hi += o.sq_hi;
    r.peak = o.peak > r.peak ? o.peak : r.peak;
    r.odd += o.odd;
}
EMSPEC_HD inline void cross_combine(emspec_cross& r, const emspec_cross& o) {
    r.lo += o.lo;
    r.hi += o.hi;
}

// ---- the three reducers.  Acc: what a lane carries, and what a window's slot of the output holds (8-byte aligned, a multiple
// of 8 bytes); start: the Acc of no sample; take: one more sample (ub: stream B's, for kStreams == 2); combine: associative and
// commutative; kFinish: the slot holds KEYS until `finish` turns them into the samples' bits (the envelope only).
struct alignas(8) WaveKeys { uint32_t lo, hi; };
struct EnvelopeRed {
    using Acc = WaveKeys;
    static constexpr int kStreams = 1;
    static constexpr bool kFinish = true;
    EMSPEC_HD static Acc start() { return Acc{kWaveLoNone, kWaveHiNone}; }
    EMSPEC_HD static void take(Acc& r, uint32_t ua, uint32_t) { wave_take(ua, r.lo, r.hi); }
    EMSPEC_HD static void combine(Acc& r, const Acc& o) {
        r.lo = o.lo < r.lo ? o.lo : r.lo;
        r.hi = o.hi > r.hi ? o.hi : r.hi;
    }
    EMSPEC_HD static Acc finish(const Acc& r) { return Acc{wave_bits(r.lo), wave_bits(r.hi)}; }
};
struct LevelRed {
    using Acc = emspec_level;
    static constexpr int kStreams = 1;
    static constexpr bool kFinish = false;
    EMSPEC_HD static Acc start() { return Acc{0, 0, 0, 0}; }
    EMSPEC_HD static void take(Acc& r, uint32_t ua, uint32_t) { level_take(r, ua); }
    EMSPEC_HD static void combine(Acc& r, const Acc& o) { level_combine(r, o); }
};
struct CrossRed {
    using Acc = emspec_cross;
    static constexpr int kStreams = 2;
    static constexpr bool kFinish = false;
    EMSPEC_HD static Acc start() { return Acc{0, 0}; }
    EMSPEC_HD static void take(Acc& r, uint32_t ua, uint32_t ub) { cross_take(r, ua, ub); }
    EMSPEC_HD static void combine(Acc& r, const Acc& o) { cross_combine(r, o); }
};

// ---- the scan.  Four samples in one load: stream A's where they lie on a 16-byte boundary, stream B's at the same indices,
// 4-byte aligned only.
struct alignas(16) WindowQuadA { uint32_t x, y, z, w; };
struct alignas(4) WindowQuadB { uint32_t x, y, z, w; };
template <int STREAMS> struct WindowQuad;
template <> struct WindowQuad<1> { WindowQuadA a; };
template <> struct WindowQuad<2> { WindowQuadA a; WindowQuadB b; };

template <class Red> EMSPEC_HD inline void window_take1(const uint32_t* xa, const uint32_t* xb, int64_t i, typename Red::Acc& r) {
    if constexpr (Red::kStreams == 2) Red::take(r, xa[i], xb[i]);
    else Red::take(r, xa[i], 0);
}
template <class Red> EMSPEC_HD inline WindowQuad<Red::kStreams> window_load4(const uint32_t* xa, const uint32_t* xb, int64_t i) {   // xa + i: 16-byte aligned
    WindowQuad<Red::kStreams> q;
    q.a = *reinterpret_cast<const WindowQuadA*>(xa + i);
    if constexpr (Red::kStreams == 2) q.b = *reinterpret_cast<const WindowQuadB*>(xb + i);
    return q;
}
template <class Red> EMSPEC_HD inline void window_take4(const WindowQuad<Red::kStreams>& q, typename Red::Acc& r) {
    if constexpr (Red::kStreams == 2) { Red::take(r, q.a.x, q.b.x); Red::take(r, q.a.y, q.b.y); Red::take(r, q.a.z, q.b.z); Red::take(r, q.a.w, q.b.w); }
    else { Red::take(r, q.a.x, 0); Red::take(r, q.a.y, 0); Red::take(r, q.a.z, 0); Red::take(r, q.a.w, 0); }
}

// Lane l of a team of T lanes takes its share of the samples [a, b) of xa (and of xb, at the same indices) into r: the elements
// in front of A's first 16-byte boundary and behind its last one singly, the quads between them T apart - four loads in flight
// while four quads remain, then one quad at a time.  Every sample is taken by exactly one lane exactly once (a sum cannot take
// a quad twice); xa and xb are 4-byte aligned only; nothing outside [a, b) is read.
template <class Red>
EMSPEC_HD inline void window_scan(const uint32_t* xa, const uint32_t* xb, int64_t a, int64_t b, int l, int T, typename Red::Acc& r) {
    int64_t A = a + (int64_t)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(xa + a) >> 2) & 3u)) & 3u);
    if (A > b) A = b;
    const int64_t nq = (b - A) >> 2, B = A + 4 * nq;
    for (int64_t i = a + l; i < A; i += T) window_take1<Red>(xa, xb, i, r);
    for (int64_t i = B + l; i < b; i += T) window_take1<Red>(xa, xb, i, r);
    int64_t j = l;
    for (; j + 3 * (int64_t)T < nq; j += 4 * (int64_t)T) {
        const auto v0 = window_load4<Red>(xa, xb, A + 4 * j), v1 = window_load4<Red>(xa, xb, A + 4 * (j + T)),
                   v2 = window_load4<Red>(xa, xb, A + 4 * (j + 2 * (int64_t)T)), v3 = window_load4<Red>(xa, xb, A + 4 * (j + 3 * (int64_t)T));
        window_take4<Red>(v0, r); window_take4<Red>(v1, r); window_take4<Red>(v2, r); window_take4<Red>(v3, r);
    }
    for (; j < nq; j += T) window_take4<Red>(window_load4<Red>(xa, xb, A + 4 * j), r);
}

// ---- the host forms: x holds rows x views streams of L samples; row p's windows are those of stream p views + a (and, for
// two streams, p views + b), `cols` columns from `first` on in groups of f -> out [rows][ceil(cols / f)] finished Accs, written
// bytewise (out need not be aligned).  The device's scan, as a team of one lane.
template <class Red>
inline void window_reduce_host(const uint32_t* x, int64_t rows, int views, int a, int b, int64_t L, int64_t first, int64_t cols, int hop, int f, void* out) {
    const int64_t Cr = (cols + f - 1) / f;
    char* o = static_cast<char*>(out);
    for (int64_t p = 0; p < rows; ++p)
        for (int64_t g = 0; g < Cr; ++g, o += sizeof(typename Red::Acc)) {
            const WindowSpan w = window_of(g, f, cols, hop, first);
            typename Red::Acc r = Red::start();
            window_scan<Red>(x + (size_t)(p * views + a) * (size_t)L, x + (size_t)(p * views + b) * (size_t)L, w.a, w.b, 0, 1, r);
            if constexpr (Red::kFinish) r = Red::finish(r);
            __builtin_memcpy(o, &r, sizeof r);
        }
}

}  // namespace emspec
