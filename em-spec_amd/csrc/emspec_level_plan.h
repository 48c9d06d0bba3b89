// emspec_level_plan.h — internal: the arithmetic of the level meters (include/emspec.h: emspec_level_*, emspec_cross_*,
// emspec_set_level_out, emspec_set_cross_out): the quantiser that turns a sample's bits into an integer in
// units of 2^-24, the limb split of a square and of a cross product, the field-wise combine of two records, and what the entries'
// arguments must obey.  Integers only behind the quantiser: a record is a sum or a maximum of integers, so it does not depend on
// the order, the split of the work or the engine's mode.  No HIP, nothing of the engine: tests/test_level_cpu.py runs it through
// a stand-alone program (tests/cdriver/level_plan_driver.cpp) without a GPU.  The kernels (level.hip.inc) and the host forms
// (emspec_level.cpp) call the SAME functions.  The windows are the envelope's (emspec_pipe_plan.h: wave_run_of, wave_span_of).
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

// The definition on host arrays, one window: x[0 .. count)
inline emspec_level level_of(const uint32_t* x, int64_t count) {
    emspec_level r = {0, 0, 0, 0};
    for (int64_t i = 0; i < count; ++i) level_take(r, x[i]);
    return r;
}
inline emspec_cross cross_of(const uint32_t* xa, const uint32_t* xb, int64_t count) {
    emspec_cross r = {0, 0};
    for (int64_t i = 0; i < count; ++i) cross_take(r, xa[i], xb[i]);
    return r;
}

// null, or the rule the arguments break.  (The FFT-size rule is the caller's: it lives with the kernels.)
inline const char* level_arg_error(int64_t S, int64_t L, int64_t n, int64_t hop, int64_t factor) {
    if (S < 0 || S > 65535) return "need 0..65535 streams";
    if (L < 0) return "the stream length must not be negative";
    if (hop < 1 || hop > n) return "hop must be in [1, fft size]";
    if (factor < 1 || factor > 65536) return "the level's factor must be in [1, 65536]";
    return nullptr;
}
// ... of a choice of streams: pair p reads streams p views + a and p views + b (a == b is allowed: the stream against itself)
inline const char* cross_pair_error(int64_t pairs, int64_t views, int64_t a, int64_t b) {
    if (views < 1 || views > 64) return "a cross record needs views in 1 .. 64";
    if (a < 0 || a >= views || b < 0 || b >= views) return "a cross record's channels a and b must be in 0 .. views - 1";
    if (pairs < 0 || pairs * views > 65535) return "need pairs x views in 0..65535 streams";
    return nullptr;
}

}  // namespace emspec
