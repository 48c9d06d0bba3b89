// emspec_level.cpp — the level meters (include/emspec.h: emspec_level_device, emspec_level_host, emspec_cross_device,
// emspec_cross_host, emspec_set_level_out, emspec_set_cross_out and the pure helpers): per stream and
// delivered column the exact sum of squares, the peak and the count of odd samples of the column's window, per pair of streams
// the exact sum of products - the samples as integers in units of 2^-24 (emspec_level_plan.h).  The device forms are
// level.hip.inc's kernels on device-resident streams; the host pipeline (emspec_host.cpp) runs the same kernels on each unit's
// staged samples while a setting is on; the host forms are the same functions of the plan header in plain C++.
#include "emspec_engine.h"
#include "emspec_level_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace emspec;

namespace {

// null, or the rule the arguments break (what the device and the host forms share)
const char* arg_error(int64_t S, int64_t L, int32_t n, int32_t hop, int32_t factor) {
    if (!supported_fft(n)) return "fft size must be a power of two in [256,16384]";
    return level_arg_error(S, L, n, hop, factor);
}

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// the sums of a record as one integer each: sq_hi 2^32 + sq_lo < 2^94, |hi 2^32 + lo| likewise
__int128 sum_of(const emspec_level& r) { return ((__int128)r.sq_hi << 32) + (__int128)r.sq_lo; }
__int128 sum_of(const emspec_cross& r) { return (__int128)r.hi * ((__int128)1 << 32) + (__int128)r.lo; }

const double kFullScaleDb = 20.0 * 24.0 * std::log10(2.0);   // 20 log10(2^24)

}  // namespace

extern "C" {

int emspec_level_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor,
                        emspec_level* level_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (const char* why = arg_error(S, L, n, hop, factor)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t C = emspec_num_columns(L, n, hop);
    if (S == 0 || C == 0) return EMSPEC_OK;
    if (!pcm_dev || !level_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(pcm_dev, 4)) return fail(e, EMSPEC_ERR_INVALID_ARG, "pcm_dev must be 4-byte aligned");
    if (!aligned(level_dev, 8)) return fail(e, EMSPEC_ERR_INVALID_ARG, "level_dev must be 8-byte aligned");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_level(pcm_dev, S, L, n / 2 - hop / 2, C, hop, factor, level_dev, reduced_columns(C, factor), (hipStream_t)hip_stream));
    return EMSPEC_OK;
}

int emspec_level_host(const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor, emspec_level* level_out) {
    if (const char* why = arg_error(S, L, n, hop, factor)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t C = emspec_num_columns(L, n, hop), Cr = reduced_columns(C, factor), off = n / 2 - hop / 2;
    if (S == 0 || C == 0) return EMSPEC_OK;
    if (!pcm || !level_out) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(pcm, 4)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "pcm must be 4-byte aligned");
    if (!aligned(level_out, 8)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "level_out must be 8-byte aligned");
    const uint32_t* x = reinterpret_cast<const uint32_t*>(pcm);
    for (int64_t s = 0; s < S; ++s)
        for (int64_t g = 0; g < Cr; ++g) {
            const int64_t c0 = g * factor, c1 = std::min<int64_t>(c0 + factor, C);
            level_out[(size_t)s * (size_t)Cr + (size_t)g] = level_of(x + (size_t)s * (size_t)L + (size_t)(c0 * hop + off), (c1 - c0) * hop);
        }
    return EMSPEC_OK;
}

int emspec_cross_device(emspec_engine* e, const float* pcm_dev, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t L, int32_t n,
                        int32_t hop, int32_t factor, emspec_cross* cross_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (const char* why = cross_pair_error(pairs, views, a, b)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (const char* why = arg_error((int64_t)pairs * views, L, n, hop, factor)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t C = emspec_num_columns(L, n, hop);
    if (pairs == 0 || C == 0) return EMSPEC_OK;
    if (!pcm_dev || !cross_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(pcm_dev, 4)) return fail(e, EMSPEC_ERR_INVALID_ARG, "pcm_dev must be 4-byte aligned");
    if (!aligned(cross_dev, 8)) return fail(e, EMSPEC_ERR_INVALID_ARG, "cross_dev must be 8-byte aligned");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_cross(pcm_dev, pairs, views, a, b, L, n / 2 - hop / 2, C, hop, factor, cross_dev, reduced_columns(C, factor),
                           (hipStream_t)hip_stream));
    return EMSPEC_OK;
}

int emspec_cross_host(const float* pcm, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t L, int32_t n, int32_t hop,
                      int32_t factor, emspec_cross* cross_out) {
    if (const char* why = cross_pair_error(pairs, views, a, b)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    if (const char* why = arg_error((int64_t)pairs * views, L, n, hop, factor)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t C = emspec_num_columns(L, n, hop), Cr = reduced_columns(C, factor), off = n / 2 - hop / 2;
    if (pairs == 0 || C == 0) return EMSPEC_OK;
    if (!pcm || !cross_out) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(pcm, 4)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "pcm must be 4-byte aligned");
    if (!aligned(cross_out, 8)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "cross_out must be 8-byte aligned");
    const uint32_t* x = reinterpret_cast<const uint32_t*>(pcm);
    for (int64_t p = 0; p < pairs; ++p)
        for (int64_t g = 0; g < Cr; ++g) {
            const int64_t c0 = g * factor, c1 = std::min<int64_t>(c0 + factor, C);
            const size_t at = (size_t)(c0 * hop + off);
            cross_out[(size_t)p * (size_t)Cr + (size_t)g] =
                cross_of(x + ((size_t)p * views + a) * (size_t)L + at, x + ((size_t)p * views + b) * (size_t)L + at, (c1 - c0) * hop);
        }
    return EMSPEC_OK;
}

int emspec_set_level_out(emspec_engine* e, emspec_level* level_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (level_out && capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the level records' capacity must not be negative");
    if (!aligned(level_out, 8)) return fail(e, EMSPEC_ERR_INVALID_ARG, "level_out must be 8-byte aligned");
    e->level_out = level_out;
    e->level_capacity = level_out ? capacity : 0;
    return EMSPEC_OK;
}

int emspec_set_cross_out(emspec_engine* e, int32_t a, int32_t b, emspec_cross* cross_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (cross_out && capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the cross records' capacity must not be negative");
    if (cross_out && (a < 0 || a > 63 || b < 0 || b > 63)) return fail(e, EMSPEC_ERR_INVALID_ARG, "a cross record's channels a and b must be in 0 .. 63");
    if (!aligned(cross_out, 8)) return fail(e, EMSPEC_ERR_INVALID_ARG, "cross_out must be 8-byte aligned");
    e->cross_out = cross_out;
    e->cross_capacity = cross_out ? capacity : 0;
    e->cross_a = cross_out ? a : 0;
    e->cross_b = cross_out ? b : 0;
    return EMSPEC_OK;
}

int64_t emspec_level_window(int64_t L, int32_t n, int32_t hop, int32_t factor, int64_t g) {
    if (n < 1 || hop < 1 || hop > n || factor < 1 || factor > 65536 || g < 0) return 0;
    const int64_t C = emspec_num_columns(L, n, hop);
    if (C <= 0 || g >= reduced_columns(C, factor)) return 0;
    return (std::min<int64_t>((g + 1) * factor, C) - g * factor) * hop;
}

int emspec_level_values(const emspec_level* level, int64_t samples, double* rms_db, double* peak_db) {
    if (!level || samples < 1) return EMSPEC_ERR_INVALID_ARG;
    const double sum = std::ldexp((double)level->sq_hi, 32) + (double)level->sq_lo;
    if (rms_db) *rms_db = sum > 0.0 ? 10.0 * std::log10(sum / (double)samples) - kFullScaleDb : -INFINITY;
    if (peak_db) *peak_db = level->peak ? 20.0 * std::log10((double)level->peak) - kFullScaleDb : -INFINITY;
    return EMSPEC_OK;
}

int emspec_cross_correlation(const emspec_level* a, const emspec_level* b, const emspec_cross* ab, double* rho) {
    if (!a || !b || !ab || !rho) return EMSPEC_ERR_INVALID_ARG;
    // each sum as one integer, rounded to binary64 once: identical channels give exactly 1, an inverted one exactly -1
    const double sa = (double)sum_of(*a), sb = (double)sum_of(*b), sab = (double)sum_of(*ab);
    const double den = std::sqrt(sa * sb);
    *rho = den > 0.0 ? std::max(-1.0, std::min(1.0, sab / den)) : 0.0;
    return EMSPEC_OK;
}

}  // extern "C"
