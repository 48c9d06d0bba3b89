// emspec_window.cpp — the reductions over the samples under each delivered column (include/emspec.h; DESIGN.md §3.12, §3.17,
// §4.13, §4.19): the waveform envelope (emspec_wave_device, emspec_wave_host, emspec_set_wave_out) - per stream and column the
// smallest and the largest sample of the column's window, in the total order of the floats - and the level meters
// (emspec_level_device, _host, emspec_cross_device, _host, emspec_set_level_out, emspec_set_cross_out and the pure helpers) -
// the exact sum of squares, the peak and the count of odd samples, per pair of streams the exact sum of products, the samples
// as integers in units of 2^-24.  The device forms are window.hip.inc's kernels on device-resident streams; the host pipeline
// (emspec_host.cpp) runs the same kernels on each unit's staged samples while a setting is on; the host forms run the same scan
// with the same reducers (emspec_window_plan.h) in plain C++.
#include "emspec_engine.h"
#include "emspec_window_plan.h"

#include <algorithm>
#include <cmath>

using namespace emspec;

namespace {

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// What one entry asks beside the shared rules: its factor rule, the alignment its output needs and what it says of a misaligned
// pcm and a misaligned output.
struct Entry { const char* factor_rule; uintptr_t out_align; const char *pcm_rule, *out_rule; };
constexpr Entry kWaveDevice{kWaveFactorRule, 8, "pcm_dev must be 4-byte aligned", "wave_dev must be 8-byte aligned"};
constexpr Entry kWaveHost{kWaveFactorRule, 4, "pcm and wave_out must be 4-byte aligned", "pcm and wave_out must be 4-byte aligned"};
constexpr Entry kLevelDevice{kLevelFactorRule, 8, "pcm_dev must be 4-byte aligned", "level_dev must be 8-byte aligned"};
constexpr Entry kLevelHost{kLevelFactorRule, 8, "pcm must be 4-byte aligned", "level_out must be 8-byte aligned"};
constexpr Entry kCrossDevice{kLevelFactorRule, 8, "pcm_dev must be 4-byte aligned", "cross_dev must be 8-byte aligned"};
constexpr Entry kCrossHost{kLevelFactorRule, 8, "pcm must be 4-byte aligned", "cross_out must be 8-byte aligned"};

// Every entry: the argument rule, the empty case, the null and alignment checks, then run(C, first) - the launch or the loop -
// over `rows` rows of `views` streams each.  e: null for the host forms.
template <class Run>
int entry(emspec_engine* e, const Entry& en, int64_t rows, int64_t views, int64_t L, int32_t n, int32_t hop, int32_t factor, const void* pcm,
          const void* out, Run&& run) {
    if (const char* why = window_arg_error(rows * views, L, n, hop, factor, supported_fft(n), en.factor_rule)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t C = emspec_num_columns(L, n, hop);
    if (rows == 0 || C == 0) return EMSPEC_OK;
    if (!pcm || !out) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(pcm, 4)) return fail(e, EMSPEC_ERR_INVALID_ARG, en.pcm_rule);
    if (!aligned(out, en.out_align)) return fail(e, EMSPEC_ERR_INVALID_ARG, en.out_rule);
    return run(C, (int64_t)(n / 2 - hop / 2));
}
// ... of a device form: launch(C, first) on the engine's device
template <class Launch>
int device_entry(emspec_engine* e, const Entry& en, int64_t rows, int64_t views, int64_t L, int32_t n, int32_t hop, int32_t factor, const void* pcm,
                 const void* out, Launch&& launch) {
    return entry(e, en, rows, views, L, n, hop, factor, pcm, out, [&](int64_t C, int64_t first) {
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, launch(C, first));
        return (int)EMSPEC_OK;
    });
}
// ... of a host form: the reducer's loop
template <class Red>
int host_entry(const Entry& en, const float* pcm, int64_t rows, int32_t views, int32_t a, int32_t b, int64_t L, int32_t n, int32_t hop, int32_t factor,
               void* out) {
    return entry(nullptr, en, rows, views, L, n, hop, factor, pcm, out, [&](int64_t C, int64_t first) {
        window_reduce_host<Red>(reinterpret_cast<const uint32_t*>(pcm), rows, views, a, b, L, first, C, hop, factor, out);
        return (int)EMSPEC_OK;
    });
}

// the sums of a record as one integer each: sq_hi 2^32 + sq_lo < 2^94, |hi 2^32 + lo| likewise
__int128 sum_of(const emspec_level& r) { return ((__int128)r.sq_hi << 32) + (__int128)r.sq_lo; }
__int128 sum_of(const emspec_cross& r) { return (__int128)r.hi * ((__int128)1 << 32) + (__int128)r.lo; }

const double kFullScaleDb = 20.0 * 24.0 * std::log10(2.0);   // 20 log10(2^24)

}  // namespace

extern "C" {

int emspec_wave_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor,
                       emspec_wave* wave_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    return device_entry(e, kWaveDevice, S, 1, L, n, hop, factor, pcm_dev, wave_dev, [&](int64_t C, int64_t first) {
        return launch_wave(pcm_dev, S, L, first, C, hop, factor, wave_dev, reduced_columns(C, factor), (hipStream_t)hip_stream);
    });
}

int emspec_wave_host(const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor, emspec_wave* wave_out) {
    return host_entry<EnvelopeRed>(kWaveHost, pcm, S, 1, 0, 0, L, n, hop, factor, wave_out);
}

int emspec_level_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor,
                        emspec_level* level_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    return device_entry(e, kLevelDevice, S, 1, L, n, hop, factor, pcm_dev, level_dev, [&](int64_t C, int64_t first) {
        return launch_level(pcm_dev, S, L, first, C, hop, factor, level_dev, reduced_columns(C, factor), (hipStream_t)hip_stream);
    });
}

int emspec_level_host(const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor, emspec_level* level_out) {
    return host_entry<LevelRed>(kLevelHost, pcm, S, 1, 0, 0, L, n, hop, factor, level_out);
}

int emspec_cross_device(emspec_engine* e, const float* pcm_dev, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t L, int32_t n,
                        int32_t hop, int32_t factor, emspec_cross* cross_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (const char* why = cross_pair_error(pairs, views, a, b)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    return device_entry(e, kCrossDevice, pairs, views, L, n, hop, factor, pcm_dev, cross_dev, [&](int64_t C, int64_t first) {
        return launch_cross(pcm_dev, pairs, views, a, b, L, first, C, hop, factor, cross_dev, reduced_columns(C, factor), (hipStream_t)hip_stream);
    });
}

int emspec_cross_host(const float* pcm, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t L, int32_t n, int32_t hop,
                      int32_t factor, emspec_cross* cross_out) {
    if (const char* why = cross_pair_error(pairs, views, a, b)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    return host_entry<CrossRed>(kCrossHost, pcm, pairs, views, a, b, L, n, hop, factor, cross_out);
}

int emspec_set_wave_out(emspec_engine* e, emspec_wave* wave_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (wave_out && capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the envelope's capacity must not be negative");
    if (!aligned(wave_out, 4)) return fail(e, EMSPEC_ERR_INVALID_ARG, "wave_out must be 4-byte aligned");
    e->wave_out = wave_out;
    e->wave_capacity = wave_out ? capacity : 0;
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
    const WindowSpan w = window_of(g, factor, C, hop, 0);
    return w.b - w.a;
}

// The factor law as a helper: the field-wise sum (peak: maximum) of `count` records - level_combine / cross_combine with checked
// adds, so that a sum no limb can hold is refused instead of wrapping.  *out is written only on success (it may be records[i]).
int emspec_level_sum(const emspec_level* records, int64_t count, emspec_level* out) {
    if (!records || !out || count < 1) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "emspec_level_sum needs records, an output and count >= 1");
    emspec_level r = LevelRed::start();
    bool wrapped = false;
    for (int64_t i = 0; i < count; ++i) {
        wrapped |= __builtin_add_overflow(r.sq_lo, records[i].sq_lo, &r.sq_lo);
        wrapped |= __builtin_add_overflow(r.sq_hi, records[i].sq_hi, &r.sq_hi);
        wrapped |= __builtin_add_overflow(r.odd, records[i].odd, &r.odd);
        r.peak = std::max(r.peak, records[i].peak);
    }
    if (wrapped) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "emspec_level_sum: a limb of the sum does not fit its field");
    *out = r;
    return EMSPEC_OK;
}

int emspec_cross_sum(const emspec_cross* records, int64_t count, emspec_cross* out) {
    if (!records || !out || count < 1) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "emspec_cross_sum needs records, an output and count >= 1");
    emspec_cross r = CrossRed::start();
    bool wrapped = false;
    for (int64_t i = 0; i < count; ++i) {
        wrapped |= __builtin_add_overflow(r.lo, records[i].lo, &r.lo);
        wrapped |= __builtin_add_overflow(r.hi, records[i].hi, &r.hi);
    }
    if (wrapped) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "emspec_cross_sum: a limb of the sum does not fit its field");
    *out = r;
    return EMSPEC_OK;
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
