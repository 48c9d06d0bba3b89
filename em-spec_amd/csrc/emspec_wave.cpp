// emspec_wave.cpp — the waveform envelope (include/emspec.h: emspec_wave_device, emspec_wave_host, emspec_set_wave_out;
// DESIGN.md §3.12, §4.13): per stream and delivered column the smallest and the largest sample of the column's window, in the
// total order of the floats.  The device form is wave.hip.inc's kernel on device-resident streams; the host pipeline
// (emspec_host.cpp) runs the same kernel on each unit's staged samples while emspec_set_wave_out is set; the host form is the
// same definition in plain C++.
#include "emspec_engine.h"

#include <algorithm>
#include <cstring>
#include <limits>

using namespace emspec;

namespace {

// null, or the rule the arguments break (what the device and the host form share)
const char* wave_arg_error(int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor) {
    if (S < 0 || S > 65535) return "need 0..65535 streams";
    if (L < 0) return "the stream length must not be negative";
    if (!supported_fft(n)) return "fft size must be a power of two in [256,16384]";
    if (hop < 1 || hop > n) return "hop must be in [1, fft size]";
    if (factor < 1 || factor > 65536) return "the envelope's factor must be in [1, 65536]";
    return nullptr;
}

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

uint32_t wave_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

}  // namespace

extern "C" {

int emspec_wave_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor,
                       emspec_wave* wave_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (const char* why = wave_arg_error(S, L, n, hop, factor)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t C = emspec_num_columns(L, n, hop);
    if (S == 0 || C == 0) return EMSPEC_OK;
    if (!pcm_dev || !wave_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(pcm_dev, 4)) return fail(e, EMSPEC_ERR_INVALID_ARG, "pcm_dev must be 4-byte aligned");
    if (!aligned(wave_dev, 8)) return fail(e, EMSPEC_ERR_INVALID_ARG, "wave_dev must be 8-byte aligned");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_wave(pcm_dev, S, L, n / 2 - hop / 2, C, hop, factor, wave_dev, reduced_columns(C, factor), (hipStream_t)hip_stream));
    return EMSPEC_OK;
}

int emspec_wave_host(const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t factor, emspec_wave* wave_out) {
    if (const char* why = wave_arg_error(S, L, n, hop, factor)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t C = emspec_num_columns(L, n, hop), Cr = reduced_columns(C, factor), off = n / 2 - hop / 2;
    if (S == 0 || C == 0) return EMSPEC_OK;
    if (!pcm || !wave_out) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(pcm, 4) || !aligned(wave_out, 4)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "pcm and wave_out must be 4-byte aligned");
    const float inf = std::numeric_limits<float>::infinity();
    for (int64_t s = 0; s < S; ++s)
        for (int64_t g = 0; g < Cr; ++g) {
            const int64_t c1 = std::min<int64_t>((g + 1) * factor, C);
            const float* x = pcm + (size_t)s * (size_t)L;
            const float *lo = nullptr, *hi = nullptr;
            uint32_t klo = 0, khi = 0;
            for (int64_t i = g * factor * hop + off; i < c1 * hop + off; ++i) {
                uint32_t u;
                std::memcpy(&u, x + i, 4);
                if ((u & 0x7fffffffu) > 0x7f800000u) continue;   // NaN
                const uint32_t k = wave_key(u);
                if (!lo || k < klo) { lo = x + i; klo = k; }
                if (!hi || k > khi) { hi = x + i; khi = k; }
            }
            emspec_wave* o = wave_out + (size_t)s * (size_t)Cr + (size_t)g;
            o->lo = inf; o->hi = -inf;
            if (lo) { std::memcpy(&o->lo, lo, 4); std::memcpy(&o->hi, hi, 4); }   // the samples' own bits
        }
    return EMSPEC_OK;
}

int emspec_set_wave_out(emspec_engine* e, emspec_wave* wave_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (wave_out && capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the envelope's capacity must not be negative");
    if (!aligned(wave_out, 4)) return fail(e, EMSPEC_ERR_INVALID_ARG, "wave_out must be 4-byte aligned");
    e->wave_out = wave_out;
    e->wave_capacity = wave_out ? capacity : 0;
    return EMSPEC_OK;
}

}  // extern "C"
