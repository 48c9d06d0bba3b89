// emspec_band_plan.h — internal: the shape rules and the workspace layout of the multi-band batch (include/emspec.h:
// emspec_batch_multiband*): which (sizes, hop, split rows) are accepted and, if not, the rule broken; each
// band's column shift and row range; where each band's raw-dB plane (and the composed raw plane of the display post-process) sits in
// the engine workspace for a chunk of streams.  Host arithmetic only, every input an argument.  No HIP: tests/test_band_plan_cpu.py
// runs it through a stand-alone program (tests/cdriver/band_plan_driver.cpp) without a GPU.
#pragma once
#include "emspec_wire_plan.h"   // al
#include <cstddef>
#include <cstdint>

namespace emspec {

constexpr int kMaxBands = 4;
// what a multi-band workspace asks for beside its streams: the 256-byte round-up of every plane behind the first
constexpr size_t kBandPad = 256 * kMaxBands;

inline bool band_size_ok(int n) { return n == 1024 || n == 2048 || n == 4096 || n == 8192 || n == 16384; }

// null when (bands, n[], hop) is an accepted shape, else the rule it breaks
inline const char* band_shape_error(int bands, const int32_t* n, int hop) {
    if (bands < 2 || bands > kMaxBands) return "bands must be in 2..4";
    if (!n) return "null argument";
    for (int k = 0; k < bands; ++k)
        if (!band_size_ok(n[k])) return "every fft size must be 1024, 2048, 4096, 8192 or 16384";
    for (int k = 1; k < bands; ++k)
        if (n[k] >= n[k - 1]) return "fft sizes must be strictly decreasing";
    if (hop < 1 || hop > n[bands - 1]) return "hop must be in [1, n[bands - 1]]";
    for (int k = 1; k < bands; ++k)
        if ((n[0] - n[k]) % (2 * hop)) return "every (n[0] - n[k]) / (2 hop) must be an integer";
    return nullptr;
}

// null when the bands - 1 split rows cut [0, rows) into accepted bands, else the rule they break
inline const char* band_split_error(int bands, const int32_t* split, int rows) {
    if (!split) return "null argument";
    for (int k = 0; k + 1 < bands; ++k)
        if (split[k] % 4) return "every split row must be a multiple of 4";
    for (int k = 1; k + 1 < bands; ++k)
        if (split[k] <= split[k - 1]) return "split rows must be strictly increasing";
    for (int k = 0; k < bands; ++k) {
        const int lo = k ? split[k - 1] : 0, hi = k + 1 < bands ? split[k] : rows;
        if (hi - lo < 64) return "every band must be at least 64 rows high";
    }
    return nullptr;
}

// The two-band form (emspec_batch_multires*, the *_multires live entries) keeps narrower rules and messages of its
// own; whatever they accept, band_shape_error(2, ...) and band_split_error(2, ...) accept too (tests/test_band_plan_cpu.py).
// null when (n_low, n_high, hop) is an accepted shape, else the rule it breaks
inline const char* multires_shape_error(int n_low, int n_high, int hop) {
    if (n_low != 8192 && n_low != 16384) return "n_low must be 8192 or 16384";
    if (n_high != 1024 && n_high != 2048 && n_high != 4096) return "n_high must be 1024, 2048 or 4096";
    if (hop < 1 || hop > n_high) return "hop must be in [1, n_high]";
    if ((n_low - n_high) % (2 * hop)) return "(n_low - n_high) / (2 hop) must be an integer";
    return nullptr;
}
// null when split_row cuts [0, rows) into two accepted bands, else the rule it breaks
inline const char* multires_split_error(int split_row, int rows) {
    if (split_row % 4 || split_row < 64 || split_row > rows - 64) return "split_row must be a multiple of 4 in [64, rows - 64]";
    return nullptr;
}

// The bands of an accepted call: band k owns rows [lo[k], hi[k]) and takes column c + shift[k] of single(n[k]).
struct BandPlan {
    int bands = 0;
    int n[kMaxBands] = {}, shift[kMaxBands] = {}, lo[kMaxBands] = {}, hi[kMaxBands] = {};
    int rows_of(int k) const { return hi[k] - lo[k]; }
};
inline BandPlan band_plan(int bands, const int32_t* n, const int32_t* split, int hop, int rows) {
    BandPlan p;
    p.bands = bands;
    for (int k = 0; k < bands; ++k) {
        p.n[k] = n[k];
        p.shift[k] = (n[0] - n[k]) / (2 * hop);
        p.lo[k] = k ? split[k - 1] : 0;
        p.hi[k] = k + 1 < bands ? split[k] : rows;
    }
    return p;
}

// The workspace of C composed columns: per stream, band k's plane is [C + 2 shift[k]][rows_k] float32, and with the display
// post-process on the composed raw dB [C][rows] lies behind them.  For a chunk of streams every plane starts on a 256-byte boundary:
// chunk_offset(k, chunk) bytes into the workspace (k = bands: the raw plane), chunk_bytes(chunk) in all
// (<= per_stream * chunk + kBandPad).
struct BandLayout {
    int bands = 0;
    size_t plane[kMaxBands + 1] = {};   // bytes per stream: the bands' planes, then the raw plane (0 without the post-process)
    size_t per_stream = 0;
    size_t chunk_offset(int k, int chunk) const {
        size_t o = 0;
        for (int i = 0; i < k; ++i) o += al(plane[i] * (size_t)chunk);
        return o;
    }
    size_t chunk_bytes(int chunk) const { return chunk_offset(bands, chunk) + plane[bands] * (size_t)chunk; }
};
inline BandLayout band_layout(const BandPlan& p, int64_t C, int rows, bool post) {
    BandLayout w;
    w.bands = p.bands;
    for (int k = 0; k < p.bands; ++k) {
        w.plane[k] = (size_t)(C + 2 * (int64_t)p.shift[k]) * (size_t)p.rows_of(k) * 4;
        w.per_stream += w.plane[k];
    }
    w.plane[p.bands] = post ? (size_t)C * (size_t)rows * 4 : 0;
    w.per_stream += w.plane[p.bands];
    return w;
}

}  // namespace emspec
