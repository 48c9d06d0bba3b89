// emspec_stereo_plan.h — internal: the arithmetic of the stereo image (include/emspec.h: emspec_stereo_*, emspec_batch_stereo_device,
// emspec_history_view_stereo*): one picture of a channel pair, brightness from the louder channel's dB,
// hue from the difference of the two.  The per-cell law, the scalars it runs on, what its arguments must obey, and the integer
// builder of the [33][256][4] palette.  binary32, one rounding per operation, no fused multiply-add (the library is built with
// -ffp-contract=off; `d * inv_pan` and `u * 16.0f` have no addition behind them to contract with).  No HIP, nothing of the
// engine: tests/test_stereo_cpu.py runs it through a stand-alone program (tests/cdriver/stereo_plan_driver.cpp) without a GPU.
// The kernels (stereo.hip.inc) and the host twin (emspec_stereo.cpp) call the SAME functions.
#pragma once
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

constexpr int kStereoPanCentre = 16, kStereoPanLevels = 33;   // balance byte 0 (all A) .. 32 (all B)
constexpr size_t kStereoPaletteBytes = (size_t)kStereoPanLevels * 256 * 4;

// The scalars of a map, computed on the host as emspec_tables.h: db_scalars does for a view.
struct StereoLaw { float lo, inv, gate, shift, inv_pan; };
inline StereoLaw stereo_law(float db_top, float db_range, float gate_db, float shift_db, float pan_range_db) {
    return StereoLaw{db_top - db_range, (float)(1.0 / (double)db_range), gate_db, shift_db, (float)(1.0 / (double)pan_range_db)};
}
// null, or the rule a map breaks
inline const char* stereo_map_error(float db_top, float db_range, float gate_db, float shift_db, float pan_range_db) {
    if (!(db_range > 0.0f)) return "a stereo map needs db_range > 0";
    if (!(pan_range_db > 0.0f)) return "a stereo map needs pan_range_db > 0";
    if (db_top != db_top || gate_db != gate_db || shift_db != shift_db) return "a stereo map must have no NaN field";
    return nullptr;
}
// null, or the rule a choice of streams breaks: pair p reads streams p views + a and p views + b
inline const char* stereo_pair_error(int64_t views, int64_t a, int64_t b) {
    if (views < 2) return "a stereo pair needs views >= 2";
    if (a < 0 || a >= views || b < 0 || b >= views) return "a stereo pair's channels a and b must be in 0 .. views - 1";
    if (a == b) return "a stereo pair's channels a and b must differ";
    return nullptr;
}

// the palette index of a shifted level: emspec_device.h: cell_index's arithmetic, and 0 for a NaN
EMSPEC_HD inline int stereo_index(const StereoLaw& w, float s) {
    if (s != s) return 0;
    float v = (s - w.lo) * w.inv;
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    if (s < w.gate) v = 0.0f;
    return (int)(v * 255.0f + 0.5f);
}

// One cell: xa, xb the two channels' dB.
//   level: the louder channel's own bits (a NaN only when both are)
//   index: of level + shift
//   pan:   16 + rint(16 clamp((xb - xa) / pan_range, -1, 1)), half to even; 16 for a gated cell and where the difference is
//          no number (a NaN channel, the same infinity in both) - u is NaN exactly then, pan_range being a number
struct StereoCell { float level; int index, pan; };
EMSPEC_HD inline StereoCell stereo_cell(const StereoLaw& w, float xa, float xb) {
    StereoCell c;
    c.level = (xb > xa || xa != xa) ? xb : xa;
    const float s = c.level + w.shift;
    const bool gated = s < w.gate;
    c.index = stereo_index(w, s);
    const float d = xb - xa;
    float u = d * w.inv_pan;
    if (u > 1.0f) u = 1.0f;
    if (u < -1.0f) u = -1.0f;
    const float t = u * 16.0f;
    c.pan = (gated || t != t) ? kStereoPanCentre : kStereoPanCentre + (int)__builtin_rintf(t);
    return c;
}

// The palette [33][256][4] from a [256][4] colour map, in integers: row 16 is the map; towards row 0 (all A) a cell's colour
// moves to the warm tint (255, 96, 32) at the cell's own brightness v = max(r, g, b), towards row 32 (all B) to the cold one
// (32, 160, 255); alpha is the map's.
inline void stereo_palette(const uint8_t* base, uint8_t* out) {
    static const int kWarm[3] = {255, 96, 32}, kCold[3] = {32, 160, 255};
    for (int pan = 0; pan < kStereoPanLevels; ++pan) {
        const int t = pan - kStereoPanCentre, w = t < 0 ? -t : t;
        const int* K = t < 0 ? kWarm : kCold;
        for (int i = 0; i < 256; ++i) {
            const uint8_t* b = base + 4 * i;
            uint8_t* o = out + ((size_t)pan * 256 + (size_t)i) * 4;
            const int v = b[0] > b[1] ? (b[0] > b[2] ? b[0] : b[2]) : (b[1] > b[2] ? b[1] : b[2]);
            for (int c = 0; c < 3; ++c) {
                const int tint = (K[c] * v + 127) / 255;
                o[c] = (uint8_t)((b[c] * (kStereoPanCentre - w) + tint * w + 8) / 16);
            }
            o[3] = b[3];
        }
    }
}

// The definition on host arrays: db [pairs * views][cells] -> level / index / pan [pairs][cells], rgba [pairs][cells][4]
// (= palette[pan][index]); any output null.
inline void stereo_compose_host(const float* db, int64_t pairs, int views, int a, int b, int64_t cells, const StereoLaw& w,
                                const uint8_t* palette, float* level, uint8_t* index, uint8_t* pan, uint8_t* rgba) {
    for (int64_t p = 0; p < pairs; ++p) {
        const float* xa = db + ((size_t)p * views + a) * (size_t)cells;
        const float* xb = db + ((size_t)p * views + b) * (size_t)cells;
        for (int64_t i = 0; i < cells; ++i) {
            const StereoCell c = stereo_cell(w, xa[i], xb[i]);
            const size_t o = (size_t)p * (size_t)cells + (size_t)i;
            if (level) __builtin_memcpy(level + o, &c.level, 4);
            if (index) index[o] = (uint8_t)c.index;
            if (pan) pan[o] = (uint8_t)c.pan;
            if (rgba) __builtin_memcpy(rgba + 4 * o, palette + ((size_t)c.pan * 256 + (size_t)c.index) * 4, 4);
        }
    }
}

}  // namespace emspec
