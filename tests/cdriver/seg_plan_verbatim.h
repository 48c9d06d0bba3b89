// seg_plan_verbatim.h — the segment planning of the walking kernels as it stood inside the launchers (fused.hip.inc launch_fused,
// exact_fused.hip.inc launch_exact_fused, exact_fused_lr.hip.inc exact_lr_seglen / exact_fused_lr_scratch_bytes /
// launch_exact_fused_lr, exact.hip.inc exact_scatter_plan / exact_scatter_scratch_bytes / launch_exact_tile_scatter, kernels.hip
// launch_walk_scatter_t / launch_tile_scatter) before em-spec_amd/csrc/emspec_seg_plan.h took it over.  The statements are those
// launchers', unchanged; device_cus() is the parameter `device_cus_` and the getenv switches of the diagnostic build are arguments
// (EMSPEC_SHARED: env_shared, a string or null; EMSPEC_SEGLEN: env_seglen, a string or null; EMSPEC_NO_WALK: use_walk).  Kept only
// to write and to re-derive tests/golden/seg_plans.json (tests/cdriver/seg_plan_driver.cpp with -DSEG_PLAN_VERBATIM); the library
// does not include it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace emspec_verbatim {

struct SegPlan { int seglen; int nlong; int tail; int short_last; };

// ---- fused.hip.inc, launch_fused: from "Segments: as long as possible" to the grid ----
struct FusedOut { SegPlan sp; int64_t nseg; bool invalid; bool streams_first; };
inline FusedOut launch_fused_plan(int64_t device_cus_, bool small_n, bool big_n, int pl_D, int pl_shared, int S, int64_t C,
                                  const char* env_shared, const char* env_seglen) {
    const int64_t ncu = device_cus_;
    int64_t nseg_want = (ncu + S - 1) / S;
    const int64_t nseg_min = (C + 1023) / 1024;
    const int64_t nseg_rounds = std::min<int64_t>(std::max<int64_t>(1, 4 * ncu / S), (C + 255) / 256);
    if (nseg_want < nseg_rounds) nseg_want = nseg_rounds;
    if (nseg_want < nseg_min) nseg_want = nseg_min;
    int64_t seg = (C + nseg_want - 1) / nseg_want;
    const int64_t seg_min = small_n ? std::max<int64_t>(16, 4 * pl_D) : (big_n ? std::max<int64_t>(32, 2 * pl_D) : std::max<int64_t>(16, 2 * pl_D));
    seg = seg < seg_min ? seg_min : seg;
    bool shared = pl_shared == 1;
    if (const char* ev = env_shared) shared = ev[0] == '1';   // lets one GPU exercise the plan
    if (!shared) {
        double best = -1.0;
        int64_t best_seg = seg;
        for (int r = 1; r <= 4; ++r) {
            int64_t ns = std::max<int64_t>(1, (int64_t)r * ncu / S);
            ns = std::min<int64_t>(ns, std::max<int64_t>(1, (C + seg_min - 1) / seg_min));   // (ceil: 16,369 columns still make 256 segments of 64)
            const int64_t sl = (C + ns - 1) / ns;
            ns = (C + sl - 1) / sl;
            const double groups = (double)S * (double)ns;
            const double rounds = std::ceil(groups / (double)ncu);
            const double eff = groups / (rounds * (double)ncu) * (double)sl / ((double)sl + 2.0 * pl_D + 3.0);
            if (eff > best * 1.002) { best = eff; best_seg = sl; }
        }
        seg = best_seg < seg_min ? seg_min : best_seg;
        if (pl_shared == 2 && seg > 1024) seg = 1024;   // two launches share the chip (emspec_batch's two-lane pipeline)
    }
    if (const char* ev = env_seglen) {   // tuning aid
        const long v = atol(ev);
        if (v >= 2) seg = v;
    }
    seg = (seg + 1) & ~(int64_t)1;
    SegPlan sp{(int)seg, 1 << 30, (int)seg, 0};
    int64_t nseg = (C + seg - 1) / seg;
    if (shared) {
        const int64_t tail = ((seg / 4) + 1) & ~(int64_t)1;
        if (tail >= seg_min && nseg >= 2) {
            const int64_t nlong = nseg - (nseg + 3) / 4;              // the last quarter (at least one segment) is cut finer
            const int64_t rest = C - nlong * seg;
            sp = SegPlan{(int)seg, (int)nlong, (int)tail, 1};
            nseg = nlong + (rest + tail - 1) / tail;
        }
    }
    FusedOut o{sp, nseg, false, false};
    if (nseg > 65535) { o.invalid = true; return o; }   // return hipErrorInvalidValue;
    o.streams_first = sp.short_last != 0;   // grid = sp.short_last ? dim3(S, nseg) : dim3(nseg, S)
    return o;
}

// ---- exact_fused.hip.inc, launch_exact_fused ----
struct ExactFusedOut { int64_t seg, nseg; bool invalid; };
inline ExactFusedOut launch_exact_fused_plan(int64_t device_cus_, int pl_D, int S, int64_t C, const char* env_seglen) {
    const int64_t ncu = device_cus_;
    const int64_t seg_min = std::max<int64_t>(64, 4 * pl_D);
    double best = -1.0;
    int64_t seg = std::max<int64_t>(seg_min, (C + 3) / 4);
    for (int r = 1; r <= 4; ++r) {
        int64_t ns = std::max<int64_t>(1, (int64_t)r * ncu / S);
        ns = std::min<int64_t>(ns, std::max<int64_t>(1, (C + seg_min - 1) / seg_min));
        const int64_t sl = (C + ns - 1) / ns;
        ns = (C + sl - 1) / sl;
        const double groups = (double)S * (double)ns;
        const double rounds = std::ceil(groups / (double)ncu);
        const double eff = groups / (rounds * (double)ncu) * (double)sl / ((double)sl + 2.0 * pl_D + 3.0);
        if (eff > best * 1.002) { best = eff; seg = sl; }
    }
    if (const char* ev = env_seglen) { const long v = atol(ev); if (v >= 2) seg = v; }
    seg = seg < 1 ? 1 : seg;
    const int64_t nseg = (C + seg - 1) / seg;
    return ExactFusedOut{seg, nseg, nseg > 65535 || seg > 0x3fffffff};   // return hipErrorInvalidValue;
}

// ---- exact_fused_lr.hip.inc ----
inline int64_t exact_lr_seglen(int64_t device_cus_, int n, int pl_D, int S, int64_t C, const char* env_seglen) {
    const int64_t ncu = device_cus_;
    const double fill = 3.0 * (double)(4096 / n);   // half-iterations of pipeline fill, in frames
    const int64_t seg_min = std::max<int64_t>(16, 2 * pl_D);   // (as launch_fused: short batches are latency cases)
    double best = -1.0;
    int64_t seg = std::max<int64_t>(seg_min, (C + 3) / 4);
    for (int r = 1; r <= 4; ++r) {
        int64_t ns = std::max<int64_t>(1, (int64_t)r * ncu / S);
        ns = std::min<int64_t>(ns, std::max<int64_t>(1, (C + seg_min - 1) / seg_min));
        const int64_t sl = (C + ns - 1) / ns;
        ns = (C + sl - 1) / sl;
        const double groups = (double)S * (double)ns;
        const double rounds = std::ceil(groups / (double)ncu);
        const double eff = groups / (rounds * (double)ncu) * (double)sl / ((double)sl + 2.0 * pl_D + fill);
        if (eff > best * 1.002) { best = eff; seg = sl; }
    }
    if (const char* ev = env_seglen) { const long v = atol(ev); if (v >= 2) seg = v; }
    return seg < 1 ? 1 : seg;
}
static constexpr int64_t kExactLrMaxGroups = 2048;
// (slots = exl::lr_slots(exact_lr_skip(n), pl.D): an argument here)
inline size_t exact_fused_lr_scratch_bytes(int64_t device_cus_, int n, int pl_D, int slots, int rl, int S, int64_t C, const char* env_seglen) {
    if (rl <= 0 || S <= 0 || C <= 0) return 0;
    const int64_t seg = exact_lr_seglen(device_cus_, n, pl_D, S, C, env_seglen);
    const int64_t nseg = (C + seg - 1) / seg;
    const int64_t groups = std::max<int64_t>(nseg, std::min<int64_t>(kExactLrMaxGroups, nseg * (int64_t)S));   // >= one stream's
    return (size_t)groups * (size_t)slots * (size_t)rl * 8;
}
struct ExactLrOut { int64_t seg, nseg, s_per; size_t per_group; bool invalid; };
inline ExactLrOut launch_exact_fused_lr_plan(int64_t device_cus_, int n, int pl_D, int slots, int rl, int S, int64_t C, bool low,
                                             size_t low_bytes, const char* env_seglen) {
    ExactLrOut o{0, 0, 0, 0, false};
    int64_t seg = exact_lr_seglen(device_cus_, n, pl_D, S, C, env_seglen);
    seg = seg < 1 ? 1 : seg;
    const int64_t nseg = (C + seg - 1) / seg;
    o.seg = seg; o.nseg = nseg;
    if (nseg > 65535 || seg > 0x3fffffff) { o.invalid = true; return o; }   // return hipErrorInvalidValue;
    const size_t per_group = (size_t)slots * (size_t)rl * 8;
    o.per_group = per_group;
    int64_t groups_cap = 65535 * (int64_t)65535;
    if (rl > 0) {
        if (!low || low_bytes < per_group * (size_t)nseg) { o.invalid = true; return o; }   // return hipErrorInvalidValue;
        groups_cap = (int64_t)(low_bytes / per_group);
    }
    const int64_t s_per = std::max<int64_t>(1, std::min<int64_t>(S, groups_cap / nseg));
    o.s_per = s_per;
    return o;
}

// ---- exact.hip.inc ----
namespace ex {
constexpr int rec_stride(int n) { return n / 2 + 4; }   // records per frame: K = n/2+1 bins + 3 pads (16-byte chunks of 4)
}
struct ExactScatterPlan { int F, rl, seg; int64_t nseg; size_t lds, scratch_per_group; };
inline ExactScatterPlan exact_scatter_plan(int64_t device_cus_, int n, int pl_rows, int pl_D, int S, int64_t C, const float* ebin_f32) {
    ExactScatterPlan sp{0, 0, 0, 0, 0, 0};
    const int nch = ex::rec_stride(n) / 4;
    int F = (1024 + nch - 1) / nch;
    F = F < 1 ? 1 : (F > 8 ? 8 : F);
    int rl = 0;
    size_t wl = (size_t)(2 * pl_D + F) * pl_rows * 8 + 1024;
    if (wl > 158 * 1024) {
        // the row split: six frames per step (two barriers per step; 2D + 6 slots), as many rows in LDS as fit
        if (!ebin_f32 || pl_rows % 4) return sp;
        F = 6;
        const int slots = 2 * pl_D + F;
        const size_t mask = (size_t)slots * ((pl_rows + 31) >> 5) * 4;   // (sized for the worst case, rl = rows)
        int rh = (int)(((size_t)158 * 1024 - 1024 - mask) / ((size_t)slots * 8)) & ~3;
        if (rh >= pl_rows || rh < 64) return sp;
        rl = pl_rows - rh;
        if (!((double)ebin_f32[rl] / (double)(n / 2) <= 0.06)) return sp;
        wl = (size_t)slots * rh * 8 + 1024 + mask;
    }
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, (int64_t)((size_t)160 * 1024 / wl)));
    const int64_t places = device_cus_ * per_cu;
    const int64_t over = 2 * pl_D + F;
    int64_t seg = (C + F - 1) / F * F;
    double best = -1.0;
    for (int r = 1; r <= 8; ++r) {
        const int64_t ns = std::max<int64_t>(1, (int64_t)r * places / S);
        int64_t sg = ((C + ns - 1) / ns + F - 1) / F * F;
        sg = sg < F ? F : sg;
        const int64_t nsg = (C + sg - 1) / sg;
        const double rounds = std::ceil((double)S * (double)nsg / (double)places);
        const double cost = rounds * (double)(sg + over);
        if (best < 0.0 || cost < best * 0.999) { best = cost; seg = sg; }
    }
    sp.F = F; sp.rl = rl; sp.seg = (int)seg; sp.nseg = (C + seg - 1) / seg; sp.lds = wl;
    sp.scratch_per_group = (size_t)(2 * pl_D + F) * rl * 8;
    return sp;
}
inline size_t exact_scatter_scratch_bytes(int64_t device_cus_, int n, int pl_rows, int pl_D, int S, int64_t C, const float* ebin_f32) {
    if (S <= 0 || C <= 0) return 0;
    const ExactScatterPlan sp = exact_scatter_plan(device_cus_, n, pl_rows, pl_D, S, C, ebin_f32);
    if (!sp.F || !sp.rl) return 0;
    const int64_t groups = std::max<int64_t>(sp.nseg, std::min<int64_t>(2048, sp.nseg * (int64_t)S));
    return (size_t)groups * sp.scratch_per_group;
}
// launch_exact_tile_scatter: the plan it launches (F = 0: tiles), the streams per launch of the walk, the tile form's geometry
struct ExactScatterOut { ExactScatterPlan sp; int64_t s_per; int tile; size_t tile_lds; int64_t ntiles; bool invalid; };
inline ExactScatterOut launch_exact_tile_scatter_plan(int64_t device_cus_, int n, int pl_rows, int pl_D, int S, int64_t C,
                                                      const float* ebin_f32, bool low, size_t low_bytes) {
    ExactScatterOut o{{0, 0, 0, 0, 0, 0}, 0, 0, 0, 0, false};
    {
        ExactScatterPlan sp = exact_scatter_plan(device_cus_, n, pl_rows, pl_D, S, C, ebin_f32);
        if (sp.F && sp.rl && (!low || low_bytes < sp.scratch_per_group * (size_t)sp.nseg)) sp.F = 0;   // no scratch: tiles
        o.sp = sp;
        if (sp.F) {
            const int64_t s_per = sp.rl ? std::max<int64_t>(1, std::min<int64_t>(S, (int64_t)(low_bytes / sp.scratch_per_group) / sp.nseg)) : S;
            o.s_per = s_per;
            return o;
        }
    }
    int tile = (int)((150 * 1024) / ((size_t)pl_rows * 8));
    tile = tile > 16 ? 16 : tile;
    o.tile = tile;
    if (tile < 1) { o.invalid = true; return o; }   // return hipErrorInvalidValue;
    const size_t lds = (size_t)tile * pl_rows * 8 + 1024;
    const int64_t ntiles = (C + tile - 1) / tile;
    o.tile_lds = lds; o.ntiles = ntiles;
    return o;
}

// ---- kernels.hip, launch_tile_scatter / launch_walk_scatter_t / launch_tile_scatter_t ----
struct WalkOut { int ch, F; size_t wl; bool walk; int64_t seg, nseg; int tile; size_t tile_lds; int64_t ntiles; bool invalid; };
inline WalkOut launch_tile_scatter_plan(int device_cus_, int n, int pl_rows, int pl_D, int S, int64_t C, bool use_walk) {
    WalkOut o{0, 0, 0, false, 0, 0, 0, 0, 0, false};
    // chunk = consecutive bins per thread: wide enough that adjacent lanes rarely share a row
    const int ch = n >= 8192 ? 32 : (n >= 2048 ? 8 : 4);
    o.ch = ch;
    {   // walking ring when it fits: F frames per step so that F * chunks-per-frame covers the 1024 threads
        const int nch = (n / 2 + 2 + ch - 1) / ch;
        int F = (1024 + nch - 1) / nch;
        F = F < 1 ? 1 : (F > 8 ? 8 : F);
        const size_t wl = (size_t)(2 * pl_D + F) * pl_rows * 4 + 1024;
        o.F = F; o.wl = wl;
        if (use_walk && pl_D >= 16 && wl <= 156 * 1024) {
            // launch_walk_scatter_t
            int64_t seg = (S * C + 4 * device_cus_ - 1) / (4 * device_cus_);   // >= 4 workgroups per CU when there is enough work
            seg = seg < 128 ? 128 : (seg > 1024 ? 1024 : seg);
            seg = (seg + F - 1) / F * F;
            const int64_t nseg = (C + seg - 1) / seg;
            o.walk = true; o.seg = seg; o.nseg = nseg;
            return o;
        }
    }
    int tile = (int)((150 * 1024) / ((size_t)pl_rows * 4));
    tile = tile > 32 ? 32 : tile;
    o.tile = tile;
    if (tile < 1) { o.invalid = true; return o; }   // return hipErrorInvalidValue;
    const size_t lds = (size_t)tile * pl_rows * 4 + 1024;
    // launch_tile_scatter_t
    const int64_t ntiles = (C + tile - 1) / tile;
    o.tile_lds = lds; o.ntiles = ntiles;
    return o;
}

}  // namespace emspec_verbatim
