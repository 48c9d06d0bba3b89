// emspec_seg_plan.h — internal: how every batch kernel that walks a stream cuts it into segments (DESIGN.md "Segment plans"):
// the fused float32 kernels (fused.hip.inc), the two EXACT fused kernels (exact_fused.hip.inc, exact_fused_lr.hip.inc) and the
// float32 and EXACT walking scatters (kernels.hip, exact.hip.inc), with the scratch sizes and the stream split that follow from
// the cut.  Host arithmetic only, and every input an argument: the launchers pass the device's CU count and, in the diagnostic
// build, their getenv switches.  No HIP: tests/test_seg_plan_cpu.py runs it through a stand-alone program
// (tests/cdriver/seg_plan_driver.cpp) without a GPU and pins every plan to tests/golden/seg_plans.json.
#pragma once
#include "emspec_kernel_plan.h"   // kLdsBytes, RouteKind
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace emspec {

// How a launch of a fused (walking) kernel cuts every stream into segments.
//   uniform plan (short_last = 0): grid = (segments, streams); segment g covers columns [g * seglen, (g + 1) * seglen).
//   shared-device plan (short_last = 1): grid = (streams, segments); segment g covers
//     [g * seglen, (g + 1) * seglen) for g < nlong, then pieces of `tail` columns.  Workgroups are dispatched in linear
//     block order, so with blockIdx.y = segment all streams' long segments start first and the launch ends on the
//     short ones: when another kernel (a collective, the gather's pack / expand) holds some CUs and the workgroups no
//     longer fill whole rounds, what is left over at the end is short.  Stream s takes the segment order rotated by s
//     (long and short segments each among themselves).
//   The uniform plan keeps round 1's dispatch order on purpose: with grid = (streams, segments) the N = 16384 kernel,
//   which re-reads its 64 KB sample window every frame and relies on L2 for it, fetched 56 KB instead of 2.8 KB per
//   column from beyond L2 (FETCH_SIZE, with and without the rotation; same speed).  The N = 4096 kernel reads every
//   sample once and is unaffected (6.2 KB per column either way), and it is the one the N > 1 bench runs.
// (seg_of_block, emspec_device.h, is the kernels' reading of it)
struct SegPlan { int seglen; int nlong; int tail; int short_last; };

// ---- the rounds-by-efficiency choice (the one r = 1..4 loop of the tree) ----
// A device that is the launch's alone: nothing takes CUs away mid-launch, so more rounds of workgroups only buy halo.  Choose
// the number of rounds r = 1..4 by what it costs: the fill of the last round (S x nseg workgroups over r x CUs) times the share
// of a workgroup's frames that are not halo (2D per segment + `fill` frames of pipeline fill), fewer rounds winning ties
// (a later r has to be 0.2 % better).  No segment is shorter than seg_min unless the stream is.  Returns the segment length.
//   64 streams x 16,369 columns on 256 CUs: 256 workgroups of 4,096 columns instead of 1,024 of 1,024 (measured 9.21 vs 9.29 ms);
//   16 streams: 256 x 1,024 instead of 1,024 x 256.
// (round 1 always replaces the initial best, -1: there is no starting length to choose)
inline int64_t seglen_by_rounds(int64_t ncu, int S, int64_t C, int D, int64_t seg_min, double fill) {
    double best = -1.0;
    int64_t best_seg = C;
    for (int r = 1; r <= 4; ++r) {
        int64_t ns = std::max<int64_t>(1, (int64_t)r * ncu / S);
        ns = std::min<int64_t>(ns, std::max<int64_t>(1, (C + seg_min - 1) / seg_min));   // (ceil: 16,369 columns still make 256 segments of 64)
        const int64_t sl = (C + ns - 1) / ns;
        ns = (C + sl - 1) / sl;
        const double groups = (double)S * (double)ns;
        const double rounds = std::ceil(groups / (double)ncu);
        const double eff = groups / (rounds * (double)ncu) * (double)sl / ((double)sl + 2.0 * D + fill);
        if (eff > best * 1.002) { best = eff; best_seg = sl; }
    }
    return best_seg;
}

// ---- the fused float32 kernels (fused.hip.inc: launch_fused) ----
enum class FusedKind { n4096_8192, small_n, big_n };   // the N = 4096 / 8192 families, fused_small, N = 16384: only seg_min differs
inline FusedKind fused_kind(RouteKind k) { return k == RouteKind::fused_small ? FusedKind::small_n : (k == RouteKind::fused_16384 ? FusedKind::big_n : FusedKind::n4096_8192); }
// nseg: segments per stream; streams_first: grid = (streams, segments) - the shared-device plan - instead of (segments, streams);
// ok false: more segments than a grid dimension holds (the launcher returns hipErrorInvalidValue)
struct FusedSegPlan { SegPlan sp; int64_t nseg; bool streams_first; bool ok; };
// shared: PlanDev::shared (0: the device is the launch's alone, 1: shared with a collective, 2: with the engine's second pipeline
// lane).  force_shared: -1, or the diagnostic build's EMSPEC_SHARED (0 / 1) in place of shared == 1.  seglen_override: the
// diagnostic build's EMSPEC_SEGLEN, applied when >= 2.
inline FusedSegPlan fused_seg_plan(int64_t ncu, int S, int64_t C, int D, FusedKind kind, int shared, int force_shared,
                                   int64_t seglen_override) {
    // Segments: as long as possible (every segment recomputes a 2D-frame halo) while the launch still
    // has at least one workgroup per CU, and - as long as segments stay >= 256 columns - about four:
    //   nseg = max(ceil(CUs/S), min(floor(4 CUs/S), ceil(C/256)), ceil(C/1024)) per stream.
    // Equal segments and a workgroup count near a multiple of the CU count keep the last round of workgroups
    // full (256 CUs: 64 streams -> 16 x 1024 columns = 1024 workgroups; 16 streams -> 64 x 256 = 1024;
    // 1 stream -> 256 x 64).  Several rounds matter when another kernel (an RCCL send/recv) holds a
    // few CUs: a workgroup fills its CU, so a one-round launch would then take two rounds
    // (tools/occupancy_probe.py: 8 chunks of 256 workgroups 13.4 -> 26.8 ms; 1024 per launch -> 16.3).
    int64_t nseg_want = (ncu + S - 1) / S;
    const int64_t nseg_min = (C + 1023) / 1024;
    // (rounded down: S x nseg <= 4 CUs, so stream counts that do not divide the CU count - 34, 36, 70 - never start a
    // nearly empty fifth round)
    const int64_t nseg_rounds = std::min<int64_t>(std::max<int64_t>(1, 4 * ncu / S), (C + 255) / 256);
    if (nseg_want < nseg_rounds) nseg_want = nseg_rounds;
    if (nseg_want < nseg_min) nseg_want = nseg_min;
    int64_t seg = (C + nseg_want - 1) / nseg_want;
    // shortest segment: as many columns as a segment has halo frames (2D; at least 16 / 32) - the choice below weighs halo
    // against idle CUs, and a batch that cannot fill the chip with longer segments is a LATENCY case: a workgroup walks its
    // segment frame after frame, so one stream of 4,081 columns took 0.18 ms as 64 segments of 64 (until late round 6 the
    // floor: 64 columns; 8D at N = 16384) and takes 0.08 ms as 256 segments of 16.  The small-N kernel has a short reach and
    // 4-8 frames per iteration: its floor was always low.
    const int64_t seg_min = kind == FusedKind::small_n ? std::max<int64_t>(16, 4 * D) : (kind == FusedKind::big_n ? std::max<int64_t>(32, 2 * D) : std::max<int64_t>(16, 2 * D));
    seg = seg < seg_min ? seg_min : seg;
    const bool is_shared = force_shared >= 0 ? force_shared == 1 : shared == 1;
    if (!is_shared) {
        // the device is this launch's alone: the four-round rule above only buys halo (~3 frames of pipeline fill)
        seg = std::max(seg_min, seglen_by_rounds(ncu, S, C, D, seg_min, 3.0));
        if (shared == 2 && seg > 1024) seg = 1024;   // two launches share the chip (emspec_batch's two-lane pipeline)
    }
    if (seglen_override >= 2) seg = seglen_override;
    seg = (seg + 1) & ~(int64_t)1;
    // Shared device (the engine has a communicator with other ranks, so RCCL transfers and the gather's pack / expand
    // kernels take CUs while this launch runs): the last quarter of every stream is cut into quarter-length pieces and
    // the grid becomes (streams, segments), so all long segments are dispatched first - the launch ends on short
    // workgroups instead of on a mostly empty extra round (a workgroup fills its CU: losing 8 CUs turned 4 rounds into 5).
    FusedSegPlan p{SegPlan{(int)seg, 1 << 30, (int)seg, 0}, (C + seg - 1) / seg, false, false};
    if (is_shared) {
        const int64_t tail = ((seg / 4) + 1) & ~(int64_t)1;
        if (tail >= seg_min && p.nseg >= 2) {
            const int64_t nlong = p.nseg - (p.nseg + 3) / 4;              // the last quarter (at least one segment) is cut finer
            const int64_t rest = C - nlong * seg;
            p.sp = SegPlan{(int)seg, (int)nlong, (int)tail, 1};
            p.nseg = nlong + (rest + tail - 1) / tail;
        }
    }
    p.streams_first = p.sp.short_last != 0;
    p.ok = p.nseg <= 65535;
    return p;
}

// The longest segment fused_seg_plan can return: every rule above cuts a stream into at least one segment, so without an
// override the length is at most max(seg_min, C) rounded up to even - one segment that is the whole stream (more streams than
// four rounds of CUs hold) - and an override is taken as given.  Nothing in the planner bounds C.
inline int64_t fused_seglen_max(int64_t C, int D, FusedKind kind, int64_t seglen_override) {
    const int64_t seg_min = kind == FusedKind::small_n ? std::max<int64_t>(16, 4 * D) : (kind == FusedKind::big_n ? std::max<int64_t>(32, 2 * D) : std::max<int64_t>(16, 2 * D));
    return (std::max(std::max(seg_min, C), seglen_override >= 2 ? seglen_override : 0) + 1) & ~(int64_t)1;
}
// fused4096_pp_kernel keeps its column bookkeeping in int, relative to the segment's first frame: half-iteration indices up
// to seglen + 2D + 3, and a remaining-samples count that starts at most at INT_MAX and falls by 2 hop per pair of
// half-iterations, hop (seglen + 2D + 5) in all; it has to stay above a thread's largest offset (under 8192) when it started
// clamped, and inside int when it did not.  2^30 samples per segment leave both a wide margin (and SegPlan holds ints).
constexpr int64_t kFusedPpMaxWalk = (int64_t)1 << 30;
inline bool fused_pp_walk_ok(int64_t seglen, int D, int hop) { return seglen >= 1 && (seglen + 2 * D + 5) * hop <= kFusedPpMaxWalk; }

// ---- the EXACT fused kernels (exact_fused.hip.inc, exact_fused_lr.hip.inc): exclusive-device plans, uniform grids ----
// Segment lengths by seglen_by_rounds, clamped only to >= 1 (seg_min bounds the candidates, not the result); seglen_override as
// above.  (Both launchers once started from max(seg_min, (C + 3) / 4): dead, round 1 always replaced it.)
// The parking kernel: seg_min = max(64, 4D), 3 half-iterations of pipeline fill.
inline int64_t exact_fused_seglen(int64_t ncu, int S, int64_t C, int D, int64_t seglen_override) {
    const int64_t seg = seglen_override >= 2 ? seglen_override : seglen_by_rounds(ncu, S, C, D, std::max<int64_t>(64, 4 * D), 3.0);
    return seg < 1 ? 1 : seg;
}
// The no-parking kernel at n = 4096 / 2048 / 1024: seg_min = max(16, 2D) (as the float32 kernels: short batches are latency
// cases), 3 half-iterations of 4096 / n frames of pipeline fill.
inline int64_t exact_lr_seglen(int64_t ncu, int n, int S, int64_t C, int D, int64_t seglen_override) {
    const int64_t seg = seglen_override >= 2 ? seglen_override : seglen_by_rounds(ncu, S, C, D, std::max<int64_t>(16, 2 * D), 3.0 * (double)(4096 / n));
    return seg < 1 ? 1 : seg;
}
// what a uniform grid of nseg segments of seg columns must satisfy (SegPlan and the kernels' column arithmetic hold ints)
inline bool exact_fused_grid_ok(int64_t nseg, int64_t seg) { return nseg <= 65535 && seg <= 0x3fffffff; }

// ---- low-row scratch of the EXACT kernels: one slice of per_group bytes per workgroup of a launch ----
// Workgroups per launch are capped so that the scratch stays small (launches of one stream are serialised anyway); one
// stream's segments always fit.
constexpr int64_t kMaxScratchGroups = 2048;
inline int64_t scratch_groups(int64_t nseg, int S) { return std::max<int64_t>(nseg, std::min<int64_t>(kMaxScratchGroups, nseg * (int64_t)S)); }
// whether a scratch of low_bytes serves a launch at all (one stream's segments)
inline bool scratch_holds_a_stream(size_t low_bytes, size_t per_group, int64_t nseg) { return low_bytes >= per_group * (size_t)nseg; }
// streams per launch: as many as the scratch has slices for (per_group == 0: no scratch, all of them)
inline int64_t streams_per_launch(int S, int64_t nseg, size_t low_bytes, size_t per_group) {
    return per_group ? std::max<int64_t>(1, std::min<int64_t>(S, (int64_t)(low_bytes / per_group) / nseg)) : S;
}

// ---- tile form of either scatter: a workgroup owns `tile` whole columns in LDS (cell bytes each: float32 4, EXACT 8) ----
struct TilePlan { int tile; size_t lds; int64_t ntiles; bool ok; };   // ok false: not even one column fits
inline TilePlan tile_scatter_plan(int rows, int64_t C, int cell, int max_tile) {
    const int tile = std::min(max_tile, (int)((150 * 1024) / ((size_t)rows * cell)));
    if (tile < 1) return TilePlan{tile, 0, 0, false};
    return TilePlan{tile, (size_t)tile * rows * cell + 1024, (C + tile - 1) / tile, true};
}

// ---- the float32 scatter (kernels.hip: launch_tile_scatter) ----
// ch: consecutive bins per thread, wide enough that adjacent lanes rarely share a row; F: frames per step of the walk, so that
// F * chunks-per-frame covers the 1024 threads; walk_lds: the walk's (2D + F)-slot ring; walk: the walking ring, else tiles;
// seg, nseg: the walk's segments (0 for tiles); tiles: zero for the walk
struct ScatterPlan { int ch, F; size_t walk_lds; bool walk; int64_t seg, nseg; TilePlan tiles; };
inline ScatterPlan scatter_plan(int ncu, int n, int rows, int D, int S, int64_t C, bool use_walk) {
    ScatterPlan p{n >= 8192 ? 32 : (n >= 2048 ? 8 : 4), 0, 0, false, 0, 0, TilePlan{0, 0, 0, false}};
    const int nch = (n / 2 + 2 + p.ch - 1) / p.ch;
    p.F = std::max(1, std::min(8, (1024 + nch - 1) / nch));
    p.walk_lds = (size_t)(2 * D + p.F) * rows * 4 + 1024;
    // measured: the walk wins when the tiles would re-read every record >= 2x (D >= 16: N=16384/512
    // 1.04e7 vs 0.94e7 col/s); for small D the tiles' independent workgroups win (N=1024: 1.8e8 vs 1.6e8)
    p.walk = use_walk && D >= 16 && p.walk_lds <= 156 * 1024;
    if (!p.walk) { p.tiles = tile_scatter_plan(rows, C, 4, 32); return p; }
    int64_t seg = (S * C + 4 * ncu - 1) / (4 * ncu);   // >= 4 workgroups per CU when there is enough work
    seg = seg < 128 ? 128 : (seg > 1024 ? 1024 : seg);
    p.seg = (seg + p.F - 1) / p.F * p.F;
    p.nseg = (C + p.seg - 1) / p.seg;
    return p;
}

// ---- the EXACT scatter (exact.hip.inc: launch_exact_tile_scatter) ----
// How the records of (n, plan) are scattered: the walking ring whole (rl = 0), the walking ring with its rows < rl in a global
// scratch (rl > 0; ebin_f32 = the plan's float32 edge table in DFT-bin units, on the host: the axis is served when at most 6 %
// of the bins lie below row rl), or 16-column tiles (F = 0).  rec_stride: records per frame (ex::rec_stride(n)).
struct ExactScatterPlan { int F, rl, seg; int64_t nseg; size_t lds, scratch_per_group; };
inline ExactScatterPlan exact_scatter_plan(int64_t ncu, int rec_stride, int n, int rows, int D, int S, int64_t C, const float* ebin_f32) {
    ExactScatterPlan sp{0, 0, 0, 0, 0, 0};
    const int nch = rec_stride / 4;
    int F = (1024 + nch - 1) / nch;
    F = F < 1 ? 1 : (F > 8 ? 8 : F);
    int rl = 0;
    size_t wl = (size_t)(2 * D + F) * rows * 8 + 1024;
    if (wl > 158 * 1024) {
        // the row split: six frames per step (two barriers per step; 2D + 6 slots), as many rows in LDS as fit
        if (!ebin_f32 || rows % 4) return sp;
        F = 6;
        const int slots = 2 * D + F;
        const size_t mask = (size_t)slots * ((rows + 31) >> 5) * 4;   // (sized for the worst case, rl = rows)
        int rh = (int)(((size_t)158 * 1024 - 1024 - mask) / ((size_t)slots * 8)) & ~3;
        if (rh >= rows || rh < 64) return sp;
        rl = rows - rh;
        if (!((double)ebin_f32[rl] / (double)(n / 2) <= 0.06)) return sp;
        wl = (size_t)slots * rh * 8 + 1024 + mask;
    }
    // Segment length by ROUNDS of workgroups (round 5; seglen_by_rounds' reasoning): the ring takes most of a CU's LDS, so the
    // workgroups of a launch run in rounds of (CUs x workgroups that fit a CU), and a launch costs rounds x (segment + its
    // 2D-frame halo + pipeline fill).  The former rule (a fixed lower bound of 8D columns) gave configs[4]'s stream-chunks of
    // five streams 62 segments each = 310 workgroups on 256 CUs: two rounds, the second a fifth full.
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, (int64_t)(kLdsBytes / wl)));
    const int64_t places = ncu * per_cu;
    const int64_t over = 2 * D + F;
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
    sp.scratch_per_group = (size_t)(2 * D + F) * rl * 8;
    return sp;
}

}  // namespace emspec
