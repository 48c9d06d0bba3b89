// seg_bound_driver.cpp — stand-alone (no HIP, no GPU): the longest segment fused_seg_plan (emspec_seg_plan.h) returns, against
//  1. the bound the header states for it, fused_seglen_max: over a sweep of CU counts, stream counts, column counts (up to
//     2^31 - 2), reaches, kernel kinds, sharing modes and the diagnostic override, every plan's segment length is positive,
//     even, at most that bound, and its segments cover the stream;
//  2. the walk fused4096_pp_kernel counts in int, fused_pp_walk_ok: on a 256-CU device, for every stream count and every stream
//     length whose batch fits 2^36 samples (256 GiB of float32 - more than the device has), at hop 256 / 512 / 1024 with the
//     reach that goes with it, the plan's segment passes, and the largest walk is printed.
// Prints "plans <n> max_walk <samples>"; every violation goes to stderr and makes the exit status 1.
//   g++ -std=c++17 -O1 -I em-spec_amd/csrc tests/cdriver/seg_bound_driver.cpp -o seg_bound && ./seg_bound
#include "emspec_seg_plan.h"
#include <cstdio>

using namespace emspec;

int main() {
    int bad = 0;
    long long plans = 0;
    const int64_t ncus[] = {1, 8, 64, 256, 304};
    const int Ss[] = {1, 3, 64, 255, 257, 1024, 1025, 65535};
    const int64_t Cs[] = {1, 15, 131, 4081, 16369, (int64_t)1 << 20, ((int64_t)1 << 23) + 1, ((int64_t)1 << 31) - 2};
    const int Ds[] = {0, 2, 4, 8, 16};
    for (int64_t ncu : ncus) for (int S : Ss) for (int64_t C : Cs) for (int D : Ds) for (int kind = 0; kind < 3; ++kind)
        for (int shared = 0; shared < 3; ++shared) for (int force = -1; force < 2; ++force) for (int64_t ovr : {(int64_t)0, (int64_t)33}) {
            const FusedSegPlan p = fused_seg_plan(ncu, S, C, D, (FusedKind)kind, shared, force, ovr);
            const int64_t top = fused_seglen_max(C, D, (FusedKind)kind, ovr);
            const int64_t seg = p.sp.seglen, tail = p.sp.tail;
            ++plans;
            bool ok = top <= 0x7fffffff && seg >= 2 && (seg & 1) == 0 && seg <= top && tail >= 2 && tail <= seg;
            // the segments cover the stream: nseg uniform ones, or nlong long ones and the rest in tails
            if (ok && !p.sp.short_last) ok = p.nseg * seg >= C && (p.nseg - 1) * seg < C;
            if (ok && p.sp.short_last) ok = p.sp.nlong * seg + (p.nseg - p.sp.nlong) * tail >= C && p.sp.nlong * seg < C;
            if (!ok) {
                ++bad;
                fprintf(stderr, "plan ncu %lld S %d C %lld D %d kind %d shared %d force %d ovr %lld: seglen %lld tail %lld nseg %lld nlong %d max %lld\n",
                        (long long)ncu, S, (long long)C, D, kind, shared, force, (long long)ovr, (long long)seg, (long long)tail,
                        (long long)p.nseg, p.sp.nlong, (long long)top);
            }
        }
    int64_t max_walk = 0;
    for (int hop : {256, 512, 1024}) for (int D : {0, 4096 / (2 * hop)}) for (int shared = 0; shared < 3; ++shared)
        for (int S = 1; S <= 65535; S = S < 1100 ? S + 1 : S * 2 + 1)
            for (int lg = 13; lg <= 36; ++lg) for (int64_t dl : {(int64_t)-1, (int64_t)0, (int64_t)4097}) {
                const int64_t L = ((int64_t)1 << lg) + dl;
                if ((int64_t)S * L > ((int64_t)1 << 36) + 4097 * (int64_t)S) continue;
                const int64_t C = (L - 4096) / hop + 1;
                const FusedSegPlan p = fused_seg_plan(256, S, C, D, FusedKind::n4096_8192, shared, -1, 0);
                ++plans;
                if (!p.ok) continue;   // (more segments than a grid holds: the launcher refuses it before the walk is looked at)
                const int64_t walk = ((int64_t)p.sp.seglen + 2 * D + 5) * hop;
                max_walk = walk > max_walk ? walk : max_walk;
                if (!fused_pp_walk_ok(p.sp.seglen, D, hop)) {
                    ++bad;
                    fprintf(stderr, "walk hop %d D %d shared %d S %d L %lld: seglen %d\n", hop, D, shared, S, (long long)L, p.sp.seglen);
                }
            }
    printf("plans %lld max_walk %lld\n", plans, (long long)max_walk);
    return bad ? 1 : 0;
}
