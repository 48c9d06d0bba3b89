// seg_plan_driver.cpp — prints the segment plans of the walking kernels (em-spec_amd/csrc/emspec_seg_plan.h) for a list of cases, as
// a JSON list with one object per case and every field of every plan: the arithmetic that sets the grid of every batch launch,
// without a GPU.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc
//       tests/cdriver/seg_plan_driver.cpp -o seg_plan_driver
// tests/test_seg_plan_cpu.py compares the output with tests/golden/seg_plans.json.  With -DSEG_PLAN_VERBATIM the same cases go
// through seg_plan_verbatim.h, the arithmetic as it stood inside the five launchers: that build wrote the fixture.
// With arguments it prints one case instead of the list (tests/test_gpu_parity.py: the plan for the device's real CU count):
//   seg_plan_driver fused ncu S C D kind shared force_shared seglen_override
//   seg_plan_driver exact_fused ncu S C D seglen_override
//   seg_plan_driver exact_lr ncu n S C D rl seglen_override
#ifdef SEG_PLAN_VERBATIM
#include "seg_plan_verbatim.h"
namespace V = emspec_verbatim;
#else
#include "emspec_seg_plan.h"
using namespace emspec;
#endif

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

bool g_first = true;
void open_record(const char* kind) { printf("%s{\"kind\": \"%s\", ", g_first ? "[\n" : ",\n", kind); g_first = false; }

#ifdef SEG_PLAN_VERBATIM
// the getenv strings the launchers read, from the cases' numbers
struct Env { std::string s; bool set; const char* get() const { return set ? s.c_str() : nullptr; } };
Env env_num(long long v, bool set) { return Env{std::to_string(v), set}; }
#endif

// kind: 0 the N = 4096 / 8192 families, 1 fused_small, 2 N = 16384; force: -1, or EMSPEC_SHARED's 0 / 1; ovr: 0, or EMSPEC_SEGLEN
void fused_case(long long ncu, int S, long long C, int D, int kind, int shared, int force, long long ovr) {
    open_record("fused");
    printf("\"case\": {\"ncu\": %lld, \"S\": %d, \"C\": %lld, \"D\": %d, \"kind\": %d, \"shared\": %d, \"force\": %d, \"ovr\": %lld}, ",
           ncu, S, C, D, kind, shared, force, ovr);
#ifdef SEG_PLAN_VERBATIM
    const V::FusedOut o = V::launch_fused_plan(ncu, kind == 1, kind == 2, D, shared, S, C, env_num(force, force >= 0).get(), env_num(ovr, ovr != 0).get());
    const V::SegPlan sp = o.sp;
    const long long nseg = o.nseg;
    const bool ok = !o.invalid, streams_first = o.invalid ? sp.short_last != 0 : o.streams_first;
#else
    const FusedSegPlan p = fused_seg_plan(ncu, S, C, D, kind == 1 ? FusedKind::small_n : (kind == 2 ? FusedKind::big_n : FusedKind::n4096_8192), shared, force, ovr);
    const SegPlan sp = p.sp;
    const long long nseg = p.nseg;
    const bool ok = p.ok, streams_first = p.streams_first;
#endif
    printf("\"seglen\": %d, \"nlong\": %d, \"tail\": %d, \"short_last\": %d, \"nseg\": %lld, \"streams_first\": %d, \"ok\": %d}",
           sp.seglen, sp.nlong, sp.tail, sp.short_last, nseg, (int)streams_first, (int)ok);
}

void exact_fused_case(long long ncu, int S, long long C, int D, long long ovr) {
    open_record("exact_fused");
    printf("\"case\": {\"ncu\": %lld, \"S\": %d, \"C\": %lld, \"D\": %d, \"ovr\": %lld}, ", ncu, S, C, D, ovr);
#ifdef SEG_PLAN_VERBATIM
    const V::ExactFusedOut o = V::launch_exact_fused_plan(ncu, D, S, C, env_num(ovr, ovr != 0).get());
    const long long seg = o.seg, nseg = o.nseg;
    const bool ok = !o.invalid;
#else
    const long long seg = exact_fused_seglen(ncu, S, C, D, ovr), nseg = (C + seg - 1) / seg;
    const bool ok = exact_fused_grid_ok(nseg, seg);
#endif
    printf("\"seg\": %lld, \"nseg\": %lld, \"ok\": %d}", seg, nseg, (int)ok);
}

// NOTE on what is pinned: in the build against emspec_seg_plan.h, "accept" and "s_per" of an exact_lr record and "launched_F",
// "s_per" and the tile fields of an exact_scatter record RESTATE the few lines of glue the launchers keep around the header's
// functions (launch_exact_fused_lr's `rl > 0 && !low` check, launch_exact_tile_scatter's "no scratch: tiles" demotion): the
// header's scratch_holds_a_stream, streams_per_launch and tile_scatter_plan are pinned through them, the launchers' own glue is
// not - a slip there would not show here.
// the no-parking kernel: rl low rows per slot in the global scratch (0: none).  The scratch is sized (emspec_api.cpp) and then
// handed to the launch: "s_per" and "accept" are the launch's answer to exactly that size, "accept_less" to one byte less than
// one stream's segments need.
void exact_lr_case(long long ncu, int n, int S, long long C, int D, int rl, long long ovr) {
    const int skip = n == 4096 ? 0 : (n == 2048 ? 1 : 2);
    const int slots = skip == 0 ? (2 * D + 2 > 3 ? 2 * D + 2 : 3) : 2 * D + (2 << skip);   // exl::lr_slots
    open_record("exact_lr");
    printf("\"case\": {\"ncu\": %lld, \"n\": %d, \"S\": %d, \"C\": %lld, \"D\": %d, \"slots\": %d, \"rl\": %d, \"ovr\": %lld}, ", ncu, n, S, C, D, slots, rl, ovr);
#ifdef SEG_PLAN_VERBATIM
    const Env e = env_num(ovr, ovr != 0);
    const size_t bytes = V::exact_fused_lr_scratch_bytes(ncu, n, D, slots, rl, S, C, e.get());
    const V::ExactLrOut o = V::launch_exact_fused_lr_plan(ncu, n, D, slots, rl, S, C, true, bytes, e.get());
    const long long seg = o.seg, nseg = o.nseg;
    const bool ok = nseg <= 65535 && seg <= 0x3fffffff;
    const size_t per_group = (size_t)slots * (size_t)rl * 8;
    const bool accept = ok && !o.invalid;
    const long long s_per = accept ? o.s_per : 0;
    const bool accept_less = ok && rl > 0 && !V::launch_exact_fused_lr_plan(ncu, n, D, slots, rl, S, C, true, per_group * (size_t)nseg - 1, e.get()).invalid;
    const long long groups = per_group ? (long long)(bytes / per_group) : 0;
#else
    const long long seg = exact_lr_seglen(ncu, n, S, C, D, ovr), nseg = (C + seg - 1) / seg;
    const bool ok = exact_fused_grid_ok(nseg, seg);
    const size_t per_group = (size_t)slots * (size_t)rl * 8;
    const long long groups = rl > 0 ? scratch_groups(nseg, S) : 0;
    const size_t bytes = (size_t)groups * per_group;
    const bool accept = ok && (rl <= 0 || scratch_holds_a_stream(bytes, per_group, nseg));
    const long long s_per = accept ? streams_per_launch(S, nseg, bytes, per_group) : 0;
    const bool accept_less = ok && rl > 0 && scratch_holds_a_stream(per_group * (size_t)nseg - 1, per_group, nseg);
#endif
    printf("\"seg\": %lld, \"nseg\": %lld, \"ok\": %d, \"per_group\": %zu, \"groups\": %lld, \"scratch_bytes\": %zu, \"accept\": %d, \"s_per\": %lld, \"accept_less\": %d}",
           seg, nseg, (int)ok, per_group, groups, bytes, (int)accept, s_per, (int)accept_less);
}

void scatter_case(int ncu, int n, int rows, int D, int S, long long C, int use_walk) {
    open_record("scatter");
    printf("\"case\": {\"ncu\": %d, \"n\": %d, \"rows\": %d, \"D\": %d, \"S\": %d, \"C\": %lld, \"use_walk\": %d}, ", ncu, n, rows, D, S, C, use_walk);
#ifdef SEG_PLAN_VERBATIM
    const V::WalkOut o = V::launch_tile_scatter_plan(ncu, n, rows, D, S, C, use_walk != 0);
    printf("\"ch\": %d, \"F\": %d, \"walk_lds\": %zu, \"walk\": %d, \"seg\": %lld, \"nseg\": %lld, \"tile\": %d, \"tile_lds\": %zu, \"ntiles\": %lld, \"ok\": %d}",
           o.ch, o.F, o.wl, (int)o.walk, (long long)o.seg, (long long)o.nseg, o.tile, o.tile_lds, (long long)o.ntiles, (int)!o.invalid);
#else
    const ScatterPlan p = scatter_plan(ncu, n, rows, D, S, C, use_walk != 0);
    printf("\"ch\": %d, \"F\": %d, \"walk_lds\": %zu, \"walk\": %d, \"seg\": %lld, \"nseg\": %lld, \"tile\": %d, \"tile_lds\": %zu, \"ntiles\": %lld, \"ok\": %d}",
           p.ch, p.F, p.walk_lds, (int)p.walk, (long long)p.seg, (long long)p.nseg, p.tiles.tile, p.tiles.lds, (long long)p.tiles.ntiles, (int)(p.walk || p.tiles.ok));
#endif
}

// axis: 0 no float32 edge table (null), 1 / 2 a log axis of `rows` rows from bin e0 = 0.0017 n / 0.1 n to bin 0.42 n (at rows =
// 1024 the row split asks for row 512: bin 0.027 n or 0.2 n - on either side of 0.06 n / 2).  low: whether the launch gets the
// scratch that was sized for it.
void exact_scatter_case(long long ncu, int n, int rows, int D, int S, long long C, int axis, int low) {
    std::vector<float> eb(rows + 1);
    const double e0 = (axis == 2 ? 0.1 : 0.0017) * n, e1 = 0.42 * n;
    for (int r = 0; r <= rows; ++r) eb[r] = (float)(e0 * std::pow(e1 / e0, (double)r / rows));
    const float* ebin = axis ? eb.data() : nullptr;
    const int Kp = n / 2 + 4;   // ex::rec_stride(n)
    open_record("exact_scatter");
    printf("\"case\": {\"ncu\": %lld, \"n\": %d, \"rows\": %d, \"D\": %d, \"S\": %d, \"C\": %lld, \"axis\": %d, \"low\": %d}, ", ncu, n, rows, D, S, C, axis, low);
#ifdef SEG_PLAN_VERBATIM
    static_assert(V::ex::rec_stride(16384) == 8196, "rec_stride");
    if (Kp != V::ex::rec_stride(n)) abort();
    const V::ExactScatterPlan sp = V::exact_scatter_plan(ncu, n, rows, D, S, C, ebin);
    const size_t bytes = V::exact_scatter_scratch_bytes(ncu, n, rows, D, S, C, ebin);
    const V::ExactScatterOut o = V::launch_exact_tile_scatter_plan(ncu, n, rows, D, S, C, low ? ebin : nullptr, low != 0, low ? bytes : 0);
    const int launched_F = o.sp.F, tile = o.tile;
    const long long s_per = o.s_per, ntiles = o.ntiles;
    const size_t tile_lds = o.tile_lds;
    const bool ok = !o.invalid;
    const long long groups = sp.scratch_per_group && bytes ? (long long)(bytes / sp.scratch_per_group) : 0;
#else
    const ExactScatterPlan sp = exact_scatter_plan(ncu, Kp, n, rows, D, S, C, ebin);
    const long long groups = sp.F && sp.rl ? scratch_groups(sp.nseg, S) : 0;
    const size_t bytes = (size_t)groups * sp.scratch_per_group;
    // the launch (launch_exact_tile_scatter): without its scratch it is handed no edge table either (emspec_api.cpp)
    ExactScatterPlan lp = exact_scatter_plan(ncu, Kp, n, rows, D, S, C, low ? ebin : nullptr);
    if (lp.F && lp.rl && (!low || !scratch_holds_a_stream(bytes, lp.scratch_per_group, lp.nseg))) lp.F = 0;
    const int launched_F = lp.F;
    const long long s_per = lp.F ? streams_per_launch(S, lp.nseg, low ? bytes : 0, lp.scratch_per_group) : 0;
    const TilePlan tp = lp.F ? TilePlan{0, 0, 0, true} : tile_scatter_plan(rows, C, 8, 16);
    const int tile = tp.tile;
    const long long ntiles = tp.ntiles;
    const size_t tile_lds = tp.lds;
    const bool ok = tp.ok;
#endif
    printf("\"F\": %d, \"rl\": %d, \"seg\": %d, \"nseg\": %lld, \"lds\": %zu, \"per_group\": %zu, \"groups\": %lld, \"scratch_bytes\": %zu, "
           "\"launched_F\": %d, \"s_per\": %lld, \"tile\": %d, \"tile_lds\": %zu, \"ntiles\": %lld, \"ok\": %d}",
           sp.F, sp.rl, sp.seg, (long long)sp.nseg, sp.lds, sp.scratch_per_group, groups, bytes, launched_F, s_per, tile, tile_lds, ntiles, (int)ok);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) {   // one case from the command line
        std::vector<long long> a;
        for (int i = 2; i < argc; ++i) a.push_back(atoll(argv[i]));
        if (!strcmp(argv[1], "fused") && a.size() == 8) fused_case(a[0], (int)a[1], a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], a[7]);
        else if (!strcmp(argv[1], "exact_fused") && a.size() == 5) exact_fused_case(a[0], (int)a[1], a[2], (int)a[3], a[4]);
        else if (!strcmp(argv[1], "exact_lr") && a.size() == 7) exact_lr_case(a[0], (int)a[1], (int)a[2], a[3], (int)a[4], (int)a[5], a[6]);
        else { fprintf(stderr, "usage: see the head of seg_plan_driver.cpp\n"); return 2; }
        printf("\n]\n");
        return 0;
    }
    // (no cross product: each axis is swept where it decides something, with the others at a value that lets it)
    const long long ncus[4] = {256, 304, 64, 1};
    const int streams[11] = {1, 2, 3, 5, 16, 34, 36, 64, 70, 257, 65535};
    const long long cols[10] = {1, 15, 16, 17, 130, 700, 4081, 16369, 262144, 8388593};
    const int reach[8] = {0, 1, 2, 8, 16, 32, 64, 1024};

    // ---- fused float32 ----
    // the device alone, the headline family at D = 8: every stream count at three lengths and every length at 1 and 64 streams
    // on 256 CUs, corners on the other CU counts
    for (int S : streams)
        for (long long C : cols)
            if (S == 1 || S == 64 || C == 17 || C == 700 || C == 16369) fused_case(256, S, C, 8, 0, 0, -1, 0);
    for (long long ncu : {304, 64, 1})
        for (int S : {1, 70, 65535})
            for (long long C : {700, 8388593}) fused_case(ncu, S, C, 8, 0, 0, -1, 0);
    // every reach and kind (seg_min), alone and shared
    for (int D : reach)
        for (int kind : {0, 1, 2})
            for (int shared : {0, 1}) fused_case(256, 3, 700, D, kind, shared, -1, 0);
    // shared with a collective (the tail cut: taken, and refused for a short tail or a single segment) and with the second lane
    // (the cap at 1,024 columns)
    for (int shared : {1, 2})
        for (int S : {1, 5, 64})
            for (long long C : {16, 700, 16369, 262144}) {
                fused_case(256, S, C, 8, 0, shared, -1, 0);
                if (S == 1 && C >= 700) fused_case(304, S, C, 16, 2, shared, -1, 0);
            }
    // the diagnostic switches: a forced plan either way, a segment length (odd: rounded up to even; below 2: ignored), more
    // segments than a grid holds
    for (int force : {0, 1})
        for (int shared : {0, 1, 2})
            for (int S : {3, 64}) fused_case(256, S, S == 3 ? 700 : 16369, 8, 0, shared, force, 0);
    for (long long ovr : {33, 64, 1})
        for (int force : {-1, 1})
            for (int S : {2, 3, 64}) fused_case(256, S, S == 2 ? 17 : (S == 3 ? 700 : 8388593), 8, S == 2 ? 1 : 0, 0, force, ovr);

    // ---- the EXACT fused kernels ----
    for (long long ncu : ncus)
        for (int S : streams)
            for (long long C : cols) {
                if (ncu == 256 ? !(S == 5 || C == 16369 || (S == 3 && C == 8388593)) : !((S == 1 || S == 65535) && (C == 700 || C == 8388593))) continue;
                exact_fused_case(ncu, S, C, 8, 0);
                exact_lr_case(ncu, 4096, S, C, 8, 448, 0);
            }
    for (int D : reach)
        for (int S : {5, 64}) {
            const long long C = S == 5 ? 700 : 16369;
            exact_fused_case(256, S, C, D, 0);
            for (int n : {4096, 2048, 1024})
                if (n == 4096 || (S == 5 && (D == 2 || D == 16))) exact_lr_case(256, n, S, C, D, D == 8 ? 0 : 64 * (D % 7 + 1), 0);
        }
    for (long long ovr : {33, 64})
        for (int S : {3, 64})
            for (long long C : {700, 262144, 8388593}) {
                if (S == 64 && C == 700) continue;
                exact_fused_case(304, S, C, 8, ovr);
                exact_lr_case(304, 4096, S, C, 8, 448, ovr);
            }

    // ---- the float32 scatter: every size's chunk width and F; D on either side of 16; a ring too large for LDS; tiles ----
    for (int n : {256, 1024, 2048, 4096, 8192, 16384})
        for (int D : {8, 16, 64}) scatter_case(256, n, 1024, D, 64, 16369, 1);
    for (int D : reach)
        for (int rows : {64, 1024}) {
            if (rows == 1024) scatter_case(256, 16384, rows, D, 1, 130, 1);
            scatter_case(304, 16384, rows, D, 5, 16369, 1);
        }
    for (long long C : {1, 8388593}) scatter_case(256, 16384, 1024, 16, 64, C, 1);
    for (int D : {8, 16, 32}) scatter_case(256, 16384, 1024, D, 3, 700, 0);
    for (int ncu : {64, 1}) for (long long C : {4081, 262144}) scatter_case(ncu, 16384, 1024, 16, 16, C, 1);
    scatter_case(256, 16384, 65536, 8, 2, 700, 1);   // (not even one column of tiles fits)

    // ---- the EXACT scatter: whole ring, row split (an axis on either side of 6 %, none), tiles; scratch and stream split ----
    for (int rows : {64, 1024})
        for (int D : reach)
            for (int axis : {0, 1, 2}) {
                if (rows == 64 && (axis != 1 || (D != 8 && D != 64 && D != 1024))) continue;
                exact_scatter_case(256, 16384, rows, D, 5, 700, axis, 1);
                if (axis == 1) exact_scatter_case(304, 16384, rows, D, 257, 262144, axis, 1);
                if (rows == 1024 && (D == 8 || D == 16 || D == 64)) exact_scatter_case(256, 8192, rows, D, 5, 700, axis, 1);
            }
    for (long long ncu : ncus)
        for (int S : {1, 64, 65535}) exact_scatter_case(ncu, 16384, 1024, 16, S, S == 64 ? 17 : 8388593, 1, S != 64);
    exact_scatter_case(256, 16384, 65536, 0, 2, 700, 1, 1);   // (not even one column of tiles fits)
    printf("\n]\n");
    return 0;
}
