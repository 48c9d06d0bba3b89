// kernel_plan_driver.cpp — prints, for a list of cases at the boundaries, which kernel serves a call, the dynamic LDS it asks for
// and the record workspaces (em-spec_amd/csrc/emspec_kernel_plan.h), as a JSON list with one object per case: the arithmetic that
// decides whether a shape is served and by what, without a GPU.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc
//       tests/cdriver/kernel_plan_driver.cpp -o kernel_plan_driver
// tests/test_kernel_plan_cpu.py compares the output with tests/golden/kernel_plans.json.  With -DKERNEL_PLAN_VERBATIM the same
// cases go through kernel_plan_verbatim.h, the statements as they stood beside the kernels and in emspec_api.cpp: that build
// wrote the fixture.
#ifdef KERNEL_PLAN_VERBATIM
#include "kernel_plan_verbatim.h"
namespace V = emspec_verbatim;
#else
#include "emspec_kernel_plan.h"
#endif
#include "emspec_tables.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace emspec;

namespace {

bool g_first = true;
void open_record(const char* kind) { printf("%s{\"kind\": \"%s\", ", g_first ? "[\n" : ",\n", kind); g_first = false; }

// FAST: no_fused is EMSPEC_NO_FUSED; the plan's D is the shape's.  ("variant": 0 in every record: the fixture was written when
// the route still took EMSPEC_FUSED_VARIANT, and its remaining records keep their bytes; the verbatim statements are handed 0.)  "seg_kind": the FusedKind of the segment plan (0 the N = 4096 / 8192 families, 1 fused_small, 2 N = 16384).
void fast_case(int n, int hop, int rows, int reassign, int no_fused) {
    open_record("fast");
    printf("\"case\": {\"n\": %d, \"hop\": %d, \"rows\": %d, \"reassign\": %d, \"no_fused\": %d, \"variant\": 0}, ", n, hop, rows, reassign, no_fused);
    const int D = latency(n, hop, reassign);
    static const char* const names[4] = {"fused_pp", "fused_small", "fused_8192", "fused_16384"};
    const char* route = "records_f32";
    int seg_kind = -1, slots = 0;
    size_t lds = 0, small_lds = 0;   // small_lds: what fused_small would ask for at this shape, served or not
    const bool small_size = n == 4096 || n == 2048 || n == 1024;
#ifdef KERNEL_PLAN_VERBATIM
    if (small_size) small_lds = V::fused_small_lds_bytes(rows, V::fused_small_slots(n, D));
    const bool supported = V::fused_supported(n, hop, rows, reassign, no_fused != 0, 0);
    const V::FusedOut o = V::launch_fused(n, hop, rows, reassign, D, no_fused != 0, 0);
    if (!o.not_supported) { route = names[o.family]; seg_kind = (int)o.kind; slots = o.slots; lds = o.lds; }
#else
    if (small_size) small_lds = fused_small_lds_bytes(rows, fused_small_slots(n, D));
    const Route r = fast_route(n, hop, rows, reassign, FastSwitches{no_fused != 0});
    const bool supported = !is_records(r);
    if (supported && fused_reach_ok(r.kind, n, hop, D)) {
        switch (r.kind) {
        case RouteKind::fused_pp: route = names[0]; seg_kind = 0; lds = fused_pp_lds_bytes(rows, hop); break;
        case RouteKind::fused_small: route = names[1]; seg_kind = 1; slots = fused_small_slots(n, D); lds = fused_small_lds_bytes(rows, slots); break;
        case RouteKind::fused_8192: route = names[2]; seg_kind = 0; lds = fused8192_lds_bytes(rows, hop); break;
        default: route = names[3]; seg_kind = 2; lds = fused16384_lds_bytes(rows); break;
        }
    }
#endif
    printf("\"D\": %d, \"supported\": %d, \"route\": \"%s\", \"seg_kind\": %d, \"slots\": %d, \"lds\": %zu, \"small_lds\": %zu}", D, (int)supported, route, seg_kind, slots, lds,
           small_lds);
}

// launch_fused handed a plan whose D is not the shape's: refused by the kernels built for the hop's own reach
void fast_reach_case(int n, int hop, int rows, int D) {
    open_record("fast_reach");
    printf("\"case\": {\"n\": %d, \"hop\": %d, \"rows\": %d, \"D\": %d}, ", n, hop, rows, D);
#ifdef KERNEL_PLAN_VERBATIM
    const bool refused = V::launch_fused(n, hop, rows, 1, D, false, 0).not_supported;
#else
    const Route r = fast_route(n, hop, rows, 1);
    const bool refused = is_records(r) || !fused_reach_ok(r.kind, n, hop, D);
#endif
    printf("\"refused\": %d}", (int)refused);
}

void frames_case(int log2n, int rows) {
    open_record("frames");
    printf("\"case\": {\"log2n\": %d, \"rows\": %d}, ", log2n, rows);
#ifdef KERNEL_PLAN_VERBATIM
    V::FramesOut o{};
    switch (log2n) {
    case 8: o = V::launch_frames_t<8>(rows); break;
    case 9: o = V::launch_frames_t<9>(rows); break;
    case 10: o = V::launch_frames_t<10>(rows); break;
    case 11: o = V::launch_frames_t<11>(rows); break;
    case 12: o = V::launch_frames_t<12>(rows); break;
    case 13: o = V::launch_frames_t<13>(rows); break;
    default: o = V::launch_frames_t<14>(rows); break;
    }
    const size_t lds = o.lds;
    const bool ok = !o.invalid;
#else
    const size_t lds = frames_lds_bytes(log2n, rows);
    const bool ok = lds <= kLdsBytes;
#endif
    printf("\"lds\": %zu, \"ok\": %d}", lds, (int)ok);
}

// the EXACT frame kernels; plain: the launch's sinks are a batch's records or a parity dump alone (not a live launch).
// "form": 0 generic, 1 the persistent N = 4096 kernel, 2 N = 16384
void exact_frames_case(int n, int rows, int S, long long nframes, int plain) {
    open_record("exact_frames");
    printf("\"case\": {\"n\": %d, \"rows\": %d, \"S\": %d, \"nframes\": %lld, \"plain\": %d}, ", n, rows, S, nframes, plain);
#ifdef KERNEL_PLAN_VERBATIM
    const V::ExactFramesOut o = V::launch_exact_frames(n, rows, S, nframes, plain != 0);
    const int form = o.form, edges_lds = o.edges_lds;
    const size_t lds = o.lds;
    const bool ok = !o.invalid;
#else
    int form = n == 16384 ? 2 : 0, edges_lds = 1;
    size_t lds;
    bool ok = true;
    if (n == 4096 && plain && exact_frames4096_persistent(rows, S, nframes)) { form = 1; lds = exact_frames4096_lds_bytes(rows); }
    else {
        const ExactFramesLds l = exact_frames_lds(exact_frames_planes(n), rows);
        lds = l.bytes; edges_lds = l.edges_lds;
        ok = n == 16384 || lds <= kLdsBytes;
    }
#endif
    printf("\"form\": %d, \"lds\": %zu, \"edges_lds\": %d, \"ok\": %d}", form, lds, edges_lds, (int)ok);
}

// axis: 0 the configured log axis (20 Hz .. 24 kHz at 48 kHz), 1 linear edges, 2 warped edges (low_end_boost 0.5), of axis_rows
// rows; the plan serves rows [row0, row0 + rows) of it (a band plan when row0 > 0 or rows < axis_rows).  parked / records:
// EMSPEC_EXACT_PARKED / EMSPEC_EXACT_RECORDS.
// A case may carry a log axis of its own, log_axis = {sample_rate, fmin, fmax} (tests/axis_cases.py): its record names the three
// beside the other fields of the case, with "axis": 0.
void exact_case(int n, int hop, int reassign, int rows, int row0, int axis_rows, int axis, int parked, int records,
                const float* log_axis = nullptr) {
    std::vector<float> hz(axis_rows + 1);
    if (axis == 1) for (int r = 0; r <= axis_rows; ++r) hz[r] = 20.0f + (24000.0f - 20.0f) * (float)r / (float)axis_rows;
    if (axis == 2) warped_edges_hz(axis_rows, 20.0f, 24000.0f, 0.5f, 1.0f, hz.data());
    const Axis ax = log_axis ? Axis{axis_rows, log_axis[0], log_axis[1], log_axis[2], nullptr}
                             : Axis{axis_rows, 48000.0f, 20.0f, 24000.0f, axis ? hz.data() : nullptr};
    const int D = latency(n, hop, reassign);
    open_record("exact");
    printf("\"case\": {\"n\": %d, \"hop\": %d, \"reassign\": %d, \"rows\": %d, \"row0\": %d, \"axis_rows\": %d, \"axis\": %d, \"parked\": %d, \"records\": %d",
           n, hop, reassign, rows, row0, axis_rows, axis, parked, records);
    if (log_axis) printf(", \"sample_rate\": %g, \"fmin\": %g, \"fmax\": %g", log_axis[0], log_axis[1], log_axis[2]);
    printf("}, ");
    static const char* const names[3] = {"exact_lr", "exact_parked", "exact_records"};
    int step, rl, slots = 0, uses = -1, lr_refused = 0;
    size_t lds = 0;
    const bool whole = row0 == 0 && rows == axis_rows;   // the engine's own plan: what emspec_uses_fused answers for
#ifdef KERNEL_PLAN_VERBATIM
    const V::ExactLadder l = V::run_columns_exact(ax, n, rows, D, row0, parked ? '1' : 0, records != 0);
    step = l.step; rl = l.rl;
    if (step == 0) { slots = V::exl::lr_slots(V::exact_lr_skip(n), D); lds = V::exl::lds_bytes(rows, rows - rl, slots); lr_refused = V::launch_exact_fused_lr_invalid(n, rows, D, rl); }
    if (step == 1) { slots = V::exf::exact_fused_slots(D); lds = V::exf::exact_fused_lds_bytes(rows, slots); }
    if (whole) uses = V::emspec_uses_fused_exact(ax, n, hop, reassign, rows, parked ? '1' : 0, records != 0);
#else
    const Route r = exact_route(n, rows, D, row0, ax, ExactSwitches{parked != 0, records != 0});
    step = r.kind == RouteKind::exact_lr ? 0 : (r.kind == RouteKind::exact_parked ? 1 : 2); rl = r.rl;
    if (step == 0) { slots = exl::lr_slots(exact_lr_skip(n), D); lds = exact_lr_lds_bytes(rows, rows - rl, slots); lr_refused = !exact_lr_split_ok(rows, rl, slots); }
    if (step == 1) { slots = exact_fused_slots(D); lds = exact_fused_lds_bytes(rows, slots); }
    if (whole) uses = is_records(r) ? 0 : 1;
#endif
    printf("\"D\": %d, \"route\": \"%s\", \"rl\": %d, \"rh\": %d, \"slots\": %d, \"lds\": %zu, \"lr_refused\": %d, \"uses_fused\": %d}",
           D, names[step], rl, step == 0 ? rows - rl : 0, slots, lds, lr_refused, uses);
}

// the no-parking kernel handed rh rows in LDS at N = 4096: its LDS, and whether the launch takes it
void exact_lr_split_case(int rows, int D, int rh) {
    open_record("exact_lr_split");
    printf("\"case\": {\"rows\": %d, \"D\": %d, \"rh\": %d}, ", rows, D, rh);
#ifdef KERNEL_PLAN_VERBATIM
    const int slots = V::exl::lr_slots(0, D);
    const size_t lds = V::exl::lds_bytes(rows, rh, slots);
    const bool ok = !V::launch_exact_fused_lr_invalid(4096, rows, D, rows - rh);
    const int fit = V::exl::rows_in_lds(rows, slots);
#else
    const int slots = exl::lr_slots(0, D);
    const size_t lds = exact_lr_lds_bytes(rows, rh, slots);
    const bool ok = exact_lr_split_ok(rows, rows - rh, slots);
    const int fit = exact_lr_rows_in_lds(rows, slots);
#endif
    printf("\"slots\": %d, \"lds\": %zu, \"ok\": %d, \"rows_in_lds\": %d}", slots, lds, (int)ok, fit);
}

// per-stream bytes of the record paths and where the second array of a chunk starts
void records_case(int n, long long C, int chunk) {
    open_record("records");
    printf("\"case\": {\"n\": %d, \"C\": %lld, \"chunk\": %d}, ", n, C, chunk);
#ifdef KERNEL_PLAN_VERBATIM
    const size_t f32 = V::run_columns_rec_per_stream(n, C);
    const V::ExactRecOut x = V::run_columns_exact_records(n, C, chunk);
    const size_t q = x.q_per_stream, key = x.key_per_stream, per = x.per_stream, extra = x.extra, off = x.key_offset;
#else
    const size_t f32 = f32_record_bytes(n, C);
    const ExactRecords x = exact_record_bytes(n, C);
    const size_t q = x.q_per_stream, key = x.key_per_stream, per = x.per_stream, extra = kChunkPad, off = second_array_offset(x.q_per_stream, chunk);
#endif
    printf("\"f32_per_stream\": %zu, \"q_per_stream\": %zu, \"key_per_stream\": %zu, \"per_stream\": %zu, \"extra\": %zu, \"key_offset\": %zu}", f32, q, key, per, extra, off);
}

// the full-rate workspace of the time reduction: dB and / or index columns of a chunk
void reduce_case(long long C, int R, int db, int idx, int chunk) {
    open_record("reduce");
    printf("\"case\": {\"C\": %lld, \"R\": %d, \"db\": %d, \"idx\": %d, \"chunk\": %d}, ", C, R, db, idx, chunk);
#ifdef KERNEL_PLAN_VERBATIM
    const V::ReduceOut o = V::reduce_streams(C, R, db != 0, idx != 0, chunk);
    const size_t per = o.per_stream, extra = o.extra, off = o.idx_offset, db_s = db ? (size_t)C * R * 4 : 0;
#else
    const size_t cells = (size_t)C * R, db_s = db ? cells * 4 : 0, per = db_s + (idx ? cells : 0), extra = kChunkPad, off = second_array_offset(db_s, chunk);
#endif
    printf("\"db_per_stream\": %zu, \"per_stream\": %zu, \"extra\": %zu, \"idx_offset\": %zu}", db_s, per, extra, off);
}

void dump_case(long long S, long long L, long long nframes, int n, int exact) {
    const size_t nb = (size_t)S * nframes * (n / 2 + 1), b_pcm = (size_t)S * L * sizeof(float);
    open_record("dump");
    printf("\"case\": {\"S\": %lld, \"L\": %lld, \"nframes\": %lld, \"n\": %d, \"exact\": %d}, \"b_pcm\": %zu, \"nb\": %zu, ", S, L, nframes, n, exact, b_pcm, nb);
#ifdef KERNEL_PLAN_VERBATIM
    const V::DumpOut o = exact ? V::emspec_parity_dump_exact(b_pcm, nb) : V::emspec_parity_dump(b_pcm, nb);
#else
    const DumpStage o = dump_stage(b_pcm, nb, exact != 0);
#endif
    printf("\"pcm\": %zu, \"power\": %zu, ", o.pcm, o.power);
    if (exact) printf("\"q\": %zu, ", o.q);
    printf("\"col\": %zu, \"row\": %zu, \"bytes\": %zu}", o.col, o.row, o.bytes);
}

// grow_chunked: the chunk and the bytes of every allocation it would try if each one failed (budget_mb: -1, or
// EMSPEC_RECORD_BUDGET_MB)
void chunk_case(size_t free_b, size_t have, size_t per_stream, size_t extra, size_t cap, int S, long long budget_mb) {
    open_record("chunk");
    printf("\"case\": {\"free\": %zu, \"have\": %zu, \"per_stream\": %zu, \"extra\": %zu, \"cap\": %zu, \"S\": %d, \"budget_mb\": %lld}, \"tries\": [",
           free_b, have, per_stream, extra, cap, S, budget_mb);
#ifdef KERNEL_PLAN_VERBATIM
    const std::string ev = std::to_string(budget_mb);
    const std::vector<V::ChunkTry> tries = V::grow_chunked(free_b, have, per_stream, extra, cap, S, budget_mb >= 0 ? ev.c_str() : nullptr);
    for (size_t i = 0; i < tries.size(); ++i) printf("%s[%d, %zu]", i ? ", " : "", tries[i].chunk, tries[i].bytes);
#else
    for (ChunkPlan p = first_chunk(free_b, have, per_stream, extra, cap, S, budget_mb);; p = next_chunk(p, per_stream, extra)) {
        printf("[%d, %zu]", p.chunk, p.bytes);
        if (p.chunk == 1) break;
        printf(", ");
    }
#endif
    printf("]}");
}

}  // namespace

int main() {
    // (no cross product: each axis is swept where it decides something, with the others at a value that lets it)
    const int sizes[7] = {256, 512, 1024, 2048, 4096, 8192, 16384};
    const int row_list[6] = {64, 512, 1024, 1028, 2048, 4096};

    // ---- FAST ----
    // every size at hop 1, the built hops and n, rows 1024, reassignment on and off; rows 64 / 1028 / 4096 at hop 512
    for (int n : sizes)
        for (int hop : {1, 256, 512, 1024, n})
            for (int re : {1, 0}) {
                if (hop > n) continue;
                fast_case(n, hop, 1024, re, 0);
                if (hop == 512 && re) for (int rows : {64, 1028, 4096, 62, 66}) fast_case(n, hop, rows, re, 0);
            }
    // fused_small: each side of the hop at which the ring stops fitting (rows 1024), and of the rows at which it does (hop 200,
    // hop 60, hop 40)
    for (int hop : {226, 227, 228, 229, 255, 257}) fast_case(4096, hop, 1024, 1, 0);
    for (int hop : {126, 127, 128, 129}) fast_case(2048, hop, 1024, 1, 0);
    for (int hop : {84, 85, 86, 87}) fast_case(1024, hop, 1024, 1, 0);
    for (int rows : {64, 928, 932, 936, 1024, 1028}) fast_case(4096, 200, rows, 1, 0);
    for (int rows : {64, 564, 568, 572, 576, 1024}) fast_case(2048, 60, rows, 1, 0);
    for (int rows : {64, 660, 664, 668, 672, 1024}) fast_case(1024, 40, rows, 1, 0);
    for (int hop : {1, 2, 227}) fast_case(4096, hop, 1024, 0, 0);   // reassignment off: no reach, every hop fits
    // N = 16384: the register park's hop at rows 1024 and its rows at hop 256 and 300
    for (int hop : {510, 511, 513, 2048}) fast_case(16384, hop, 1024, 1, 0);
    for (int rows : {64, 512, 516, 520, 524}) fast_case(16384, 256, rows, 1, 0);
    for (int rows : {600, 604, 608, 612, 616}) fast_case(16384, 300, rows, 1, 0);
    // the diagnostic switch
    for (int n : {1024, 4096, 8192, 16384})
        for (int hop : {256, 512, 300}) fast_case(n, hop, 1024, 1, 1);
    // a plan whose reach is not the shape's
    for (int D : {0, 8, 9}) { fast_reach_case(4096, 256, 1024, D); fast_reach_case(4096, 300, 1024, D); }
    for (int D : {4, 5}) { fast_reach_case(4096, 512, 1024, D); fast_reach_case(8192, 1024, 1024, D); }
    for (int D : {8, 9, 16, 17}) { fast_reach_case(8192, 512, 1024, D); fast_reach_case(16384, 512, 1024, D); }

    // ---- frames_kernel: every size, the rows of the list and the rows at which N = 16384 stops fitting ----
    for (int l = 8; l <= 14; ++l)
        for (int rows : row_list) frames_case(l, rows);
    for (int rows : {4096, 5880, 5884, 5888, 5892, 5896, 5900, 5904}) frames_case(14, rows);

    // ---- the EXACT frame kernels ----
    for (int n : sizes)
        for (int rows : row_list) exact_frames_case(n, rows, 2, 40, 1);
    for (int rows : {1024, 1032, 1036, 1040, 1044}) { exact_frames_case(4096, rows, 2, 40, 1); exact_frames_case(4096, rows, 2, 40, 0); }   // the 80 KB rule
    for (long long nf : {31, 32, 33}) exact_frames_case(4096, 1024, 2, nf, 1);                                               // S * nframes >= 64
    exact_frames_case(4096, 1024, 1, 64, 1);
    exact_frames_case(4096, 1024, 1, 63, 1);
    for (int rows : {2928, 2932, 2936, 2940}) exact_frames_case(16384, rows, 2, 40, 1);   // the edges leave LDS
    for (int rows : {2944, 2952, 3068, 3072, 4096}) exact_frames_case(8192, rows, 2, 40, 1);

    // ---- the EXACT route ----
    // every size at the built hops, hop 1 and n, rows 64 / 1024 / 1028 / 4096, reassignment on and off, the log axis
    for (int n : sizes)
        for (int hop : {1, 256, 512, 1024, n})
            for (int rows : {64, 1024, 1028, 4096}) {
                if (hop > n || (rows != 1024 && hop != 256)) continue;
                exact_case(n, hop, 1, rows, 0, rows, 0, 0, 0);
                if (rows == 1024) exact_case(n, hop, 0, rows, 0, rows, 0, 0, 0);
            }
    // the three axes on either side of the hop and of the rows at which the parked kernel stops fitting, and the switches
    for (int axis : {0, 1, 2}) {
        for (int hop : {227, 228, 254, 255, 256, 257}) exact_case(4096, hop, 1, 1024, 0, 1024, axis, 0, 0);
        for (int rows : {936, 940, 944, 948}) exact_case(4096, 255, 1, rows, 0, rows, axis, 0, 0);
        for (int n : {1024, 2048, 4096, 8192}) {
            exact_case(n, 256, 1, 1024, 0, 1024, axis, 1, 0);
            exact_case(n, 256, 1, 1024, 0, 1024, axis, 0, 1);
            exact_case(n, 256, 1, 1024, 0, 1024, axis, 1, 1);
        }
        // the rows at which the no-parking kernel's ring stops fitting whole (rl = 0 below)
        for (int rows = 584; rows <= 632; rows += 4) exact_case(4096, 256, 1, rows, 0, rows, axis, 0, 0);
        for (int n : {2048, 1024}) for (int rows : {64, 512, 600, 640, 1024}) exact_case(n, 128, 1, rows, 0, rows, axis, 0, 0);
    }
    // band plans of a 2048-row table: the Hz test is on row row0 + rl
    for (int row0 : {0, 64, 512, 1024})
        for (int axis : {0, 2}) {
            exact_case(4096, 256, 1, 1024, row0, 2048, axis, 0, 0);
            exact_case(4096, 256, 1, 512, row0, 2048, axis, 0, 0);
        }
    // a long reach: D = 1024 and past it
    for (int hop : {1, 2, 3}) { exact_case(4096, hop, 1, 64, 0, 64, 0, 0, 0); exact_case(1024, hop, 1, 64, 0, 64, 0, 0, 0); }
    // the row split of the no-parking kernel at rows 1024 around what fits
    for (int D : {8, 9, 16}) for (int rh : {568, 576, 584, 592, 1024, 0}) exact_lr_split_case(1024, D, rh);
    exact_lr_split_case(1024, 8, 578);
    exact_lr_split_case(64, 8, 64);

    // ---- record workspaces ----
    for (int n : sizes)
        for (long long C : {1, 700, 16369}) records_case(n, C, C == 700 ? 5 : 1);
    records_case(16384, 8388593, 3);
    records_case(16384, 31, 64);
    for (int db : {0, 1}) for (int idx : {0, 1}) { reduce_case(701, 1024, db, idx, 3); reduce_case(15, 68, db, idx, 7); }
    for (int exact : {0, 1}) {
        dump_case(2, 10240, 24, 4096, exact);
        dump_case(1, 256, 1, 256, exact);
        dump_case(3, 16384 + 511 * 7, 7, 16384, exact);
        dump_case(65535, 4097, 1, 4096, exact);
    }
    // the budget rule: free memory below the 256 MiB floor, between the floor and the cap, above the cap; one stream larger than the
    // budget; S % chunk != 0; what the engine already holds counts; the diagnostic override; a failing device query (free = 4 cap)
    const size_t MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;
    const size_t per = 16369 * (size_t)8196 * 12;   // EXACT records of 16,369 columns at N = 16384: 1.5 GiB
    for (size_t free_b : {(size_t)0, 100 * MiB, 1023 * MiB, 1025 * MiB, 8 * GiB, 31 * GiB, 33 * GiB, 200 * GiB}) {
        chunk_case(free_b, 0, per, 256, 8 * GiB, 16, -1);
        chunk_case(free_b, 0, 3 * MiB + 12345, 0, 4 * GiB, 1000, -1);
    }
    chunk_case(100 * MiB, 4 * GiB, 3 * MiB + 12345, 0, 4 * GiB, 1000, -1);   // what the engine holds counts
    chunk_case(200 * GiB, 0, per, 256, 8 * GiB, 3, -1);         // more budget than streams
    chunk_case(200 * GiB, 0, 9 * GiB, 256, 8 * GiB, 7, -1);     // one stream larger than the budget
    chunk_case(200 * GiB, 0, 700 * MiB, 1024, 4 * GiB, 7, -1);  // chunk 5 of 7 streams
    chunk_case(4 * (4 * GiB), 0, per, 0, 4 * GiB, 16, -1);
    for (long long mb : {0, 1, 64, 3000, 100000}) chunk_case(200 * GiB, 0, 20 * MiB, 256, 8 * GiB, 64, mb);

    // ---- row counts that are no power of two: the cases of tests/row_grid_cases.py (appended, so that every earlier record keeps
    // its line).  17, 25, 129, 250 and 255 quads; the records-only rows above the ring gate; every column kernel of either mode ----
    const int sweep[5] = {68, 100, 516, 1000, 1020};
    const int fast_shapes[12][2] = {{4096, 256}, {4096, 512}, {4096, 1024}, {4096, 300}, {2048, 128}, {1024, 256}, {1024, 100},
                                    {8192, 512}, {8192, 1024}, {16384, 512}, {8192, 256}, {512, 64}};
    for (const auto& s : fast_shapes) {
        for (int rows : sweep) fast_case(s[0], s[1], rows, 1, 0);
        fast_case(s[0], s[1], 1000, 0, 0);
    }
    for (int rows : {2052, 4092}) { fast_case(4096, 256, rows, 1, 0); fast_case(16384, 512, rows, 1, 0); }
    const int exact_shapes[6][2] = {{4096, 256}, {4096, 300}, {2048, 128}, {1024, 256}, {8192, 512}, {16384, 512}};
    for (const auto& s : exact_shapes)
        for (int rows : sweep) exact_case(s[0], s[1], 1, rows, 0, rows, 0, 0, 0);
    for (int rows : sweep) exact_case(4096, 256, 1, rows, 0, rows, 2, 0, 0);
    for (int rows : {2052, 4092}) exact_case(4096, 256, 1, rows, 0, rows, 0, 0, 0);
    for (int rows : {68, 1020}) exact_case(4096, 256, 1, rows, 0, rows, 2, 1, 0);   // the parked kernel where the switch asks for it

    // ---- other sample rates and log axes: the cases of tests/axis_cases.py (appended).  The FAST route does not look at the axis:
    // only the shapes that have no record at 1024 rows yet.  The EXACT route does, through the low-share rule ----
    fast_case(4096, 300, 1024, 1, 0);
    const float axes[6][3] = {{44100.0f, 20.0f, 22050.0f}, {8000.0f, 30.0f, 4000.0f}, {32000.0f, 55.0f, 16000.0f},
                              {96000.0f, 20.0f, 20000.0f}, {192000.0f, 10.0f, 96000.0f}, {48000.0f, 2000.0f, 4000.0f}};
    const int axis_shapes[5][2] = {{4096, 256}, {2048, 128}, {1024, 256}, {8192, 512}, {16384, 512}};
    for (const auto& a : axes) {
        for (const auto& s : axis_shapes)
            for (int rows : {1024, 68}) exact_case(s[0], s[1], 1, rows, 0, rows, 0, 0, 0, a);
        exact_case(4096, 256, 1, 4092, 0, 4092, 0, 0, 0, a);
    }
    printf("\n]\n");
    return 0;
}
