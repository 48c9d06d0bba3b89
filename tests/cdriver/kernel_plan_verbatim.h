// kernel_plan_verbatim.h — the kernel choice, the LDS budgets and the record workspaces as they stood beside the kernels and in
// emspec_api.cpp before em-spec_amd/csrc/emspec_kernel_plan.h took them over: the statements unchanged, the getenv switches and
// the device's free bytes as arguments, each launcher cut down to what it decided.  Never included by the library;
// tests/cdriver/kernel_plan_driver.cpp built with -DKERNEL_PLAN_VERBATIM wrote tests/golden/kernel_plans.json from it, once.
// (latency, Axis and low_share_ok of emspec_tables.h and al of emspec_wire_plan.h were where they are: used from there.)
#pragma once
#include "emspec_tables.h"
#include "emspec_wire_plan.h"
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace emspec_verbatim {
using emspec::al;
using emspec::Axis;
using emspec::latency;
using emspec::low_share_ok;
struct float2 { float x, y; };
struct double2 { double x, y; };
struct uint2 { unsigned x, y; };

// ---- emspec_device.h, kernels.hip ----
template <int N> struct PaddedSize { static constexpr int value = N + (N >> 4); };
constexpr int mid_tw_entries(int log2n) {
    int s0 = 4, n = 0;
    while (log2n - s0 > 4) { n += 15 << (log2n - s0 - 4); s0 += 4; }
    return (n + 1) & ~1;   // keep the next region 16-byte aligned
}
// launch_frames_t<LOG2N>: the size, and whether the launch is refused
struct FramesOut { size_t lds; bool invalid; };
template <int LOG2N>
FramesOut launch_frames_t(int rows) {
    constexpr int N = 1 << LOG2N;
    const size_t lds = (size_t)(PaddedSize<N>::value + mid_tw_entries(LOG2N)) * sizeof(float2) + (size_t)(rows + 1) * sizeof(float);
    if (lds > 160 * 1024) return FramesOut{lds, true};
    return FramesOut{lds, false};
}

// ---- fused_r8 / fused_pp / fused_small / fused_n8192 / fused_n16384 .hip.inc ----
namespace f8 { constexpr int LOG2N = 12, N = 4096, T = 512; }
namespace f13 { constexpr int N = 8192, M = 4096, T = 512; }
static size_t fused_r8_lds_bytes(int rows, int hop) {
    const int slots = 2 * (f8::N / (2 * hop)) + 2;
    return (size_t)2 * f8::N * sizeof(float2) + (size_t)slots * rows * 4 + (size_t)(rows + 4) * 4 + 1024 +
           (size_t)(7 * 64 + 7 * 8) * sizeof(float2);
}
static size_t fused_pp_lds_bytes(int rows, int hop) { return fused_r8_lds_bytes(rows, hop) + 16; }
static int fused_small_slots(int n, int D) { return 2 * D + 2 * (4096 / n); }   // n = 4096, 2048, 1024
static size_t fused_small_lds_bytes(int rows, int slots) {
    return (size_t)2 * 4096 * sizeof(float2) + (size_t)slots * rows * 4 + (size_t)(rows + 4) * 4 + 1024 +
           (size_t)(7 * 64 + 7 * 8) * sizeof(float2) + 16;   // + the two arrival counters of the product form
}
static size_t fused8192_lds_bytes(int rows, int hop) {
    const int slots = 2 * (f13::N / (2 * hop)) + 1;
    return (size_t)2 * f13::M * sizeof(float2) + (size_t)slots * rows * 4 + (size_t)(rows + 4) * 4 + 1024 +
           (size_t)(7 * 64 + 7 * 8) * sizeof(float2);
}
namespace f14 {
constexpr int LOG2N = 14, N = 16384, T = 1024;
constexpr int NQ = 8;    // 8 float4 per thread park the 32 x 1024 ring cells that share the transform's region
constexpr int FFT_BYTES = PaddedSize<N>::value * (int)sizeof(float2);
constexpr int PARKED_CELLS = NQ * 4 * 1024;
constexpr int RING_OFF = FFT_BYTES - PARKED_CELLS * 4;
constexpr int RES_BYTES = 4096;
static_assert(RING_OFF >= 0 && RING_OFF % 16 == 0, "ring offset");
}  // namespace f14
static bool fused16384_supported(int hop, int rows, int reassign) {
    if (hop < 1 || hop > f14::N) return false;
    if (rows % 4 || rows < 64 || rows > 1024) return false;
    const int D = reassign ? (f14::N + 2 * hop - 1) / (2 * hop) : 0;
    const int64_t cells = (int64_t)(2 * D + 1) * rows;
    return cells <= (int64_t)f14::PARKED_CELLS + f14::RES_BYTES / 4;
}
static size_t fused16384_lds_bytes(int rows) {
    return (size_t)f14::FFT_BYTES + f14::RES_BYTES + (size_t)mid_tw_entries(f14::LOG2N) * sizeof(float2) + (size_t)(rows + 4) * 4 + 1024;
}

// ---- fused.hip.inc (diag_no_fused(), fused_variant(): EMSPEC_NO_FUSED, EMSPEC_FUSED_VARIANT as arguments) ----
static bool fused_supported(int n, int hop, int rows, int reassign, bool diag_no_fused, int fused_variant) {
    if (diag_no_fused) return false;
    // the default (r8) kernel is built for hop 256, 512 and 1024 (the diagnostic A/B variants for hop 256 only);
    // N = 8192 (fused_n8192.hip.inc) for hop 512 and 1024; N = 16384 for any hop whose ring fits the register park
    const bool rows_ok = rows % 4 == 0 && rows >= 64 && rows <= 1024;
    if (n == f14::N) return fused_variant == 0 && fused16384_supported(hop, rows, reassign);
    if (n == f13::N) return fused_variant == 0 && (hop == 512 || hop == 1024) && rows_ok;
    const bool r8_hop = hop == 256 || ((fused_variant == 0 || fused_variant >= 3) && (hop == 512 || hop == 1024));
    if (n == f8::N && r8_hop) return rows_ok;
    if (n == 4096 || n == 2048 || n == 1024) {   // fused_small.hip.inc: any hop whose ring (2D + F column slots) fits in LDS
        const int D = reassign ? (n + 2 * hop - 1) / (2 * hop) : 0;
        return (fused_variant == 0 || fused_variant == 3) && rows_ok && hop >= 1 && hop <= n &&
               fused_small_lds_bytes(rows, fused_small_slots(n, D)) <= (size_t)160 * 1024;
    }
    return false;
}
enum class FusedKind { n4096_8192, small_n, big_n };
// launch_fused down to its choice: the family it launches (0 pp / r8, 1 small, 2 N = 8192, 3 N = 16384), the FusedKind it hands
// the segment plan, the dynamic LDS of the product kernel of that family and, for fused_small, the slots
struct FusedOut { bool not_supported; int family; FusedKind kind; size_t lds; int slots; };
static FusedOut launch_fused(int n, int pl_hop, int pl_rows, int pl_reassign, int pl_D, bool diag_no_fused, int fused_variant) {
    const bool big_n = n == f14::N;
    const bool r8_shape = n == f8::N && (pl_hop == 256 || pl_hop == 512 || pl_hop == 1024);
    const bool small_n = (n == 4096 || n == 2048 || n == 1024) && !r8_shape;   // fused_small: ring sized from pl.D at run time
    if (!fused_supported(n, pl_hop, pl_rows, pl_reassign, diag_no_fused, fused_variant) || (!small_n && !big_n && pl_D > n / (2 * pl_hop)))
        return FusedOut{true, -1, FusedKind::n4096_8192, 0, 0};
    const FusedKind kind = small_n ? FusedKind::small_n : (big_n ? FusedKind::big_n : FusedKind::n4096_8192);
    if (big_n) return FusedOut{false, 3, kind, fused16384_lds_bytes(pl_rows), 0};
    if (small_n) {
        const int slots = fused_small_slots(n, pl_D);
        return FusedOut{false, 1, kind, fused_small_lds_bytes(pl_rows, slots), slots};
    }
    if (n == f13::N) return FusedOut{false, 2, kind, fused8192_lds_bytes(pl_rows, pl_hop), 0};
    return FusedOut{false, 0, kind, fused_pp_lds_bytes(pl_rows, pl_hop), 0};
}

// ---- exact.hip.inc ----
namespace ex {
constexpr int rec_stride(int n) { return n / 2 + 4; }   // records per frame: K = n/2+1 bins + 3 pads (16-byte chunks of 4)
}
struct ExactSinks { int edges_lds = 1; };
// LDS of a frame kernel: its planes, and the binary64 row edges when they fit beside them (else read from global memory)
static size_t exact_frames_lds(size_t planes, int rows, ExactSinks& sk) {
    const size_t edges = (size_t)(rows + 1) * sizeof(double);
    sk.edges_lds = planes + edges <= 160 * 1024 ? 1 : 0;
    return planes + (sk.edges_lds ? edges : 0);
}
// form: 0 the generic kernel, 1 the persistent N = 4096 kernel, 2 N = 16384
struct ExactFramesOut { int form; size_t lds; int edges_lds; bool invalid; };
template <int LOG2N>
static ExactFramesOut launch_exact_frames_t(int rows) {
    constexpr int N = 1 << LOG2N;
    ExactSinks sk2;
    const size_t lds = exact_frames_lds((size_t)2 * PaddedSize<N>::value * sizeof(double), rows, sk2);
    if (lds > 160 * 1024) return ExactFramesOut{0, lds, sk2.edges_lds, true};
    return ExactFramesOut{0, lds, sk2.edges_lds, false};
}
// (dump_only || rec_only: the sinks of the launch - a batch's records or a parity dump)
static ExactFramesOut launch_exact_frames(int n, int rows, int S, int64_t nframes, bool dump_or_rec_only) {
    if (n == 4096) {
        // the persistent kernel when its 80 KB fit twice per CU (rows <= 1024) and the launch is a batch
        const size_t lds = (size_t)2 * 4096 * 8 + (size_t)(7 * 64 + 7 * 8) * 16 + (size_t)(rows + 1) * 8;
        if (lds <= 80 * 1024 && S * nframes >= 64 && dump_or_rec_only) return ExactFramesOut{1, lds, 1, false};
    }
    if (n == 16384) {
        ExactSinks sk2;
        const size_t planes = (size_t)2 * 8192 * sizeof(double) + (size_t)4 * (128 + 16 + 2) * sizeof(double2);   // swizzled, unpadded
        const size_t lds = exact_frames_lds(planes, rows, sk2);
        return ExactFramesOut{2, lds, sk2.edges_lds, false};
    }
    switch (n) {
    case 256: return launch_exact_frames_t<8>(rows);
    case 512: return launch_exact_frames_t<9>(rows);
    case 1024: return launch_exact_frames_t<10>(rows);
    case 2048: return launch_exact_frames_t<11>(rows);
    case 4096: return launch_exact_frames_t<12>(rows);
    default: return launch_exact_frames_t<13>(rows);
    }
}

// ---- exact_fused.hip.inc (diag_exact_records(): EMSPEC_EXACT_RECORDS as an argument) ----
namespace exf {
constexpr int LOG2N = 12, N = 4096, T = 512;
inline int region_cells(int rows, int slots) { return slots * rows > 2 * N ? slots * rows : 2 * N; }
inline int edge_cells(int rows) { return (rows + 2) & ~1; }
static int exact_fused_slots(int D) { return 2 * D + 2 > 3 ? 2 * D + 2 : 3; }
static size_t exact_fused_lds_bytes(int rows, int slots) {
    return ((size_t)region_cells(rows, slots) + (size_t)edge_cells(rows)) * 8 + (size_t)(4 * 64 + 4 * 8) * 16 + 1024 + 32;
}
}  // namespace exf
static bool exact_fused_supported(int n, int pl_rows, int pl_D, bool diag_exact_records) {
    if (diag_exact_records) return false;
    if (n != exf::N || pl_rows % 4 || pl_rows < 64 || pl_rows > 1024 || pl_D < 0 || pl_D > 1024) return false;
    return exf::exact_fused_lds_bytes(pl_rows, exf::exact_fused_slots(pl_D)) <= (size_t)160 * 1024;
}

// ---- exact_fused_lr.hip.inc ----
namespace exl {
constexpr int LOG2N = 12, N = 4096, T = 512;
using exf::edge_cells;
inline int lr_slots(int S, int D) { return S == 0 ? (2 * D + 2 > 3 ? 2 * D + 2 : 3) : 2 * D + (2 << S); }
// LDS budget: planes + ring + edges + pass twiddles + LUT + counters
inline int ring_cells(int rh, int slots) { return slots * rh > 1024 ? slots * rh : 1024; }
// (+ one bit per low-row cell, [slots][mask_words]: which cells of the global scratch took an add - only those are swapped out)
inline int mask_words(int rl) { return (rl + 31) >> 5; }
static size_t lds_bytes(int rows, int rh, int slots) {
    return ((size_t)2 * N + (size_t)ring_cells(rh, slots) + (size_t)edge_cells(rows)) * 8 + (size_t)(4 * 64 + 4 * 8) * 16 + 1024 + 32 +
           (size_t)slots * mask_words(rows - rh) * 4;
}
// How many of the R rows stay in LDS beside the planes (a multiple of 8; R when the whole ring fits)
static int rows_in_lds(int rows, int slots) {
    const size_t fixed = lds_bytes(rows, 0, slots) - (size_t)ring_cells(0, slots) * 8;
    const size_t avail = (size_t)160 * 1024 > fixed ? (size_t)160 * 1024 - fixed : 0;
    int rh = (int)(avail / ((size_t)slots * 8));
    rh = rh > rows ? rows : (rh & ~7);
    while (rh > 0 && lds_bytes(rows, rh, slots) > (size_t)160 * 1024) rh -= 8;
    return rh < 0 ? 0 : rh;
}
}  // namespace exl
static int exact_lr_skip(int n) { return n == 4096 ? 0 : (n == 2048 ? 1 : (n == 1024 ? 2 : -1)); }   // the kernel's S
static int exact_fused_lr_low_rows(int n, int pl_rows, int pl_D, bool diag_exact_records) {
    if (diag_exact_records) return -1;
    const int sk = exact_lr_skip(n);
    if (sk < 0 || pl_rows % 4 || pl_rows < 64 || pl_rows > 1024 || pl_D < 0 || pl_D > 1024) return -1;
    const int slots = exl::lr_slots(sk, pl_D);
    const int rh = exl::rows_in_lds(pl_rows, slots);
    const int rl = pl_rows - rh;
    if (rh < 8 || (rl & 3)) return -1;
    return rl;
}
// launch_exact_fused_lr's check of the rl it is handed
static bool launch_exact_fused_lr_invalid(int n, int pl_rows, int pl_D, int rl) {
    const int slots = exl::lr_slots(exact_lr_skip(n), pl_D);
    const int rh = pl_rows - rl;
    if (rl < 0 || (rl & 3) || rh < 8 || exl::lds_bytes(pl_rows, rh, slots) > (size_t)160 * 1024) return true;
    return false;
}

// ---- emspec_api.cpp (EMSPEC_EXACT_PARKED's first character as an argument: 0 when unset) ----
static int exact_lr_rows(const Axis& axis, int n, int pd_rows, int pd_D, int row0, char exact_parked, bool diag_exact_records) {
    if (exact_parked) { if (exact_parked == '1') return -1; }   // A/B aid: round 4's kernel
    const int rl = exact_fused_lr_low_rows(n, pd_rows, pd_D, diag_exact_records);
    if (rl <= 0) return rl;
    return low_share_ok(axis, row0 + rl) ? rl : -1;
}
// emspec_uses_fused, EXACT engines (cfg_rows: the engine's rows)
static int emspec_uses_fused_exact(const Axis& axis, int n, int hop, int reassign, int cfg_rows, char exact_parked, bool diag_exact_records) {
    if (n < 1 || hop < 1) return 0;
    const int pd_rows = cfg_rows;
    const int pd_D = latency(n, hop, reassign);
    return (exact_lr_rows(axis, n, pd_rows, pd_D, 0, exact_parked, diag_exact_records) >= 0 || exact_fused_supported(n, pd_rows, pd_D, diag_exact_records)) ? 1 : 0;
}
// run_columns_exact's ladder (emspec_debug_phase_cycles ran the same one): 0 the no-parking kernel with rl, 1 the parking kernel,
// 2 records
struct ExactLadder { int step; int rl; };
static ExactLadder run_columns_exact(const Axis& axis, int n, int pd_rows, int pd_D, int row0, char exact_parked, bool diag_exact_records) {
    const int rl = exact_lr_rows(axis, n, pd_rows, pd_D, row0, exact_parked, diag_exact_records);
    if (rl >= 0) return ExactLadder{0, rl};
    if (exact_fused_supported(n, pd_rows, pd_D, diag_exact_records)) return ExactLadder{1, 0};
    return ExactLadder{2, 0};
}

// record workspaces: run_columns, run_columns_exact, reduce_streams
static size_t run_columns_rec_per_stream(int n, int64_t C) {
    const size_t rec_per_stream = (size_t)C * (n / 2 + 2) * sizeof(uint2);   // frame stride K+1 (even)
    return rec_per_stream;
}
struct ExactRecOut { size_t q_per_stream, key_per_stream, per_stream, extra, key_offset; };
static ExactRecOut run_columns_exact_records(int n, int64_t C, int chunk) {
    const size_t Kp = (size_t)ex::rec_stride(n);
    const size_t q_per_stream = (size_t)C * Kp * sizeof(long long), key_per_stream = (size_t)C * Kp * sizeof(uint32_t);
    return ExactRecOut{q_per_stream, key_per_stream, q_per_stream + key_per_stream, 256, ((q_per_stream * chunk + 255) & ~(size_t)255)};
}
struct ReduceOut { size_t per_stream, extra, idx_offset; };
static ReduceOut reduce_streams(int64_t C, int R, bool db, bool index_or_rgba, int chunk) {
    const size_t cells = (size_t)C * R;
    const size_t db_s = db ? cells * 4 : 0, idx_s = index_or_rgba ? cells : 0;
    return ReduceOut{db_s + idx_s, 256, ((db_s * chunk + 255) & ~(size_t)255)};
}
// grow_chunked: the chunks it asks grow() for, in order, when every allocation fails (ev: EMSPEC_RECORD_BUDGET_MB or null)
struct ChunkTry { int chunk; size_t bytes; };
static std::vector<ChunkTry> grow_chunked(size_t free_b, size_t have, size_t per_stream, size_t extra, size_t cap, int S, const char* ev) {
    std::vector<ChunkTry> tries;
    size_t budget = (free_b + have) / 4;
    budget = budget < ((size_t)256 << 20) ? ((size_t)256 << 20) : (budget > cap ? cap : budget);
    if (ev) budget = (size_t)atol(ev) << 20;   // test hook: force several stream-chunks
    int chunk = (int)(budget / per_stream);
    chunk = chunk < 1 ? 1 : (chunk > S ? S : chunk);
    for (;;) {
        tries.push_back(ChunkTry{chunk, per_stream * (size_t)chunk + extra});
        if (chunk == 1) return tries;
        chunk = (chunk + 1) / 2;
    }
}
// staging of the two parity dumps
struct DumpOut { size_t bytes, pcm, power, q, col, row; };
static DumpOut emspec_parity_dump(size_t b_pcm, size_t nb) {
    DumpOut o{al(b_pcm) + 3 * al(nb * 4) + 256, 0, 0, 0, 0, 0};
    size_t base = 0;
    o.pcm = base; base += al(b_pcm);
    o.power = base; base += al(nb * 4);
    o.col = base; base += al(nb * 4);
    o.row = base;
    return o;
}
static DumpOut emspec_parity_dump_exact(size_t b_pcm, size_t nb) {
    DumpOut o{al(b_pcm) + 2 * al(nb * 8) + 2 * al(nb * 4) + 256, 0, 0, 0, 0, 0};
    size_t base = 0;
    o.pcm = base; base += al(b_pcm);
    o.power = base; base += al(nb * 8);
    o.q = base; base += al(nb * 8);
    o.col = base; base += al(nb * 4);
    o.row = base;
    return o;
}

}  // namespace emspec_verbatim
