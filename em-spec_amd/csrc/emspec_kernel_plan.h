// emspec_kernel_plan.h — internal: which kernel serves a call and whether it fits in LDS (DESIGN.md "Kernel plan"): the LDS limit and
// the shape gates, the dynamic-LDS size of every product kernel, the route of a FAST and of an EXACT call, and the record
// workspaces of the shapes without a fused kernel (bytes per stream, sub-allocation offsets, the budget and chunk rule).  Host
// arithmetic only, and every input an argument: the launchers pass the device's free bytes and, in the diagnostic build, their
// getenv switches.  No HIP: tests/test_kernel_plan_cpu.py runs it through a stand-alone program
// (tests/cdriver/kernel_plan_driver.cpp) without a GPU and pins every answer to tests/golden/kernel_plans.json.
#pragma once
#include "emspec_tables.h"      // latency, Axis, low_share_ok
#include "emspec_wire_plan.h"   // al
#include <cstddef>
#include <cstdint>

// the few integer helpers below that a kernel's LDS carve-up and its host formula share
#ifdef __HIPCC__
#define EMSPEC_HD __host__ __device__
#else
#define EMSPEC_HD
#endif

namespace emspec {

constexpr size_t kLdsBytes = 160 * 1024;   // LDS of a CU: the most a workgroup's dynamic allocation may ask for
// the rows every kernel with a column ring in LDS serves (the records paths take any rows the engine accepts)
inline bool ring_rows_ok(int rows) { return rows % 4 == 0 && rows >= 64 && rows <= 1024; }
inline bool exact_reach_ok(int D) { return D >= 0 && D <= 1024; }

// ---- shared with the kernels: sizes of LDS regions ----
template <int N> struct PaddedSize { static constexpr int value = N + (N >> 4); };   // the in-place buffer: 1 pad slot per 16
constexpr int padded_size(int n) { return n + (n >> 4); }
// middle-pass twiddles of frames_kernel / fused16384_kernel: 15 << B0 entries per pass
constexpr int mid_tw_entries(int log2n) {
    int s0 = 4, n = 0;
    while (log2n - s0 > 4) { n += 15 << (log2n - s0 - 4); s0 += 4; }
    return (n + 1) & ~1;   // keep the next region 16-byte aligned
}
constexpr size_t kTw8Entries = 7 * 64 + 7 * 8;    // pass twiddles the radix-8 float32 kernels stage (float2)
constexpr size_t kTwXEntries = 4 * 64 + 4 * 8;    // ... and the EXACT fused kernels (double2)
namespace ex {
constexpr int rec_stride(int n) { return n / 2 + 4; }   // records per frame: K = n/2+1 bins + 3 pads (16-byte chunks of 4)
}
namespace f14 {   // fused16384_kernel (fused_n16384.hip.inc)
constexpr int LOG2N = 14, N = 16384, T = 1024;
constexpr int NQ = 8;    // 8 float4 per thread park the 32 x 1024 ring cells that share the transform's region
constexpr int FFT_BYTES = PaddedSize<N>::value * 8;   // float2
// The ring starts RING_OFF bytes into the region, so that exactly NQ * 4096 cells (128 KB) lie inside the padded
// transform buffer (136 KB) and the rest - up to 1024 cells, the 33rd slot at hop 512 - lies in RES_BYTES of its own
// right behind it: resident, never parked (it used to take a 33rd register and the only spill of the frame loop).
constexpr int PARKED_CELLS = NQ * 4 * 1024;
constexpr int RING_OFF = FFT_BYTES - PARKED_CELLS * 4;
constexpr int RES_BYTES = 4096;
static_assert(RING_OFF >= 0 && RING_OFF % 16 == 0, "ring offset");
}  // namespace f14
namespace exf {   // exact_fused4096_kernel (exact_fused.hip.inc): the ring parked under the two binary64 planes
EMSPEC_HD inline int region_cells(int rows, int slots) { return slots * rows > 2 * 4096 ? slots * rows : 2 * 4096; }
EMSPEC_HD inline int edge_cells(int rows) { return (rows + 2) & ~1; }
}  // namespace exf
namespace exl {   // exact_fused4096_lr_kernel (exact_fused_lr.hip.inc): rows >= rl of the ring beside the planes
// ring slots: 2 D + 2 FPT columns are live at once (at half-iteration k the F team scatters block k - 2 and takes the FPT
// columns of block k - 3, shifted by D, out)
EMSPEC_HD inline int lr_slots(int S, int D) { return S == 0 ? (2 * D + 2 > 3 ? 2 * D + 2 : 3) : 2 * D + (2 << S); }
EMSPEC_HD inline int ring_cells(int rh, int slots) { return slots * rh > 1024 ? slots * rh : 1024; }
// (+ one bit per low-row cell, [slots][mask_words]: which cells of the global scratch took an add - only those are swapped out)
EMSPEC_HD inline int mask_words(int rl) { return (rl + 31) >> 5; }
}  // namespace exl

// ---- ring slots ----
// The N = 4096 family at hop 256 / 512 / 1024 and N = 8192 size their ring at compile time for the hop's full reach (Geo<HOP>)
inline int fused_pp_slots(int hop) { return 2 * latency(4096, hop, 1) + 2; }
inline int fused8192_slots(int hop) { return 2 * latency(8192, hop, 1) + 1; }
inline int fused_small_slots(int n, int D) { return 2 * D + 2 * (4096 / n); }   // n = 4096, 2048, 1024
// N = 16384: 2D + 1 slots of `rows` cells, as many as the register park and the resident slot hold
inline bool fused16384_ring_fits(int rows, int D) { return (int64_t)(2 * D + 1) * rows <= (int64_t)f14::PARKED_CELLS + f14::RES_BYTES / 4; }
inline int exact_fused_slots(int D) { return 2 * D + 2 > 3 ? 2 * D + 2 : 3; }
inline int exact_lr_skip(int n) { return n == 4096 ? 0 : (n == 2048 ? 1 : (n == 1024 ? 2 : -1)); }   // the no-parking kernel's S

// ---- dynamic LDS of every product kernel ----
inline size_t frames_lds_bytes(int log2n, int rows) {
    return (size_t)(padded_size(1 << log2n) + mid_tw_entries(log2n)) * 8 + (size_t)(rows + 1) * 4;
}
// two 4096-point float2 images, the ring, the row edges, the palette, the pass twiddles
inline size_t fused_ring_lds_bytes(int rows, int slots) {
    return (size_t)2 * 4096 * 8 + (size_t)slots * rows * 4 + (size_t)(rows + 4) * 4 + 1024 + kTw8Entries * 8;
}
inline size_t fused_pp_lds_bytes(int rows, int hop) { return fused_ring_lds_bytes(rows, fused_pp_slots(hop)) + 16; }   // + the two arrival counters
inline size_t fused_small_lds_bytes(int rows, int slots) { return fused_ring_lds_bytes(rows, slots) + 16; }
inline size_t fused8192_lds_bytes(int rows, int hop) { return fused_ring_lds_bytes(rows, fused8192_slots(hop)); }
inline size_t fused16384_lds_bytes(int rows) {
    return (size_t)f14::FFT_BYTES + f14::RES_BYTES + (size_t)mid_tw_entries(f14::LOG2N) * 8 + (size_t)(rows + 4) * 4 + 1024;
}
// EXACT frame kernels: the planes, and the binary64 row edges when they fit beside them (else read from global memory)
struct ExactFramesLds { size_t bytes; int edges_lds; };
inline ExactFramesLds exact_frames_lds(size_t planes, int rows) {
    const size_t edges = (size_t)(rows + 1) * 8;
    const int in_lds = planes + edges <= kLdsBytes ? 1 : 0;
    return ExactFramesLds{planes + (in_lds ? edges : 0), in_lds};
}
inline size_t exact_frames_planes(int n) {   // generic: two padded planes; N = 16384: swizzled, unpadded, + its pass twiddles
    return n == 16384 ? (size_t)2 * 8192 * 8 + (size_t)4 * (128 + 16 + 2) * 16 : (size_t)2 * padded_size(n) * 8;
}
inline size_t exact_frames4096_lds_bytes(int rows) { return (size_t)2 * 4096 * 8 + kTw8Entries * 16 + (size_t)(rows + 1) * 8; }
// the persistent N = 4096 kernel: when its LDS fits twice per CU (rows <= 1024) and the launch is a batch
inline bool exact_frames4096_persistent(int rows, int S, int64_t nframes) {
    return exact_frames4096_lds_bytes(rows) <= 80 * 1024 && S * nframes >= 64;
}
inline size_t exact_fused_lds_bytes(int rows, int slots) {
    return ((size_t)exf::region_cells(rows, slots) + (size_t)exf::edge_cells(rows)) * 8 + kTwXEntries * 16 + 1024 + 32;
}
// planes + ring + edges + pass twiddles + LUT + counters + the low rows' mask
inline size_t exact_lr_lds_bytes(int rows, int rh, int slots) {
    return ((size_t)2 * 4096 + (size_t)exl::ring_cells(rh, slots) + (size_t)exf::edge_cells(rows)) * 8 + kTwXEntries * 16 + 1024 + 32 +
           (size_t)slots * exl::mask_words(rows - rh) * 4;
}
// How many of the R rows stay in LDS beside the planes (a multiple of 8; R when the whole ring fits)
inline int exact_lr_rows_in_lds(int rows, int slots) {
    const size_t fixed = exact_lr_lds_bytes(rows, 0, slots) - (size_t)exl::ring_cells(0, slots) * 8;
    const size_t avail = kLdsBytes > fixed ? kLdsBytes - fixed : 0;
    int rh = (int)(avail / ((size_t)slots * 8));
    rh = rh > rows ? rows : (rh & ~7);
    while (rh > 0 && exact_lr_lds_bytes(rows, rh, slots) > kLdsBytes) rh -= 8;
    return rh < 0 ? 0 : rh;
}
// what launch_exact_fused_lr asks of the rl it is handed
inline bool exact_lr_split_ok(int rows, int rl, int slots) {
    return rl >= 0 && !(rl & 3) && rows - rl >= 8 && exact_lr_lds_bytes(rows, rows - rl, slots) <= kLdsBytes;
}

// ---- the route: the kernel family that serves a call ----
enum class RouteKind { fused_pp, fused_small, fused_8192, fused_16384, records_f32, exact_lr, exact_parked, exact_records };
struct Route { RouteKind kind; int rl; };   // rl: exact_lr's rows per slot in the global scratch (0: the whole ring in LDS)
inline bool is_records(Route r) { return r.kind == RouteKind::records_f32 || r.kind == RouteKind::exact_records; }
// the diagnostic build's switches (the product: all off)
struct FastSwitches { bool no_fused = false; };                        // EMSPEC_NO_FUSED
struct ExactSwitches { bool parked = false; bool records = false; };   // EMSPEC_EXACT_PARKED, EMSPEC_EXACT_RECORDS

// FAST: the N = 4096 family is built for hop 256, 512 and 1024, N = 8192
// for hop 512 and 1024, N = 16384 for any hop whose ring fits the register park, fused_small for N = 4096 / 2048 / 1024 at any
// hop whose ring (2D + F column slots) fits in LDS; everything else goes through per-bin records.
inline Route fast_route(int n, int hop, int rows, int reassign, FastSwitches sw = {}) {
    const Route records{RouteKind::records_f32, 0};
    auto serves = [&](bool yes, RouteKind k) { return yes ? Route{k, 0} : records; };
    if (sw.no_fused) return records;
    const int D = latency(n, hop < 1 ? 1 : hop, reassign);
    if (n == 16384) return serves(hop >= 1 && hop <= n && ring_rows_ok(rows) && fused16384_ring_fits(rows, D), RouteKind::fused_16384);
    if (n == 8192) return serves((hop == 512 || hop == 1024) && ring_rows_ok(rows), RouteKind::fused_8192);
    if (n == 4096 && (hop == 256 || hop == 512 || hop == 1024)) return serves(ring_rows_ok(rows), RouteKind::fused_pp);
    if (n == 4096 || n == 2048 || n == 1024)
        return serves(ring_rows_ok(rows) && hop >= 1 && hop <= n &&
                          fused_small_lds_bytes(rows, fused_small_slots(n, D)) <= kLdsBytes, RouteKind::fused_small);
    return records;
}
// (fused_small and N = 16384 size their ring from the plan's D at run time; the others are built for the hop's own reach)
inline bool fused_reach_ok(RouteKind k, int n, int hop, int D) {
    return !(k == RouteKind::fused_pp || k == RouteKind::fused_8192) || D <= latency(n, hop, 1);
}

// EXACT.  The no-parking kernel serves N = 4096 / 2048 / 1024 with rl low rows of every slot in a global scratch; each bin that
// lands below row rl costs a device-scope atomic instead of an LDS one, so an AXIS is served when at most 6 % of a frame's bins
// lie below it (on the default log axis at hop 256: rl = 456 of 1024 rows, about 40 of 2,049 bins; a linear axis has 44 % there).
// exact_lr_low_rows: rl for the shape, or -1.  row0: the plan's first row in the engine's table (a band plan of the
// multi-resolution batch; the Hz test is on its row rl).  Then the kernel that parks the ring under the planes (N = 4096, any
// axis), then per-bin records.
inline int exact_lr_low_rows(int n, int rows, int D) {
    const int sk = exact_lr_skip(n);
    if (sk < 0 || !ring_rows_ok(rows) || !exact_reach_ok(D)) return -1;
    const int rh = exact_lr_rows_in_lds(rows, exl::lr_slots(sk, D)), rl = rows - rh;
    return (rh < 8 || (rl & 3)) ? -1 : rl;
}
inline bool exact_parked_fits(int n, int rows, int D) {
    return n == 4096 && ring_rows_ok(rows) && exact_reach_ok(D) && exact_fused_lds_bytes(rows, exact_fused_slots(D)) <= kLdsBytes;
}
inline Route exact_route(int n, int rows, int D, int row0, const Axis& axis, ExactSwitches sw = {}) {
    if (sw.records) return Route{RouteKind::exact_records, 0};
    const int rl = sw.parked ? -1 : exact_lr_low_rows(n, rows, D);
    if (rl == 0 || (rl > 0 && low_share_ok(axis, row0 + rl))) return Route{RouteKind::exact_lr, rl};
    return Route{exact_parked_fits(n, rows, D) ? RouteKind::exact_parked : RouteKind::exact_records, 0};
}

// ---- record workspaces (the shapes without a fused kernel) and the other chunked engine workspaces ----
inline size_t f32_record_bytes(int n, int64_t C) { return (size_t)C * (n / 2 + 2) * 8; }   // per stream: frame stride K + 1 (even) of uint2
// EXACT: the (q, key) arrays of a chunk of streams in d_hist, q first
struct ExactRecords { size_t q_per_stream, key_per_stream, per_stream; };
inline ExactRecords exact_record_bytes(int n, int64_t C) {
    const size_t cells = (size_t)C * (size_t)ex::rec_stride(n);
    return ExactRecords{cells * 8, cells * 4, cells * 12};
}
constexpr size_t kChunkPad = 256;   // what a two-array workspace asks for beside its streams: the second array's round-up
inline size_t second_array_offset(size_t first_per_stream, int chunk) { return al(first_per_stream * (size_t)chunk); }
// staging of the two parity dumps in d_stage: the samples, then the per-bin arrays of nb entries
struct DumpStage { size_t pcm, power, q, col, row, bytes; };   // (q: EXACT only)
inline DumpStage dump_stage(size_t b_pcm, size_t nb, bool exact) {
    DumpStage d{0, al(b_pcm), 0, 0, 0, 0};
    d.q = d.power + (exact ? al(nb * 8) : 0);
    d.col = exact ? d.q + al(nb * 8) : d.power + al(nb * 4);
    d.row = d.col + al(nb * 4);
    d.bytes = d.row + al(nb * 4) + 256;
    return d;
}
// Streams are processed in chunks so that a workspace stays bounded.  The budget follows the device: a quarter of what is free
// (counting what the engine already holds), at least 256 MiB, at most `cap` (budget_mb >= 0: the diagnostic build's
// EMSPEC_RECORD_BUDGET_MB instead); the first chunk is as many of the S streams as the budget holds, at least one.  When the
// allocation fails all the same, the chunk is halved (next_chunk) and tried again.
struct ChunkPlan { int chunk; size_t bytes; };
inline ChunkPlan chunk_plan(size_t per_stream, size_t extra, int chunk) { return ChunkPlan{chunk, per_stream * (size_t)chunk + extra}; }
inline ChunkPlan first_chunk(size_t free_b, size_t have, size_t per_stream, size_t extra, size_t cap, int S, int64_t budget_mb) {
    const size_t floor_b = (size_t)256 << 20;
    size_t budget = (free_b + have) / 4;
    budget = budget < floor_b ? floor_b : (budget > cap ? cap : budget);
    if (budget_mb >= 0) budget = (size_t)budget_mb << 20;
    const int chunk = (int)(budget / per_stream);
    return chunk_plan(per_stream, extra, chunk < 1 ? 1 : (chunk > S ? S : chunk));
}
inline ChunkPlan next_chunk(ChunkPlan p, size_t per_stream, size_t extra) { return chunk_plan(per_stream, extra, (p.chunk + 1) / 2); }

}  // namespace emspec
