// emspec_history_plan.h — internal: the arithmetic of the live history (include/emspec.h: emspec_set_live_history,
// emspec_history_view): a ring of W delivered dB columns per stream of a streaming session, and views
// that read it back reduced by a factor.  Where a column lives, what the ring holds after a launch, which of a launch's columns
// are stored when it emits more than W, whether a view fits, and the slot runs a group's columns occupy across the wrap.
// Integer arithmetic only.  No HIP, nothing of the engine: tests/test_history_plan_cpu.py runs it through a stand-alone program
// (tests/cdriver/history_plan_driver.cpp) without a GPU.  Host and kernels (live_history.hip.inc) share it.
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

constexpr int64_t kHistoryMaxColumns = 1 << 20;   // W per stream, at most
constexpr int kHistoryMaxFactor = 65536;          // columns per group of a view, at most (as emspec_set_time_reduce)

// Column c of a stream - the c-th finished column its session has emitted since the stream was (re)started - lives in slot c mod W.
EMSPEC_HD inline int64_t history_slot(int64_t c, int64_t W) { return c % W; }
// After `end` columns were emitted the ring holds [history_first(end, W), end).
EMSPEC_HD inline int64_t history_first(int64_t end, int64_t W) { return end > W ? end - W : 0; }
// A launch emits columns [c0, c0 + count) of a stream, one wave or workgroup per column: those below history_keep_from are not
// stored - the launch's last W are, each in a slot of its own (W consecutive columns have W distinct slots), so no slot is
// written twice in one launch.
EMSPEC_HD inline int64_t history_keep_from(int64_t c0, int64_t count, int64_t W) { return count > W ? c0 + count - W : c0; }
EMSPEC_HD inline bool history_stores(int64_t c, int64_t c0, int64_t count, int64_t W) {
    return c >= c0 && c < c0 + count && c >= history_keep_from(c0, count, W);
}

// A view of one stream: groups g in [0, groups) of f columns from column `first` on; group g covers
// [first + g f, min(first + (g + 1) f, end)) - only the last group may be short.  It fits when its first column is held and
// every group has a column: first >= the first held column, first + (groups - 1) f < end.  (No product overflows: the
// comparison is made on the quotient.)
enum HistoryViewError { kHistoryViewOk = 0, kHistoryViewArg = 1, kHistoryViewRange = 2 };
inline int history_view_check(int64_t first, int64_t f, int64_t groups, int64_t end, int64_t W) {
    if (f < 1 || f > kHistoryMaxFactor || groups < 1 || W < 1) return kHistoryViewArg;
    if (first < history_first(end, W) || first >= end) return kHistoryViewRange;
    return groups - 1 <= (end - 1 - first) / f ? kHistoryViewOk : kHistoryViewRange;
}
// the columns of group g of a view that fits: [c0, c1), at least one and at most min(f, W)
struct HistoryGroup { int64_t c0, c1; };
EMSPEC_HD inline HistoryGroup history_group(int64_t first, int64_t f, int64_t g, int64_t end) {
    const int64_t c0 = first + g * f;
    return HistoryGroup{c0, c0 + f < end ? c0 + f : end};
}
// ... and the slots they occupy, in column order: [slot0, slot0 + n0), then, across the wrap, [0, n1)  (n0 >= 1, n1 >= 0,
// n0 + n1 = count <= W)
struct HistoryRuns { int64_t slot0, n0, n1; };
EMSPEC_HD inline HistoryRuns history_runs(int64_t c0, int64_t count, int64_t W) {
    const int64_t slot0 = history_slot(c0, W);
    const int64_t n0 = count < W - slot0 ? count : W - slot0;
    return HistoryRuns{slot0, n0, count - n0};
}
// What the kernel does instead of a modulo per group: a view that fits has g f < W for each of its groups
// ((groups - 1) f < end - first <= W), so the first slot of group g is slot(first) + g f, wrapped once.
EMSPEC_HD inline int history_group_slot(int slot_first, int gf, int W) {
    const int s = slot_first + gf;
    return s >= W ? s - W : s;
}
// the next column's slot: the wrap is one compare
EMSPEC_HD inline int history_next_slot(int slot, int W) { return slot + 1 == W ? 0 : slot + 1; }

// the ring of a session: [S][W][rows] float32
inline size_t history_ring_bytes(int S, int64_t W, int rows) { return (size_t)S * (size_t)W * (size_t)rows * 4; }
// a view's outputs: [streams][groups][rows] cells (4 bytes of dB, 1 of index, 4 of RGBA each)
inline size_t history_view_cells(int streams, int64_t groups, int rows) { return (size_t)streams * (size_t)groups * (size_t)rows; }

}  // namespace emspec
