// pipe_plan_verbatim.h — the plan arithmetic of the host-buffer pipeline AS IT WAS in emspec_host.cpp before it was reshaped:
// PipeItem, pipe_units, pipe_items, Stage / Set, stage_layout, Span, spans_of, span_of and host_batch's two per-stream formulas
// and output estimate, moved out unchanged but for `inline`.  It is the generator of tests/golden/pipe_plans.json
// (pipe_plan_driver.cpp with -DPIPE_PLAN_VERBATIM) and is not part of the library: do not bring it up to date.
#pragma once
#include "../../include/emspec.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace emspec {

// One unit of the host pipelines: `sc` whole streams from stream s0 on - or, when the batch has fewer streams than the pipeline
// needs units (BASELINE configs[1] is ONE stream), a run of columns [c0, c0 + cn) of one stream, computed as a batch of its own
// from the frames that reach those columns: D more on either side (a bin moves at most D columns), whose own columns - `skip` in
// front, the rest behind - are computed and left on the device.  Every frame that adds to a kept column is in the run and no
// other frame can reach it, so the kept columns are the whole batch's (EXACT mode: the same bytes; float32: the same sums in
// another order, as between any two launches).
struct PipeItem { int s0, sc; int64_t c0, cn, first_sample, samples, skip, cols; };

// How many units a batch is cut into.  A unit costs ~0.2 ms (EXACT: 0.4) on the compute stream whatever its size: a launch of
// the fused kernel takes 0.11-0.18 ms however few columns it has - a workgroup WALKS its segment, 2 D halo frames and the ring's
// start-up before the first column leaves (emspec_batch_device on 49 columns: 113 us on the GPU, 5 us to enqueue) - the units'
// kernels run one after the other, and each unit adds ~40 us of event waits and copy start-up.  Behind that, three stages
// overlap: with u units a call takes about
//     max(u x 0.2 ms,  M + (sum - M) / u),   M = the longest of [bytes in / 45 GB/s, kernel time, bytes out / 45 GB/s].
// Until late round 6 the count was fixed (sixteen, or one per stream below that): 8 streams x 2^18 samples took 1.65 ms - eight
// units - for 0.5 ms of copies and kernels.  The kernel rates are the bench line's, rounded; at most sixteen units.
inline int pipe_units(bool exact, int n, int64_t columns, size_t bytes_in, size_t bytes_out) {
    const double rate = (n <= 1024 ? 3.4e8 : n <= 2048 ? 2.2e8 : n <= 4096 ? 1.15e8 : n <= 8192 ? 5e7 : 2.2e7) / (exact ? (n > 4096 ? 2.8 : 2.1) : 1.0);
    const double t_in = (double)bytes_in / 45e9, t_out = (double)bytes_out / 45e9, t_k = (double)columns / rate;
    const double longest = std::max(t_in, std::max(t_k, t_out)), sum = t_in + t_k + t_out, per_unit = exact ? 0.4e-3 : 0.2e-3;
    int best = 1;
    double best_t = sum + per_unit;
    for (int u = 2; u <= 16; ++u) {
        const double t = std::max(u * per_unit, longest + (sum - longest) / u);
        if (t < best_t * 0.995) { best = u; best_t = t; }   // (not one unit more for nothing)
    }
    return best;
}

// (f: the engine's time reduction.  A run starts on a multiple of f, so that every group of f columns lies in one unit - the
// lengths are then multiples of f but for the stream's last run - and a batch of fewer than two groups per stream is not cut)
inline std::vector<PipeItem> pipe_items(int S, int64_t L, int64_t C, int n, int hop, int D, size_t per_stream_bytes, bool by_time, int target, int f) {
    std::vector<PipeItem> items;
    // runs of columns: when there are fewer than `target` streams; at least 16,384 columns per run - a unit costs ~0.2 ms
    // (pipe_units) whatever its size, and 16 MB each way over PCIe take 0.35 ms (measured with 2,048-column runs: one stream
    // of 2^22 samples 1.49 ms instead of 0.84 in one piece)
    const int64_t pieces = by_time && S < target ? std::min<int64_t>((target + S - 1) / S, std::min(C / 16384, C / f)) : 1;
    if (pieces > 1) {
        for (int s = 0; s < S; ++s)
            for (int64_t t = 0; t < pieces; ++t) {
                PipeItem it;
                it.s0 = s; it.sc = 1;
                it.c0 = C * t / pieces / f * f;
                it.cn = (t + 1 < pieces ? C * (t + 1) / pieces / f * f : C) - it.c0;
                const int64_t f0 = std::max<int64_t>(it.c0 - D, 0), f1 = std::min<int64_t>(it.c0 + it.cn + D, C);   // frames [f0, f1)
                it.first_sample = f0 * hop;
                it.samples = (f1 - f0 - 1) * hop + n;
                it.skip = it.c0 - f0;
                it.cols = f1 - f0;
                items.push_back(it);
            }
        return items;
    }
    // chunks of streams: about `target` per batch (pipe_units), bounded by 1 GiB of staging per set; a chunk of a few streams
    // still fills the chip (segments are cut per launch)
    int chunk = (S + target - 1) / target;
    const int fit = (int)(((size_t)1 << 30) / per_stream_bytes);
    chunk = chunk > fit ? fit : chunk;
    chunk = chunk < 1 ? 1 : chunk;
    for (int s0 = 0; s0 < S; s0 += chunk) items.push_back(PipeItem{s0, std::min(chunk, S - s0), 0, C, 0, L, 0, C});
    return items;
}

inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

// Staging bytes per stream (pipe_items: the 1 GiB cap per set) and the bytes a call delivers (pipe_units), as host_batch states them
inline size_t per_stream_bytes(size_t in_s, int64_t L, bool dec, int V, size_t col_cells, size_t out_cells, size_t wire_s, int64_t C, int pkk,
                               bool want_db, bool stage_db, bool want_rgba, bool want_idx, int f) {
    size_t per_stream = al(in_s) + (dec ? al((size_t)L * 4 * V) : 0) +
                        V * (al(stage_db ? col_cells * 4 : 0) + al(want_rgba ? col_cells * 4 : 0) + al(want_idx ? col_cells : 0) + al(wire_s) +
                             al((size_t)C * pkk * sizeof(emspec_peak)));
    if (f > 1)   // full-rate dB / index (no full-rate RGBA) and the reduced arrays
        per_stream = al(in_s) + (dec ? al((size_t)L * 4 * V) : 0) +
                     V * (al(want_db ? col_cells * 4 : 0) + al(want_idx || want_rgba ? col_cells : 0) + al(wire_s) +
                          al(want_db ? out_cells * 4 : 0) + al(want_rgba ? out_cells * 4 : 0) + al(want_idx ? out_cells : 0));
    return per_stream;
}
inline size_t bytes_out_estimate(bool packed, int S, int V, size_t out_cells, int64_t C, int pkk, bool want_db, bool want_rgba, bool want_idx) {
    return packed ? (size_t)S * V * out_cells / 5 : (size_t)S * V * out_cells * ((want_db ? 4 : 0) + (want_rgba ? 4 : 0) + (want_idx ? 1 : 0)) +
                                                        (size_t)S * V * C * pkk * sizeof(emspec_peak);
}

// (db / rgba / idx: what the unit's kernels write; odb / orgba / oidx: what is delivered - the same arrays, or with a time
// reduction the reduced columns beside them)
// (peaks: the unit's peak lists, emspec_batch_peaks)
struct Set { float* pcm; float* db; uint8_t* rgba; uint8_t* idx; uint8_t* wire; char* raw; float* odb; uint8_t* orgba; uint8_t* oidx; emspec_peak* peaks; };

// The staging set: every array at the size the largest unit needs (the wire images: one slot of `wire` bytes per stream).
struct Stage {
    size_t in = 0, db = 0, rgba = 0, idx = 0, wire = 0;
    size_t raw = 0;  // PCM entries: the unit's raw frames, which the decode kernel turns into `in`
    size_t rdb = 0, rrgba = 0, ridx = 0;   // time reduction: the unit's reduced columns (db / idx then hold the full-rate ones)
    bool reduced = false;
    size_t peaks = 0;   // emspec_batch_peaks: k (pos, dB) pairs per kept column of the unit
    int chunk = 1;   // streams in the largest unit
    size_t bytes() const { return in + db + rgba + idx + wire * chunk + raw + rdb + rrgba + ridx + peaks; }
    Set at(char* stage, int b) const {
        char* base = stage + (size_t)b * bytes();
        Set q{(float*)base, db ? (float*)(base + in) : nullptr, rgba ? (uint8_t*)(base + in + db) : nullptr,
              idx ? (uint8_t*)(base + in + db + rgba) : nullptr, wire ? (uint8_t*)(base + in + db + rgba + idx) : nullptr,
              raw ? base + in + db + rgba + idx + wire * chunk : nullptr, nullptr, nullptr, nullptr, nullptr};
        char* r = base + in + db + rgba + idx + wire * chunk + raw;
        q.odb = reduced ? (rdb ? (float*)r : nullptr) : q.db;
        q.orgba = reduced ? (rrgba ? (uint8_t*)(r + rdb) : nullptr) : q.rgba;
        q.oidx = reduced ? (ridx ? (uint8_t*)(r + rdb + rrgba) : nullptr) : q.idx;
        q.peaks = peaks ? (emspec_peak*)(r + rdb + rrgba + ridx) : nullptr;
        return q;
    }
};

// (V streams per unit of PipeItem::sc, frame_bytes of raw input each: 1 and 0 for the float entries, whose units are streams)
// (f > 1: dB and / or index at full rate - the index also when only RGBA is wanted - and the delivered arrays at the reduced rate)
// (peaks_k > 0: a region of peaks_k pairs per kept column)
inline Stage stage_layout(const std::vector<PipeItem>& items, int R, bool db, bool rgba, bool idx, size_t wire_s, int V, int frame_bytes, int f, int peaks_k) {
    Stage g;
    size_t cells = 0, rcells = 0;
    for (const PipeItem& it : items) {
        rcells = std::max(rcells, (size_t)((it.cn + f - 1) / f) * R * it.sc * V);
        g.in = std::max(g.in, al((size_t)it.samples * 4 * it.sc * V));
        g.raw = std::max(g.raw, frame_bytes ? al((size_t)it.samples * frame_bytes * it.sc) : 0);
        cells = std::max(cells, (size_t)it.cols * R * it.sc * V);
        g.chunk = std::max(g.chunk, it.sc * V);
        g.peaks = std::max(g.peaks, al((size_t)it.cn * it.sc * V * peaks_k * sizeof(emspec_peak)));
    }
    g.reduced = f > 1;
    g.db = db ? al(cells * 4) : 0;
    g.rgba = rgba && !g.reduced ? al(cells * 4) : 0;
    g.idx = idx || (rgba && g.reduced) ? al(cells) : 0;
    g.wire = al(wire_s);
    if (g.reduced) {
        g.rdb = db ? al(rcells * 4) : 0;
        g.rrgba = rgba ? al(rcells * 4) : 0;
        g.ridx = idx ? al(rcells) : 0;
    }
    return g;
}

// Where a unit's kept columns come from in its set and go in the caller's arrays: cell offsets and count.  A unit of whole
// streams is one span; a run of columns is one span per stream (V > 1: the views of the unit's source).
// (C: the columns a stream is computed at; f: the time reduction - Cr = ceil(C / f) columns of it are delivered, a run's
// ceil(cn / f) from column c0 / f on, out of the unit's reduced array, which holds the kept columns only)
struct Span { size_t from, to, cells; };
inline int spans_of(const PipeItem& it, int64_t C, int V) { return it.cn == C ? 1 : it.sc * V; }
inline Span span_of(const PipeItem& it, int64_t C, int R, int V, int k, int f) {
    if (f == 1) {
        if (it.cn == C) return Span{0, (size_t)it.s0 * V * C * R, (size_t)it.cn * R * it.sc * V};
        return Span{((size_t)k * it.cols + (size_t)it.skip) * R, (((size_t)it.s0 * V + k) * C + (size_t)it.c0) * R, (size_t)it.cn * R};
    }
    const size_t Cr = (size_t)((C + f - 1) / f), crn = (size_t)((it.cn + f - 1) / f);
    if (it.cn == C) return Span{0, (size_t)it.s0 * V * Cr * R, crn * R * it.sc * V};
    return Span{(size_t)k * crn * R, (((size_t)it.s0 * V + k) * Cr + (size_t)(it.c0 / f)) * R, crn * R};
}

}  // namespace emspec
