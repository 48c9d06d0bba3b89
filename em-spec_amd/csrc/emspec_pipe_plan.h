// emspec_pipe_plan.h — internal: the plan of the host-buffer pipeline (emspec_host.cpp): how a batch is cut into units, how a
// unit's arrays lie in a staging set, which cells each unit delivers.  No HIP, nothing of the engine: tests/test_pipe_plan_cpu.py.
#pragma once
#include "../../include/emspec.h"
#include "emspec_wire_plan.h"   // al
#include <algorithm>
#include <numeric>
#include <vector>

namespace emspec {
// One unit of the host pipelines: `sc` whole streams from stream s0 on - or, when the batch has fewer streams than the pipeline
// needs units ("Few streams"), a run of columns [c0, c0 + cn) of one stream, computed as a batch of its own from the
// frames that reach those columns: D more on either side (a bin moves at most D columns), whose own columns - `skip` in front,
// the rest behind - are computed and left on the device.  The kept columns are the whole batch's (EXACT mode: the same bytes).
struct PipeItem { int s0, sc; int64_t c0, cn, first_sample, samples, skip, cols; };

// How many units a batch is cut into ("How many units").  A unit costs ~0.2 ms (EXACT: 0.4) on the compute stream
// whatever its size, and behind that three stages overlap: with u units a call takes about
//     max(u x 0.2 ms,  M + (sum - M) / u),   M = the longest of [bytes in / 45 GB/s, kernel time, bytes out / 45 GB/s].
// The kernel rates are the bench line's, rounded; at most sixteen units.
inline int pipe_units(bool exact, int n, int64_t columns, size_t bytes_in, size_t bytes_out) {
    const double rate = (n <= 1024 ? 3.4e8 : n <= 2048 ? 2.2e8 : n <= 4096 ? 1.15e8 : n <= 8192 ? 5e7 : 2.2e7) / (exact ? (n > 4096 ? 2.8 : 2.1) : 1.0);
    const double t_in = (double)bytes_in / 45e9, t_out = (double)bytes_out / 45e9, t_k = (double)columns / rate;
    const double longest = std::max(t_in, std::max(t_k, t_out)), sum = t_in + t_k + t_out, per_unit = exact ? 0.4e-3 : 0.2e-3;
    int best = 1; double best_t = sum + per_unit;
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
    // (pipe_units) whatever its size, and 16 MB each way over PCIe take 0.35 ms ("Few streams")
    const int64_t pieces = by_time && S < target ? std::min<int64_t>((target + S - 1) / S, std::min(C / 16384, C / f)) : 1;
    if (pieces > 1) {
        for (int s = 0; s < S; ++s)
            for (int64_t t = 0; t < pieces; ++t) {
                const int64_t c0 = C * t / pieces / f * f, cn = (t + 1 < pieces ? C * (t + 1) / pieces / f * f : C) - c0;
                const int64_t f0 = std::max<int64_t>(c0 - D, 0), f1 = std::min<int64_t>(c0 + cn + D, C);   // frames [f0, f1)
                items.push_back(PipeItem{s, 1, c0, cn, f0 * hop, (f1 - f0 - 1) * hop + n, c0 - f0, f1 - f0});
            }
        return items;
    }
    // chunks of streams: about `target` per batch (pipe_units), bounded by 1 GiB of staging per set; a chunk of a few streams
    // still fills the chip (segments are cut per launch)
    const int fit = (int)(((size_t)1 << 30) / per_stream_bytes);
    const int chunk = std::max(std::min((S + target - 1) / target, fit), 1);
    for (int s0 = 0; s0 < S; s0 += chunk) items.push_back(PipeItem{s0, std::min(chunk, S - s0), 0, C, 0, L, 0, C});
    return items;
}

// What a call delivers: one row per array, in the order of a set's layout.  `host`: the caller's array (null: not copied out -
// the packed entries stage the index for the wire images only); `unit`: bytes per cell - peaks: per column, k pairs - or 0
// without that array.  Where the unit's copy lies in a staging set: Stage::out_off.  kWave: the waveform envelope of the samples
// (emspec_set_wave_out), one pair per DELIVERED column.  kSLevel .. kSRgba: the stereo image (emspec_batch_pcm_stereo; DESIGN.md
// §3.16), one cell per PAIR cell - a pair is the V streams of one source, so a unit's sc sources give sc pairs.  kLevel: the
// level records of the samples (emspec_set_level_out), one per stream and DELIVERED column, as the envelope's
// pairs; kCross: the cross records of two views of each source (emspec_set_cross_out), one per SOURCE and delivered column.
enum { kDb, kRgba, kIdx, kPeaks, kWave, kSLevel, kSIdx, kSPan, kSRgba, kLevel, kCross, kOutRows };
struct OutRow { char* host; size_t unit; };
inline bool stereo_rows(const OutRow* o) { return o[kSLevel].unit || o[kSIdx].unit || o[kSPan].unit || o[kSRgba].unit; }
// The bytes `streams` streams leave the device with (pipe_units): the rows' - or the wire images', about a fifth of the index
// (the envelope's 8 bytes per delivered column are not counted, nor the level meters' 24 and 16: a batch is cut the same way
// with and without them)
inline size_t bytes_out_estimate(const OutRow* o, bool packed, size_t streams, int64_t C, int64_t Cr, int R) {
    const size_t cell = o[kDb].unit + o[kRgba].unit + o[kIdx].unit;
    return packed ? streams * Cr * R / 5 : streams * Cr * R * cell + streams * C * o[kPeaks].unit;
}
// ... of a stereo job instead: its pairs' cells (no other row is set beside them but the envelope's)
inline size_t stereo_bytes_out(const OutRow* o, size_t pairs, int64_t C, int R) {
    return pairs * C * R * (o[kSLevel].unit + o[kSIdx].unit + o[kSPan].unit + o[kSRgba].unit);
}

// (db / rgba / idx: what the unit's kernels write; odb / orgba / oidx: what is delivered - the same arrays, or with a time
// reduction the reduced columns beside them; peaks: the unit's peak lists, emspec_batch_peaks)
// slevel / sidx / span / srgba: the stereo image of the unit's pairs, composed from db
// level / cross: the level and cross records of the unit's delivered columns
struct Set { float* pcm; float* db; uint8_t* rgba; uint8_t* idx; uint8_t* wire; char* raw; float* odb; uint8_t* orgba; uint8_t* oidx; emspec_peak* peaks; emspec_wave* wave;
             float* slevel; uint8_t* sidx; uint8_t* span; uint8_t* srgba; emspec_level* level; emspec_cross* cross; };
// The staging set: every array at the size the largest unit needs, in the order of off()'s list.
struct Stage {
    size_t in = 0, db = 0, rgba = 0, idx = 0, wire = 0;   // (wire: one slot of that many bytes per stream of the unit)
    size_t raw = 0;                                       // PCM entries: the unit's raw frames, which the decode kernel turns into `in`
    size_t rdb = 0, rrgba = 0, ridx = 0;                  // time reduction: the reduced columns (db / idx then hold the full-rate ones)
    size_t peaks = 0;                                     // emspec_batch_peaks: k (pos, dB) pairs per kept column of the unit
    size_t wave = 0;                                      // emspec_set_wave_out: a pair per delivered column of the unit; behind every
                                                          // array above, so that a job without an envelope keeps every offset and size
    size_t stereo[4] = {};                                // emspec_batch_pcm_stereo: level, index, pan, RGBA per pair cell of the unit;
                                                          // behind the envelope's and empty for every other job, for the same reason
    size_t level = 0, cross = 0;                          // emspec_set_level_out / _cross_out: a record per stream (per source) and
                                                          // delivered column of the unit; last and empty while cleared, likewise
    bool reduced = false; int chunk = 1;                  // (chunk: streams in the largest unit)
    size_t off(int a) const {   // byte offset in a set of its a-th array
        const size_t s[17] = {in, db, rgba, idx, wire * chunk, raw, rdb, rrgba, ridx, peaks, wave, stereo[0], stereo[1], stereo[2], stereo[3],
                              level, cross};
        return std::accumulate(s, s + a, (size_t)0);
    }
    size_t bytes() const { return off(17); }
    // ... of row w's delivered copy: the reduced array, or without a reduction what the kernels wrote (kLevel, kCross: arrays
    // 15 and 16, behind the stereo rows)
    size_t out_off(int w) const { return off(w >= kSLevel ? 11 + (w - kSLevel) : w == kWave ? 10 : w == kPeaks ? 9 : reduced ? 6 + w : 1 + w); }
    Set at(char* stage, int b) const {
        char* base = stage + (size_t)b * bytes();
        auto p = [&](size_t have, size_t o) { return have ? base + o : nullptr; };
        return Set{(float*)base, (float*)p(db, off(1)), (uint8_t*)p(rgba, off(2)), (uint8_t*)p(idx, off(3)), (uint8_t*)p(wire, off(4)), p(raw, off(5)),
                   (float*)p(reduced ? rdb : db, out_off(kDb)), (uint8_t*)p(reduced ? rrgba : rgba, out_off(kRgba)),
                   (uint8_t*)p(reduced ? ridx : idx, out_off(kIdx)), (emspec_peak*)p(peaks, out_off(kPeaks)),
                   (emspec_wave*)p(wave, out_off(kWave)), (float*)p(stereo[0], out_off(kSLevel)), (uint8_t*)p(stereo[1], out_off(kSIdx)),
                   (uint8_t*)p(stereo[2], out_off(kSPan)), (uint8_t*)p(stereo[3], out_off(kSRgba)),
                   (emspec_level*)p(level, out_off(kLevel)), (emspec_cross*)p(cross, out_off(kCross))};
    }
};

// The arrays of a set behind its input, for `cells` full-rate cells, `rcells` reduced ones, the peak lists of `cols` columns and
// the envelope pairs (and level records) of `rcols` delivered columns and the cross records of `prcols` sources' delivered columns.
// Full rate: the rows' own arrays, but the dB also for the peaks kernel and the stereo image (of `pcells` pair cells), and with
// f > 1 the index in place of RGBA.
inline Stage stage_arrays(const OutRow* o, int f, size_t cells, size_t rcells, size_t cols, size_t rcols, size_t wire_s, size_t pcells = 0,
                          size_t prcols = 0) {
    Stage g;
    g.reduced = f > 1;
    g.db = o[kDb].unit || o[kPeaks].unit || stereo_rows(o) ? al(cells * 4) : 0;
    g.rgba = o[kRgba].unit && !g.reduced ? al(cells * 4) : 0;
    g.idx = o[kIdx].unit || (o[kRgba].unit && g.reduced) ? al(cells) : 0;
    g.wire = al(wire_s);
    if (g.reduced) { g.rdb = al(rcells * o[kDb].unit); g.rrgba = al(rcells * o[kRgba].unit); g.ridx = al(rcells * o[kIdx].unit); }
    g.peaks = al(cols * o[kPeaks].unit);
    g.wave = al(rcols * o[kWave].unit);
    for (int w = 0; w < 4; ++w) g.stereo[w] = al(pcells * o[kSLevel + w].unit);
    g.level = al(rcols * o[kLevel].unit);
    g.cross = al(prcols * o[kCross].unit);
    return g;
}
// Staging bytes per stream (pipe_items' 1 GiB cap): the input (`dec_s`: a PCM source's decoded floats), each view's arrays and
// the source's stereo image and cross records
inline size_t per_stream_bytes(const OutRow* o, size_t in_s, size_t dec_s, int V, int64_t C, int64_t Cr, int R, size_t wire_s, int f) {
    size_t pair = 0;
    for (int w = kSLevel; w <= kSRgba; ++w) pair += al((size_t)C * R * o[w].unit);
    pair += al((size_t)Cr * o[kCross].unit);
    return al(in_s) + (dec_s ? al(dec_s) : 0) + V * stage_arrays(o, f, (size_t)C * R, (size_t)Cr * R, (size_t)C, (size_t)Cr, wire_s).bytes() + pair;
}
// The set of a batch (V streams per unit of PipeItem::sc, frame_bytes of raw input each: 1 and 0 for the float entries)
inline Stage stage_layout(const std::vector<PipeItem>& items, int R, const OutRow* o, size_t wire_s, int V, int frame_bytes, int f) {
    size_t in = 0, raw = 0, cells = 0, rcells = 0, cols = 0, rcols = 0, pcells = 0, prcols = 0; int chunk = 1;
    for (const PipeItem& it : items) {
        in = std::max(in, al((size_t)it.samples * 4 * it.sc * V));
        raw = std::max(raw, frame_bytes ? al((size_t)it.samples * frame_bytes * it.sc) : 0);
        cells = std::max(cells, (size_t)it.cols * R * it.sc * V);
        rcells = std::max(rcells, (size_t)((it.cn + f - 1) / f) * R * it.sc * V);
        cols = std::max(cols, (size_t)it.cn * it.sc * V);
        rcols = std::max(rcols, (size_t)((it.cn + f - 1) / f) * it.sc * V);
        chunk = std::max(chunk, it.sc * V);
        pcells = std::max(pcells, (size_t)it.cols * R * it.sc);
        prcols = std::max(prcols, (size_t)((it.cn + f - 1) / f) * it.sc);
    }
    Stage g = stage_arrays(o, f, cells, rcells, cols, rcols, wire_s, pcells, prcols);
    g.in = in; g.raw = raw; g.chunk = chunk;
    return g;
}

// Where a unit's kept columns come from in its set and go in the caller's arrays: cell offsets and count.  A unit of whole
// streams is one span; a run of columns is one span per stream (V > 1: the views of the unit's source).  With a time reduction
// f, Cr = ceil(C / f) columns are delivered, a run's ceil(cn / f) from column c0 / f on, out of the unit's reduced array.
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

// The stereo image of a unit: its sc sources are sc pairs of V streams, composed over ALL the unit's columns (a run's halo
// columns included: the compose kernel takes streams one whole array apart) - one span per unit, that of a job of single-view
// streams, in pair cells
inline Span stereo_span_of(const PipeItem& it, int64_t C, int R) { return span_of(it, C, R, 1, 0, 1); }

// The waveform envelope of a unit (window.hip.inc), in pairs = delivered columns.  Its kernel reads the unit's
// staged samples: the first window starts WaveRun::first samples into each of the unit's streams (off = n / 2 - hop / 2 past
// the first sample of the unit's first kept column), `cols` = the kept columns in groups of f - a run starts on a multiple of
// f, so its groups are the stream's - and writes ceil(cn / f) pairs per stream, stream after stream, into the set's array.
struct WaveRun { int64_t first, cols, pairs; };
inline WaveRun wave_run_of(const PipeItem& it, int n, int hop, int f) {
    return WaveRun{it.skip * hop + (n / 2 - hop / 2), it.cn, (it.cn + f - 1) / f};
}
// ... and which pairs span k of the unit delivers (spans_of): from the set's pair array to the caller's [streams][Cr]
inline Span wave_span_of(const PipeItem& it, int64_t C, int V, int k, int f) {
    const size_t Cr = (size_t)((C + f - 1) / f), crn = (size_t)((it.cn + f - 1) / f);
    if (it.cn == C) return Span{0, (size_t)it.s0 * V * Cr, crn * it.sc * V};
    return Span{(size_t)k * crn, ((size_t)it.s0 * V + k) * Cr + (size_t)(it.c0 / f), crn};
}

// The level records of a unit (window.hip.inc) lie and travel exactly as the envelope's pairs: wave_run_of,
// wave_span_of.  The cross records are one per SOURCE and delivered column: the unit's sc sources as sc streams of one view -
// a run of columns is one source (sc = 1), so a pair never straddles a unit.
inline Span cross_span_of(const PipeItem& it, int64_t C, int f) { return wave_span_of(it, C, 1, 0, f); }
}  // namespace emspec
