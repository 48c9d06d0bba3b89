// emspec_live_plan.h — internal: the host arithmetic of a streaming session (emspec_live.cpp): the descriptor the
// kernels read per stream, the session's geometry - a list of bands, whatever its kind - with every byte size derived from it,
// the rule that refuses a call which does not fit the open session, the kernels each launch runs, the per-stream counters, and
// the steps of each call that decide which column an output slot holds.  Integer arithmetic only.  No HIP, nothing of the engine:
// tests/test_live_plan_cpu.py and tests/test_live_band_plan_cpu.py run it through a stand-alone program
// (tests/cdriver/live_plan_driver.cpp) without a GPU.
#pragma once
#include "emspec_band_plan.h"
#include "emspec_tables.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

// the one rule below that the overlay kernel and the host share (as in emspec_kernel_plan.h)
#ifndef EMSPEC_HD
#ifdef __HIPCC__
#define EMSPEC_HD __host__ __device__
#else
#define EMSPEC_HD
#endif
#endif

namespace emspec {

// ---- live multi-stream streaming (emspec_columns / emspec_push_samples_multi; live.hip.inc) ----
// One launch serves S live streams: grid = (frames per stream + 1, S).  Workgroup (f, s) with f < frames[s] transforms
// frame j0[s] + f of stream s and scatters it into that stream's column ring in HBM (device-scope atomics); the LAST of a
// stream's workgroups to finish (an arrival counter per stream) finalises the columns the launch completed, straight into the
// caller's (page-locked) output, and clears their ring slots.  Workgroup (gridDim.x - 1, s) moves the stream's new samples
// from the page-locked staging block into its device sample ring for later launches.
struct LiveStream {        // per stream and launch; read by the kernel from page-locked host memory
    long long j0;          // absolute index of the stream's first frame in this launch (= frames fed so far)
    long long newbase;     // absolute index of fresh[s][0]: samples below it are in the device sample ring
    int frames;            // frames of this stream in this launch (0 .. gridDim.x - 1)
    int newcount;          // samples in fresh[s] to move into the sample ring
    int out_at;            // first column slot of the stream's output block this launch writes
    int flush;             // != 0: no frames; finalise `flush` pending columns starting at column j0 - D (emspec_columns_flush)
};
// (the kernel reads it from page-locked memory and from the kernel arguments: the layout is part of the launch)
static_assert(sizeof(LiveStream) == 32 && std::is_trivially_copyable<LiveStream>::value, "LiveStream: 32 bytes, copied as bytes");
static_assert(offsetof(LiveStream, j0) == 0 && offsetof(LiveStream, newbase) == 8 && offsetof(LiveStream, frames) == 16 &&
                  offsetof(LiveStream, newcount) == 20 && offsetof(LiveStream, out_at) == 24 && offsetof(LiveStream, flush) == 28,
              "LiveStream: field offsets");

// per-sample-block form: frames per stream and launch, at most - about 2,048 workgroups per launch, 8..64 per stream
inline int live_frames_per_launch(int S) { return std::max(8, std::min(64, 2048 / std::max(1, S))); }
// whole frames in `total` samples
inline int64_t frames_after(int64_t total, int n, int hop) { return total >= n ? (total - n) / hop + 1 : 0; }

// ---- the session at its first fft size: fixed by its first call ----
// What every kind of session shares: streams, hop, the feeding form, the staging block, the device sample ring, the output
// layout.  Its column rings are the bands' (LiveSession below).
struct LiveGeometry {
    int S = 0, n = 0, hop = 0, reassign = -1, D = 0;
    int form = 0;             // 0 none, 1 per-frame (emspec_columns), 2 per-sample-block (emspec_push_samples_multi)
    int mmax = 0;             // frames per stream and launch, at most
    int64_t cap = 0;          // samples per stream the staging block holds (form 1: n; form 2: mmax * hop)
    int ring_mask = 0;        // device sample ring per stream: ring_mask + 1 >= n + cap samples, a power of two (form 2)

    // Every size below is in bytes.
    size_t sring_bytes() const { return (size_t)S * ((size_t)ring_mask + 1) * 4; }   // [S][ring_mask + 1] float32
    size_t desc_bytes() const { return (size_t)S * sizeof(LiveStream); }
    size_t fresh_bytes() const { return (size_t)S * cap * 4; }                       // staging samples [S][cap] float32
    size_t decoded_bytes() const { return fresh_bytes(); }                           // PCM session: the same block on the device
    size_t raw_bytes(int views, int frame_bytes) const { return (size_t)(S / views) * cap * frame_bytes; }   // [sources][cap] frames
    size_t raw_stride(int frame_bytes) const { return (size_t)cap * frame_bytes; }                           // ... one source's
    size_t out_bytes(int R, int64_t cols) const { return (size_t)S * cols * R * 4; }  // [S][cols][R] float32 or RGBA8
    // ... in it, the CELL (4 bytes) where column `col` of stream s starts, and the bytes of `count` columns
    static size_t out_cell(int R, int64_t cols, int s, int64_t col) { return ((size_t)s * cols + col) * R; }
    static size_t columns_bytes(int R, int64_t count) { return (size_t)count * R * 4; }
    static size_t pstate_bytes(int R) { return (size_t)(R + 4) * 4; }                 // post-process state, per stream
    // where a stream's samples go in the staging block: float samples, or bytes of raw frames (per SOURCE) of a PCM session
    size_t fresh_at(int s, int pend) const { return (size_t)s * cap + pend; }
    size_t raw_at(int source, int pend, int frame_bytes) const { return ((size_t)source * cap + pend) * frame_bytes; }
};

inline LiveGeometry live_geometry(int S, int n, int hop, int reassign, int form) {
    LiveGeometry g;
    g.S = S; g.n = n; g.hop = hop; g.reassign = reassign; g.form = form;
    g.D = latency(n, hop, reassign);
    // (a staging block of at most 2^17 samples per stream: at a large hop fewer frames per launch instead of megabytes pinned)
    g.mmax = form == 1 ? 1 : std::max(1, std::min(live_frames_per_launch(S), (1 << 17) / hop));
    g.cap = form == 1 ? n : (int64_t)g.mmax * hop;
    int ring = 1;
    while (ring < n + g.cap) ring <<= 1;
    g.ring_mask = ring - 1;
    return g;
}

// ---- the session: a list of K >= 1 bands of the row table ----
// Single-resolution (emspec_columns, emspec_push_samples*): one band, every row at n.  Two-band (*_multires): rows below
// split_row at n_low, the rest at n_high.  Multi-band (*_multiband): the caller's 2..4 bands.  The counters, descriptors and
// push / flush / frame steps below are those of the first band's fft size (`g`); a band adds what its frame launch and its
// column ring need.
enum LiveKind { kLiveNone = 0, kLiveSingle, kLiveTwoBand, kLiveMultiBand };

// What a call asks for, from its arguments alone: compared with the open session (live_mismatch) and, on a session's first
// call, turned into its geometry (live_session) - after the ABI's shape checks, no arithmetic before them.
struct LiveAsk {
    int kind = kLiveNone, S = 0, hop = 0, reassign = 0, form = 0;
    BandPlan p;   // sizes and row ranges (its shifts are not read)
};
inline LiveAsk live_ask(int kind, int S, const BandPlan& p, int hop, int reassign, int form) {
    LiveAsk a;
    a.kind = kind; a.S = S; a.hop = hop; a.reassign = reassign ? 1 : 0; a.form = form; a.p = p;
    return a;
}
inline LiveAsk live_ask_single(int S, int n, int hop, int reassign, int form, int rows) {
    BandPlan p;
    p.bands = 1; p.n[0] = n; p.hi[0] = rows;
    return live_ask(kLiveSingle, S, p, hop, reassign, form);
}
inline LiveAsk live_ask_two_band(int S, int n_low, int n_high, int hop, int split, int reassign, int form, int rows) {
    BandPlan p;
    p.bands = 2; p.n[0] = n_low; p.n[1] = n_high; p.hi[0] = p.lo[1] = split; p.hi[1] = rows;
    return live_ask(kLiveTwoBand, S, p, hop, reassign, form);
}
inline LiveAsk live_ask_bands(int S, const BandPlan& p, int hop, int reassign, int form) {
    return live_ask(kLiveMultiBand, S, p, hop, reassign, form);
}

// One band of the session: rows [lo, hi) of the output column from fft size n.  Its frames run frame_shift ahead of the first
// band's, its frame j sits on emitted column j - shift, and its ring is indexed by the emitted column.
struct LiveBand {
    int n = 0, lo = 0, hi = 0;
    int shift = 0;         // (n[0] - n) / (2 hop)
    int D = 0;             // latency(n, hop, reassign): the band's own
    int frame_shift = 0;   // 2 shift
    int lat_extra = 0;     // D_0 - D: what the frame kernel adds to its plan's D to finalise the emitted column
    int slots = 0;         // column-ring slots per stream: mmax + shift + D_0 + D (band 0: 2 D_0 + mmax)
    int rows() const { return hi - lo; }
};

struct LiveSession {
    LiveGeometry g;        // at n[0]: mmax, cap, ring_mask, D, the staging and output sizes
    int kind = kLiveNone;
    int bands = 0;
    LiveBand b[kMaxBands];
    // Every size below is in bytes.  Band k's column ring, per stream and of all S streams, `cell` bytes per cell (FAST 4,
    // EXACT 8): [slots][rows]
    size_t ring_bytes(int k, size_t cell) const { return (size_t)b[k].slots * b[k].rows() * cell; }
    size_t rings_bytes(int k, size_t cell) const { return (size_t)g.S * ring_bytes(k, cell); }
    size_t done_bytes() const { return (size_t)g.S * 4 * bands; }   // arrival counters, one set per band: band k's at done + k S
    // the workgroups per stream of band k's frame launch, without the ingest workgroup: on a stream's first frame (priming) the
    // band transforms frames 0 .. 2 shift at once
    int launch_frames(int k, int frames, bool priming) const { return frames + (priming ? b[k].frame_shift : 0); }
    // The finalize rule.  A band defers its finalize to a second kernel when the launch completes more than inline_max columns
    // per stream (inline they are one workgroup's serial round trips to the memory side, ~2 us per column) or its transform is
    // small (n < 2048: its workgroup has n / 16 threads, too few for 1024 rows).  The bands of a single-resolution or two-band
    // session decide each alone.  Those of a multi-band session decide together: when ANY band would defer, EVERY band's frame
    // launch only scatters and one kernel finalises all bands' rows - K + 1 launches, not up to 2 K.
    bool together() const { return kind == kLiveMultiBand; }
    bool defers(int k, int frames, int inline_max) const {
        if (frames > inline_max) return true;
        for (int i = together() ? 0 : k; i < (together() ? bands : k + 1); ++i)
            if (b[i].n < 2048) return true;
        return false;
    }
    // the session was opened with these bands (sizes and row ranges)
    bool same_bands(const BandPlan& p) const {
        if (p.bands != bands) return false;
        for (int k = 0; k < bands; ++k)
            if (p.n[k] != b[k].n || p.lo[k] != b[k].lo || p.hi[k] != b[k].hi) return false;
        return true;
    }
};

// a: an accepted call (the ABI's shape and split checks passed)
inline LiveSession live_session(const LiveAsk& a) {
    LiveSession m;
    m.g = live_geometry(a.S, a.p.n[0], a.hop, a.reassign, a.form);
    m.kind = a.kind;
    m.bands = a.p.bands;
    // Band k's frames run 2 shift ahead and its ring is indexed by the emitted column.  A call that feeds long frames
    // j .. j + m - 1 finds emitted columns >= j - D unfinalised, and the band's last frame, j + m - 1 + 2 shift = emitted column
    // j + m - 1 + shift, adds up to D_k columns further: m + shift + D + D_k columns are live at once (reassign on:
    // D = D_k + shift, i.e. m + 2 shift + 2 D_k).
    for (int k = 0; k < m.bands; ++k) {
        LiveBand& b = m.b[k];
        b.n = a.p.n[k]; b.lo = a.p.lo[k]; b.hi = a.p.hi[k];
        b.shift = (a.p.n[0] - b.n) / (2 * a.hop);
        b.D = latency(b.n, a.hop, a.reassign);
        b.frame_shift = 2 * b.shift;
        b.lat_extra = m.g.D - b.D;
        b.slots = m.g.mmax + b.shift + m.g.D + b.D;
    }
    return m;
}

// Null, or why a call that asks for `a` does not fit the open session (EMSPEC_ERR_STATE, include/emspec.h): a multi-band
// session and a two-band one refuse each other's calls even at K = 2, and nothing of a session changes mid-stream.
inline const char* live_mismatch(const LiveSession& open, const LiveAsk& a) {
    if (open.kind == kLiveNone) return nullptr;
    if (open.kind != a.kind) {
        if (open.kind == kLiveMultiBand)
            return "the live session is a multi-band one (emspec_columns_multiband / emspec_push_samples_multiband); call emspec_reset() first";
        if (a.kind == kLiveMultiBand) return "the live session is not a multi-band one; call emspec_reset() before a multi-band call";
        return open.kind == kLiveTwoBand ? "the live session is a multi-resolution one (emspec_columns_multires / emspec_push_samples_multires); call emspec_reset() first"
                                         : "the live session is a single-resolution one; call emspec_reset() before a multi-resolution call";
    }
    const LiveGeometry& g = open.g;
    if (a.S == g.S && a.hop == g.hop && a.reassign == g.reassign && a.form == g.form && open.same_bands(a.p)) return nullptr;
    return a.kind == kLiveMultiBand ? "streams / bands / fft sizes / split rows / hop / reassign / feeding mode changed mid-stream; call emspec_reset() first"
           : a.kind == kLiveTwoBand ? "streams / fft sizes / hop / split row / reassign / feeding mode changed mid-stream; call emspec_reset() first"
                                    : "streams / fft size / hop / reassign / feeding mode changed mid-stream; call emspec_reset() first";
}

// ---- the launches of one call's round, in order (emspec_live.cpp: live_launch runs them; nothing else decides a launch) ----
// mlaunch: the most frames any stream has in the round (0: it only moves samples into the sample rings); flush: no frames, one
// pending column per stream; priming: some stream's first frame.  Only launches that reach the device are listed.
enum LiveStepKind { kStepFrames = 0, kStepFinalize, kStepFinalizeBands };
struct LiveStep {
    int what = kStepFrames;
    int band = 0;           // kStepFrames, kStepFinalize: the band
    int groups = 0;         // kStepFrames: workgroups per stream without the ingest workgroup
    int ncol = 0;           // the finalizes: columns per stream, at most
    bool defer = false;     // kStepFrames: the launch only scatters; a finalize step follows unless no stream has a frame
    bool ingest = false;    // kStepFrames: carries the ingest workgroup (band 0's)
};
struct LiveSteps {
    int count = 0;
    LiveStep step[2 * kMaxBands + 1];
    void add(int what, int band, int groups, int ncol, bool defer = false, bool ingest = false) {
        step[count++] = LiveStep{what, band, groups, ncol, defer, ingest};
    }
};
// per_band: the diagnostic build's A/B aid (EMSPEC_LIVE_FINALIZE_PER_BAND) - a multi-band session's one finalize for all bands
// as K finalizes, band after band
inline LiveSteps live_steps(const LiveSession& m, int mlaunch, bool flush, bool priming, int inline_max, bool per_band = false) {
    LiveSteps t;
    const bool joint = m.together() && !per_band;
    // the columns a launch completes are the first band's frame count for every band
    const int ncol = flush ? 1 : mlaunch;
    for (int k = 0; k < m.bands; ++k) {
        // a band behind the first: no launch when no stream has a frame (a block that only fills the sample ring: the first
        // band's ingest workgroup did that)
        if (k > 0 && !flush && mlaunch <= 0) break;
        const bool defer = !flush && m.defers(k, mlaunch, inline_max);
        if (!flush) t.add(kStepFrames, k, m.launch_frames(k, mlaunch, priming), 0, defer, k == 0);
        // each band alone: its finalize directly behind its frames; together: behind the last band's
        if ((flush || defer) && ncol > 0 && !m.together()) t.add(kStepFinalize, k, 0, ncol);
    }
    if (m.together() && (flush || m.defers(0, mlaunch, inline_max)) && ncol > 0) {
        if (joint) t.add(kStepFinalizeBands, 0, 0, ncol);
        for (int k = 0; !joint && k < m.bands; ++k) t.add(kStepFinalize, k, 0, ncol);
    }
    return t;
}

// ---- per stream: frames fed, columns emitted, samples received, samples in the device ring, samples in the staging block ----
struct LiveCounters {
    std::vector<int64_t> fed, emitted, seen, newbase;
    std::vector<int> pend;
    void open(int S) { fed.assign(S, 0); emitted.assign(S, 0); seen.assign(S, 0); newbase.assign(S, 0); pend.assign(S, 0); }
    void reset_stream(int s) { fed[s] = 0; emitted[s] = 0; seen[s] = 0; newbase[s] = 0; pend[s] = 0; }
    int streams() const { return (int)fed.size(); }
    // A flush emits columns that later frames would still have added to: the stream is at its end.
    bool flushed(int s, int D) const { return emitted[s] > std::max<int64_t>(fed[s] - D, 0); }
    bool pending(int s) const { return fed[s] > emitted[s]; }   // frames fed whose columns were not emitted yet
    bool any_pending() const {
        for (int s = 0; s < streams(); ++s)
            if (pending(s)) return true;
        return false;
    }
    // a PCM session keeps every stream's `pend` equal (the raw block is per source): that count
    int pcm_staged() const { return pend[0]; }
};

// emspec_push_columns*: the most columns a block of `count` samples completes on any stream (no session of the block form: on a
// fresh stream)
inline int64_t live_push_columns(const LiveGeometry& g, const LiveCounters& c, int64_t count, int n, int hop, int reassign) {
    const int D = latency(n, hop, reassign ? 1 : 0);
    auto cols = [&](int64_t fed, int64_t seen) {
        const int64_t after = frames_after(seen + count, n, hop);
        return (after > D ? after - D : 0) - (fed > D ? fed - D : 0);
    };
    if (g.form != 2) return cols(0, 0);
    int64_t most = 0;
    for (int s = 0; s < g.S; ++s) most = std::max(most, cols(c.fed[s], c.seen[s]));
    return most;
}

// ---- the descriptors of a launch ----
// every stream in the same state: the descriptor goes into the kernel arguments
inline bool live_uniform(const LiveStream* d, int S) {
    for (int s = 1; s < S; ++s)
        if (std::memcmp(&d[s], &d[0], sizeof(LiveStream)) != 0) return false;
    return true;
}
// multi-resolution session: some stream's first frame, i.e. its short band's first 2 shift + 1
inline bool live_priming(const LiveStream* d, int S) {
    for (int s = 0; s < S; ++s)
        if (d[s].j0 == 0 && d[s].frames > 0) return true;
    return false;
}

// ---- emspec_columns: one frame per stream ----
inline void live_frame_fill(const LiveGeometry& g, const LiveCounters& c, LiveStream* d) {
    for (int s = 0; s < g.S; ++s) d[s] = LiveStream{c.fed[s], c.fed[s] * (long long)g.hop, 1, 0, 0, 0};
}
// after the launch: out_columns[s] (may be null) = the column stream s emitted, or -1
inline void live_frame_commit(const LiveGeometry& g, LiveCounters& c, int64_t* out_columns) {
    for (int s = 0; s < g.S; ++s) {
        const int64_t col = c.fed[s] - g.D;
        c.fed[s] += 1;
        if (col >= 0) c.emitted[s] = col + 1;
        if (out_columns) out_columns[s] = col >= 0 ? col : -1;
    }
}

// ---- emspec_columns_flush: one pending column per stream ----
inline void live_flush_fill(const LiveGeometry& g, const LiveCounters& c, LiveStream* d) {
    for (int s = 0; s < g.S; ++s)   // (a stream with nothing pending emits the empty column: "column -1")
        d[s] = LiveStream{c.pending(s) ? c.emitted[s] + g.D : (long long)g.D - 1, 0, 0, 0, 0, 1};
}
inline void live_flush_commit(const LiveGeometry& g, LiveCounters& c, int64_t* out_columns) {
    for (int s = 0; s < g.S; ++s) {
        const bool has = c.pending(s);
        if (out_columns) out_columns[s] = has ? c.emitted[s] : -1;
        if (has) c.emitted[s] += 1;
    }
}

// ---- emspec_push_samples*: a block of `count` samples per stream, in rounds of at most one staging block ----
struct LivePush {
    std::vector<int64_t> produced, first, nc;   // per stream: columns so far, the first of them (-1: none), this round's
    std::vector<int> M;                         // per stream: this round's frames
    int64_t used = 0;                           // samples of the block taken so far
    int64_t take = 0;                           // this round's samples per stream
    int maxpend = 0;                            // the fullest stream's staged samples before the round (a PCM session: every stream's)
    int mx = 0;                                 // the most frames any stream has in this round
    explicit LivePush(int S) : produced(S, 0), first(S, -1), nc(S, 0), M(S, 0) {}
};
// step 1: how much of the block this round takes.  Stream s's samples are then copied to g.fresh_at(s, c.pend[s]) (a PCM
// session: source i's frames to g.raw_at(i, p.maxpend, frame bytes)) from offset p.used of its block - before step 2.
inline void live_push_take(const LiveGeometry& g, const LiveCounters& c, LivePush& p, int64_t count) {
    p.maxpend = 0;
    for (int s = 0; s < g.S; ++s) p.maxpend = std::max(p.maxpend, c.pend[s]);
    p.take = std::min<int64_t>(count - p.used, g.cap - p.maxpend);
}
// step 2: the samples are staged; the round's frames, columns and descriptors (direct: the kernel writes the caller's block, at
// the columns produced so far; else a staging block from 0).  false: no launch -
// a block that completes no frame (an audio worklet hands over 128 samples at a time) only joins the staging block: no launch,
// no synchronisation until a frame is due or the block is full.
inline bool live_push_round(const LiveGeometry& g, LiveCounters& c, LivePush& p, bool direct, LiveStream* d) {
    for (int s = 0; s < g.S; ++s) {
        c.pend[s] += (int)p.take;
        c.seen[s] += p.take;
    }
    p.used += p.take;
    p.mx = 0;
    for (int s = 0; s < g.S; ++s) {
        p.M[s] = (int)(frames_after(c.seen[s], g.n, g.hop) - c.fed[s]);
        p.mx = std::max(p.mx, p.M[s]);
    }
    if (p.mx == 0 && p.maxpend + p.take < g.cap) return false;
    for (int s = 0; s < g.S; ++s) {
        const int64_t c0 = std::max<int64_t>(c.fed[s] - g.D, 0), c1 = c.fed[s] + p.M[s] - g.D;
        p.nc[s] = c1 > c0 ? c1 - c0 : 0;
        d[s] = LiveStream{c.fed[s], c.newbase[s], p.M[s], c.pend[s], direct ? (int)p.produced[s] : 0, 0};
        if (p.nc[s] > 0 && p.first[s] < 0) p.first[s] = c0;
    }
    return true;
}
// step 3: after the launch (and after the round's columns were copied out of a staging block: p.nc[s] of them to column
// p.produced[s] of the caller's)
inline void live_push_commit(const LiveGeometry& g, LiveCounters& c, LivePush& p) {
    for (int s = 0; s < g.S; ++s) {
        c.newbase[s] = c.seen[s];
        c.pend[s] = 0;
        c.fed[s] += p.M[s];
        if (p.nc[s] > 0) { p.produced[s] += p.nc[s]; c.emitted[s] = c.fed[s] - g.D; }
    }
}

// ---- overlays of the live calls (emspec_set_live_peaks / emspec_set_live_wave; live_overlay.hip.inc) ----
// Which slot of the stream's output block the i-th column of a launch goes to (i < frames; flush form: i < flush), or -1 when
// the launch does not write it: column c = j0 - D + i; columns below 0 are not emitted - or, in the per-frame form (empty_col),
// emitted as the empty column.  The rule of live_finalize_column (live.hip.inc), shared with the overlay kernel.
EMSPEC_HD inline int live_out_slot(long long j0, int out_at, int D, int i, bool empty_col) {
    if (empty_col) return out_at + i;
    const long long below = j0 - D < 0 ? D - j0 : 0;
    return i < below ? -1 : out_at + i - (int)below;
}
// A call delivers [S][cols][rows]; beside it peaks_out[(s cols + slot) k + i] and wave_out[s cols + slot].
inline int64_t live_overlay_pair(int64_t cols, int s, int64_t slot) { return (int64_t)s * cols + slot; }
// the capacity rule: S cols per (per = k for the peaks, 1 for the envelope) pairs must fit, without overflow for any int64 cols
inline bool live_overlay_fits(int S, int64_t cols, int per, int64_t capacity) {
    if (cols <= 0 || S <= 0) return true;
    return capacity >= 0 && cols <= capacity / ((int64_t)S * per);
}
// The envelope's pair ring, per stream [wslots] pairs of 8 bytes: frame j's pair - the key-min / key-max of the hop samples
// [j hop + off, j hop + off + hop), off = n / 2 - hop / 2, all inside frame j - goes to slot j % wslots when frame j arrives and is
// read when column j is emitted, D frames later.  A launch feeds frames j0 .. j0 + M - 1 (M <= mmax) and emits columns
// j0 - D .. j0 + M - 1 - D.  Those at or above j0 belong to frames of the same launch: the emitting wave takes them from the
// samples, not from the ring, so the kernel needs no order between its waves.  The others, [j0 - D, j0), were written by
// earlier launches, and the launch's own writes [j0, j0 + M) must not land on them: D + M distinct slots, wslots >= D + mmax.
// That is also enough over time: slot j % wslots is written again by frame j + D + mmax, and the launch that brings frame j + D
// (and emits column j, at the latest) ends at frame j + D + mmax - 1 or earlier.  A flush emits columns of [fed - D, fed) from
// the ring alone.  Every slot is written before it is read (column c is only emitted after frame c was fed since the
// stream's last reset): emspec_reset_stream clears nothing.
inline int live_wave_slots(const LiveGeometry& g) { return g.D + g.mmax; }
inline size_t live_wave_ring_bytes(const LiveGeometry& g) { return (size_t)g.S * live_wave_slots(g) * 8; }
inline int live_wave_offset(const LiveGeometry& g) { return g.n / 2 - g.hop / 2; }
// the device block that holds the delivered dB while peaks are set, laid out like the launch's output: [S][cols][R] float32,
// and the page-locked staging blocks of pageable overlay outputs: [S][cols][k] and [S][cols] pairs
inline size_t live_peaks_bytes(const LiveGeometry& g, int64_t cols, int k) { return (size_t)g.S * cols * k * 8; }
inline size_t live_wave_bytes(const LiveGeometry& g, int64_t cols) { return (size_t)g.S * cols * 8; }

// ---- the live level meters (emspec_set_live_level / emspec_set_live_cross) ----
// The records of frame j - the factor-1 level record of every stream and, per pair, the cross record, over the envelope's hop
// samples - live in two more rings beside the pair ring, slot j % slots, by the same argument: slots = live_wave_slots(g).  A
// pair is the streams p views + a and p views + b of the session (emspec_window_plan.h: cross_pair_error), so the session's
// stream count must be a multiple of `views`; a stream that is not channel a of its pair writes no cross record.
constexpr int kLiveLevelRecord = 24, kLiveCrossRecord = 16;   // sizeof(emspec_level), sizeof(emspec_cross) (include/emspec.h)
// null, or why a session of S streams cannot deliver cross records of `views` streams per pair (EMSPEC_ERR_INVALID_ARG)
inline const char* live_cross_error(int S, int views) {
    if (views < 1 || S % views != 0) return "the session's streams are not a multiple of the views set with emspec_set_live_cross";
    return nullptr;
}
inline int live_cross_pairs(int S, int views) { return views >= 1 ? S / views : 0; }
// A cross record multiplies the two streams of a pair sample by sample, so channel a's wave reads channel b's samples at its
// own frame's indices: both streams must have received, staged and framed the same (emspec_reset_stream, the one call that
// moves a single stream, is refused while a cross is set; this is the check for a setting that arrives after it)
inline bool live_pairs_in_step(const LiveCounters& c, int views, int a, int b) {
    for (int p = 0; views >= 1 && (p + 1) * views <= c.streams(); ++p) {
        const int sa = p * views + a, sb = p * views + b;
        if (c.fed[sa] != c.fed[sb] || c.seen[sa] != c.seen[sb] || c.newbase[sa] != c.newbase[sb] || c.pend[sa] != c.pend[sb]) return false;
    }
    return true;
}
inline size_t live_level_ring_bytes(const LiveGeometry& g) { return (size_t)g.S * live_wave_slots(g) * kLiveLevelRecord; }
inline size_t live_cross_ring_bytes(const LiveGeometry& g, int views) {
    return (size_t)live_cross_pairs(g.S, views) * live_wave_slots(g) * kLiveCrossRecord;
}
// the caller's arrays level_out[s cols + slot] and cross_out[p cols + slot] and the page-locked staging blocks of pageable ones:
// [S][cols] and [S / views][cols] records
inline size_t live_level_bytes(const LiveGeometry& g, int64_t cols) { return (size_t)g.S * cols * kLiveLevelRecord; }
inline size_t live_cross_bytes(const LiveGeometry& g, int views, int64_t cols) {
    return (size_t)live_cross_pairs(g.S, views) * cols * kLiveCrossRecord;
}

// ---- PCM session: the staged samples into the device sample rings, no frame ----
inline void live_drain_fill(const LiveGeometry& g, const LiveCounters& c, LiveStream* d) {
    for (int s = 0; s < g.S; ++s) d[s] = LiveStream{c.fed[s], c.newbase[s], 0, c.pend[s], 0, 0};
}
inline void live_drain_commit(const LiveGeometry& g, LiveCounters& c) {
    for (int s = 0; s < g.S; ++s) { c.newbase[s] = c.seen[s]; c.pend[s] = 0; }
}

}  // namespace emspec
