// emspec_launch.h — host-callable launchers of the HIP kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "emspec_audio_plan.h"
#include "emspec_band_plan.h"
#include "emspec_device.h"
#include "emspec_history_plan.h"
#include "emspec_live_plan.h"
#include "emspec_stereo_plan.h"
#include "emspec_window_plan.h"
#include "emspec_wire_plan.h"

namespace emspec {

// ---- live multi-stream streaming: the launch and its per-stream descriptor LiveStream are described in emspec_live_plan.h ----
struct LiveSinks {
    const LiveStream* streams = nullptr;   // [S]; null: not a live launch
    LiveStream uni{};                      // uniform != 0: every stream's descriptor (the kernel then does not read `streams`)
    int uniform = 0;
    const float* fresh = nullptr;          // [S][fresh_stride] samples the device ring does not hold yet
    long long fresh_stride = 0;
    float* sring = nullptr;                // [S][ring_mask + 1] device sample ring: absolute sample a sits at a & ring_mask
    int ring_mask = 0;
    unsigned* done = nullptr;              // [S] arrival counters, zero between launches
    float* out_db = nullptr;               // [S][out_cols][rows], or null
    uint32_t* out_rgba = nullptr;          // [S][out_cols][rows] RGBA8, or null
    int out_cols = 0;
    // band geometry (multi-resolution live session; a single-resolution launch passes 0 / rows / 0 / 0 / 0):
    // the launch's plan serves rows [row0, row0 + plan rows) of an output column of out_rows rows, and its ring is indexed by
    // the EMITTED column: frame j of the band sits on column j - col_shift, and the band runs frame_shift frames ahead of the
    // descriptors' (the long band's) frame count - frames 0 .. frame_shift all at once on a stream's first frame
    int row0 = 0, out_rows = 0;
    int frame_shift = 0;                   // 2 shift = (n_low - n_high) / hop for the short band
    int col_shift = 0;                     // shift for the short band
    int lat_extra = 0;                     // latency of the emitted column - the plan's own D (the short band: D_low - D_high)
    int no_ingest = 0;                     // the other band's launch moves the new samples into the sample ring
    int empty_col = 0;                     // per-frame form: a frame that completes no column yet emits the empty column
    int defer_finalize = 0;                // the frame kernel only scatters; live_finalize_kernel (one workgroup per column) follows
    const uint32_t* lut = nullptr;
#ifdef EMSPEC_DIAG
    unsigned long long* stamps = nullptr;  // [S][8] 100 MHz wall-clock stamps of each stream's first workgroup (tools/live_phases.py)
#endif
};

// Where frames_kernel sends its per-bin results.
struct FrameSinks {
    // parity dump (all three or none): [stream][frame][K]
    float* power = nullptr;
    int32_t* col = nullptr;
    int32_t* row = nullptr;
    // compact per-bin records for the tile-scatter kernel: [stream][frame][K] of
    // (float bits of |X_h|^2, key) with key = (dcol+32768)<<16 | row, or 0xFFFFFFFF when dropped
    uint2* records = nullptr;
    // histogram scatter (global float atomics): hist[stream][slots][rows]
    float* hist = nullptr;
    int64_t hist_slots = 0;    // slots per stream in `hist`
    int64_t total_cols = 0;    // valid absolute columns are [0,total_cols)
    int32_t ring = 0;          // !=0: slot = col % hist_slots (streaming ring), else slot = col
    int64_t col_offset = 0;    // added to the frame index to get its absolute column (streaming)
    LiveSinks live{};                 // live multi-stream launch (uses hist / hist_slots / fin_map)
    DbMap fin_map{};                  // ... its "dB + colour" stage
};

// Where the exact-mode frame kernels send their per-bin results (exact.hip.inc)
struct ExactSinks {
    // parity dump (power/col/row together, q optional): [stream][frame][K]
    double* power = nullptr;
    int32_t* col = nullptr;
    int32_t* row = nullptr;
    long long* q = nullptr;
    // per-bin records for exact_tile_scatter_kernel: [stream][frame][ex::rec_stride(n)] of the bin's fixed-point
    // energy and key = (dcol+32768)<<16 | row, or 0xFFFFFFFF when dropped
    long long* rec_q = nullptr;
    uint32_t* rec_key = nullptr;
    // histogram (global u64 atomics; the streaming ring): hist[stream][slots][rows]
    unsigned long long* hist = nullptr;
    int64_t hist_slots = 0;
    int64_t total_cols = 0;
    int32_t ring = 0;
    int64_t col_offset = 0;
    int32_t edges_lds = 1;     // set by the launcher: the binary64 edge table is staged in LDS (0: read from global memory)
    LiveSinks live{};          // live multi-stream launch (uses hist / hist_slots / fin_map)
    ExactDbMap fin_map{};
};
hipError_t launch_exact_frames(int n, const ExactPlanDev& pl, const float* pcm, int64_t L, int S, int64_t frame0,
                               int64_t nframes, const ExactSinks& sinks, hipStream_t st);
// (ebin_f32 / low / low_bytes: the plan's float32 edge table on the host and a zeroed u64 scratch of
// exact_scatter_scratch_bytes - with them a ring that does not fit LDS is walked with its sparse low rows in that scratch,
// every record read once; without them, or on an axis with > 6 % of the bins down there: 16-column tiles, records read 3x)
size_t exact_scatter_scratch_bytes(int n, const ExactPlanDev& pl, int S, int64_t C, const float* ebin_f32);
hipError_t launch_exact_tile_scatter(const long long* rec_q, const uint32_t* rec_key, int n, const ExactPlanDev& pl,
                                     const ExactDbMap& m, const uint8_t* lut, int S, int64_t C, float* db, uint8_t* rgba,
                                     uint8_t* index, hipStream_t st, const float* ebin_f32 = nullptr,
                                     unsigned long long* low = nullptr, size_t low_bytes = 0);
// EXACT mode: the kernel family that serves the plan (emspec_kernel_plan.h: exact_route, with the diagnostic build's switches) -
// the no-parking kernel with Route::rl low rows, the parking kernel, or per-bin records.  row0: the plan's first row in the
// engine's table, axis: the engine's
Route exact_route(int n, const ExactPlanDev& pl, int row0, const Axis& axis);
// EXACT mode, one kernel (exact_fused.hip.inc): N = 4096 at every hop whose u64 column ring fits in LDS
hipError_t launch_exact_fused(int n, const ExactPlanDev& pl, const ExactDbMap& m, const uint8_t* lut, const float* pcm,
                              int64_t L, int S, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st,
                              unsigned long long* stamps = nullptr, int64_t* stamp_groups = nullptr);
// EXACT mode, one kernel without parking (exact_fused_lr.hip.inc): the ring's rows >= rl in LDS beside the planes, rows < rl
// in a per-workgroup scratch in global memory (device-scope atomics only); rl is the route's.
size_t exact_fused_lr_scratch_bytes(int n, const ExactPlanDev& pl, int rl, int S, int64_t C);
hipError_t launch_exact_fused_lr(int n, const ExactPlanDev& pl, const ExactDbMap& m, const uint8_t* lut, const float* pcm,
                                 int64_t L, int S, int64_t C, int rl, unsigned long long* low, size_t low_bytes, float* db,
                                 uint8_t* rgba, uint8_t* index, hipStream_t st, unsigned long long* stamps = nullptr,
                                 int64_t* stamp_groups = nullptr);

// the device word a kernel raises when a bounded wait times out (kernels.hip: g_kernel_error); -1 if it cannot be read
int read_kernel_error(bool clear);

bool supported_fft(int n);

// One workgroup per frame: frames [frame0, frame0+nframes) of each of S streams.
hipError_t launch_frames(int n, const PlanDev& pl, const float* pcm, int64_t L, int S,
                         int64_t frame0, int64_t nframes, const FrameSinks& sinks, hipStream_t st);

// records of all C frames of S streams -> finished columns.  One workgroup per (32-column tile,
// stream): LDS histogram of the tile, frames [c0-D, c0+tile+D) streamed through it.
hipError_t launch_tile_scatter(const uint2* records, int n, const PlanDev& pl, const DbMap& m, const uint8_t* lut,
                               int S, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st);

// Fused batch path (LDS column ring): returns hipErrorNotSupported when (n,hop,rows)
// has no fused specialisation; the caller then uses launch_frames + launch_tile_scatter.
hipError_t launch_fused(int n, const PlanDev& pl, const DbMap& m, const uint8_t* lut,
                        const float* pcm, int64_t L, int S, int64_t total_cols,
                        float* db, uint8_t* rgba, uint8_t* index, hipStream_t st,
                        unsigned long long* stamps = nullptr, int64_t* stamp_groups = nullptr);
// display post-process (AGC + temporal smoothing) over finished columns, see post.hip.inc
hipError_t launch_postprocess(const float* db, float* out_db, uint8_t* rgba, uint8_t* index, int S, int64_t C, int R,
                              float sm, float agc, float db_top, const DbMap& dm, const uint8_t* lut, float* peak,
                              float* gain, hipStream_t st);
// multi-band batch, the multi-resolution batch being its two-band case (multiband.hip.inc): up to kMaxBands bands' raw dB -> the
// composed columns [S][C][R]: dB and / or palette index and RGBA (any output null).  Band k's
// plane is [S][C + 2 shift[k]][rows[k]] and serves the quads of rows from q0[k] on, up to the next band's q0; an unused slot has
// q0 = R / 4 (no quad reaches it) and any valid plane
struct BandSrc {
    const float* plane[kMaxBands];
    int shift[kMaxBands], rows[kMaxBands], q0[kMaxBands];
};
hipError_t launch_multiband_compose(const BandSrc& b, int S, int64_t C, int R, const DbMap& dm, const uint8_t* lut, float* db,
                                    uint8_t* rgba, uint8_t* index, hipStream_t st);
// live multi-stream calls (live_launch.hip.inc): flush of pending columns, display post-process of a launch's columns.
// The frame launches themselves go through launch_frames / launch_exact_frames with sinks.live set and
// nframes = (largest per-stream frame count) + 1.
// (ncol: the largest number of columns any stream emits - grid (ncol, S), one workgroup per column)
hipError_t launch_live_flush(bool exact, const LiveSinks& lv, void* cells, int slots, int rows, int D, const DbMap& m,
                             const ExactDbMap& xm, int S, int ncol, hipStream_t st);
// ... of a live multi-band session: every band's rows of each column in ONE launch (live_finalize_bands_kernel).  Band k: its ring
// [S][slots][rows], the first of its rows in the output column, and its conversion (FAST: m, EXACT: xm).  lv.row0 is not read.
struct LiveBandRings {
    int bands = 0;
    void* cells[kMaxBands] = {};
    int slots[kMaxBands] = {}, rows[kMaxBands] = {}, row0[kMaxBands] = {};
    DbMap m[kMaxBands] = {};
    ExactDbMap xm[kMaxBands] = {};
};
hipError_t launch_live_finalize_bands(bool exact, const LiveSinks& lv, const LiveBandRings& r, int D, int S, int ncol, hipStream_t st);
hipError_t launch_live_post(const LiveSinks& lv, const float* raw, int raw_cols, int rows, int D, float sm, float agc, float db_top,
                            const DbMap& dm, float* pstate, int S, hipStream_t st);
// The overlays of a live launch (live_overlay.hip.inc; emspec_set_live_peaks / _wave / _level / _cross): one kernel behind the
// launch's last kernel, on the same descriptors.  lv.out_db / lv.out_cols: the CALLER's dB destination and the stride of every
// block below; `units`: the most frames (flush form: columns) any stream has in the launch.
struct LiveOverlay {
    // spectral peaks (k == 0: off): the delivered dB on the device, [S][out_cols][rows] - the frame / flush / post kernels wrote
    // it there instead of the caller's block, which this kernel fills from its LDS copy - and peaks [S][out_cols][k] pairs
    const float* db = nullptr;
    float2* peaks = nullptr;
    int k = 0, rows = 0;
    float min_db = 0.0f;
    // waveform envelope (wave == null: off): wave [S][out_cols] pairs; the pair ring [S][wslots] (emspec_live_plan.h)
    uint2* wave = nullptr;
    uint2* wring = nullptr;
    int wslots = 0, hop = 0, off = 0;
    int D = 0;   // latency of the emitted column
    // level meters (level / cross == null: off), over the envelope's samples: level [S][out_cols] records and their ring
    // [S][wslots]; cross [S / views][out_cols] records of the streams p views + a and p views + b, their ring [S / views][wslots].
    // With either set, wslots / hop / off are read as for the envelope, and S is a multiple of views.
    emspec_level* level = nullptr;
    emspec_level* lring = nullptr;
    emspec_cross* cross = nullptr;
    emspec_cross* xring = nullptr;
    int views = 1, a = 0, b = 0;
};
hipError_t launch_live_overlay(const LiveSinks& lv, const LiveOverlay& ov, int S, int units, hipStream_t st);
// The live history (live_history.hip.inc; emspec_set_live_history; geometry: emspec_history_plan.h).  The store: one kernel
// behind the launch's last kernel, on the same descriptors, lv.out_db / lv.out_cols / units as for the overlay.
struct LiveHistory {
    const float* db = nullptr;   // the delivered dB on the device, [S][lv.out_cols][rows] (as LiveOverlay::db)
    float* ring = nullptr;       // [S][W][rows]: column c of stream s in slot c mod W
    long long* ends = nullptr;   // [S]: columns emitted so far, kept for the view kernel
    int W = 0, rows = 0;
    int D = 0;                   // latency of the emitted column
    int fill_out = 0;            // != 0: this kernel writes lv.out_db (no overlay kernel does)
};
hipError_t launch_live_history_store(const LiveSinks& lv, const LiveHistory& h, int S, int units, hipStream_t st);
// The view: groups g in [0, groups) of f columns from column `first` on, of streams [stream0, stream0 + streams) ->
// [streams][groups][rows] dB, palette index of (dB + shift) under `map` (its scale is not read), RGBA = lut[index]; any null.
struct HistoryView {
    const float* ring = nullptr;
    const long long* ends = nullptr;
    int W = 0, rows = 0, stream0 = 0;
    long long first = 0;
    int slot_first = 0;          // first mod W
    int f = 1, groups = 0;
    DbMap map{};
    float shift = 0.0f;
    const uint32_t* lut = nullptr;
    float* db = nullptr;
    uint8_t* index = nullptr;
    uint32_t* rgba = nullptr;
};
int history_view_split(int streams, int64_t groups, int rows, int f);   // waves a group's columns are cut over (1: no split)
hipError_t launch_history_view(const HistoryView& v, int streams, hipStream_t st);
// The stereo image (stereo.hip.inc; the law: emspec_stereo_plan.h).  Outputs [pairs][cells] (rgba + [4]), any of them null.
struct StereoOut {
    float* level = nullptr;
    uint8_t* index = nullptr;
    uint8_t* pan = nullptr;
    uint32_t* rgba = nullptr;
};
// The compose kernel: db [pairs * views][cells], pair p's channels in streams p views + a and p views + b; pal [33][256] RGBA.
struct StereoCompose {
    const float* db = nullptr;
    int views = 2, a = 0, b = 1;
    long long cells = 0;
    StereoLaw law{};
    const uint32_t* pal = nullptr;
    StereoOut out;
};
hipError_t launch_stereo_compose(const StereoCompose& s, int pairs, hipStream_t st);
// The stereo history view: HistoryView's groups of the rings of streams stream0 + p views + a / + b, pair p in [0, pairs) ->
// [pairs][groups][rows].
struct StereoView {
    const float* ring = nullptr;
    const long long* ends = nullptr;
    int W = 0, rows = 0, stream0 = 0;
    long long first = 0;
    int slot_first = 0;
    int f = 1, groups = 0;
    int views = 2, a = 0, b = 1;
    StereoLaw law{};
    const uint32_t* pal = nullptr;
    StereoOut out;
};
hipError_t launch_stereo_view(const StereoView& v, int pairs, hipStream_t st);
// The live audio history (live_audio.hip.inc; emspec_set_live_audio; geometry: emspec_audio_plan.h).  The store: one kernel
// behind the launch's other kernels, on the same descriptors (lv.fresh / lv.fresh_stride / lv.streams); `most`: the most
// samples any stream brings in the launch.
struct LiveAudio {
    uint32_t* ring = nullptr;    // [S][stride] samples as words: sample a of stream s in slot a mod W
    long long W = 0, stride = 0; // stride = audio_stride(W)
    int form = 0, n = 0, hop = 0;   // the session's feeding form (1 per-frame, 2 block), frame length and hop
};
hipError_t launch_live_audio_store(const LiveSinks& lv, const LiveAudio& a, int S, int64_t most, hipStream_t st);
// The view: samples [first, first + n0 + n1) of streams [stream0, stream0 + streams) -> out [streams][out_stride] words;
// slot0 = first mod W, n0 / n1 the range's runs before and behind the wrap (audio_runs).
struct AudioView {
    const uint32_t* ring = nullptr;
    long long W = 0, stride = 0;
    int stream0 = 0;
    long long slot0 = 0, n0 = 0, n1 = 0;
    uint32_t* out = nullptr;
    long long out_stride = 0;
};
hipError_t launch_audio_view(const AudioView& v, int streams, hipStream_t st);
// the gather's wire image (pack.hip.inc; its sizes and the pack workspace `scratch` of wire_scratch_bytes: emspec_wire_plan.h).
// wire_total_ptr: where in the workspace the pack leaves the image's size
uint64_t* wire_total_ptr(void* scratch, int64_t columns);
hipError_t launch_wire_pack(const uint8_t* index, int64_t columns, int rows, uint8_t* wire, void* scratch, hipStream_t st);
hipError_t launch_wire_unpack(const uint8_t* wire, int64_t columns, int rows, uint8_t* index, hipStream_t st);
// time reduction (reduce.hip.inc): groups of f consecutive columns of each stream -> one, by maximum; [S] streams of C columns
// of R cells, in_stride cells apart, -> ceil(C / f) columns, out_stride cells apart.  db_out needs db_in; idx_out and / or
// rgba_out (= LUT[reduced index]) need idx_in; what is not asked for is not read.
hipError_t launch_reduce_columns(const float* db_in, const uint8_t* idx_in, int S, int64_t C, int R, int f, size_t in_stride,
                                 size_t out_stride, const uint8_t* lut, float* db_out, uint8_t* idx_out, uint8_t* rgba_out,
                                 hipStream_t st);
// spectral peaks (peaks.hip.inc): per column of db [columns][R] the k loudest local maxima at or above min_db, loudest first, as
// (position in row units, dB) pairs into peaks [columns][k] (8 bytes each; unused slots (-1, -inf)).  R % 4 == 0, 4 <= R <= 4096,
// 1 <= k <= 32, min_db not NaN, db 16-byte and peaks 8-byte aligned; any number of columns (the grid strides, 64-bit offsets).
hipError_t launch_peaks(const float* db, int64_t columns, int R, int k, float min_db, void* peaks, hipStream_t st);
// waveform envelope (window.hip.inc): per stream (S of them, `stride` samples apart, 4-byte aligned) and group of f columns of `hop`
// samples, from `first` samples into the stream on, `cols` columns in all, the pair (lo, hi) of the group's samples in the total
// order of the floats (-0.0 < +0.0, NaN skipped, none: (+inf, -inf)) into out [S] x ceil(cols / f) pairs of 8 bytes, out_stride
// pairs apart, 8-byte aligned.  The caller guarantees first + cols * hop <= the samples a stream holds.
hipError_t launch_wave(const float* pcm, int S, int64_t stride, int64_t first, int64_t cols, int hop, int f, void* out, int64_t out_stride,
                       hipStream_t st);
// level meters (window.hip.inc): the envelope's windows - S streams `stride` samples apart, groups of f columns of `hop` samples
// from `first` on, `cols` columns - give one 24-byte level record each (sum of squares in two limbs, peak, odd count; the
// samples in units of 2^-24) into out [S] x ceil(cols / f), out_stride records apart, 8-byte aligned; launch_cross: per pair p
// of streams p views + a and p views + b one 16-byte cross record (sum of products in two limbs) into out [pairs] x ceil(cols / f).
// The caller guarantees first + cols * hop <= the samples a stream holds and f * hop <= 2^30.
hipError_t launch_level(const float* pcm, int S, int64_t stride, int64_t first, int64_t cols, int hop, int f, void* out, int64_t out_stride,
                        hipStream_t st);
hipError_t launch_cross(const float* pcm, int pairs, int views, int a, int b, int64_t stride, int64_t first, int64_t cols, int hop, int f,
                        void* out, int64_t out_stride, hipStream_t st);
// PCM front end (pcm.hip.inc): `frames` interleaved frames of `sources` sources (source i at src + i * src_stride_bytes, device
// memory or page-locked host memory, any byte offset that is a multiple of the sample size) -> float32 streams, stream
// i * views + v at out + (i * views + v) * out_stride.  sample_type: kPcmS16 .. kPcmF32 (the values of include/emspec.h's
// EMSPEC_PCM_*; emspec_pcm.cpp asserts it), 1 .. kPcmMaxChannels channels, 1 .. kPcmMaxViews views, mix [views][channels].
enum { kPcmS16 = 1, kPcmS24 = 2, kPcmS32 = 3, kPcmF32 = 4, kPcmMaxChannels = 8, kPcmMaxViews = 8 };
struct PcmMix { float w[kPcmMaxViews * kPcmMaxChannels]; };   // [view][kPcmMaxChannels]
hipError_t launch_pcm_decode(const void* src, int sample_type, int channels, int views, const float* mix, int sources, int64_t frames,
                             int64_t src_stride_bytes, float* out, int64_t out_stride, hipStream_t st);
// FAST mode: the kernel family that serves the shape (emspec_kernel_plan.h: fast_route, with the diagnostic build's switches);
// fused_supported: it is not the records path
Route fused_route(int n, int hop, int rows, int reassign);
bool fused_supported(int n, int hop, int rows, int reassign);
int device_cus();           // compute units of the current device
#ifdef EMSPEC_DIAG          // diagnostic build only (libemspec_diag.so, include/emspec_debug.h)
hipError_t launch_row_lookup_probe(const float* ebin, int rows, int log_rows, const float* kh, int64_t count, int32_t* out_hint,
                                   int32_t* out_exact, hipStream_t st);
hipError_t launch_occupy(int groups, int usec, unsigned* sink, hipStream_t st);
hipError_t launch_recip_probe(const float* d, int64_t count, float* out_short, float* out_ieee, hipStream_t st);
hipError_t launch_recip64_probe(const double* d, int64_t count, double* out_short, double* out_ieee, hipStream_t st);
#endif

}  // namespace emspec
