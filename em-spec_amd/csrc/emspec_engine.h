// emspec_engine.h — internal: the engine object behind the C ABI (include/emspec.h), shared by
// emspec_api.cpp (engine, batch, streaming) and emspec_comm.cpp (RCCL gather of finished columns).
#pragma once
// the library is built with -fvisibility=hidden: only the C ABI of include/emspec.h is exported
#pragma GCC visibility push(default)
#include "../../include/emspec.h"
#pragma GCC visibility pop
#include "emspec_launch.h"
#include "emspec_live_plan.h"
#include "emspec_tables.h"

#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

struct emspec_engine;
namespace emspec {
struct Plan {
    int n = 0;
    // the rows this plan serves: the engine's whole table (row0 = 0, rows = cfg.rows), or a band of it for the
    // multi-resolution and multi-band batches (emspec_multiband.cpp) - h_ebin / d_ebin (/ h_ebin64, d_ebin64) are then that slice of the
    // full table, and d_tw / d_tw64 belong to the full plan of the same n
    int row0 = 0, rows = 0;
    float2* d_tw = nullptr;
    float* d_ebin = nullptr;
    std::vector<float> h_tw, h_ebin;
    std::vector<double> h_ebin64;   // the binary64 edge table (h_ebin is this one rounded once per entry)
    // EXACT mode (cfg.mode == EMSPEC_MODE_EXACT): the binary64 tables
    double2* d_tw64 = nullptr;
    double* d_ebin64 = nullptr;
};
// Live multi-stream streaming session (emspec_live.cpp; include/emspec.h: emspec_columns / emspec_push_samples_multi):
// S streams, each with its own sample position, sample ring and pending-column ring, advanced together by ONE launch per call.
// Geometry + counters (emspec_live_plan.h: their arithmetic and every buffer size) + the buffers, which outlive a reset.
struct LivePcm {   // PCM session (emspec_push_samples_pcm; form 2 only): S = sources * views streams fed from raw interleaved frames
    int views = 0;                        // 0: a float session
    emspec_pcm_format fmt{};
};
struct LiveState {
    LiveSession ss;   // the geometry: ss.g at the first band's fft size, and the bands (ss.kind == kLiveNone: no session)
    LiveCounters c;
    LivePcm pcm;
    // the bands' column rings, band k's [S][slots_k][rows_k] float32 (FAST) / u64 (EXACT)
    void* d_cells[kMaxBands] = {}; size_t cells_bytes[kMaxBands] = {};
    float* d_sring = nullptr; size_t sring_bytes = 0;   // [S][ring_mask + 1]
    unsigned* d_done = nullptr; size_t done_bytes = 0;  // [S] arrival counters ([bands][S] with several bands: one set per band)
    float* d_raw = nullptr; size_t raw_bytes = 0;       // display post-process: raw dB [S][mmax][rows]
    float* d_pstate = nullptr; size_t pstate_bytes = 0; // display post-process: [S][rows + 4] (AGC level, initialised, -, -, previous column)
    // page-locked, device-visible host buffers: descriptors [S], staging samples [S][cap], staging outputs [S][mmax][rows]
    void* h_desc = nullptr; size_t desc_bytes = 0;
    float* h_fresh = nullptr; size_t fresh_bytes = 0;
    float* h_odb = nullptr; size_t odb_bytes = 0;
    uint8_t* h_orgba = nullptr; size_t orgba_bytes = 0;
    unsigned long long* stamps = nullptr;   // diagnostic build: [S][8] page-locked, set by emspec_debug_live_stamps
    // PCM session: the staging block holds the raw frames ([sources][cap] frames, page-locked; the decode kernel reads it in
    // place) and the frame kernels read the decoded block on the device.  Every stream of the session has the same `pend`.
    uint8_t* h_raw = nullptr; size_t hraw_bytes = 0;     // [S / pcm.views][cap] frames
    float* d_fresh = nullptr; size_t dfresh_bytes = 0;   // [S][cap] decoded samples
    // overlays (emspec_set_live_peaks / emspec_set_live_wave; live_overlay.hip.inc), allocated by the first launch that needs them:
    // the post-processed dB on the device while peaks and the display post-process are both on (without the post-process d_raw
    // holds the delivered dB), the envelope's pair ring [S][wslots], page-locked staging of pageable outputs [S][cols][k] / [S][cols]
    float* d_pdb = nullptr; size_t pdb_bytes = 0;
    void* d_wring = nullptr; size_t wring_bytes = 0;
    void* h_opeaks = nullptr; size_t opeaks_bytes = 0;
    void* h_owave = nullptr; size_t owave_bytes = 0;
    // live level meters (emspec_set_live_level / emspec_set_live_cross), as the envelope's: the record rings [S][wslots] x 24 bytes
    // and [S / views][wslots] x 16 bytes, page-locked staging of pageable outputs [S][cols] / [S / views][cols] records
    void* d_lring = nullptr; size_t lring_bytes = 0;
    void* d_xring = nullptr; size_t xring_bytes = 0;
    void* h_olevel = nullptr; size_t olevel_bytes = 0;
    void* h_ocross = nullptr; size_t ocross_bytes = 0;
    // live history (emspec_set_live_history; live_history.hip.inc, emspec_history_plan.h), allocated by the first call of the
    // session while a history is set: the ring [S][W][rows] float32 and, for the view kernel, the columns each stream has
    // emitted [S] (written by the store kernel; the host's own count is c.emitted).  view_done: recorded behind a device view
    // on the caller's stream, waited for by the engine's stream, so that later launches do not overwrite what a view still reads
    float* d_hring = nullptr; size_t hring_bytes = 0;
    long long* d_hends = nullptr; size_t hends_bytes = 0;
    hipEvent_t view_done = nullptr;
    // live audio history (emspec_set_live_audio; live_audio.hip.inc, emspec_audio_plan.h), allocated by the first call of the
    // session while an audio history is set: the ring [S][audio_stride(W)] samples.  What a stream holds follows from the
    // counters above (audio_end).  audio_done: as view_done, behind a device view or re-analysis on the caller's stream
    uint32_t* d_aring = nullptr; size_t aring_bytes = 0;
    hipEvent_t audio_done = nullptr;
    LiveStream* desc() const { return reinterpret_cast<LiveStream*>(h_desc); }
};

// emspec_api.cpp: the plan cache and the per-shape constants handed to the kernels (their arithmetic: emspec_tables.h, as latency())
int check_shape(const emspec_engine* e, int n, int hop);
int get_plan(emspec_engine* e, int n, Plan** out);
int get_band_plan(emspec_engine* e, int n, int row0, int rows, Plan** out);   // rows [row0, row0 + rows) of the table
// columns of S device-resident streams -> dB / RGBA / index of the plan's rows, no display post-process (emspec_api.cpp)
int run_plan_columns(emspec_engine* e, const Plan& p, const float* pcm, int32_t S, int64_t L, int32_t hop, int32_t reassign,
                     int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st);
// device workspace *ptr for `per_stream` bytes per stream (+ extra): streams per chunk by the records path's budget
int grow_chunked(emspec_engine* e, void** ptr, size_t* have, size_t per_stream, size_t extra, size_t cap, int S, int* chunk_out);
// that workspace, then rc = body(s0, sc, chunk) for chunk after chunk of the S streams: sc <= chunk streams from s0 on
template <class Body>
int for_stream_chunks(emspec_engine* e, void** ptr, size_t* have, size_t per_stream, size_t extra, size_t cap, int S, Body&& body) {
    int chunk = 1, rc;
    if ((rc = grow_chunked(e, ptr, have, per_stream, extra, cap, S, &chunk))) return rc;
    for (int s0 = 0; s0 < S; s0 += chunk)
        if ((rc = body(s0, S - s0 < chunk ? S - s0 : chunk, chunk))) return rc;
    return EMSPEC_OK;
}
// emspec_api.cpp: emspec_batch_device at FULL rate whatever the engine's time reduction (the unit function of the host
// pipeline, which reduces a unit's columns itself), and the device entries' reduced form: `full` computes the full-rate dB and /
// or index columns [sc][C][rows] of streams [s0, s0 + sc) into the engine workspace, chunk after chunk of streams (grow_chunked),
// and the reduction writes the caller's [S][ceil(C / f)][rows] arrays
int batch_device_full(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign, float* db,
                      uint8_t* rgba, uint8_t* index, hipStream_t st);
using FullRun = std::function<int(int s0, int sc, float* db, uint8_t* index)>;
int reduce_streams(emspec_engine* e, int32_t S, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st, const FullRun& full);
inline int64_t reduced_columns(int64_t C, int f) { return (C + f - 1) / f; }
PlanDev plan_dev(const emspec_engine* e, const Plan& p, int hop, int reassign);
ExactPlanDev exact_plan_dev(const emspec_engine* e, const Plan& p, int hop, int reassign);
ExactDbMap exact_db_map(const emspec_engine* e, int n, const ExactPlanDev& pd);
DbMap db_map(const emspec_engine* e, int n);
bool host_pinned(const void* p);   // p is null or page-locked host memory the device can address
// emspec_host.cpp: the host-buffer path of emspec_batch, emspec_batch_packed, emspec_batch_multires, the PCM and the peaks
// entries.  S streams of L host samples -> the columns of emspec_num_columns(L, n, hop) into host arrays (out), or one wire image
// per stream (pk), or peak lists (pko), through staging sets on the device; `run` computes one unit (sc streams of `samples`
// samples, staged) on the compute stream.
struct PackedOut { uint8_t* wire; int64_t capacity; int64_t* offsets; };
// emspec_batch_peaks: instead of columns, the k loudest peaks at or above min_db of every column, [S][columns][k] (f = 1 only)
struct PeaksOut { emspec_peak* peaks; int k; float min_db; };
// emspec_batch_pcm_stereo: instead of columns, the stereo image of each source's channels a and b (views of its format) under
// `law`, [S][columns][rows] per output (any null; f = 1 only)
struct StereoHostOut { int a, b; StereoLaw law; float* level; uint8_t* index; uint8_t* pan; uint8_t* rgba; };
using HostRun = std::function<int(const float* pcm, int sc, int64_t samples, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st)>;
struct HostJob {
    const void* src = nullptr;   // float32 [S][L] - or, with `dec`, raw interleaved frames: S SOURCES of L frames
    int S = 0;
    int64_t L = 0;
    int n = 0, hop = 0;
    // the unit rule: whole streams, at least min_streams of them per unit (or all S) - or runs of a stream's columns with halo_D
    // columns on either side when the batch has too few streams
    bool whole_streams = false;
    int halo_D = 0, min_streams = 1;
    // what is delivered: exactly one of out / pk / pko / stereo (and beside it, while emspec_set_wave_out is set, the envelope of the
    // streams' samples: emspec_engine::wave_out; while emspec_set_level_out / emspec_set_cross_out are set, their level and cross
    // records: emspec_engine::level_out, cross_out)
    const emspec_out* out = nullptr;
    const PackedOut* pk = nullptr;
    const PeaksOut* pko = nullptr;
    const StereoHostOut* stereo = nullptr;   // (needs dec: a pair is the views of one source)
    // (emspec_batch_pcm, emspec_batch_pcm_packed): the copy-in stage moves the raw bytes, the decode kernel (pcm.hip.inc) fills
    // the unit's float streams in front of `run`, which then sees sc * dec->views streams, and the outputs are those of
    // S * dec->views streams
    const emspec_pcm_format* dec = nullptr;
    HostRun run;
};
int host_batch(emspec_engine* e, const HostJob& job);
// (with the engine's time reduction f > 1, `run` still computes FULL-rate columns - dB and / or index, never RGBA - into the
// unit's staging set; host_batch launches the reduction behind it and delivers ceil(columns / f) columns per stream)
// emspec_pcm.cpp: null, or what is wrong with the format (names the field); bytes per interleaved frame of a valid format
const char* pcm_format_error(const emspec_pcm_format* f);
int pcm_frame_bytes(const emspec_pcm_format& f);
// the decode kernel (pcm.hip.inc) for a valid format
hipError_t pcm_decode(const void* src, const emspec_pcm_format& f, int sources, int64_t frames, int64_t src_stride_bytes, float* out,
                      int64_t out_stride, hipStream_t st);
// emspec_multiband.cpp: what the multi-resolution batch and the multi-resolution live session accept (the rules and their messages:
// emspec_band_plan.h)
int multires_check(emspec_engine* e, int32_t S, int32_t n_low, int32_t n_high, int32_t hop, int32_t split_row);
void live_destroy(emspec_engine* e);   // emspec_live.cpp: called by emspec_destroy
void live_reset(emspec_engine* e);     // drops the live session's stream state (emspec_reset); buffers are kept
bool live_pending(const emspec_engine* e);   // some stream of either session has fed frames whose columns were not emitted yet
// emspec_history.cpp: the live history's buffers.  history_ready: the session's ring while a history is set (nothing otherwise) -
// called by every streaming call once the session's streams are known and before anything is fed; history_free: one session's
// ring; history_destroy: everything (called by live_destroy)
int history_ready(emspec_engine* e, LiveState& lv);
void history_free(LiveState& lv);
void history_destroy(emspec_engine* e);
// ... what its views share with the stereo views (emspec_stereo.cpp): the session of an EMSPEC_SESSION_* (null: neither), and
// the address the device uses for page-locked host memory aligned to `align` bytes (null: pageable, misaligned or null)
LiveState* history_session(emspec_engine* e, int32_t session);
void* pinned_view(const void* p, size_t align);
// emspec_stereo.cpp: the engine's stereo palette on the device (built at the first use: the default colour map's brightness),
// and its buffers' end (called by emspec_destroy)
int stereo_palette_ready(emspec_engine* e);
void stereo_destroy(emspec_engine* e);
// emspec_audio.cpp: the live audio history's buffers, as their history twins.  audio_store: the store kernel of one launch of
// the session, behind its other kernels (nothing while no audio history is set, and for a flush)
int audio_ready(emspec_engine* e, LiveState& lv);
void audio_free(LiveState& lv);
void audio_destroy(emspec_engine* e);
int audio_store(emspec_engine* e, LiveState& lv, const LiveSinks& ls, bool flush);
}  // namespace emspec

struct emspec_engine {
    emspec_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    // host-buffer pipeline (emspec_host.cpp): H2D and D2H copy streams beside the compute stream,
    // [in | computed | out] events per staging set, the packed images' headers in pinned host memory
    hipStream_t stream_in = nullptr, stream_out = nullptr;
    hipEvent_t pipe_ev[9] = {};
    uint8_t* h_hdr = nullptr; size_t h_hdr_bytes = 0;
    void* d_packscratch = nullptr; size_t packscratch_bytes = 0;
    std::string arch;
    mutable std::string err;
    std::map<int, emspec::Plan> plans;
    // band plans of the multi-resolution batch, keyed by (n, row0, rows): kept apart from `plans` (keyed by n only)
    std::map<std::tuple<int, int, int>, emspec::Plan> band_plans;
    std::vector<float> custom_edges_hz;   // rows+1 entries when emspec_set_row_edges_hz was called
    uint8_t* d_lut = nullptr;
    // batch workspace (generic path per-bin records; host-API staging)
    float* d_hist = nullptr;
    size_t hist_bytes = 0;
    bool exact() const { return cfg.mode == EMSPEC_MODE_EXACT; }
    // EXACT fused kernel (exact_fused_lr.hip.inc): the ring's low rows, [workgroup][slots][rl] u64; launches that use it
    // are serialised across HIP streams through xlow_event
    unsigned long long* d_xlow = nullptr;
    size_t xlow_bytes = 0;
    hipEvent_t xlow_event = nullptr;
    bool xlow_used = false;
    char* d_stage = nullptr;
    size_t stage_bytes = 0;
    // display post-process (emspec_set_display)
    float smoothing = 0.0f, agc = 0.0f;
    float* d_raw = nullptr; size_t raw_bytes = 0;      // raw dB columns of a batch
    float* d_post = nullptr; size_t post_bytes = 0;    // post-processed dB when the caller wants none
    float* d_peak = nullptr; size_t peak_bytes = 0;    // column peaks + gains
    // multi-resolution and multi-band batches (emspec_multiband.cpp): the bands' raw dB (+ the composed raw dB for the post-process)
    float* d_mres = nullptr; size_t mres_bytes = 0;
    // time reduction (emspec_set_time_reduce): the factor, and the device entries' full-rate columns of a chunk
    // of streams (dB and / or palette index), which reduce.hip.inc's kernel collapses into the caller's arrays
    int time_reduce = 1;
    char* d_full = nullptr; size_t full_bytes = 0;
    // waveform envelope (emspec_set_wave_out): the caller's pair array the host pipeline also fills, or null
    emspec_wave* wave_out = nullptr; int64_t wave_capacity = 0;
    // level meters (emspec_set_level_out / emspec_set_cross_out): the caller's record arrays the host pipeline
    // also fills, or null; cross_a / cross_b: the views of each PCM source whose products the cross records sum
    emspec_level* level_out = nullptr; int64_t level_capacity = 0;
    emspec_cross* cross_out = nullptr; int64_t cross_capacity = 0; int cross_a = 0, cross_b = 0;
    // overlays of the streaming calls (emspec_set_live_peaks / emspec_set_live_wave), for both sessions below: the caller's
    // arrays (null: off) and their capacities in pairs
    emspec_peak* live_peaks = nullptr; int64_t live_peaks_capacity = 0; int live_peaks_k = 0; float live_peaks_min_db = 0.0f;
    emspec_wave* live_wave = nullptr; int64_t live_wave_capacity = 0;
    // ... and their level meters (emspec_set_live_level / emspec_set_live_cross): capacities in records; a pair of the cross is
    // streams p live_cross_views + live_cross_a and + live_cross_b of a session
    emspec_level* live_level = nullptr; int64_t live_level_capacity = 0;
    emspec_cross* live_cross = nullptr; int64_t live_cross_capacity = 0; int live_cross_views = 1, live_cross_a = 0, live_cross_b = 0;
    // live history (emspec_set_live_history; emspec_history.cpp): W columns per stream of both sessions below (0: off), and the
    // page-locked staging blocks of a host view's pageable outputs (dB, index, RGBA)
    int64_t history_W = 0;
    void* h_view[3] = {}; size_t view_bytes[3] = {};
    // stereo image (emspec_stereo.cpp): the palette [33][256][4] on the device (null until first used or set),
    // and the page-locked staging blocks of a host stereo view's pageable outputs (level, index, pan, RGBA)
    uint8_t* d_stereo_pal = nullptr;
    void* h_sview[4] = {}; size_t sview_bytes[4] = {};
    // live audio history (emspec_set_live_audio; emspec_audio.cpp): W samples per stream of both sessions below (0: off), the
    // page-locked staging block of a host view's pageable output, and the device blocks of a re-analysis (emspec_audio_batch*):
    // the viewed samples [streams][count] and the host form's dB / RGBA / index columns
    int64_t audio_W = 0;
    void* h_aview = nullptr; size_t aview_bytes = 0;
    float* d_apcm = nullptr; size_t apcm_bytes = 0;
    void* d_aout[3] = {}; size_t aout_bytes[3] = {};
    // streaming (emspec_live.cpp): the live multi-stream session, and the single-stream calls' own (emspec_column,
    // emspec_push_samples: the same machinery with one stream); independent of each other
    emspec::LiveState live, one;
    // multi-GPU gather of finished columns (emspec_comm.cpp); opaque here so this header needs no rccl.h
    struct emspec_comm_state* comm = nullptr;
};

namespace emspec {
// records the message on the engine (or, for e == nullptr, as the thread's emspec_create error) and returns code
int fail(const emspec_engine* e, int code, const std::string& msg);
// (re)allocates *ptr to at least `want` bytes of device memory
int grow(emspec_engine* e, void** ptr, size_t* have, size_t want);
void comm_destroy(emspec_engine* e);   // emspec_comm.cpp: called by emspec_destroy
bool comm_shares_device(const emspec_engine* e);   // the engine has a communicator with other ranks (world > 1)
}  // namespace emspec

#define HIPCHK(e, call)                                                                          \
    do {                                                                                         \
        hipError_t _r = (call);                                                                  \
        if (_r != hipSuccess)                                                                    \
            return emspec::fail((e), _r == hipErrorOutOfMemory ? EMSPEC_ERR_OUT_OF_MEMORY : EMSPEC_ERR_HIP, \
                                std::string(#call) + ": " + hipGetErrorString(_r));              \
    } while (0)
