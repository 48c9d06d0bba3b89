// emspec_live.cpp — the streaming calls behind the C ABI (include/emspec.h): the live multi-stream session (emspec_columns,
// emspec_columns_flush, emspec_push_samples_multi, emspec_push_columns_multi, emspec_reset_stream, emspec_live_streams; its
// multi-resolution form emspec_columns_multires, emspec_push_samples_multires, emspec_push_columns_multires: two bands of the
// row table, each with its own fft size, frame launch and column ring, one output column - DESIGN.md §3.8) and,
// since round 6 on the same machinery with one stream, the renderer's own calls: emspec_column (= computeSpectrogramColumn),
// emspec_column_flush, emspec_push_samples, emspec_push_columns.  Two independent sessions per engine: e->live and e->one.
//
// What it serves: BASELINE.json configs[2] is "64 concurrent 48 kHz streams" and north_star's renderer call is per frame
// (computeSpectrogramColumn(audioFrame, fftSize, hop, reassign)); the reference's README.md:36 ("automatically start
// visualizing your system audio") is the live case.  With one engine per stream that is S launches + S synchronisations
// per hop on the host thread; here the S streams of one engine advance together: ONE kernel launch and ONE stream
// synchronisation per call, samples read by the kernel from page-locked host memory, finished columns written by the kernel
// into page-locked host memory (the caller's own buffers when they come from emspec_host_alloc) - no copy engine involved.
// No reference file:line exists (the reference source is private, README.md:73); SURVEY.md §8(f) row 4 is the streaming glue.
// Device side: live.hip.inc / live_launch.hip.inc.
// This file holds the HIP side only: allocations, copies, launches, synchronisations, the ABI's checks and messages.  What a
// session's buffers measure, which call fits the open session, which kernels a launch runs and which column a call's output slot
// holds - the geometry (a list of bands for every kind of session), the per-stream counters, the descriptors and the steps of
// every launch - is emspec_live_plan.h, plain integer code that tests/test_live_plan_cpu.py runs on the CPU.
#include "emspec_engine.h"
#ifdef EMSPEC_DIAG
#pragma GCC visibility push(default)
#include "../../include/emspec_debug.h"
#pragma GCC visibility pop
#endif

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace emspec;

namespace {
constexpr int kInlineFinalize = 2;   // a launch that completes more columns per stream than this finalises them in a second kernel

int pinned_grow(emspec_engine* e, void** p, size_t* have, size_t want) {
    if (*have >= want) return EMSPEC_OK;
    if (*p) { (void)hipHostFree(*p); *p = nullptr; *have = 0; }
    HIPCHK(e, hipHostMalloc(p, want, hipHostMallocDefault));
    *have = want;
    return EMSPEC_OK;
}

// the address the device uses for page-locked host memory, or null when p is not such memory
void* device_view(const void* p) {
    if (!p || !host_pinned(p)) return nullptr;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return d;
}

// drops the session; the buffers and their capacities stay
void live_forget(LiveState& lv) {
    lv.ss = LiveSession{};
    lv.c = LiveCounters{};
    lv.pcm = LivePcm{};
}

// first call of a session: every allocation, then the state.  One column ring and one set of arrival counters per band.
// pcm: a PCM session - its staging block holds raw frames (live_open_pcm), not floats.
int live_open(emspec_engine* e, LiveState& lv, const LiveAsk& ask, bool pcm = false) {
    const LiveSession ss = live_session(ask);
    const LiveGeometry& g = ss.g;
    const size_t cell = e->exact() ? 8 : 4;
    int rc;
    for (int k = 0; k < ss.bands; ++k)
        if ((rc = grow(e, &lv.d_cells[k], &lv.cells_bytes[k], ss.rings_bytes(k, cell)))) return rc;
    if (g.form == 2 && (rc = grow(e, (void**)&lv.d_sring, &lv.sring_bytes, g.sring_bytes()))) return rc;
    if ((rc = grow(e, (void**)&lv.d_done, &lv.done_bytes, ss.done_bytes()))) return rc;
    if ((rc = pinned_grow(e, &lv.h_desc, &lv.desc_bytes, g.desc_bytes()))) return rc;
    if (g.form == 2 && !pcm && (rc = pinned_grow(e, (void**)&lv.h_fresh, &lv.fresh_bytes, g.fresh_bytes()))) return rc;
    for (int k = 0; k < ss.bands; ++k) HIPCHK(e, hipMemsetAsync(lv.d_cells[k], 0, ss.rings_bytes(k, cell), e->stream));
    HIPCHK(e, hipMemsetAsync(lv.d_done, 0, ss.done_bytes(), e->stream));
    if (lv.d_pstate) HIPCHK(e, hipMemsetAsync(lv.d_pstate, 0, lv.pstate_bytes, e->stream));
    lv.ss = ss;
    lv.c.open(g.S);
    return EMSPEC_OK;
}

// (a multi-band call's shape and split rows were checked by its entry)
int live_check(emspec_engine* e, const LiveState& lv, const LiveAsk& ask, int rows) {
    const LiveGeometry& g = lv.ss.g;
    const BandPlan& p = ask.p;
    int rc = ask.kind == kLiveTwoBand ? multires_check(e, ask.S, p.n[0], p.n[1], ask.hop, p.hi[0]) : check_shape(e, p.n[0], ask.hop);
    if (rc) return rc;
    if (rows != e->cfg.rows) return fail(e, EMSPEC_ERR_INVALID_ARG, "rows does not match the engine configuration");
    if (ask.S < 1 || ask.S > 65535) return fail(e, EMSPEC_ERR_INVALID_ARG, "streams must be in 1..65535");
    if (const char* why = live_mismatch(lv.ss, ask)) return fail(e, EMSPEC_ERR_STATE, why);
    // Feeding a flushed stream again would emit its last columns a second time, holding only the new frames' energy.
    for (int s = 0; s < g.S; ++s)
        if (lv.c.flushed(s, g.D))
            return fail(e, EMSPEC_ERR_STATE, "stream " + std::to_string(s) + " was flushed: reset it (emspec_reset / emspec_reset_stream) before feeding it again");
    return EMSPEC_OK;
}

// the display post-process needs the raw columns on the device and its per-stream state
int live_post_buffers(emspec_engine* e, LiveState& lv) {
    const int R = e->cfg.rows;
    int rc;
    if ((rc = grow(e, (void**)&lv.d_raw, &lv.raw_bytes, lv.ss.g.out_bytes(R, lv.ss.g.mmax)))) return rc;
    const size_t want = lv.ss.g.S * LiveGeometry::pstate_bytes(R);
    if (lv.pstate_bytes < want) {
        if ((rc = grow(e, (void**)&lv.d_pstate, &lv.pstate_bytes, want))) return rc;
        HIPCHK(e, hipMemsetAsync(lv.d_pstate, 0, lv.pstate_bytes, e->stream));
    }
    return EMSPEC_OK;
}

// One launch of the session: the frame kernel (or, flush = true, the flush kernel) and, with the display post-process on,
// the post kernel behind it.  dst_db / dst_rgba: device-visible destinations laid out [S][out_cols][rows].
// raw_cols: an upper bound of the output slots any stream uses (out_at + the columns it emits): the stride of the raw block - the
// caller's max_columns may be far larger than what a call completes.
// dst_peaks / dst_wave: the overlays' device-visible destinations ([S][out_cols][k] and [S][out_cols] pairs; null: off) - the
// overlay kernel goes behind the launch's last kernel.  While peaks are wanted the delivered dB goes to a device block laid out
// like the destination (d_raw, or d_pdb behind the post kernel) and the overlay kernel writes dst_db from its copy of it.
// dst_level / dst_cross: the level meters' destinations ([S][out_cols] and [S / views][out_cols] records; null: off), written by
// the same overlay kernel from the envelope's samples.
// While a history is set (emspec_set_live_history) the delivered dB takes the same way, and the store kernel (live_history.hip.inc)
// goes behind the launch too: it copies every delivered column into the session's ring and, without peaks, writes dst_db.
// While an audio history is set (emspec_set_live_audio) the audio store kernel (live_audio.hip.inc) goes last.
int live_launch(emspec_engine* e, LiveState& lv, const float* fresh, int64_t fresh_stride, int mlaunch, bool flush, float* dst_db,
                uint8_t* dst_rgba, int out_cols, int raw_cols, bool empty_col, emspec_peak* dst_peaks = nullptr,
                emspec_wave* dst_wave = nullptr, emspec_level* dst_level = nullptr, emspec_cross* dst_cross = nullptr) {
    int rc;
    const LiveGeometry& g = lv.ss.g;
    const int R = e->cfg.rows;
    const bool post = e->smoothing > 0.0f || e->agc > 0.0f;
    if (post && (rc = live_post_buffers(e, lv))) return rc;
    // (a launch without a frame - one that only moves samples into the ring - completes no column: no overlay)
    const bool overlay = (dst_peaks || dst_wave || dst_level || dst_cross) && (flush || mlaunch > 0), peaks = overlay && dst_peaks;
    const bool hist = e->history_W > 0 && (flush || mlaunch > 0);
    const bool devdb = peaks || hist;   // the delivered dB goes to a device block first
    if (devdb) {
        const size_t want = g.out_bytes(R, std::max(out_cols, 1));
        if (post ? (rc = grow(e, (void**)&lv.d_pdb, &lv.pdb_bytes, want)) : (rc = grow(e, (void**)&lv.d_raw, &lv.raw_bytes, want))) return rc;
    }
    if (overlay && dst_wave && (rc = grow(e, &lv.d_wring, &lv.wring_bytes, live_wave_ring_bytes(g)))) return rc;
    if (overlay && dst_level && (rc = grow(e, &lv.d_lring, &lv.lring_bytes, live_level_ring_bytes(g)))) return rc;
    if (overlay && dst_cross && (rc = grow(e, &lv.d_xring, &lv.xring_bytes, live_cross_ring_bytes(g, e->live_cross_views)))) return rc;
    LiveSinks ls;
    ls.streams = lv.desc();
    ls.fresh = fresh;
    ls.fresh_stride = fresh_stride;
    ls.sring = g.form == 2 ? lv.d_sring : nullptr;
    ls.ring_mask = g.ring_mask;
    ls.done = lv.d_done;
    ls.out_cols = out_cols;
    ls.out_rows = R;
    ls.empty_col = empty_col ? 1 : 0;
    ls.lut = reinterpret_cast<const uint32_t*>(e->d_lut);
    // every stream in the same state: the descriptor goes into the kernel arguments
    ls.uniform = live_uniform(lv.desc(), g.S) ? 1 : 0;
    ls.uni = lv.desc()[0];
#ifdef EMSPEC_DIAG
    ls.stamps = lv.stamps;
#endif
    // with the post-process the frame kernel's columns are raw dB on the device, laid out like the destination
    // (a call without outputs - a priming block - may complete more columns than its max_columns: out_cols bounds the raw
    // block's stride only where it is an output's stride)
    if (post) {
        raw_cols = std::max(1, (dst_db || dst_rgba || overlay || hist) ? std::min(raw_cols, out_cols) : raw_cols);
        if (g.out_bytes(R, raw_cols) > lv.raw_bytes && (rc = grow(e, (void**)&lv.d_raw, &lv.raw_bytes, g.out_bytes(R, raw_cols)))) return rc;
        ls.out_db = lv.d_raw;
        ls.out_rgba = nullptr;
        ls.out_cols = raw_cols;
    } else {
        ls.out_db = devdb ? lv.d_raw : dst_db;
        ls.out_rgba = reinterpret_cast<uint32_t*>(dst_rgba);
    }
    const DbMap m = db_map(e, g.n);
    const bool exact = e->exact();
    const LiveSession& ss = lv.ss;
    // band k's plan and - once a step needs them - its conversions (EXACT: xpd, xm; lo / inv_range / gate do not depend on the fft
    // size: every band indexes the palette as the batch's composition does)
    struct Band { Plan* p; DbMap bm; ExactPlanDev xpd; ExactDbMap xm; bool ready; } band[kMaxBands];
    for (int k = 0; k < ss.bands; ++k) {
        const LiveBand& b = ss.b[k];
        // (one band: the engine's own plan at n - nothing new in the plan cache)
        if ((rc = ss.bands == 1 ? get_plan(e, b.n, &band[k].p) : get_band_plan(e, b.n, b.lo, b.rows(), &band[k].p))) return rc;
        band[k].ready = false;
    }
    const auto ready = [&](int k) -> const Band& {
        Band& d = band[k];
        if (d.ready) return d;
        d.bm = db_map(e, ss.b[k].n);
        d.xpd = exact ? exact_plan_dev(e, *d.p, g.hop, g.reassign) : ExactPlanDev{};
        d.xm = exact ? exact_db_map(e, ss.b[k].n, d.xpd) : ExactDbMap{};
        d.ready = true;
        return d;
    };
    // band k's sinks: rows [lo, hi) of the output column, finalised in place (live.hip.inc: live_finalize_column) from the band's
    // own ring with the band's own arrival counters
    const auto sinks = [&](int k, bool defer) {
        const LiveBand& b = ss.b[k];
        LiveSinks bs = ls;
        bs.row0 = b.lo;
        bs.frame_shift = b.frame_shift;
        bs.col_shift = b.shift;
        bs.lat_extra = b.lat_extra;
        bs.no_ingest = k ? 1 : 0;
        bs.done = lv.d_done + (size_t)k * g.S;
        bs.defer_finalize = defer ? 1 : 0;
        return bs;
    };
#ifdef EMSPEC_DIAG
    // A/B aid (tools/live_multiband_rate.py): a multi-band session's finalize as K launches, one live_finalize_kernel per band
    static const bool per_band = [] { const char* ev = getenv("EMSPEC_LIVE_FINALIZE_PER_BAND"); return ev && ev[0] == '1'; }();
#else
    constexpr bool per_band = false;
#endif
    // the launches, in the order and with the sizes emspec_live_plan.h lists (live_steps: the rule, run on the CPU by the tests)
    const LiveSteps steps = live_steps(ss, mlaunch, flush, live_priming(lv.desc(), g.S), kInlineFinalize, per_band);
    for (int i = 0; i < steps.count; ++i) {
        const LiveStep& st = steps.step[i];
        if (st.what == kStepFinalizeBands) {
            LiveBandRings fin;
            fin.bands = ss.bands;
            for (int k = 0; k < ss.bands; ++k) {
                const Band& d = ready(k);
                fin.cells[k] = lv.d_cells[k];
                fin.slots[k] = ss.b[k].slots; fin.rows[k] = ss.b[k].rows(); fin.row0[k] = ss.b[k].lo;
                fin.m[k] = d.bm;
                fin.xm[k] = d.xm;
            }
            HIPCHK(e, launch_live_finalize_bands(exact, ls, fin, g.D, g.S, st.ncol, e->stream));
            continue;
        }
        const Band& d = ready(st.band);
        const LiveBand& b = ss.b[st.band];
        void* cells = lv.d_cells[st.band];
        if (st.what == kStepFinalize) {
            HIPCHK(e, launch_live_flush(exact, sinks(st.band, false), cells, b.slots, b.rows(), g.D, d.bm, d.xm, g.S, st.ncol, e->stream));
        } else if (exact) {
            ExactSinks xs;
            xs.hist = reinterpret_cast<unsigned long long*>(cells);
            xs.hist_slots = b.slots; xs.total_cols = INT64_MAX; xs.ring = 1;
            xs.live = sinks(st.band, st.defer);
            xs.fin_map = d.xm;
            HIPCHK(e, launch_exact_frames(b.n, d.xpd, nullptr, 0, g.S, 0, (int64_t)st.groups + 1, xs, e->stream));
        } else {
            FrameSinks sk;
            sk.hist = reinterpret_cast<float*>(cells);
            sk.hist_slots = b.slots; sk.total_cols = INT64_MAX; sk.ring = 1;
            sk.live = sinks(st.band, st.defer);
            sk.fin_map = d.bm;
            HIPCHK(e, launch_frames(b.n, plan_dev(e, *d.p, g.hop, g.reassign), nullptr, 0, g.S, 0, (int64_t)st.groups + 1, sk, e->stream));
        }
    }
    if (post) {
        ls.out_db = devdb ? lv.d_pdb : dst_db;
        ls.out_rgba = reinterpret_cast<uint32_t*>(dst_rgba);
        ls.out_cols = out_cols;
        HIPCHK(e, launch_live_post(ls, lv.d_raw, raw_cols, R, g.D, e->smoothing, e->agc, e->cfg.db_top, m, lv.d_pstate, g.S, e->stream));
    }
    if (overlay) {
        LiveOverlay ov;
        if (peaks) {
            ov.db = post ? lv.d_pdb : lv.d_raw;
            ov.peaks = reinterpret_cast<float2*>(dst_peaks);
            ov.k = e->live_peaks_k;
            ov.rows = R;
            ov.min_db = e->live_peaks_min_db;
        }
        if (dst_wave) {
            ov.wave = reinterpret_cast<uint2*>(dst_wave);
            ov.wring = reinterpret_cast<uint2*>(lv.d_wring);
        }
        if (dst_level) {
            ov.level = dst_level;
            ov.lring = static_cast<emspec_level*>(lv.d_lring);
        }
        if (dst_cross) {
            ov.cross = dst_cross;
            ov.xring = static_cast<emspec_cross*>(lv.d_xring);
            ov.views = e->live_cross_views; ov.a = e->live_cross_a; ov.b = e->live_cross_b;
        }
        if (dst_wave || dst_level || dst_cross) {   // the sample reducers' shared geometry
            ov.wslots = live_wave_slots(g);
            ov.hop = g.hop;
            ov.off = live_wave_offset(g);
        }
        ov.D = g.D;
        ls.out_db = dst_db;
        ls.out_cols = out_cols;
        HIPCHK(e, launch_live_overlay(ls, ov, g.S, flush ? 1 : mlaunch, e->stream));
    }
    if (hist) {
        LiveHistory h;
        h.db = post ? lv.d_pdb : lv.d_raw;
        h.ring = lv.d_hring;
        h.ends = lv.d_hends;
        h.W = (int)e->history_W;
        h.rows = R;
        h.D = g.D;
        h.fill_out = peaks ? 0 : 1;   // (with peaks the overlay kernel has written dst_db)
        ls.out_db = dst_db;
        ls.out_cols = out_cols;
        HIPCHK(e, launch_live_history_store(ls, h, g.S, flush ? 1 : mlaunch, e->stream));
    }
    // while an audio history is set (emspec_set_live_audio): the samples this launch moved to the device, into the session's
    // sample ring - also for a launch without a frame; a flush brings none
    if (e->audio_W > 0 && (rc = audio_store(e, lv, ls, flush))) return rc;
    return EMSPEC_OK;
}

// A failure between a launch and its synchronisation leaves the session half advanced and kernels in flight on buffers the
// caller owns: drain the stream and drop the session, so that the caller restarts from emspec_reset() semantics.
int live_abandon(emspec_engine* e, LiveState& lv, int code) {
    const std::string msg = e->err;
    (void)hipStreamSynchronize(e->stream);
    live_forget(lv);
    e->err = msg + " (stream state was reset)";
    return code;
}

// the synchronisation that ends a launch (or a round of launches), or the session with it
int live_sync(emspec_engine* e, LiveState& lv) {
    if (hipStreamSynchronize(e->stream) != hipSuccess) return live_abandon(e, lv, fail(e, EMSPEC_ERR_HIP, "hipStreamSynchronize failed"));
    return EMSPEC_OK;
}

// Where a call's kernels write: the caller's buffers when they are page-locked, else the session's page-locked staging blocks
// ([S][cols][rows] x 4 bytes each), copied back after the synchronisation.
struct LiveDest {
    float* db = nullptr;
    uint8_t* rgba = nullptr;
    bool stage_db = false, stage_rgba = false;
    bool direct = false;   // nothing is staged, and the caller's layout may be the launch's (in_place_ok)
    // the overlays (emspec_set_live_peaks / emspec_set_live_wave; null: off), as the outputs above
    emspec_peak* peaks = nullptr;
    emspec_wave* wave = nullptr;
    bool stage_peaks = false, stage_wave = false;
    // ... and the level meters (emspec_set_live_level / emspec_set_live_cross)
    emspec_level* level = nullptr;
    emspec_cross* cross = nullptr;
    bool stage_level = false, stage_cross = false;
    bool staged() const { return stage_db || stage_rgba || stage_peaks || stage_wave || stage_level || stage_cross; }
};
// (the overlay kernel stores whole pairs: a page-locked array that is not 8-byte aligned is staged like a pageable one)
void* device_view8(const void* p) { return reinterpret_cast<uintptr_t>(p) % 8 ? nullptr : device_view(p); }
// together: every given output is staged unless all of them can be written in place; otherwise each output decides for itself
int live_dest(emspec_engine* e, LiveState& lv, float* out_db, uint8_t* out_rgba, int cols, LiveDest& d, bool together = false,
              bool in_place_ok = true) {
    d.db = reinterpret_cast<float*>(device_view(out_db));
    d.rgba = reinterpret_cast<uint8_t*>(device_view(out_rgba));
    d.peaks = reinterpret_cast<emspec_peak*>(device_view8(e->live_peaks));
    d.wave = reinterpret_cast<emspec_wave*>(device_view8(e->live_wave));
    d.level = reinterpret_cast<emspec_level*>(device_view8(e->live_level));
    d.cross = reinterpret_cast<emspec_cross*>(device_view8(e->live_cross));
    d.stage_db = out_db && !d.db;
    d.stage_rgba = out_rgba && !d.rgba;
    d.stage_peaks = e->live_peaks && !d.peaks;
    d.stage_wave = e->live_wave && !d.wave;
    d.stage_level = e->live_level && !d.level;
    d.stage_cross = e->live_cross && !d.cross;
    d.direct = !d.staged() && in_place_ok;
    if (together && !d.direct) {
        d.stage_db = out_db != nullptr; d.stage_rgba = out_rgba != nullptr; d.db = nullptr; d.rgba = nullptr;
        d.stage_peaks = e->live_peaks != nullptr; d.stage_wave = e->live_wave != nullptr;
        d.stage_level = e->live_level != nullptr; d.stage_cross = e->live_cross != nullptr;
    }
    const size_t bytes = lv.ss.g.out_bytes(e->cfg.rows, cols);
    int rc;
    if (d.stage_peaks && (rc = pinned_grow(e, &lv.h_opeaks, &lv.opeaks_bytes, live_peaks_bytes(lv.ss.g, cols, e->live_peaks_k)))) return rc;
    if (d.stage_wave && (rc = pinned_grow(e, &lv.h_owave, &lv.owave_bytes, live_wave_bytes(lv.ss.g, cols)))) return rc;
    if (d.stage_peaks) d.peaks = reinterpret_cast<emspec_peak*>(lv.h_opeaks);
    if (d.stage_wave) d.wave = reinterpret_cast<emspec_wave*>(lv.h_owave);
    if (d.stage_level && (rc = pinned_grow(e, &lv.h_olevel, &lv.olevel_bytes, live_level_bytes(lv.ss.g, cols)))) return rc;
    if (d.stage_cross && (rc = pinned_grow(e, &lv.h_ocross, &lv.ocross_bytes, live_cross_bytes(lv.ss.g, e->live_cross_views, cols)))) return rc;
    if (d.stage_level) d.level = reinterpret_cast<emspec_level*>(lv.h_olevel);
    if (d.stage_cross) d.cross = reinterpret_cast<emspec_cross*>(lv.h_ocross);
    if (d.stage_db && (rc = pinned_grow(e, (void**)&lv.h_odb, &lv.odb_bytes, bytes))) return rc;
    if (d.stage_rgba && (rc = pinned_grow(e, (void**)&lv.h_orgba, &lv.orgba_bytes, bytes))) return rc;
    if (d.stage_db) d.db = lv.h_odb;
    if (d.stage_rgba) d.rgba = lv.h_orgba;
    return EMSPEC_OK;
}
// The staged columns to the caller.  p == null: one column per stream, [S][rows] (emspec_columns, the flush); else the round's
// columns of a push: p->nc[s] columns of stream s, from the front of its mmax staged columns to column p->produced[s] of its
// max_columns.
// The staged overlays go the same way - k pairs, one pair, one level record per stream and column, one cross record per pair of
// streams and column (a pair's streams are in step: channel a's counts are the pair's) - to the arrays the engine's settings name.
void live_copy_back(const emspec_engine* e, const LiveState& lv, const LiveDest& d, float* out_db, uint8_t* out_rgba, int R,
                    const LivePush* p = nullptr, int64_t max_columns = 1) {
    const int k = e->live_peaks_k;
    if (!p) {
        if (d.stage_db) std::memcpy(out_db, lv.h_odb, lv.ss.g.out_bytes(R, 1));
        if (d.stage_rgba) std::memcpy(out_rgba, lv.h_orgba, lv.ss.g.out_bytes(R, 1));
        if (d.stage_peaks) std::memcpy(e->live_peaks, lv.h_opeaks, live_peaks_bytes(lv.ss.g, 1, k));
        if (d.stage_wave) std::memcpy(e->live_wave, lv.h_owave, live_wave_bytes(lv.ss.g, 1));
        if (d.stage_level) std::memcpy(e->live_level, lv.h_olevel, live_level_bytes(lv.ss.g, 1));
        if (d.stage_cross) std::memcpy(e->live_cross, lv.h_ocross, live_cross_bytes(lv.ss.g, e->live_cross_views, 1));
        return;
    }
    for (int s = 0; s < lv.ss.g.S; ++s) {
        if (p->nc[s] <= 0) continue;
        const size_t from = LiveGeometry::out_cell(R, lv.ss.g.mmax, s, 0), to = LiveGeometry::out_cell(R, max_columns, s, p->produced[s]);
        if (d.stage_db) std::memcpy(out_db + to, lv.h_odb + from, LiveGeometry::columns_bytes(R, p->nc[s]));
        if (d.stage_rgba) std::memcpy(out_rgba + to * 4, lv.h_orgba + from * 4, LiveGeometry::columns_bytes(R, p->nc[s]));
        const int64_t pfrom = live_overlay_pair(lv.ss.g.mmax, s, 0), pto = live_overlay_pair(max_columns, s, p->produced[s]);
        if (d.stage_peaks)
            std::memcpy(e->live_peaks + pto * k, reinterpret_cast<const emspec_peak*>(lv.h_opeaks) + pfrom * k, (size_t)p->nc[s] * k * sizeof(emspec_peak));
        if (d.stage_wave)
            std::memcpy(e->live_wave + pto, reinterpret_cast<const emspec_wave*>(lv.h_owave) + pfrom, (size_t)p->nc[s] * sizeof(emspec_wave));
        if (d.stage_level)
            std::memcpy(e->live_level + pto, reinterpret_cast<const emspec_level*>(lv.h_olevel) + pfrom, (size_t)p->nc[s] * sizeof(emspec_level));
        if (d.stage_cross && s % e->live_cross_views == e->live_cross_a) {
            const int pr = s / e->live_cross_views;
            std::memcpy(e->live_cross + live_overlay_pair(max_columns, pr, p->produced[s]),
                        reinterpret_cast<const emspec_cross*>(lv.h_ocross) + live_overlay_pair(lv.ss.g.mmax, pr, 0), (size_t)p->nc[s] * sizeof(emspec_cross));
        }
    }
}
}  // namespace

namespace {
// ---- PCM session (emspec_push_samples_pcm): raw frames staged on the host, decoded on the device at launch time ----
bool pcm_same_format(const emspec_pcm_format& a, const emspec_pcm_format& b) {
    return a.sample_type == b.sample_type && a.channels == b.channels && a.views == b.views &&
           std::memcmp(a.mix, b.mix, sizeof(float) * a.views * a.channels) == 0;
}

// (behind live_open: the session's streams are sources * views)
int live_open_pcm(emspec_engine* e, LiveState& lv, const emspec_pcm_format& fmt) {
    int rc;
    if ((rc = pinned_grow(e, (void**)&lv.h_raw, &lv.hraw_bytes, lv.ss.g.raw_bytes(fmt.views, pcm_frame_bytes(fmt))))) return rc;
    if ((rc = grow(e, (void**)&lv.d_fresh, &lv.dfresh_bytes, lv.ss.g.decoded_bytes()))) return rc;
    lv.pcm = LivePcm{fmt.views, fmt};
    return EMSPEC_OK;
}

// the staged raw frames (pend of them per source) -> d_fresh, on the engine's stream in front of the frame launch
int live_decode_pending(emspec_engine* e, LiveState& lv) {
    HIPCHK(e, pcm_decode(lv.h_raw, lv.pcm.fmt, lv.ss.g.S / lv.pcm.views, lv.c.pcm_staged(), lv.ss.g.raw_stride(pcm_frame_bytes(lv.pcm.fmt)),
                         lv.d_fresh, lv.ss.g.cap, e->stream));
    return EMSPEC_OK;
}

// Moves the staged frames of a PCM session into the device sample rings without a frame (they complete none: a block that
// does is launched by the call that brings it).  emspec_reset_stream runs it first, so that the streams of a session never
// differ in what they have staged - the raw block is per source.
int live_pcm_drain(emspec_engine* e, LiveState& lv) {
    if (!lv.pcm.views || lv.c.pcm_staged() == 0) return EMSPEC_OK;
    int rc;
    live_drain_fill(lv.ss.g, lv.c, lv.desc());
    if ((rc = live_decode_pending(e, lv))) return live_abandon(e, lv, rc);
    if ((rc = live_launch(e, lv, lv.d_fresh, lv.ss.g.cap, 0, false, nullptr, nullptr, 1, 1, false))) return live_abandon(e, lv, rc);
    if ((rc = live_sync(e, lv))) return rc;
    live_drain_commit(lv.ss.g, lv.c);
    return EMSPEC_OK;
}

// ---- the calls, on one of the engine's two sessions ----

// the overlays' capacity rule: a call that delivers [S][cols][rows] writes S cols k peaks, S cols envelope pairs, S cols level
// records and (S / views) cols cross records - and a session whose streams are no multiple of `views` has no pairs
int live_overlay_check(emspec_engine* e, const LiveState& lv, int S, int64_t cols) {
    if (e->live_peaks && !live_overlay_fits(S, cols, e->live_peaks_k, e->live_peaks_capacity))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the array set with emspec_set_live_peaks is too small: the call needs streams x columns x k pairs");
    if (e->live_wave && !live_overlay_fits(S, cols, 1, e->live_wave_capacity))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the array set with emspec_set_live_wave is too small: the call needs streams x columns pairs");
    if (e->live_level && !live_overlay_fits(S, cols, 1, e->live_level_capacity))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the array set with emspec_set_live_level is too small: the call needs streams x columns records");
    if (e->live_cross) {
        if (const char* why = live_cross_error(S, e->live_cross_views)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
        // (an open session whose streams emspec_reset_stream moved apart before the setting arrived)
        if (lv.c.streams() == S && !live_pairs_in_step(lv.c, e->live_cross_views, e->live_cross_a, e->live_cross_b))
            return fail(e, EMSPEC_ERR_STATE, "the streams of a pair are out of step (emspec_reset_stream before emspec_set_live_cross); call emspec_reset() first");
        if (!live_overlay_fits(live_cross_pairs(S, e->live_cross_views), cols, 1, e->live_cross_capacity))
            return fail(e, EMSPEC_ERR_INVALID_ARG, "the array set with emspec_set_live_cross is too small: the call needs pairs x columns records");
    }
    return EMSPEC_OK;
}

// some stream of either session has frames fed: the overlays that are taken when a frame arrives (the envelope, the level and
// cross records) cannot start - their columns still to come would lack what earlier frames left
bool live_fed(const emspec_engine* e) {
    for (const LiveState* lv : {&e->live, &e->one})
        for (int s = 0; s < lv->c.streams(); ++s)
            if (lv->ss.g.form != 0 && lv->c.fed[s] > 0) return true;
    return false;
}

static_assert(sizeof(emspec_level) == kLiveLevelRecord && sizeof(emspec_cross) == kLiveCrossRecord, "the rings' record sizes (emspec_live_plan.h)");

// the time reduction (emspec_set_time_reduce) serves the batch entries only: every streaming call refuses while it is on
const char* const kNoLiveReduce = "the streaming calls return full-rate columns: not available while a time reduction is set (emspec_set_time_reduce(e, 1) turns it off)";

// (ask: the session the entry's arguments describe, form 1.  The frames are n[0] samples long; a band behind the first reads the
// newest n[k] of them - on a stream's first frame all of it, frames 0 .. 2 shift)
int columns_impl(emspec_engine* e, LiveState& lv, const float* frames, const LiveAsk& ask, float* out_db, uint8_t* out_rgba,
                 int32_t rows, int64_t* out_columns) {
    if (e && e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    if (!e || !frames) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = live_check(e, lv, ask, rows);
    if (rc) return rc;
    if ((rc = live_overlay_check(e, lv, ask.S, 1))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const bool opened = lv.ss.g.form == 0;
    if (opened && (rc = live_open(e, lv, ask))) return rc;
    if ((rc = history_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    if ((rc = audio_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    // the frames: read by the kernel where they are when the caller's block is page-locked, else staged
    const float* src = reinterpret_cast<const float*>(device_view(frames));
    if (!src) {
        if ((rc = pinned_grow(e, (void**)&lv.h_fresh, &lv.fresh_bytes, lv.ss.g.fresh_bytes()))) return rc;
        std::memcpy(lv.h_fresh, frames, lv.ss.g.fresh_bytes());
        src = lv.h_fresh;
    }
    LiveDest d;   // (one column per stream: each output in place or staged on its own)
    if ((rc = live_dest(e, lv, out_db, out_rgba, 1, d))) return rc;
    live_frame_fill(lv.ss.g, lv.c, lv.desc());
    if ((rc = live_launch(e, lv, src, lv.ss.g.n, 1, false, d.db, d.rgba, 1, 1, true, d.peaks, d.wave, d.level, d.cross))) return live_abandon(e, lv, rc);
    if ((rc = live_sync(e, lv))) return rc;
    live_copy_back(e, lv, d, out_db, out_rgba, e->cfg.rows);
    live_frame_commit(lv.ss.g, lv.c, out_columns);
    return EMSPEC_OK;
}

int flush_impl(emspec_engine* e, LiveState& lv, float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    if (rows != e->cfg.rows) return fail(e, EMSPEC_ERR_INVALID_ARG, "rows does not match the engine configuration");
    if (lv.ss.g.form == 0 || !lv.c.any_pending()) return fail(e, EMSPEC_ERR_STATE, "no pending column");
    int rc;
    if ((rc = live_overlay_check(e, lv, lv.ss.g.S, 1))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = history_ready(e, lv))) return rc;
    LiveDest d;   // (as emspec_columns; the staging blocks are sized for a push's mmax columns at once)
    if ((rc = live_dest(e, lv, out_db, out_rgba, lv.ss.g.mmax, d))) return rc;
    live_flush_fill(lv.ss.g, lv.c, lv.desc());
    if ((rc = live_launch(e, lv, nullptr, 0, 0, true, d.db, d.rgba, 1, 1, true, d.peaks, d.wave, d.level, d.cross))) return live_abandon(e, lv, rc);
    if ((rc = live_sync(e, lv))) return rc;
    live_copy_back(e, lv, d, out_db, out_rgba, e->cfg.rows);
    live_flush_commit(lv.ss.g, lv.c, out_columns);
    return EMSPEC_OK;
}

int64_t push_columns_impl(const emspec_engine* e, const LiveState& lv, int64_t count, int32_t n, int32_t hop, int32_t reassign) {
    if (!e || count < 0 || !supported_fft(n) || hop < 1 || hop > n) return -1;
    return live_push_columns(lv.ss.g, lv.c, count, n, hop, reassign);
}

// (ask: the session the entry's arguments describe, form 2.  With more than one band max_columns bounds what the block may
// complete whether or not an output is given: it is the stride of every block the launch writes)
// (fmt != null: the PCM form - `block` holds raw interleaved frames, `count` of them per source, source i at block + i * stride
// BYTES, and ask.S = sources * fmt->views; as with several bands, max_columns always bounds what a block completes)
int push_impl(emspec_engine* e, LiveState& lv, const void* block, const LiveAsk& ask, int64_t count, int64_t stride, float* out_db,
              uint8_t* out_rgba, int32_t rows, int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns,
              const emspec_pcm_format* fmt = nullptr) {
    if (e && e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    const float* samples = static_cast<const float*>(block);
    const int fb = fmt ? pcm_frame_bytes(*fmt) : 1;   // (the float form's stride counts samples)
    if (!e || (!block && count > 0) || count < 0 || stride / fb < count) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument, negative count or stride < count");
    int rc = live_check(e, lv, ask, rows);
    if (rc) return rc;
    if (lv.ss.g.form != 0 && (fmt != nullptr) != (lv.pcm.views != 0))
        return fail(e, EMSPEC_ERR_STATE, lv.pcm.views ? "the live session is a PCM one (emspec_push_samples_pcm); call emspec_reset() before a float call"
                                                      : "the live session is a float one; call emspec_reset() before a PCM call");
    if (lv.ss.g.form != 0 && fmt && !pcm_same_format(*fmt, lv.pcm.fmt))
        return fail(e, EMSPEC_ERR_STATE, "the PCM format changed mid-stream; call emspec_reset() first");
    if (max_columns < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "max_columns must be >= 0");
    const int64_t expect = push_columns_impl(e, lv, count, ask.p.n[0], ask.hop, ask.reassign);
    // (an overlay is an output too: its slots are the columns of [S][max_columns]; so is the history, whose columns pass
    // through a device block of that layout)
    if ((out_db || out_rgba || ask.p.bands > 1 || fmt || e->live_peaks || e->live_wave || e->live_level || e->live_cross || e->history_W > 0) &&
        expect > max_columns)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "output holds fewer columns than this block completes (" + std::to_string(expect) +
                                                   "); size it with emspec_push_columns() / emspec_push_columns_multi()");
    if ((rc = live_overlay_check(e, lv, ask.S, max_columns))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const bool opened = lv.ss.g.form == 0;
    if (opened) {
        if ((rc = live_open(e, lv, ask, fmt != nullptr))) return rc;
        if (fmt && (rc = live_open_pcm(e, lv, *fmt))) { live_forget(lv); return rc; }
    }
    if ((rc = history_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    if ((rc = audio_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    const LiveGeometry& g = lv.ss.g;
    // Unlike the one-column calls, a push decides for both outputs together: page-locked outputs are written in place
    // ([S][max_columns][rows], every round at the columns produced so far) only when BOTH are page-locked and max_columns fits
    // the launch's int; otherwise both go through a staging block of mmax columns per launch.  The overlays' arrays count as
    // outputs here; and while peaks or a history are set the delivered dB also lives in a device block with the launch's
    // layout, so a block of more than mmax columns is staged.
    LiveDest d;
    if ((rc = live_dest(e, lv, out_db, out_rgba, g.mmax, d, true, max_columns <= (e->live_peaks || e->history_W > 0 ? g.mmax : 0x7fffffff)))) return rc;
    LivePush p(g.S);
    bool inflight = false;
    while (p.used < count) {
        // the kernel of the previous round reads the staging block and the descriptors: wait before refilling them
        if (inflight && (rc = live_sync(e, lv))) return rc;
        inflight = false;
        live_push_take(g, lv.c, p, count);
        // (a PCM session: the raw frames of each source; every stream has the same pend - emspec_reset_stream sees to it)
        for (int i = 0; fmt && i < g.S / lv.pcm.views; ++i)
            std::memcpy(lv.h_raw + g.raw_at(i, p.maxpend, fb), static_cast<const char*>(block) + (size_t)i * stride + (size_t)p.used * fb,
                        (size_t)p.take * fb);
        for (int s = 0; !fmt && s < g.S; ++s)
            std::memcpy(lv.h_fresh + g.fresh_at(s, lv.c.pend[s]), samples + (size_t)s * stride + p.used, (size_t)p.take * 4);
        if (!live_push_round(g, lv.c, p, d.direct, lv.desc())) continue;   // no frame is due and the staging block has room
        if (fmt && (rc = live_decode_pending(e, lv))) return live_abandon(e, lv, rc);
        if ((rc = live_launch(e, lv, fmt ? lv.d_fresh : lv.h_fresh, g.cap, p.mx, false, d.db, d.rgba, d.direct ? (int)max_columns : g.mmax,
                              d.direct ? (int)std::min<int64_t>(std::max<int64_t>(expect, 1), 0x7fffffff) : g.mmax, false, d.peaks, d.wave, d.level, d.cross)))
            return live_abandon(e, lv, rc);
        inflight = true;
        if (d.staged()) {
            if ((rc = live_sync(e, lv))) return rc;
            inflight = false;
            live_copy_back(e, lv, d, out_db, out_rgba, e->cfg.rows, &p, max_columns);
        }
        live_push_commit(g, lv.c, p);
    }
    if (inflight && (rc = live_sync(e, lv))) return rc;
    for (int s = 0; s < g.S; ++s) {
        if (out_counts) out_counts[s] = p.produced[s];
        if (out_first_columns) out_first_columns[s] = p.first[s];
    }
    return EMSPEC_OK;
}

void live_free(LiveState& lv) {
    for (void* ring : lv.d_cells) (void)hipFree(ring);
    (void)hipFree(lv.d_sring);
    (void)hipFree(lv.d_done); (void)hipFree(lv.d_raw); (void)hipFree(lv.d_pstate);
    if (lv.h_desc) (void)hipHostFree(lv.h_desc);
    if (lv.h_fresh) (void)hipHostFree(lv.h_fresh);
    if (lv.h_odb) (void)hipHostFree(lv.h_odb);
    if (lv.h_orgba) (void)hipHostFree(lv.h_orgba);
    if (lv.h_raw) (void)hipHostFree(lv.h_raw);
    (void)hipFree(lv.d_fresh);
    (void)hipFree(lv.d_pdb); (void)hipFree(lv.d_wring);
    if (lv.h_opeaks) (void)hipHostFree(lv.h_opeaks);
    if (lv.h_owave) (void)hipHostFree(lv.h_owave);
    (void)hipFree(lv.d_lring); (void)hipFree(lv.d_xring);
    if (lv.h_olevel) (void)hipHostFree(lv.h_olevel);
    if (lv.h_ocross) (void)hipHostFree(lv.h_ocross);
    history_free(lv);
    audio_free(lv);
    lv = LiveState{};
}
}  // namespace

namespace emspec {
void live_destroy(emspec_engine* e) { live_free(e->live); live_free(e->one); history_destroy(e); audio_destroy(e); }
void live_reset(emspec_engine* e) { live_forget(e->live); live_forget(e->one); }
bool live_pending(const emspec_engine* e) {
    return e->live.c.any_pending() || e->one.c.any_pending();
}
}  // namespace emspec

extern "C" {

// ---- the live multi-stream session (e->live)
int32_t emspec_live_streams(const emspec_engine* e) { return e ? e->live.ss.g.S : 0; }

int emspec_columns(emspec_engine* e, const float* frames, int32_t streams, int32_t n, int32_t hop, int32_t reassign,
                   float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    return columns_impl(e, e->live, frames, live_ask_single(streams, n, hop, reassign, 1, e->cfg.rows), out_db, out_rgba, rows, out_columns);
}

int emspec_columns_flush(emspec_engine* e, float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    return flush_impl(e, e->live, out_db, out_rgba, rows, out_columns);
}

int64_t emspec_push_columns_multi(const emspec_engine* e, int64_t count, int32_t n, int32_t hop, int32_t reassign) {
    return e ? push_columns_impl(e, e->live, count, n, hop, reassign) : -1;
}

int emspec_push_samples_multi(emspec_engine* e, const float* samples, int32_t streams, int64_t count, int64_t stride,
                              int32_t n, int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                              int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    return push_impl(e, e->live, samples, live_ask_single(streams, n, hop, reassign, 2, e->cfg.rows), count, stride, out_db, out_rgba, rows,
                     max_columns, out_counts, out_first_columns);
}

// ---- the live session's multi-resolution form: rows below split_row from n_low, the rest from n_high, one
// column per hop with the latency of n_low.  emspec_columns_flush / emspec_reset_stream / emspec_live_streams serve it as above.
int emspec_columns_multires(emspec_engine* e, const float* frames, int32_t streams, int32_t n_low, int32_t n_high, int32_t hop,
                            int32_t split_row, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                            int64_t* out_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    // (a shape the batch rejects is rejected with the same words, before n_high = 0 could pass for "single resolution")
    if (const char* why = multires_shape_error(n_low, n_high, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    return columns_impl(e, e->live, frames, live_ask_two_band(streams, n_low, n_high, hop, split_row, reassign, 1, e->cfg.rows), out_db, out_rgba,
                        rows, out_columns);
}

int64_t emspec_push_columns_multires(const emspec_engine* e, int64_t count, int32_t n_low, int32_t n_high, int32_t hop,
                                     int32_t reassign) {
    if (!e || multires_shape_error(n_low, n_high, hop)) return -1;
    return push_columns_impl(e, e->live, count, n_low, hop, reassign);
}

int emspec_push_samples_multires(emspec_engine* e, const float* samples, int32_t streams, int64_t count, int64_t stride,
                                 int32_t n_low, int32_t n_high, int32_t hop, int32_t split_row, int32_t reassign, float* out_db,
                                 uint8_t* out_rgba, int32_t rows, int64_t max_columns, int64_t* out_counts,
                                 int64_t* out_first_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (const char* why = multires_shape_error(n_low, n_high, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    return push_impl(e, e->live, samples, live_ask_two_band(streams, n_low, n_high, hop, split_row, reassign, 2, e->cfg.rows), count, stride,
                     out_db, out_rgba, rows, max_columns, out_counts, out_first_columns);
}

// ---- the live session's multi-band form: 2..4 bands of the row table, band k from n[k], one column per hop with
// the latency of n[0].  emspec_columns_flush / emspec_reset_stream / emspec_live_streams and the overlays serve it as above.
// Shapes and split rows: the multi-band batch's rules and words (emspec_band_plan.h), before anything is fed.
static int multiband_entry_check(emspec_engine* e, int32_t bands, const int32_t* n, const int32_t* split_rows, int32_t hop) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    if (const char* why = band_shape_error(bands, n, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (const char* why = band_split_error(bands, split_rows, e->cfg.rows)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    return EMSPEC_OK;
}

int emspec_columns_multiband(emspec_engine* e, const float* frames, int32_t streams, int32_t bands, const int32_t* n,
                             const int32_t* split_rows, int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                             int64_t* out_columns) {
    if (int rc = multiband_entry_check(e, bands, n, split_rows, hop)) return rc;
    const BandPlan bp = band_plan(bands, n, split_rows, hop, e->cfg.rows);
    return columns_impl(e, e->live, frames, live_ask_bands(streams, bp, hop, reassign, 1), out_db, out_rgba, rows, out_columns);
}

int64_t emspec_push_columns_multiband(const emspec_engine* e, int64_t count, int32_t bands, const int32_t* n, int32_t hop,
                                      int32_t reassign) {
    if (!e || band_shape_error(bands, n, hop)) return -1;
    return push_columns_impl(e, e->live, count, n[0], hop, reassign);
}

int emspec_push_samples_multiband(emspec_engine* e, const float* samples, int32_t streams, int64_t count, int64_t stride,
                                  int32_t bands, const int32_t* n, const int32_t* split_rows, int32_t hop, int32_t reassign,
                                  float* out_db, uint8_t* out_rgba, int32_t rows, int64_t max_columns, int64_t* out_counts,
                                  int64_t* out_first_columns) {
    if (int rc = multiband_entry_check(e, bands, n, split_rows, hop)) return rc;
    const BandPlan bp = band_plan(bands, n, split_rows, hop, e->cfg.rows);
    return push_impl(e, e->live, samples, live_ask_bands(streams, bp, hop, reassign, 2), count, stride, out_db, out_rgba, rows, max_columns,
                     out_counts, out_first_columns);
}

// ---- the live session fed raw interleaved frames (include/emspec.h, PCM front end): sources * views streams
static int pcm_entry_check(emspec_engine* e, const emspec_pcm_format* fmt, int32_t sources) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (const char* why = pcm_format_error(fmt)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (sources < 1 || sources > 65535) return fail(e, EMSPEC_ERR_INVALID_ARG, "sources * views (the session's streams) must be in 1..65535");
    return EMSPEC_OK;
}

int emspec_push_samples_pcm(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources, int64_t count,
                            int64_t stride_bytes, int32_t n, int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba,
                            int32_t rows, int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns) {
    if (int rc = pcm_entry_check(e, fmt, sources)) return rc;
    return push_impl(e, e->live, block, live_ask_single(sources * fmt->views, n, hop, reassign, 2, e->cfg.rows), count, stride_bytes, out_db,
                     out_rgba, rows, max_columns, out_counts, out_first_columns, fmt);
}

int emspec_push_samples_pcm_multires(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources,
                                     int64_t count, int64_t stride_bytes, int32_t n_low, int32_t n_high, int32_t hop,
                                     int32_t split_row, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                                     int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns) {
    if (int rc = pcm_entry_check(e, fmt, sources)) return rc;
    if (const char* why = multires_shape_error(n_low, n_high, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    return push_impl(e, e->live, block, live_ask_two_band(sources * fmt->views, n_low, n_high, hop, split_row, reassign, 2, e->cfg.rows), count,
                     stride_bytes, out_db, out_rgba, rows, max_columns, out_counts, out_first_columns, fmt);
}

int emspec_push_samples_pcm_multiband(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources,
                                      int64_t count, int64_t stride_bytes, int32_t bands, const int32_t* n, const int32_t* split_rows,
                                      int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                                      int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns) {
    if (int rc = pcm_entry_check(e, fmt, sources)) return rc;
    if (int rc = multiband_entry_check(e, bands, n, split_rows, hop)) return rc;
    const BandPlan bp = band_plan(bands, n, split_rows, hop, e->cfg.rows);
    return push_impl(e, e->live, block, live_ask_bands(sources * fmt->views, bp, hop, reassign, 2), count, stride_bytes, out_db, out_rgba, rows,
                     max_columns, out_counts, out_first_columns, fmt);
}

// ---- the renderer's own calls: ONE stream, the same machinery on the engine's second session (e->one).  Until round 5
// these ran separate code: a frame copy + one to three launches per call (27.8 us, EXACT 39.7 us per emspec_column call).
int emspec_column(emspec_engine* e, const float* frame, int32_t n, int32_t hop, int32_t reassign, float* out_db,
                  uint8_t* out_rgba, int32_t rows, int64_t* out_column) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    int64_t c = -1;
    const int rc = columns_impl(e, e->one, frame, live_ask_single(1, n, hop, reassign, 1, e->cfg.rows), out_db, out_rgba, rows, &c);
    if (rc == EMSPEC_OK && out_column) *out_column = c;
    return rc;
}

int emspec_column_flush(emspec_engine* e, float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_column) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    int64_t c = -1;
    const int rc = flush_impl(e, e->one, out_db, out_rgba, rows, &c);
    if (rc == EMSPEC_OK && out_column) *out_column = c;
    return rc;
}

int64_t emspec_push_columns(const emspec_engine* e, int64_t count, int32_t n, int32_t hop, int32_t reassign) {
    return e ? push_columns_impl(e, e->one, count, n, hop, reassign) : -1;
}

int emspec_push_samples(emspec_engine* e, const float* samples, int64_t count, int32_t n, int32_t hop, int32_t reassign,
                        float* out_db, uint8_t* out_rgba, int32_t rows, int64_t max_columns, int64_t* out_count,
                        int64_t* out_first_column) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    int64_t cnt = 0, first = -1;
    const int rc = push_impl(e, e->one, samples, live_ask_single(1, n, hop, reassign, 2, e->cfg.rows), count, count, out_db, out_rgba, rows,
                             max_columns, &cnt, &first);
    if (rc == EMSPEC_OK) {
        if (out_count) *out_count = cnt;
        if (out_first_column) *out_first_column = first;
    }
    return rc;
}

#ifdef EMSPEC_DIAG
// diagnostic build (include/emspec_debug.h): where the live frame kernel stamps its phases - stamps[S][8], page-locked host
// memory of the caller (NULL: off)
int emspec_debug_live_stamps(emspec_engine* e, uint64_t* stamps) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    e->live.stamps = reinterpret_cast<unsigned long long*>(device_view(stamps));
    if (stamps && !e->live.stamps) return fail(e, EMSPEC_ERR_INVALID_ARG, "stamps must be page-locked host memory");
    return EMSPEC_OK;
}
#endif

// ---- the overlays of every streaming call above, on both sessions (live_overlay.hip.inc)
int emspec_set_live_peaks(emspec_engine* e, int32_t k, float min_db, emspec_peak* peaks_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (!peaks_out) {
        e->live_peaks = nullptr; e->live_peaks_capacity = 0; e->live_peaks_k = 0;
        return EMSPEC_OK;
    }
    if (k < 1 || k > 32) return fail(e, EMSPEC_ERR_INVALID_ARG, "k must be in 1..32");
    if (min_db != min_db) return fail(e, EMSPEC_ERR_INVALID_ARG, "min_db must not be NaN");
    if (capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the peaks' capacity must not be negative");
    const int R = e->cfg.rows;
    if (R % 4 || R < 4 || R > 4096) return fail(e, EMSPEC_ERR_INVALID_ARG, "peaks need engine rows that are a multiple of 4 in 4..4096");
    if (reinterpret_cast<uintptr_t>(peaks_out) % 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "peaks_out must be 4-byte aligned");
    e->live_peaks = peaks_out; e->live_peaks_capacity = capacity; e->live_peaks_k = k; e->live_peaks_min_db = min_db;
    return EMSPEC_OK;
}

int emspec_set_live_wave(emspec_engine* e, emspec_wave* wave_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (!wave_out) {
        e->live_wave = nullptr; e->live_wave_capacity = 0;
        return EMSPEC_OK;
    }
    if (capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the envelope's capacity must not be negative");
    if (reinterpret_cast<uintptr_t>(wave_out) % 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "wave_out must be 4-byte aligned");
    if (e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    // the pair of a column is taken when its frame arrives: a stream that already has frames has columns without a pair
    if (live_fed(e))
        return fail(e, EMSPEC_ERR_STATE, "the envelope needs the samples of every column still to come: a session has frames fed; call emspec_reset() first");
    e->live_wave = wave_out; e->live_wave_capacity = capacity;
    return EMSPEC_OK;
}

// the level meters: the envelope's rules (a column's records are taken when its frame arrives), 8-byte records
int emspec_set_live_level(emspec_engine* e, emspec_level* level_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (!level_out) {
        e->live_level = nullptr; e->live_level_capacity = 0;
        return EMSPEC_OK;
    }
    if (capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the level records' capacity must not be negative");
    if (reinterpret_cast<uintptr_t>(level_out) % 8) return fail(e, EMSPEC_ERR_INVALID_ARG, "level_out must be 8-byte aligned");
    if (e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    if (live_fed(e))
        return fail(e, EMSPEC_ERR_STATE, "the level records need the samples of every column still to come: a session has frames fed; call emspec_reset() first");
    e->live_level = level_out; e->live_level_capacity = capacity;
    return EMSPEC_OK;
}

int emspec_set_live_cross(emspec_engine* e, int32_t views, int32_t a, int32_t b, emspec_cross* cross_out, int64_t capacity) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (!cross_out) {
        e->live_cross = nullptr; e->live_cross_capacity = 0; e->live_cross_views = 1; e->live_cross_a = e->live_cross_b = 0;
        return EMSPEC_OK;
    }
    if (const char* why = cross_pair_error(0, views, a, b)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "the cross records' capacity must not be negative");
    if (reinterpret_cast<uintptr_t>(cross_out) % 8) return fail(e, EMSPEC_ERR_INVALID_ARG, "cross_out must be 8-byte aligned");
    if (e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    if (live_fed(e))
        return fail(e, EMSPEC_ERR_STATE, "the cross records need the samples of every column still to come: a session has frames fed; call emspec_reset() first");
    e->live_cross = cross_out; e->live_cross_capacity = capacity;
    e->live_cross_views = views; e->live_cross_a = a; e->live_cross_b = b;
    return EMSPEC_OK;
}

int emspec_reset_stream(emspec_engine* e, int32_t stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    LiveState& lv = e->live;
    if (lv.ss.g.form == 0) return fail(e, EMSPEC_ERR_STATE, "no live session");
    if (stream < 0 || stream >= lv.ss.g.S) return fail(e, EMSPEC_ERR_INVALID_ARG, "stream out of range");
    // a cross record multiplies the two streams of a pair sample by sample: they must stay in step
    if (e->live_cross)
        return fail(e, EMSPEC_ERR_STATE, "emspec_set_live_cross is set: the streams of a pair restart together (emspec_reset), or clear the setting first");
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = live_pcm_drain(e, lv)) return rc;
    const int R = e->cfg.rows;
    const size_t cell = e->exact() ? 8 : 4, perp = LiveGeometry::pstate_bytes(R);
    for (int k = 0; k < lv.ss.bands; ++k) {   // every band's ring
        const size_t per = lv.ss.ring_bytes(k, cell);
        HIPCHK(e, hipMemsetAsync(reinterpret_cast<char*>(lv.d_cells[k]) + stream * per, 0, per, e->stream));
    }
    if (lv.d_pstate) HIPCHK(e, hipMemsetAsync(reinterpret_cast<char*>(lv.d_pstate) + stream * perp, 0, perp, e->stream));
    lv.c.reset_stream(stream);
    return EMSPEC_OK;
}

}  // extern "C"
