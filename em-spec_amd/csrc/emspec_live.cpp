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
// session's buffers measure and which column a call's output slot holds - the geometry, the per-stream counters, the
// descriptors of every launch - is emspec_live_plan.h, plain integer code that tests/test_live_plan_cpu.py runs on the CPU.
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
    lv.g = LiveGeometry{};
    lv.c = LiveCounters{};
    lv.pcm = LivePcm{};
    lv.mb = LiveBandGeometry{};
}

// first call of a session: every allocation, then the state.  n_high != 0: a multi-resolution session (n = n_low; rows below
// `split` from n, the rest from n_high).
// pcm: a PCM session - its staging block holds raw frames (live_open_pcm), not floats.
// bp != null: a multi-band session (n = bp->n[0], n_high = 0): K rings and K sets of arrival counters, everything else that of
// the single-resolution session at n[0].
int live_open(emspec_engine* e, LiveState& lv, int S, int n, int hop, int reassign, int form, int n_high = 0, int split = 0,
              bool pcm = false, const BandPlan* bp = nullptr) {
    const LiveBandGeometry mb = bp ? live_band_geometry(S, *bp, hop, reassign, form) : LiveBandGeometry{};
    const LiveGeometry g = bp ? mb.g : live_geometry(S, n, hop, reassign, form, n_high, split);
    const int R = e->cfg.rows;
    const size_t cell = e->exact() ? 8 : 4;
    // the rings: band 0's, then those of the bands behind it (a multi-resolution session: the short band's)
    const int K = bp ? mb.bands : n_high ? 2 : 1;
    size_t ring[kMaxBands] = {g.rings_bytes(R, cell), g.rings_high_bytes(R, cell)};
    for (int k = 0; bp && k < K; ++k) ring[k] = mb.rings_bytes(k, cell);
    const size_t done = bp ? mb.done_bytes() : g.done_bytes();
    int rc;
    if ((rc = grow(e, &lv.d_cells, &lv.cells_bytes, ring[0]))) return rc;
    for (int k = 1; k < K; ++k)
        if ((rc = grow(e, &lv.d_cells_band[k - 1], &lv.cells_band_bytes[k - 1], ring[k]))) return rc;
    if (form == 2 && (rc = grow(e, (void**)&lv.d_sring, &lv.sring_bytes, g.sring_bytes()))) return rc;
    if ((rc = grow(e, (void**)&lv.d_done, &lv.done_bytes, done))) return rc;
    if ((rc = pinned_grow(e, &lv.h_desc, &lv.desc_bytes, g.desc_bytes()))) return rc;
    if (form == 2 && !pcm && (rc = pinned_grow(e, (void**)&lv.h_fresh, &lv.fresh_bytes, g.fresh_bytes()))) return rc;
    HIPCHK(e, hipMemsetAsync(lv.d_cells, 0, ring[0], e->stream));
    for (int k = 1; k < K; ++k) HIPCHK(e, hipMemsetAsync(lv.d_cells_band[k - 1], 0, ring[k], e->stream));
    HIPCHK(e, hipMemsetAsync(lv.d_done, 0, done, e->stream));
    if (lv.d_pstate) HIPCHK(e, hipMemsetAsync(lv.d_pstate, 0, lv.pstate_bytes, e->stream));
    lv.g = g;
    lv.mb = mb;
    lv.c.open(S);
    return EMSPEC_OK;
}

// (bp != null: a multi-band call - its shape and split rows were checked by the entry, n is bp->n[0] and n_high is 0)
int live_check(emspec_engine* e, const LiveState& lv, int S, int n, int hop, int reassign, int rows, int form, int n_high = 0,
               int split = 0, const BandPlan* bp = nullptr) {
    const LiveGeometry& g = lv.g;
    int rc = n_high ? multires_check(e, S, n, n_high, hop, split) : check_shape(e, n, hop);
    if (rc) return rc;
    if (rows != e->cfg.rows) return fail(e, EMSPEC_ERR_INVALID_ARG, "rows does not match the engine configuration");
    if (S < 1 || S > 65535) return fail(e, EMSPEC_ERR_INVALID_ARG, "streams must be in 1..65535");
    if (g.form != 0 && (bp != nullptr) != (lv.mb.bands != 0))
        return fail(e, EMSPEC_ERR_STATE, lv.mb.bands ? "the live session is a multi-band one (emspec_columns_multiband / emspec_push_samples_multiband); call emspec_reset() first"
                                                     : "the live session is not a multi-band one; call emspec_reset() before a multi-band call");
    if (g.form != 0 && bp && (S != g.S || hop != g.hop || reassign != g.reassign || form != g.form || !lv.mb.same_bands(*bp)))
        return fail(e, EMSPEC_ERR_STATE, "streams / bands / fft sizes / split rows / hop / reassign / feeding mode changed mid-stream; call emspec_reset() first");
    if (g.form != 0 && (n_high != 0) != (g.n_high != 0))
        return fail(e, EMSPEC_ERR_STATE, g.n_high ? "the live session is a multi-resolution one (emspec_columns_multires / emspec_push_samples_multires); call emspec_reset() first"
                                                  : "the live session is a single-resolution one; call emspec_reset() before a multi-resolution call");
    if (g.form != 0 && (S != g.S || n != g.n || hop != g.hop || reassign != g.reassign || form != g.form || n_high != g.n_high ||
                        split != g.split))
        return fail(e, EMSPEC_ERR_STATE, n_high ? "streams / fft sizes / hop / split row / reassign / feeding mode changed mid-stream; call emspec_reset() first"
                                                : "streams / fft size / hop / reassign / feeding mode changed mid-stream; call emspec_reset() first");
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
    if ((rc = grow(e, (void**)&lv.d_raw, &lv.raw_bytes, lv.g.out_bytes(R, lv.g.mmax)))) return rc;
    const size_t want = lv.g.S * LiveGeometry::pstate_bytes(R);
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
// While a history is set (emspec_set_live_history) the delivered dB takes the same way, and the store kernel (live_history.hip.inc)
// goes behind the launch too: it copies every delivered column into the session's ring and, without peaks, writes dst_db.
// While an audio history is set (emspec_set_live_audio) the audio store kernel (live_audio.hip.inc) goes last.
int live_launch(emspec_engine* e, LiveState& lv, const float* fresh, int64_t fresh_stride, int mlaunch, bool flush, float* dst_db,
                uint8_t* dst_rgba, int out_cols, int raw_cols, bool empty_col, emspec_peak* dst_peaks = nullptr,
                emspec_wave* dst_wave = nullptr) {
    int rc;
    const LiveGeometry& g = lv.g;
    const int R = e->cfg.rows;
    const bool post = e->smoothing > 0.0f || e->agc > 0.0f;
    if (post && (rc = live_post_buffers(e, lv))) return rc;
    // (a launch without a frame - one that only moves samples into the ring - completes no column: no overlay)
    const bool overlay = (dst_peaks || dst_wave) && (flush || mlaunch > 0), peaks = overlay && dst_peaks;
    const bool hist = e->history_W > 0 && (flush || mlaunch > 0);
    const bool devdb = peaks || hist;   // the delivered dB goes to a device block first
    if (devdb) {
        const size_t want = g.out_bytes(R, std::max(out_cols, 1));
        if (post ? (rc = grow(e, (void**)&lv.d_pdb, &lv.pdb_bytes, want)) : (rc = grow(e, (void**)&lv.d_raw, &lv.raw_bytes, want))) return rc;
    }
    if (overlay && dst_wave && (rc = grow(e, &lv.d_wring, &lv.wring_bytes, live_wave_ring_bytes(g)))) return rc;
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
    const bool priming = live_priming(lv.desc(), g.S);   // multi-resolution session: the short band's first 2 shift + 1 frames
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
    // a multi-band session: its flush is one launch for all bands, and its bands defer their finalize together or not at all
    // (emspec_live_band_plan.h: defers) - to one launch of live_finalize_bands_kernel behind the last band's frames
    const LiveBandGeometry& mb = lv.mb;
    const bool bands_defer = mb.bands && !flush && mb.defers(mlaunch, kInlineFinalize);
    // One band: its frame launch (or, flush = true, the flush kernel) on rows [p.row0, p.row0 + p.rows) of the output column.
    // A single-resolution session is one band of all rows; a multi-resolution one runs the long band, then the short band,
    // each finalising its own rows of the same column in place (live.hip.inc: live_finalize_column).
    // bl: the band's sinks; frames: the largest per-stream frame count of the band in this launch.
    const auto band = [&](const Plan& p, const LiveSinks& bl, void* cells, int slots, int frames) -> int {
        const DbMap bm = db_map(e, p.n);
        const ExactPlanDev xpd = exact ? exact_plan_dev(e, p, g.hop, g.reassign) : ExactPlanDev{};
        // (lo / inv_range / gate do not depend on the fft size: both bands index the palette as the batch's composition does)
        const ExactDbMap xm = exact ? exact_db_map(e, p.n, xpd) : ExactDbMap{};
        // many columns per stream: the frame kernel only scatters and a second kernel finalises them, one workgroup per column
        // (inline they are one workgroup's serial round trips to the memory side, ~2 us per column)
        // ... and so does a small transform: its workgroup has n / 16 (EXACT: n / 8) threads, and 1024 rows through 16 threads
        // are 8 serial batches of round trips (emspec_column at N = 256: 32.6 us per call against 25.7 at N = 4096)
        const bool defer = mb.bands ? bands_defer : !flush && (mlaunch > kInlineFinalize || p.n < 2048);
        LiveSinks bs = bl;
        bs.defer_finalize = defer ? 1 : 0;
        if (flush) {
            HIPCHK(e, launch_live_flush(exact, bs, cells, slots, p.rows, g.D, bm, xm, g.S, 1, e->stream));
        } else if (exact) {
            ExactSinks xs;
            xs.hist = reinterpret_cast<unsigned long long*>(cells);
            xs.hist_slots = slots; xs.total_cols = INT64_MAX; xs.ring = 1;
            xs.live = bs;
            xs.fin_map = xm;
            HIPCHK(e, launch_exact_frames(p.n, xpd, nullptr, 0, g.S, 0, (int64_t)frames + 1, xs, e->stream));
        } else {
            FrameSinks sk;
            sk.hist = reinterpret_cast<float*>(cells);
            sk.hist_slots = slots; sk.total_cols = INT64_MAX; sk.ring = 1;
            sk.live = bs;
            sk.fin_map = bm;
            HIPCHK(e, launch_frames(p.n, plan_dev(e, p, g.hop, g.reassign), nullptr, 0, g.S, 0, (int64_t)frames + 1, sk, e->stream));
        }
        // (the columns a launch completes are the long band's frame count for either band)
        if (defer && !mb.bands) HIPCHK(e, launch_live_flush(exact, bs, cells, slots, p.rows, g.D, bm, xm, g.S, mlaunch, e->stream));
        return EMSPEC_OK;
    };
    Plan* p;
    if (mb.bands) {
        Plan* pb[kMaxBands];
        LiveBandRings fin;
        fin.bands = mb.bands;
        for (int k = 0; k < mb.bands; ++k) {
            const LiveBand& b = mb.b[k];
            if ((rc = get_band_plan(e, b.n, b.lo, b.rows(), &pb[k]))) return rc;
            fin.cells[k] = k ? lv.d_cells_band[k - 1] : lv.d_cells;
            fin.slots[k] = b.slots; fin.rows[k] = b.rows(); fin.row0[k] = b.lo;
            if (!(flush || bands_defer)) continue;   // (the conversions are the bands kernel's alone)
            fin.m[k] = db_map(e, b.n);
            if (exact) fin.xm[k] = exact_db_map(e, b.n, exact_plan_dev(e, *pb[k], g.hop, g.reassign));
        }
        // band 0's frame launch carries the ingest workgroup; the others follow without one, and not at all when no stream has
        // a frame
        for (int k = 0; !flush && k < mb.bands && (k == 0 || mlaunch > 0); ++k) {
            const LiveBand& b = mb.b[k];
            LiveSinks bs = ls;
            bs.row0 = b.lo;
            bs.frame_shift = b.frame_shift;
            bs.col_shift = b.shift;
            bs.lat_extra = b.lat_extra;
            bs.no_ingest = k ? 1 : 0;
            bs.done = lv.d_done + (size_t)k * g.S;
            if ((rc = band(*pb[k], bs, fin.cells[k], b.slots, mb.launch_frames(k, mlaunch, priming)))) return rc;
        }
        if (flush || bands_defer) {
            const int ncol = flush ? 1 : mlaunch;
#ifdef EMSPEC_DIAG
            // A/B aid (tools/live_multiband_rate.py): the K-launch form, one live_finalize_kernel per band
            static const bool per_band = [] { const char* ev = getenv("EMSPEC_LIVE_FINALIZE_PER_BAND"); return ev && ev[0] == '1'; }();
            for (int k = 0; per_band && k < mb.bands; ++k) {
                LiveSinks bs = ls;
                bs.row0 = fin.row0[k];
                HIPCHK(e, launch_live_flush(exact, bs, fin.cells[k], fin.slots[k], fin.rows[k], g.D, fin.m[k], fin.xm[k], g.S, ncol, e->stream));
            }
            if (per_band) fin.bands = 0;   // (the launcher does nothing without bands)
#endif
            HIPCHK(e, launch_live_finalize_bands(exact, ls, fin, g.D, g.S, ncol, e->stream));
        }
    } else if (!g.n_high) {
        if ((rc = get_plan(e, g.n, &p))) return rc;
        if ((rc = band(*p, ls, lv.d_cells, g.slots, mlaunch))) return rc;
    } else {
        Plan* ph;
        if ((rc = get_band_plan(e, g.n, 0, g.split, &p))) return rc;
        if ((rc = get_band_plan(e, g.n_high, g.split, R - g.split, &ph))) return rc;
        if ((rc = band(*p, ls, lv.d_cells, g.slots, mlaunch))) return rc;
        // the short band: no launch when no stream has a frame (a block that only fills the sample ring: the long band's
        // ingest workgroup did that)
        if (flush || mlaunch > 0) {
            LiveSinks hs = ls;
            hs.row0 = g.split;
            hs.frame_shift = 2 * g.shift;
            hs.col_shift = g.shift;
            hs.lat_extra = g.D - g.D_high;
            hs.no_ingest = 1;
            hs.done = lv.d_done + g.S;
            if ((rc = band(*ph, hs, lv.d_cells_band[0], g.slots_high, mlaunch + (priming ? 2 * g.shift : 0)))) return rc;
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
    d.stage_db = out_db && !d.db;
    d.stage_rgba = out_rgba && !d.rgba;
    d.stage_peaks = e->live_peaks && !d.peaks;
    d.stage_wave = e->live_wave && !d.wave;
    d.direct = !d.stage_db && !d.stage_rgba && !d.stage_peaks && !d.stage_wave && in_place_ok;
    if (together && !d.direct) {
        d.stage_db = out_db != nullptr; d.stage_rgba = out_rgba != nullptr; d.db = nullptr; d.rgba = nullptr;
        d.stage_peaks = e->live_peaks != nullptr; d.stage_wave = e->live_wave != nullptr;
    }
    const size_t bytes = lv.g.out_bytes(e->cfg.rows, cols);
    int rc;
    if (d.stage_peaks && (rc = pinned_grow(e, &lv.h_opeaks, &lv.opeaks_bytes, live_peaks_bytes(lv.g, cols, e->live_peaks_k)))) return rc;
    if (d.stage_wave && (rc = pinned_grow(e, &lv.h_owave, &lv.owave_bytes, live_wave_bytes(lv.g, cols)))) return rc;
    if (d.stage_peaks) d.peaks = reinterpret_cast<emspec_peak*>(lv.h_opeaks);
    if (d.stage_wave) d.wave = reinterpret_cast<emspec_wave*>(lv.h_owave);
    if (d.stage_db && (rc = pinned_grow(e, (void**)&lv.h_odb, &lv.odb_bytes, bytes))) return rc;
    if (d.stage_rgba && (rc = pinned_grow(e, (void**)&lv.h_orgba, &lv.orgba_bytes, bytes))) return rc;
    if (d.stage_db) d.db = lv.h_odb;
    if (d.stage_rgba) d.rgba = lv.h_orgba;
    return EMSPEC_OK;
}
// The staged columns to the caller.  p == null: one column per stream, [S][rows] (emspec_columns, the flush); else the round's
// columns of a push: p->nc[s] columns of stream s, from the front of its mmax staged columns to column p->produced[s] of its
// max_columns.
// The staged overlays go the same way, k pairs and one pair per column, to the arrays the engine's settings name.
void live_copy_back(const emspec_engine* e, const LiveState& lv, const LiveDest& d, float* out_db, uint8_t* out_rgba, int R,
                    const LivePush* p = nullptr, int64_t max_columns = 1) {
    const int k = e->live_peaks_k;
    if (!p) {
        if (d.stage_db) std::memcpy(out_db, lv.h_odb, lv.g.out_bytes(R, 1));
        if (d.stage_rgba) std::memcpy(out_rgba, lv.h_orgba, lv.g.out_bytes(R, 1));
        if (d.stage_peaks) std::memcpy(e->live_peaks, lv.h_opeaks, live_peaks_bytes(lv.g, 1, k));
        if (d.stage_wave) std::memcpy(e->live_wave, lv.h_owave, live_wave_bytes(lv.g, 1));
        return;
    }
    for (int s = 0; s < lv.g.S; ++s) {
        if (p->nc[s] <= 0) continue;
        const size_t from = LiveGeometry::out_cell(R, lv.g.mmax, s, 0), to = LiveGeometry::out_cell(R, max_columns, s, p->produced[s]);
        if (d.stage_db) std::memcpy(out_db + to, lv.h_odb + from, LiveGeometry::columns_bytes(R, p->nc[s]));
        if (d.stage_rgba) std::memcpy(out_rgba + to * 4, lv.h_orgba + from * 4, LiveGeometry::columns_bytes(R, p->nc[s]));
        const int64_t pfrom = live_overlay_pair(lv.g.mmax, s, 0), pto = live_overlay_pair(max_columns, s, p->produced[s]);
        if (d.stage_peaks)
            std::memcpy(e->live_peaks + pto * k, reinterpret_cast<const emspec_peak*>(lv.h_opeaks) + pfrom * k, (size_t)p->nc[s] * k * sizeof(emspec_peak));
        if (d.stage_wave)
            std::memcpy(e->live_wave + pto, reinterpret_cast<const emspec_wave*>(lv.h_owave) + pfrom, (size_t)p->nc[s] * sizeof(emspec_wave));
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
    if ((rc = pinned_grow(e, (void**)&lv.h_raw, &lv.hraw_bytes, lv.g.raw_bytes(fmt.views, pcm_frame_bytes(fmt))))) return rc;
    if ((rc = grow(e, (void**)&lv.d_fresh, &lv.dfresh_bytes, lv.g.decoded_bytes()))) return rc;
    lv.pcm = LivePcm{fmt.views, fmt};
    return EMSPEC_OK;
}

// the staged raw frames (pend of them per source) -> d_fresh, on the engine's stream in front of the frame launch
int live_decode_pending(emspec_engine* e, LiveState& lv) {
    HIPCHK(e, pcm_decode(lv.h_raw, lv.pcm.fmt, lv.g.S / lv.pcm.views, lv.c.pcm_staged(), lv.g.raw_stride(pcm_frame_bytes(lv.pcm.fmt)),
                         lv.d_fresh, lv.g.cap, e->stream));
    return EMSPEC_OK;
}

// Moves the staged frames of a PCM session into the device sample rings without a frame (they complete none: a block that
// does is launched by the call that brings it).  emspec_reset_stream runs it first, so that the streams of a session never
// differ in what they have staged - the raw block is per source.
int live_pcm_drain(emspec_engine* e, LiveState& lv) {
    if (!lv.pcm.views || lv.c.pcm_staged() == 0) return EMSPEC_OK;
    int rc;
    live_drain_fill(lv.g, lv.c, lv.desc());
    if ((rc = live_decode_pending(e, lv))) return live_abandon(e, lv, rc);
    if ((rc = live_launch(e, lv, lv.d_fresh, lv.g.cap, 0, false, nullptr, nullptr, 1, 1, false))) return live_abandon(e, lv, rc);
    if ((rc = live_sync(e, lv))) return rc;
    live_drain_commit(lv.g, lv.c);
    return EMSPEC_OK;
}

// ---- the calls, on one of the engine's two sessions ----

// the overlays' capacity rule: a call that delivers [S][cols][rows] writes S cols k peaks and S cols envelope pairs
int live_overlay_check(emspec_engine* e, int S, int64_t cols) {
    if (e->live_peaks && !live_overlay_fits(S, cols, e->live_peaks_k, e->live_peaks_capacity))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the array set with emspec_set_live_peaks is too small: the call needs streams x columns x k pairs");
    if (e->live_wave && !live_overlay_fits(S, cols, 1, e->live_wave_capacity))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the array set with emspec_set_live_wave is too small: the call needs streams x columns pairs");
    return EMSPEC_OK;
}

// the time reduction (emspec_set_time_reduce) serves the batch entries only: every streaming call refuses while it is on
const char* const kNoLiveReduce = "the streaming calls return full-rate columns: not available while a time reduction is set (emspec_set_time_reduce(e, 1) turns it off)";

// (n_high != 0: the multi-resolution form - n is n_low, the frames are n_low samples long and the short band reads the newest
// n_high of them; on a stream's first frame it reads all of it, frames 0 .. 2 shift.  bp != null: the multi-band form, n = n[0],
// every shorter band as that short band)
int columns_impl(emspec_engine* e, LiveState& lv, const float* frames, int32_t streams, int32_t n, int32_t hop, int32_t reassign,
                 float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns, int32_t n_high = 0, int32_t split = 0,
                 const BandPlan* bp = nullptr) {
    if (e && e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    if (!e || !frames) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    reassign = reassign ? 1 : 0;
    int rc = live_check(e, lv, streams, n, hop, reassign, rows, 1, n_high, split, bp);
    if (rc) return rc;
    if ((rc = live_overlay_check(e, streams, 1))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const bool opened = lv.g.form == 0;
    if (opened && (rc = live_open(e, lv, streams, n, hop, reassign, 1, n_high, split, false, bp))) return rc;
    if ((rc = history_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    if ((rc = audio_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    // the frames: read by the kernel where they are when the caller's block is page-locked, else staged
    const float* src = reinterpret_cast<const float*>(device_view(frames));
    if (!src) {
        if ((rc = pinned_grow(e, (void**)&lv.h_fresh, &lv.fresh_bytes, lv.g.fresh_bytes()))) return rc;
        std::memcpy(lv.h_fresh, frames, lv.g.fresh_bytes());
        src = lv.h_fresh;
    }
    LiveDest d;   // (one column per stream: each output in place or staged on its own)
    if ((rc = live_dest(e, lv, out_db, out_rgba, 1, d))) return rc;
    live_frame_fill(lv.g, lv.c, lv.desc());
    if ((rc = live_launch(e, lv, src, n, 1, false, d.db, d.rgba, 1, 1, true, d.peaks, d.wave))) return live_abandon(e, lv, rc);
    if ((rc = live_sync(e, lv))) return rc;
    live_copy_back(e, lv, d, out_db, out_rgba, e->cfg.rows);
    live_frame_commit(lv.g, lv.c, out_columns);
    return EMSPEC_OK;
}

int flush_impl(emspec_engine* e, LiveState& lv, float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    if (rows != e->cfg.rows) return fail(e, EMSPEC_ERR_INVALID_ARG, "rows does not match the engine configuration");
    if (lv.g.form == 0 || !lv.c.any_pending()) return fail(e, EMSPEC_ERR_STATE, "no pending column");
    int rc;
    if ((rc = live_overlay_check(e, lv.g.S, 1))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = history_ready(e, lv))) return rc;
    LiveDest d;   // (as emspec_columns; the staging blocks are sized for a push's mmax columns at once)
    if ((rc = live_dest(e, lv, out_db, out_rgba, lv.g.mmax, d))) return rc;
    live_flush_fill(lv.g, lv.c, lv.desc());
    if ((rc = live_launch(e, lv, nullptr, 0, 0, true, d.db, d.rgba, 1, 1, true, d.peaks, d.wave))) return live_abandon(e, lv, rc);
    if ((rc = live_sync(e, lv))) return rc;
    live_copy_back(e, lv, d, out_db, out_rgba, e->cfg.rows);
    live_flush_commit(lv.g, lv.c, out_columns);
    return EMSPEC_OK;
}

int64_t push_columns_impl(const emspec_engine* e, const LiveState& lv, int64_t count, int32_t n, int32_t hop, int32_t reassign) {
    if (!e || count < 0 || !supported_fft(n) || hop < 1 || hop > n) return -1;
    return live_push_columns(lv.g, lv.c, count, n, hop, reassign);
}

// (n_high != 0, or bp != null: the multi-resolution / multi-band form - n is n_low / n[0]; max_columns then bounds what the block may complete whether or not an
// output is given: it is the stride of every block the launch writes)
// (fmt != null: the PCM form - `block` holds raw interleaved frames, `count` of them per source, source i at block + i * stride
// BYTES, and streams = sources * fmt->views; as for the multi-resolution form, max_columns always bounds what a block completes)
int push_impl(emspec_engine* e, LiveState& lv, const void* block, int32_t streams, int64_t count, int64_t stride, int32_t n,
              int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows, int64_t max_columns,
              int64_t* out_counts, int64_t* out_first_columns, int32_t n_high = 0, int32_t split = 0,
              const emspec_pcm_format* fmt = nullptr, const BandPlan* bp = nullptr) {
    if (e && e->time_reduce > 1) return fail(e, EMSPEC_ERR_STATE, kNoLiveReduce);
    const float* samples = static_cast<const float*>(block);
    const int fb = fmt ? pcm_frame_bytes(*fmt) : 1;   // (the float form's stride counts samples)
    if (!e || (!block && count > 0) || count < 0 || stride / fb < count) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument, negative count or stride < count");
    reassign = reassign ? 1 : 0;
    int rc = live_check(e, lv, streams, n, hop, reassign, rows, 2, n_high, split, bp);
    if (rc) return rc;
    if (lv.g.form != 0 && (fmt != nullptr) != (lv.pcm.views != 0))
        return fail(e, EMSPEC_ERR_STATE, lv.pcm.views ? "the live session is a PCM one (emspec_push_samples_pcm); call emspec_reset() before a float call"
                                                      : "the live session is a float one; call emspec_reset() before a PCM call");
    if (lv.g.form != 0 && fmt && !pcm_same_format(*fmt, lv.pcm.fmt))
        return fail(e, EMSPEC_ERR_STATE, "the PCM format changed mid-stream; call emspec_reset() first");
    if (max_columns < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "max_columns must be >= 0");
    const int64_t expect = push_columns_impl(e, lv, count, n, hop, reassign);
    // (an overlay is an output too: its slots are the columns of [S][max_columns]; so is the history, whose columns pass
    // through a device block of that layout)
    if ((out_db || out_rgba || n_high || bp || fmt || e->live_peaks || e->live_wave || e->history_W > 0) && expect > max_columns)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "output holds fewer columns than this block completes (" + std::to_string(expect) +
                                                   "); size it with emspec_push_columns() / emspec_push_columns_multi()");
    if ((rc = live_overlay_check(e, streams, max_columns))) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const bool opened = lv.g.form == 0;
    if (opened) {
        if ((rc = live_open(e, lv, streams, n, hop, reassign, 2, n_high, split, fmt != nullptr, bp))) return rc;
        if (fmt && (rc = live_open_pcm(e, lv, *fmt))) { live_forget(lv); return rc; }
    }
    if ((rc = history_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    if ((rc = audio_ready(e, lv))) { if (opened) live_forget(lv); return rc; }
    const LiveGeometry& g = lv.g;
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
                              d.direct ? (int)std::min<int64_t>(std::max<int64_t>(expect, 1), 0x7fffffff) : g.mmax, false, d.peaks, d.wave)))
            return live_abandon(e, lv, rc);
        inflight = true;
        if (d.stage_db || d.stage_rgba || d.stage_peaks || d.stage_wave) {
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
    (void)hipFree(lv.d_cells); (void)hipFree(lv.d_sring);
    for (void* ring : lv.d_cells_band) (void)hipFree(ring);
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
int32_t emspec_live_streams(const emspec_engine* e) { return e ? e->live.g.S : 0; }

int emspec_columns(emspec_engine* e, const float* frames, int32_t streams, int32_t n, int32_t hop, int32_t reassign,
                   float* out_db, uint8_t* out_rgba, int32_t rows, int64_t* out_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    return columns_impl(e, e->live, frames, streams, n, hop, reassign, out_db, out_rgba, rows, out_columns);
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
    return push_impl(e, e->live, samples, streams, count, stride, n, hop, reassign, out_db, out_rgba, rows, max_columns, out_counts,
                     out_first_columns);
}

// ---- the live session's multi-resolution form: rows below split_row from n_low, the rest from n_high, one
// column per hop with the latency of n_low.  emspec_columns_flush / emspec_reset_stream / emspec_live_streams serve it as above.
int emspec_columns_multires(emspec_engine* e, const float* frames, int32_t streams, int32_t n_low, int32_t n_high, int32_t hop,
                            int32_t split_row, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                            int64_t* out_columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    // (a shape the batch rejects is rejected with the same words, before n_high = 0 could pass for "single resolution")
    if (const char* why = multires_shape_error(n_low, n_high, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    return columns_impl(e, e->live, frames, streams, n_low, hop, reassign, out_db, out_rgba, rows, out_columns, n_high, split_row);
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
    return push_impl(e, e->live, samples, streams, count, stride, n_low, hop, reassign, out_db, out_rgba, rows, max_columns,
                     out_counts, out_first_columns, n_high, split_row);
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
    return columns_impl(e, e->live, frames, streams, n[0], hop, reassign, out_db, out_rgba, rows, out_columns, 0, 0, &bp);
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
    return push_impl(e, e->live, samples, streams, count, stride, n[0], hop, reassign, out_db, out_rgba, rows, max_columns, out_counts,
                     out_first_columns, 0, 0, nullptr, &bp);
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
    return push_impl(e, e->live, block, sources * fmt->views, count, stride_bytes, n, hop, reassign, out_db, out_rgba, rows, max_columns,
                     out_counts, out_first_columns, 0, 0, fmt);
}

int emspec_push_samples_pcm_multires(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources,
                                     int64_t count, int64_t stride_bytes, int32_t n_low, int32_t n_high, int32_t hop,
                                     int32_t split_row, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                                     int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns) {
    if (int rc = pcm_entry_check(e, fmt, sources)) return rc;
    if (const char* why = multires_shape_error(n_low, n_high, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    return push_impl(e, e->live, block, sources * fmt->views, count, stride_bytes, n_low, hop, reassign, out_db, out_rgba, rows,
                     max_columns, out_counts, out_first_columns, n_high, split_row, fmt);
}

int emspec_push_samples_pcm_multiband(emspec_engine* e, const void* block, const emspec_pcm_format* fmt, int32_t sources,
                                      int64_t count, int64_t stride_bytes, int32_t bands, const int32_t* n, const int32_t* split_rows,
                                      int32_t hop, int32_t reassign, float* out_db, uint8_t* out_rgba, int32_t rows,
                                      int64_t max_columns, int64_t* out_counts, int64_t* out_first_columns) {
    if (int rc = pcm_entry_check(e, fmt, sources)) return rc;
    if (int rc = multiband_entry_check(e, bands, n, split_rows, hop)) return rc;
    const BandPlan bp = band_plan(bands, n, split_rows, hop, e->cfg.rows);
    return push_impl(e, e->live, block, sources * fmt->views, count, stride_bytes, n[0], hop, reassign, out_db, out_rgba, rows,
                     max_columns, out_counts, out_first_columns, 0, 0, fmt, &bp);
}

// ---- the renderer's own calls: ONE stream, the same machinery on the engine's second session (e->one).  Until round 5
// these ran separate code: a frame copy + one to three launches per call (27.8 us, EXACT 39.7 us per emspec_column call).
int emspec_column(emspec_engine* e, const float* frame, int32_t n, int32_t hop, int32_t reassign, float* out_db,
                  uint8_t* out_rgba, int32_t rows, int64_t* out_column) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    int64_t c = -1;
    const int rc = columns_impl(e, e->one, frame, 1, n, hop, reassign, out_db, out_rgba, rows, &c);
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
    const int rc = push_impl(e, e->one, samples, 1, count, count, n, hop, reassign, out_db, out_rgba, rows, max_columns, &cnt, &first);
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
    for (const LiveState* lv : {&e->live, &e->one})
        for (int s = 0; s < lv->c.streams(); ++s)
            if (lv->g.form != 0 && lv->c.fed[s] > 0)
                return fail(e, EMSPEC_ERR_STATE, "the envelope needs the samples of every column still to come: a session has frames fed; call emspec_reset() first");
    e->live_wave = wave_out; e->live_wave_capacity = capacity;
    return EMSPEC_OK;
}

int emspec_reset_stream(emspec_engine* e, int32_t stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    LiveState& lv = e->live;
    if (lv.g.form == 0) return fail(e, EMSPEC_ERR_STATE, "no live session");
    if (stream < 0 || stream >= lv.g.S) return fail(e, EMSPEC_ERR_INVALID_ARG, "stream out of range");
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = live_pcm_drain(e, lv)) return rc;
    const int R = e->cfg.rows;
    const size_t cell = e->exact() ? 8 : 4, perp = LiveGeometry::pstate_bytes(R);
    // every band's ring: a multi-band session's K, a multi-resolution session's two, else the one
    const int K = lv.mb.bands ? lv.mb.bands : lv.g.n_high ? 2 : 1;
    for (int k = 0; k < K; ++k) {
        const size_t per = lv.mb.bands ? lv.mb.ring_bytes(k, cell) : k ? lv.g.ring_high_bytes(R, cell) : lv.g.ring_bytes(R, cell);
        HIPCHK(e, hipMemsetAsync(reinterpret_cast<char*>(k ? lv.d_cells_band[k - 1] : lv.d_cells) + stream * per, 0, per, e->stream));
    }
    if (lv.d_pstate) HIPCHK(e, hipMemsetAsync(reinterpret_cast<char*>(lv.d_pstate) + stream * perp, 0, perp, e->stream));
    lv.c.reset_stream(stream);
    return EMSPEC_OK;
}

}  // extern "C"
