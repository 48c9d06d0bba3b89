// emspec_stereo.cpp — the stereo image behind the C ABI (include/emspec.h: emspec_stereo_*, emspec_make_stereo_colormap,
// emspec_set_stereo_colormap, emspec_batch_stereo_device, emspec_batch_pcm_stereo, emspec_history_view_stereo*; DESIGN.md §3.16,
// §4.18): level and balance of a channel pair in one picture.  The device form is stereo.hip.inc's compose kernel on any dB
// array; the batch forms run it behind emspec_batch_device's kernels on an engine workspace (device entry) or inside each
// unit's staging set of the host pipeline (emspec_host.cpp), so that only the image leaves the device; the live form is the
// stereo history view, on the rings of emspec_history.cpp; the host form is the same definition in plain C++.  The arithmetic
// of all of them is emspec_stereo_plan.h's.
#include "emspec_engine.h"

#include <cstring>
#include <string>
#include <vector>

using namespace emspec;

namespace {

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// the map of a call: the caller's, or for NULL the engine's configuration, shift 0, 12 dB to either side
emspec_stereo_map map_of(const emspec_engine* e, const emspec_stereo_map* map) {
    return map ? *map : emspec_stereo_map{e->cfg.db_top, e->cfg.db_range, e->cfg.gate_db, 0.0f, 12.0f};
}
const char* map_error(const emspec_stereo_map& m) { return stereo_map_error(m.db_top, m.db_range, m.gate_db, m.shift_db, m.pan_range_db); }
StereoLaw law_of(const emspec_stereo_map& m) { return stereo_law(m.db_top, m.db_range, m.gate_db, m.shift_db, m.pan_range_db); }

// null, or the rule the outputs break (what the device entries share)
const char* out_error(const void* level, const void* index, const void* pan, const void* rgba) {
    if (!level && !index && !pan && !rgba) return "a stereo image needs at least one output";
    if (!aligned(level, 16) || !aligned(rgba, 16) || !aligned(index, 4) || !aligned(pan, 4))
        return "a stereo image's level and RGBA outputs must be 16-byte aligned, its index and pan outputs 4-byte aligned";
    return nullptr;
}

// what the batch entries check in front of their work
int batch_stereo_check(emspec_engine* e, int32_t n, int32_t hop, int32_t views, int32_t a, int32_t b, const emspec_stereo_map& m) {
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (const char* why = stereo_pair_error(views, a, b)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (const char* why = map_error(m)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (e->cfg.rows % 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "the stereo image needs engine rows that are a multiple of 4 (cells % 4 == 0)");
    if (e->time_reduce > 1)
        return fail(e, EMSPEC_ERR_STATE, "the stereo image is that of full-rate columns: not available while a time reduction is set (emspec_set_time_reduce(e, 1) turns it off)");
    return EMSPEC_OK;
}

// Every check of a stereo view, then its launch on `st`: the outputs are device-visible.
int view_launch(emspec_engine* e, int32_t session, int32_t stream0, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t first,
                int32_t factor, int64_t groups, const emspec_stereo_map* map, float* level, uint8_t* index, uint8_t* pan, uint8_t* rgba,
                hipStream_t st) {
    LiveState* lvp = history_session(e, session);
    if (e->history_W <= 0) return fail(e, EMSPEC_ERR_STATE, "no live history is set (emspec_set_live_history)");
    if (!lvp) return fail(e, EMSPEC_ERR_STATE, "session must be EMSPEC_SESSION_MULTI or EMSPEC_SESSION_ONE");
    LiveState& lv = *lvp;
    if (lv.ss.g.form == 0 || !lv.d_hring) return fail(e, EMSPEC_ERR_STATE, "the session has not started: it has no history");
    if (factor < 1 || factor > kHistoryMaxFactor) return fail(e, EMSPEC_ERR_INVALID_ARG, "a view's factor must be in 1..65536");
    if (groups < 1) return fail(e, EMSPEC_ERR_INVALID_ARG, "a view needs at least one group");
    if (const char* why = stereo_pair_error(views, a, b)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (pairs < 1 || pairs > 65535 || stream0 < 0 || (int64_t)stream0 + (int64_t)pairs * views > lv.ss.g.S)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the view's streams (pairs x views from stream0 on) must lie inside the session's 0.." + std::to_string(lv.ss.g.S - 1));
    if (!level && !index && !pan && !rgba) return fail(e, EMSPEC_ERR_INVALID_ARG, "a stereo image needs at least one output");
    const emspec_stereo_map m = map_of(e, map);
    if (const char* why = map_error(m)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    const int64_t W = e->history_W;
    for (int p = 0; p < pairs; ++p)
        for (int s : {stream0 + p * views + a, stream0 + p * views + b}) {
            const int64_t end = lv.c.emitted[s];
            if (history_view_check(first, factor, groups, end, W) != kHistoryViewOk)
                return fail(e, EMSPEC_ERR_INVALID_ARG, "the view's columns " + std::to_string(first) + " + " + std::to_string(groups) + " groups of " +
                                                           std::to_string(factor) + " are not held for stream " + std::to_string(s) + ": it holds [" +
                                                           std::to_string(history_first(end, W)) + ", " + std::to_string(end) + ")");
        }
    if (const char* why = out_error(level, index, pan, rgba)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (rgba)
        if (int rc = stereo_palette_ready(e)) return rc;
    StereoView v;
    v.ring = lv.d_hring;
    v.ends = lv.d_hends;
    v.W = (int)W;
    v.rows = e->cfg.rows;
    v.stream0 = stream0;
    v.first = first;
    v.slot_first = (int)history_slot(first, W);
    v.f = factor;
    v.groups = (int)groups;   // (<= W: every group has a held column of its own)
    v.views = views, v.a = a, v.b = b;
    v.law = law_of(m);
    v.pal = reinterpret_cast<const uint32_t*>(e->d_stereo_pal);
    v.out = StereoOut{level, index, pan, reinterpret_cast<uint32_t*>(rgba)};
    HIPCHK(e, launch_stereo_view(v, pairs, st));
    return EMSPEC_OK;
}

}  // namespace

namespace emspec {
int stereo_palette_ready(emspec_engine* e) {
    if (e->d_stereo_pal) return EMSPEC_OK;
    std::vector<uint8_t> base(1024), pal(kStereoPaletteBytes);
    make_colormap(0.5f, base.data());   // (the default colour map: emspec_tables.h: default_lut, the same bytes)
    stereo_palette(base.data(), pal.data());
    HIPCHK(e, hipMalloc((void**)&e->d_stereo_pal, kStereoPaletteBytes));
    HIPCHK(e, hipMemcpyAsync(e->d_stereo_pal, pal.data(), kStereoPaletteBytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));   // (the callers' kernels may run on any stream)
    return EMSPEC_OK;
}
void stereo_destroy(emspec_engine* e) {
    (void)hipFree(e->d_stereo_pal);
    e->d_stereo_pal = nullptr;
    for (int i = 0; i < 4; ++i) {
        if (e->h_sview[i]) (void)hipHostFree(e->h_sview[i]);
        e->h_sview[i] = nullptr; e->sview_bytes[i] = 0;
    }
}
}  // namespace emspec

extern "C" {

int emspec_stereo_default_map(const emspec_engine* e, emspec_stereo_map* map) {
    if (!e || !map) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    *map = map_of(e, nullptr);
    return EMSPEC_OK;
}

int emspec_make_stereo_colormap(float brightness, uint8_t* out) {
    if (!out || !(brightness >= 0.0f)) return EMSPEC_ERR_INVALID_ARG;
    uint8_t base[1024];
    make_colormap(brightness, base);
    stereo_palette(base, out);
    return EMSPEC_OK;
}

int emspec_set_stereo_colormap(emspec_engine* e, const uint8_t* rgba) {
    if (!e || !rgba) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = stereo_palette_ready(e)) return rc;
    HIPCHK(e, hipMemcpyAsync(e->d_stereo_pal, rgba, kStereoPaletteBytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return EMSPEC_OK;
}

int emspec_stereo_device(emspec_engine* e, const float* db_dev, int32_t pairs, int32_t views, int32_t a, int32_t b, int64_t cells,
                         const emspec_stereo_map* map, float* level_dev, uint8_t* index_dev, uint8_t* pan_dev, uint8_t* rgba_dev,
                         void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (pairs < 0 || pairs > 65535) return fail(e, EMSPEC_ERR_INVALID_ARG, "pairs must be in 0..65535");
    if (const char* why = stereo_pair_error(views, a, b)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (cells < 0 || cells % 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "a stereo image needs cells % 4 == 0 (and cells >= 0)");
    const emspec_stereo_map m = map_of(e, map);
    if (const char* why = map_error(m)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (const char* why = out_error(level_dev, index_dev, pan_dev, rgba_dev)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (pairs == 0 || cells == 0) return EMSPEC_OK;
    if (!db_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(db_dev, 16)) return fail(e, EMSPEC_ERR_INVALID_ARG, "db_dev must be 16-byte aligned");
    if (cells / 4 > (int64_t)0x7fffffff * 256) return fail(e, EMSPEC_ERR_INVALID_ARG, "at most 2^41 cells per stream");
    HIPCHK(e, hipSetDevice(e->device));
    if (rgba_dev)
        if (int rc = stereo_palette_ready(e)) return rc;
    StereoCompose s;
    s.db = db_dev, s.views = views, s.a = a, s.b = b, s.cells = cells;
    s.law = law_of(m);
    s.pal = reinterpret_cast<const uint32_t*>(e->d_stereo_pal);
    s.out = StereoOut{level_dev, index_dev, pan_dev, reinterpret_cast<uint32_t*>(rgba_dev)};
    HIPCHK(e, launch_stereo_compose(s, pairs, (hipStream_t)hip_stream));
    return EMSPEC_OK;
}

int emspec_stereo_host(const float* db, int64_t pairs, int32_t views, int32_t a, int32_t b, int64_t cells, const emspec_stereo_map* map,
                       const uint8_t* palette, float* level, uint8_t* index, uint8_t* pan, uint8_t* rgba) {
    if (pairs < 0 || cells < 0) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "pairs and cells must not be negative");
    if (const char* why = stereo_pair_error(views, a, b)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    if (cells % 4) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "a stereo image needs cells % 4 == 0");
    if (!map) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "null map");
    if (const char* why = map_error(*map)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    if (!level && !index && !pan && !rgba) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "a stereo image needs at least one output");
    if (rgba && !palette) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "the RGBA output needs a palette");
    if (!aligned(db, 4) || !aligned(level, 4)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "db and level must be 4-byte aligned");
    if (pairs == 0 || cells == 0) return EMSPEC_OK;
    if (!db) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "null argument");
    stereo_compose_host(db, pairs, views, a, b, cells, law_of(*map), palette, level, index, pan, rgba);
    return EMSPEC_OK;
}

int emspec_batch_stereo_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign,
                               int32_t views, int32_t a, int32_t b, const emspec_stereo_map* map, float* level_dev, uint8_t* index_dev,
                               uint8_t* pan_dev, uint8_t* rgba_dev, void* hip_stream) {
    if (!e || !pcm_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    const emspec_stereo_map m = map_of(e, map);
    int rc = batch_stereo_check(e, n, hop, views, a, b, m);
    if (rc) return rc;
    if (S < 1 || S > 65535 || L < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need 1..65535 streams of at least fft-size samples");
    if (S % views) return fail(e, EMSPEC_ERR_INVALID_ARG, "the streams must be whole pairs: S % views == 0");
    if (const char* why = out_error(level_dev, index_dev, pan_dev, rgba_dev)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    HIPCHK(e, hipSetDevice(e->device));
    if (rgba_dev && (rc = stereo_palette_ready(e))) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const int R = e->cfg.rows;
    const int64_t C = emspec_num_columns(L, n, hop);
    StereoCompose s;
    s.views = views, s.a = a, s.b = b, s.cells = C * R;
    s.law = law_of(m);
    s.pal = reinterpret_cast<const uint32_t*>(e->d_stereo_pal);
    // the dB of a chunk of PAIRS goes to the engine workspace the peaks' device entry uses (never beside a time reduction: see
    // the check above), sized by the records path's budget rule with a pair's views streams as its unit: a chunk boundary
    // falls between pairs
    return for_stream_chunks(e, (void**)&e->d_full, &e->full_bytes, (size_t)views * C * R * 4, 256, (size_t)4 << 30, S / views, [&](int p0, int pc, int) -> int {
        float* wdb = reinterpret_cast<float*>(e->d_full);
        if (int rc = batch_device_full(e, pcm_dev + (size_t)p0 * views * L, pc * views, L, n, hop, reassign, wdb, nullptr, nullptr, st)) return rc;
        const size_t o = (size_t)p0 * C * R;
        s.db = wdb;
        s.out = StereoOut{level_dev ? level_dev + o : nullptr, index_dev ? index_dev + o : nullptr, pan_dev ? pan_dev + o : nullptr,
                          rgba_dev ? reinterpret_cast<uint32_t*>(rgba_dev) + o : nullptr};
        HIPCHK(e, launch_stereo_compose(s, pc, st));
        return EMSPEC_OK;
    });
}

int emspec_batch_pcm_stereo(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames, int32_t n,
                            int32_t hop, int32_t reassign, int32_t a, int32_t b, const emspec_stereo_map* map, float* out_level,
                            uint8_t* out_index, uint8_t* out_pan, uint8_t* out_rgba) {
    if (!e || !src) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (const char* why = pcm_format_error(fmt)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    const emspec_stereo_map m = map_of(e, map);
    int rc = batch_stereo_check(e, n, hop, fmt->views, a, b, m);
    if (rc) return rc;
    if (sources < 1 || frames < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need at least one source of at least fft-size frames");
    if ((int64_t)sources * fmt->views > 0x7fffffff) return fail(e, EMSPEC_ERR_INVALID_ARG, "too many streams (sources * views)");
    if (!out_level && !out_index && !out_pan && !out_rgba) return fail(e, EMSPEC_ERR_INVALID_ARG, "a stereo image needs at least one output");
    if (!aligned(out_level, 4)) return fail(e, EMSPEC_ERR_INVALID_ARG, "out_level must be 4-byte aligned");
    HIPCHK(e, hipSetDevice(e->device));
    if (out_rgba && (rc = stereo_palette_ready(e))) return rc;
    const StereoHostOut so{a, b, law_of(m), out_level, out_index, out_pan, out_rgba};
    HostJob job;
    job.src = src, job.S = sources, job.L = frames, job.n = n, job.hop = hop, job.dec = fmt;
    // units as emspec_batch_pcm cuts them: whole sources (a pair is always inside one unit), or runs of one source's columns
    job.whole_streams = e->smoothing > 0.0f || e->agc > 0.0f, job.halo_D = latency(n, hop, reassign);
    job.stereo = &so;
    job.run = [=](const float* p, int sc, int64_t samples, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
        return batch_device_full(e, p, sc, samples, n, hop, reassign, db, rgba, index, st);
    };
    return host_batch(e, job);
}

int emspec_history_view_stereo_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t pairs, int32_t views, int32_t a,
                                      int32_t b, int64_t first_column, int32_t factor, int64_t groups, const emspec_stereo_map* map,
                                      float* level_dev, uint8_t* index_dev, uint8_t* pan_dev, uint8_t* rgba_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);   // (NULL: the default stream, as for every device entry)
    if (int rc = view_launch(e, session, stream0, pairs, views, a, b, first_column, factor, groups, map, level_dev, index_dev, pan_dev,
                             rgba_dev, st))
        return rc;
    // (ordered as emspec_history_view_device: behind every launch so far; the launches to come wait for the view)
    LiveState& lv = *history_session(e, session);
    if (st != e->stream) {
        HIPCHK(e, hipEventRecord(lv.view_done, st));
        HIPCHK(e, hipStreamWaitEvent(e->stream, lv.view_done, 0));
    }
    return EMSPEC_OK;
}

int emspec_history_view_stereo(emspec_engine* e, int32_t session, int32_t stream0, int32_t pairs, int32_t views, int32_t a, int32_t b,
                               int64_t first_column, int32_t factor, int64_t groups, const emspec_stereo_map* map, float* out_level,
                               uint8_t* out_index, uint8_t* out_pan, uint8_t* out_rgba) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    // each output in place when it is page-locked (and aligned for the kernel's stores), else through a page-locked block
    void* const out[4] = {out_level, out_index, out_pan, out_rgba};
    const size_t per[4] = {4, 1, 1, 4}, align[4] = {16, 4, 4, 16};
    void* dst[4] = {};
    bool staged[4] = {};
    // (sized only once the view is known to fit: groups <= W then)
    const bool sized = e->history_W > 0 && pairs >= 1 && pairs <= 65535 && groups >= 1 && groups <= e->history_W;
    const size_t cells = sized ? history_view_cells(pairs, groups, e->cfg.rows) : 0;
    for (int i = 0; i < 4; ++i) {
        if (!out[i]) continue;
        dst[i] = pinned_view(out[i], align[i]);
        if (dst[i] || !sized) { if (!dst[i]) dst[i] = out[i]; continue; }   // (a view that cannot fit is refused below, unlaunched)
        const size_t want = cells * per[i];
        if (e->sview_bytes[i] < want) {
            if (e->h_sview[i]) { (void)hipHostFree(e->h_sview[i]); e->h_sview[i] = nullptr; e->sview_bytes[i] = 0; }
            HIPCHK(e, hipHostMalloc(&e->h_sview[i], want, hipHostMallocDefault));
            e->sview_bytes[i] = want;
        }
        dst[i] = e->h_sview[i];
        staged[i] = true;
    }
    if (int rc = view_launch(e, session, stream0, pairs, views, a, b, first_column, factor, groups, map, static_cast<float*>(dst[0]),
                             static_cast<uint8_t*>(dst[1]), static_cast<uint8_t*>(dst[2]), static_cast<uint8_t*>(dst[3]), e->stream))
        return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int i = 0; i < 4; ++i)
        if (staged[i]) std::memcpy(out[i], e->h_sview[i], cells * per[i]);
    return EMSPEC_OK;
}

}  // extern "C"
