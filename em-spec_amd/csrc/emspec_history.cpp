// emspec_history.cpp — the live history behind the C ABI (include/emspec.h: emspec_set_live_history, emspec_live_history,
// emspec_history_view_device, emspec_history_view): the setting, the rings' allocation, and the views.
// The store into the ring is part of every live launch (emspec_live.cpp: live_launch); the kernels are live_history.hip.inc;
// where a column lives, what a ring holds and whether a view fits is emspec_history_plan.h, plain integer code that
// tests/test_history_plan_cpu.py runs on the CPU.  This file holds the HIP side only: allocations, launches, the ABI's checks
// and messages.
#include "emspec_engine.h"

#include <cstring>

using namespace emspec;

namespace emspec {
LiveState* history_session(emspec_engine* e, int32_t session) {
    return session == EMSPEC_SESSION_MULTI ? &e->live : session == EMSPEC_SESSION_ONE ? &e->one : nullptr;
}

// the address the device uses for page-locked host memory aligned to `align` bytes, or null (as emspec_live.cpp: device_view)
void* pinned_view(const void* p, size_t align) {
    if (!p || reinterpret_cast<uintptr_t>(p) % align || !host_pinned(p)) return nullptr;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return d;
}
}  // namespace emspec

namespace {
LiveState* session_of(emspec_engine* e, int32_t session) { return history_session(e, session); }

// Every check of a view, then its launch on `st`: db / index / rgba are device-visible.
int view_launch(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first, int32_t factor, int64_t groups,
                const emspec_view_map* map, float* db, uint8_t* index, uint8_t* rgba, hipStream_t st) {
    LiveState* lvp = session_of(e, session);
    if (e->history_W <= 0) return fail(e, EMSPEC_ERR_STATE, "no live history is set (emspec_set_live_history)");
    if (!lvp) return fail(e, EMSPEC_ERR_STATE, "session must be EMSPEC_SESSION_MULTI or EMSPEC_SESSION_ONE");
    LiveState& lv = *lvp;
    if (lv.ss.g.form == 0 || !lv.d_hring) return fail(e, EMSPEC_ERR_STATE, "the session has not started: it has no history");
    if (factor < 1 || factor > kHistoryMaxFactor) return fail(e, EMSPEC_ERR_INVALID_ARG, "a view's factor must be in 1..65536");
    if (groups < 1) return fail(e, EMSPEC_ERR_INVALID_ARG, "a view needs at least one group");
    if (streams < 1 || stream0 < 0 || stream0 > lv.ss.g.S - streams)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the view's streams must lie inside the session's 0.." + std::to_string(lv.ss.g.S - 1));
    if (!db && !index && !rgba) return fail(e, EMSPEC_ERR_INVALID_ARG, "a view needs at least one output");
    if (map && !(map->db_range > 0.0f && map->db_top == map->db_top && map->gate_db == map->gate_db && map->shift_db == map->shift_db))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "a view's map needs db_range > 0 and no NaN field");
    const int64_t W = e->history_W;
    for (int s = stream0; s < stream0 + streams; ++s) {
        const int64_t end = lv.c.emitted[s];
        if (history_view_check(first, factor, groups, end, W) != kHistoryViewOk)
            return fail(e, EMSPEC_ERR_INVALID_ARG, "the view's columns " + std::to_string(first) + " + " + std::to_string(groups) + " groups of " +
                                                       std::to_string(factor) + " are not held for stream " + std::to_string(s) + ": it holds [" +
                                                       std::to_string(history_first(end, W)) + ", " + std::to_string(end) + ")");
    }
    if (reinterpret_cast<uintptr_t>(db) % 16 || reinterpret_cast<uintptr_t>(rgba) % 16 || reinterpret_cast<uintptr_t>(index) % 4)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "a view's dB and RGBA outputs must be 16-byte aligned, its index output 4-byte aligned");
    HistoryView v;
    v.ring = lv.d_hring;
    v.ends = lv.d_hends;
    v.W = (int)W;
    v.rows = e->cfg.rows;
    v.stream0 = stream0;
    v.first = first;
    v.slot_first = (int)history_slot(first, W);
    v.f = factor;
    v.groups = (int)groups;   // (<= W: every group has a held column of its own)
    // the law: the configuration's scalars as every kernel gets them (emspec_tables.h: db_scalars), or the same arithmetic on the map's
    emspec_config c = e->cfg;
    if (map) { c.db_top = map->db_top; c.db_range = map->db_range; c.gate_db = map->gate_db; }
    const DbScalars m = db_scalars(c, 4096);   // (the fft size enters the scale only, which a view does not read)
    v.map = DbMap{m.scale, m.lo, m.inv_range, m.gate};
    v.shift = map ? map->shift_db : 0.0f;
    v.lut = reinterpret_cast<const uint32_t*>(e->d_lut);
    v.db = db;
    v.index = index;
    v.rgba = reinterpret_cast<uint32_t*>(rgba);
    HIPCHK(e, launch_history_view(v, streams, st));
    return EMSPEC_OK;
}
}  // namespace

namespace emspec {
int history_ready(emspec_engine* e, LiveState& lv) {
    if (e->history_W <= 0) return EMSPEC_OK;
    int rc;
    const bool fresh = lv.hends_bytes < (size_t)lv.ss.g.S * 8;
    if ((rc = grow(e, (void**)&lv.d_hring, &lv.hring_bytes, history_ring_bytes(lv.ss.g.S, e->history_W, e->cfg.rows)))) return rc;
    if ((rc = grow(e, (void**)&lv.d_hends, &lv.hends_bytes, (size_t)lv.ss.g.S * 8))) return rc;
    if (fresh) HIPCHK(e, hipMemsetAsync(lv.d_hends, 0, lv.hends_bytes, e->stream));
    if (!lv.view_done) HIPCHK(e, hipEventCreateWithFlags(&lv.view_done, hipEventDisableTiming));
    return EMSPEC_OK;
}
void history_free(LiveState& lv) {
    (void)hipFree(lv.d_hring); (void)hipFree(lv.d_hends);
    lv.d_hring = nullptr; lv.hring_bytes = 0;
    lv.d_hends = nullptr; lv.hends_bytes = 0;
    if (lv.view_done) (void)hipEventDestroy(lv.view_done);
    lv.view_done = nullptr;
}
void history_destroy(emspec_engine* e) {
    for (int i = 0; i < 3; ++i) {
        if (e->h_view[i]) (void)hipHostFree(e->h_view[i]);
        e->h_view[i] = nullptr; e->view_bytes[i] = 0;
    }
}
}  // namespace emspec

extern "C" {

int emspec_set_live_history(emspec_engine* e, int64_t columns) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (columns < 0 || columns > kHistoryMaxColumns) return fail(e, EMSPEC_ERR_INVALID_ARG, "the history's columns per stream must be in 0..1048576");
    if (columns == 0) {
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, hipStreamSynchronize(e->stream));   // (a store kernel may still be writing)
        history_free(e->live);
        history_free(e->one);
        e->history_W = 0;
        return EMSPEC_OK;
    }
    if (e->cfg.rows % 4 || e->cfg.rows < 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "the history needs engine rows that are a multiple of 4");
    // a ring holds the columns since each stream's start: a stream that already has frames has columns that were not stored
    for (const LiveState* lv : {&e->live, &e->one})
        for (int s = 0; s < lv->c.streams(); ++s)
            if (lv->ss.g.form != 0 && lv->c.fed[s] > 0)
                return fail(e, EMSPEC_ERR_STATE, "the history needs every column of a stream since its start: a session has frames fed; call emspec_reset() first");
    if (columns != e->history_W) {   // (a ring of another W: the next call of each session allocates its own)
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        history_free(e->live);
        history_free(e->one);
    }
    e->history_W = columns;
    return EMSPEC_OK;
}

int64_t emspec_live_history(const emspec_engine* e, int32_t session, int32_t stream, int64_t* first_column) {
    if (!e || e->history_W <= 0) return -1;
    const LiveState* lv = session_of(const_cast<emspec_engine*>(e), session);
    if (!lv || lv->ss.g.form == 0 || stream < 0 || stream >= lv->ss.g.S) return -1;
    const int64_t end = lv->c.emitted[stream];
    if (first_column) *first_column = history_first(end, e->history_W);
    return end;
}

int emspec_history_view_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_column,
                               int32_t factor, int64_t groups, const emspec_view_map* map, float* db_dev, uint8_t* index_dev,
                               uint8_t* rgba_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);   // (NULL: the default stream, as for every device entry)
    if (int rc = view_launch(e, session, stream0, streams, first_column, factor, groups, map, db_dev, index_dev, rgba_dev, st)) return rc;
    // (the streaming calls synchronise the engine's stream before they return, so the view is behind every launch so far; the
    // launches to come wait for it)
    LiveState& lv = *session_of(e, session);
    if (st != e->stream) {
        HIPCHK(e, hipEventRecord(lv.view_done, st));
        HIPCHK(e, hipStreamWaitEvent(e->stream, lv.view_done, 0));
    }
    return EMSPEC_OK;
}

int emspec_history_view(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_column, int32_t factor,
                        int64_t groups, const emspec_view_map* map, float* out_db, uint8_t* out_index, uint8_t* out_rgba) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    // each output in place when it is page-locked (and aligned for the kernel's stores), else through a page-locked block
    void* const out[3] = {out_db, out_index, out_rgba};
    const size_t per[3] = {4, 1, 4}, align[3] = {16, 4, 16};
    void* dst[3] = {};
    bool staged[3] = {};
    // (sized only once the view is known to fit: groups <= W then)
    const bool sized = e->history_W > 0 && streams >= 1 && streams <= 65535 && groups >= 1 && groups <= e->history_W;
    for (int i = 0; i < 3; ++i) {
        if (!out[i]) continue;
        dst[i] = pinned_view(out[i], align[i]);
        if (dst[i] || !sized) { if (!dst[i]) dst[i] = out[i]; continue; }   // (a view that cannot fit is refused below, unlaunched)
        const size_t want = history_view_cells(streams, groups, e->cfg.rows) * per[i];
        if (e->view_bytes[i] < want) {
            if (e->h_view[i]) { (void)hipHostFree(e->h_view[i]); e->h_view[i] = nullptr; e->view_bytes[i] = 0; }
            HIPCHK(e, hipHostMalloc(&e->h_view[i], want, hipHostMallocDefault));
            e->view_bytes[i] = want;
        }
        dst[i] = e->h_view[i];
        staged[i] = true;
    }
    if (int rc = view_launch(e, session, stream0, streams, first_column, factor, groups, map, static_cast<float*>(dst[0]),
                             static_cast<uint8_t*>(dst[1]), static_cast<uint8_t*>(dst[2]), e->stream))
        return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int i = 0; i < 3; ++i)
        if (staged[i]) std::memcpy(out[i], e->h_view[i], history_view_cells(streams, groups, e->cfg.rows) * per[i]);
    return EMSPEC_OK;
}

}  // extern "C"
