// emspec_audio.cpp — the live audio history behind the C ABI (include/emspec.h: emspec_set_live_audio, emspec_live_audio,
// emspec_audio_view_device, emspec_audio_view, emspec_audio_batch_device, emspec_audio_batch): the
// setting, the rings' allocation, the store behind every live launch (called by emspec_live.cpp: live_launch), the views and
// the re-analysis.  The kernels are live_audio.hip.inc; where a sample lives, what a ring holds, which of a launch's samples are
// stored and whether a view fits is emspec_audio_plan.h, plain integer code that tests/test_audio_plan_cpu.py runs on the CPU.
// This file holds the HIP side only: allocations, launches, the ABI's checks and messages.
#include "emspec_engine.h"

#include <algorithm>
#include <cstring>

using namespace emspec;

namespace {
LiveState* session_of(emspec_engine* e, int32_t session) {
    return session == EMSPEC_SESSION_MULTI ? &e->live : session == EMSPEC_SESSION_ONE ? &e->one : nullptr;
}
// the samples stream s of the session has in its ring's numbering: from the session's own counters
int64_t stream_end(const LiveState& lv, int s) { return audio_end(lv.ss.g.form, lv.c.fed[s], lv.c.newbase[s], lv.ss.g.n, lv.ss.g.hop); }

// Every check of a view: nothing is launched or written when it fails.
// (with_out = false: the re-analysis, whose output is the engine's own workspace)
int view_check(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first, int64_t count, const void* out,
               int64_t stride, bool with_out = true) {
    LiveState* lvp = session_of(e, session);
    if (e->audio_W <= 0) return fail(e, EMSPEC_ERR_STATE, "no live audio history is set (emspec_set_live_audio)");
    if (!lvp) return fail(e, EMSPEC_ERR_STATE, "session must be EMSPEC_SESSION_MULTI or EMSPEC_SESSION_ONE");
    const LiveState& lv = *lvp;
    if (lv.ss.g.form == 0 || !lv.d_aring) return fail(e, EMSPEC_ERR_STATE, "the session has not started: it has no audio history");
    if (count < 1) return fail(e, EMSPEC_ERR_INVALID_ARG, "an audio view needs at least one sample");
    if (streams < 1 || stream0 < 0 || stream0 > lv.ss.g.S - streams)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the view's streams must lie inside the session's 0.." + std::to_string(lv.ss.g.S - 1));
    if (with_out && !out) return fail(e, EMSPEC_ERR_INVALID_ARG, "an audio view needs an output");
    if (with_out && reinterpret_cast<uintptr_t>(out) % 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "an audio view's output must be 4-byte aligned");
    if (stride < count) return fail(e, EMSPEC_ERR_INVALID_ARG, "an audio view's stride must be at least its count");
    const int64_t W = e->audio_W;
    for (int s = stream0; s < stream0 + streams; ++s) {
        const int64_t end = stream_end(lv, s);
        if (audio_view_check(first, count, stride, end, W) != kAudioViewOk)
            return fail(e, EMSPEC_ERR_INVALID_ARG, "the view's samples [" + std::to_string(first) + ", " + std::to_string(first) + " + " +
                                                       std::to_string(count) + ") are not held for stream " + std::to_string(s) + ": it holds [" +
                                                       std::to_string(audio_first(end, W)) + ", " + std::to_string(end) + ")");
    }
    return EMSPEC_OK;
}

// a checked view's launch on `st`: out is device-visible
int view_launch(emspec_engine* e, const LiveState& lv, int32_t stream0, int32_t streams, int64_t first, int64_t count, float* out,
                int64_t stride, hipStream_t st) {
    const AudioRuns r = audio_runs(first, count, e->audio_W);
    AudioView v;
    v.ring = lv.d_aring;
    v.W = e->audio_W;
    v.stride = audio_stride(e->audio_W);
    v.stream0 = stream0;
    v.slot0 = r.slot0; v.n0 = r.n0; v.n1 = r.n1;
    v.out = reinterpret_cast<uint32_t*>(out);
    v.out_stride = stride;
    HIPCHK(e, launch_audio_view(v, streams, st));
    return EMSPEC_OK;
}

// (the streaming calls synchronise the engine's stream before they return, so work enqueued on `st` is behind every launch so
// far; the launches to come wait for it)
int order_behind(emspec_engine* e, LiveState& lv, hipStream_t st) {
    if (st == e->stream) return EMSPEC_OK;
    HIPCHK(e, hipEventRecord(lv.audio_done, st));
    HIPCHK(e, hipStreamWaitEvent(e->stream, lv.audio_done, 0));
    return EMSPEC_OK;
}

void* pinned_view4(const void* p) {
    if (!p || reinterpret_cast<uintptr_t>(p) % 4 || !host_pinned(p)) return nullptr;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return d;
}
}  // namespace

namespace emspec {
int audio_ready(emspec_engine* e, LiveState& lv) {
    if (e->audio_W <= 0) return EMSPEC_OK;
    int rc;
    if ((rc = grow(e, (void**)&lv.d_aring, &lv.aring_bytes, audio_ring_bytes(lv.ss.g.S, e->audio_W)))) return rc;
    if (!lv.audio_done) HIPCHK(e, hipEventCreateWithFlags(&lv.audio_done, hipEventDisableTiming));
    return EMSPEC_OK;
}
void audio_free(LiveState& lv) {
    (void)hipFree(lv.d_aring);
    lv.d_aring = nullptr; lv.aring_bytes = 0;
    if (lv.audio_done) (void)hipEventDestroy(lv.audio_done);
    lv.audio_done = nullptr;
}
void audio_destroy(emspec_engine* e) {
    if (e->h_aview) (void)hipHostFree(e->h_aview);
    e->h_aview = nullptr; e->aview_bytes = 0;
    (void)hipFree(e->d_apcm);
    e->d_apcm = nullptr; e->apcm_bytes = 0;
    for (int i = 0; i < 3; ++i) {
        (void)hipFree(e->d_aout[i]);
        e->d_aout[i] = nullptr; e->aout_bytes[i] = 0;
    }
}
int audio_store(emspec_engine* e, LiveState& lv, const LiveSinks& ls, bool flush) {
    if (e->audio_W <= 0 || flush || !lv.d_aring || !ls.fresh) return EMSPEC_OK;
    const LiveGeometry& g = lv.ss.g;
    int64_t most = 0;
    for (int s = 0; s < g.S; ++s) {
        const LiveStream& d = lv.desc()[s];
        most = std::max(most, audio_fresh(g.form, d.j0, d.newbase, d.newcount, d.frames, d.flush, g.n, g.hop).count);
    }
    LiveAudio a;
    a.ring = lv.d_aring;
    a.W = e->audio_W;
    a.stride = audio_stride(e->audio_W);
    a.form = g.form; a.n = g.n; a.hop = g.hop;
    HIPCHK(e, launch_live_audio_store(ls, a, g.S, most, e->stream));
    return EMSPEC_OK;
}
}  // namespace emspec

extern "C" {

int emspec_set_live_audio(emspec_engine* e, int64_t samples) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (samples < 0 || samples > kAudioMaxSamples) return fail(e, EMSPEC_ERR_INVALID_ARG, "the audio history's samples per stream must be in 0..268435456");
    if (samples == 0) {
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, hipStreamSynchronize(e->stream));   // (a store kernel may still be writing)
        audio_free(e->live);
        audio_free(e->one);
        audio_destroy(e);
        e->audio_W = 0;
        return EMSPEC_OK;
    }
    // a ring holds the samples since each stream's start: a stream that already has samples has some that were not stored
    for (const LiveState* lv : {&e->live, &e->one})
        for (int s = 0; s < lv->c.streams(); ++s)
            if (lv->ss.g.form != 0 && (lv->c.fed[s] > 0 || lv->c.seen[s] > 0))
                return fail(e, EMSPEC_ERR_STATE, "the audio history needs every sample of a stream since its start: a session has samples fed; call emspec_reset() first");
    if (samples != e->audio_W) {   // (a ring of another W: the next call of each session allocates its own)
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        audio_free(e->live);
        audio_free(e->one);
    }
    e->audio_W = samples;
    return EMSPEC_OK;
}

int64_t emspec_live_audio(const emspec_engine* e, int32_t session, int32_t stream, int64_t* first_sample) {
    if (!e || e->audio_W <= 0) return -1;
    const LiveState* lv = session_of(const_cast<emspec_engine*>(e), session);
    if (!lv || lv->ss.g.form == 0 || stream < 0 || stream >= lv->ss.g.S) return -1;
    const int64_t end = stream_end(*lv, stream);
    if (first_sample) *first_sample = audio_first(end, e->audio_W);
    return end;
}

int emspec_audio_view_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample, int64_t count,
                             float* pcm_dev, int64_t stride, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);   // (NULL: the default stream, as for every device entry)
    if (int rc = view_check(e, session, stream0, streams, first_sample, count, pcm_dev, stride)) return rc;
    LiveState& lv = *session_of(e, session);
    if (int rc = view_launch(e, lv, stream0, streams, first_sample, count, pcm_dev, stride, st)) return rc;
    return order_behind(e, lv, st);
}

int emspec_audio_view(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample, int64_t count,
                      float* pcm, int64_t stride) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = view_check(e, session, stream0, streams, first_sample, count, pcm, stride)) return rc;
    LiveState& lv = *session_of(e, session);
    // in place when the output is page-locked, else through a page-locked block [streams][count]
    float* dst = static_cast<float*>(pinned_view4(pcm));
    const bool staged = !dst;
    if (staged) {
        const size_t want = (size_t)streams * (size_t)count * 4;   // (count <= W <= 2^28, streams <= 65535)
        if (e->aview_bytes < want) {
            if (e->h_aview) { (void)hipHostFree(e->h_aview); e->h_aview = nullptr; e->aview_bytes = 0; }
            HIPCHK(e, hipHostMalloc(&e->h_aview, want, hipHostMallocDefault));
            e->aview_bytes = want;
        }
        dst = static_cast<float*>(e->h_aview);
    }
    if (int rc = view_launch(e, lv, stream0, streams, first_sample, count, dst, staged ? count : stride, e->stream)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int sv = 0; staged && sv < streams; ++sv)
        std::memcpy(pcm + (size_t)sv * (size_t)stride, static_cast<const float*>(e->h_aview) + (size_t)sv * (size_t)count, (size_t)count * 4);
    return EMSPEC_OK;
}

int emspec_audio_batch_device(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample, int64_t count,
                              int32_t n, int32_t hop, int32_t reassign, float* db_dev, uint8_t* rgba_dev, uint8_t* index_dev,
                              void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    // the view's checks (the workspace is only grown once the range is known to fit), then the batch's
    if (int rc = view_check(e, session, stream0, streams, first_sample, count, nullptr, count, false)) return rc;
    if (int rc = check_shape(e, n, hop)) return rc;
    if (count < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "a re-analysis needs at least fft-size samples");
    LiveState& lv = *session_of(e, session);
    if (int rc = grow(e, (void**)&e->d_apcm, &e->apcm_bytes, (size_t)streams * (size_t)count * 4)) return rc;
    if (int rc = view_launch(e, lv, stream0, streams, first_sample, count, e->d_apcm, count, st)) return rc;
    const int rc = emspec_batch_device(e, e->d_apcm, streams, count, n, hop, reassign, db_dev, rgba_dev, index_dev, hip_stream);
    if (int rc2 = order_behind(e, lv, st)) return rc ? rc : rc2;
    return rc;
}

int emspec_audio_batch(emspec_engine* e, int32_t session, int32_t stream0, int32_t streams, int64_t first_sample, int64_t count,
                       int32_t n, int32_t hop, int32_t reassign, const emspec_out* out) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (!out) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    HIPCHK(e, hipSetDevice(e->device));
    if (int rc = view_check(e, session, stream0, streams, first_sample, count, nullptr, count, false)) return rc;
    if (int rc = check_shape(e, n, hop)) return rc;
    if (count < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "a re-analysis needs at least fft-size samples");
    // one window's worth: device blocks for the wanted outputs, the device entry, plain copies out
    const int64_t C = reduced_columns(emspec_num_columns(count, n, hop), e->time_reduce);
    const size_t cells = (size_t)streams * (size_t)C * (size_t)e->cfg.rows;
    void* const host[3] = {out->db, out->rgba, out->index};
    const size_t per[3] = {4, 4, 1};
    void* dev[3] = {};
    for (int i = 0; i < 3; ++i) {
        if (!host[i]) continue;
        if (int rc = grow(e, &e->d_aout[i], &e->aout_bytes[i], cells * per[i])) return rc;
        dev[i] = e->d_aout[i];
    }
    if (int rc = emspec_audio_batch_device(e, session, stream0, streams, first_sample, count, n, hop, reassign, static_cast<float*>(dev[0]),
                                           static_cast<uint8_t*>(dev[1]), static_cast<uint8_t*>(dev[2]), e->stream))
        return rc;
    for (int i = 0; i < 3; ++i)
        if (host[i]) HIPCHK(e, hipMemcpyAsync(host[i], dev[i], cells * per[i], hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return EMSPEC_OK;
}

}  // extern "C"
