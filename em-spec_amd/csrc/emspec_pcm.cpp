// emspec_pcm.cpp — the PCM front end behind the C ABI (include/emspec.h: emspec_pcm_frame_bytes, emspec_pcm_decode_device,
// emspec_batch_pcm, emspec_batch_pcm_packed): format validation, the decode kernel by itself, and the host-buffer entries,
// which hand the pipeline driver (emspec_host.cpp) a decode stage in front of the float entries' own unit function.  The live
// entries (emspec_push_samples_pcm, _multires) sit with the session they feed, in emspec_live.cpp.  Kernel: pcm.hip.inc.
#include "emspec_engine.h"

#include <cmath>

using namespace emspec;

static_assert(kPcmS16 == EMSPEC_PCM_S16 && kPcmS24 == EMSPEC_PCM_S24 && kPcmS32 == EMSPEC_PCM_S32 && kPcmF32 == EMSPEC_PCM_F32 &&
                  kPcmMaxChannels == EMSPEC_PCM_MAX_CHANNELS && kPcmMaxViews == EMSPEC_PCM_MAX_VIEWS,
              "the kernel layer's constants are the ABI's");

hipError_t emspec::pcm_decode(const void* src, const emspec_pcm_format& f, int sources, int64_t frames, int64_t src_stride_bytes,
                              float* out, int64_t out_stride, hipStream_t st) {
    return launch_pcm_decode(src, f.sample_type, f.channels, f.views, f.mix, sources, frames, src_stride_bytes, out, out_stride, st);
}

const char* emspec::pcm_format_error(const emspec_pcm_format* f) {
    if (!f) return "null format";
    if (f->sample_type < EMSPEC_PCM_S16 || f->sample_type > EMSPEC_PCM_F32) return "format.sample_type is not one of EMSPEC_PCM_S16 / _S24 / _S32 / _F32";
    if (f->channels < 1 || f->channels > EMSPEC_PCM_MAX_CHANNELS) return "format.channels must be in 1..8";
    if (f->views < 1 || f->views > EMSPEC_PCM_MAX_VIEWS) return "format.views must be in 1..8";
    if (f->reserved != 0) return "format.reserved must be 0";
    for (int i = 0; i < f->views * f->channels; ++i)
        if (!std::isfinite(f->mix[i])) return "format.mix holds a weight that is not finite";
    return nullptr;
}

int emspec::pcm_frame_bytes(const emspec_pcm_format& f) {
    return (f.sample_type == EMSPEC_PCM_S16 ? 2 : f.sample_type == EMSPEC_PCM_S24 ? 3 : 4) * f.channels;
}

extern "C" {

int64_t emspec_pcm_frame_bytes(const emspec_pcm_format* fmt) { return pcm_format_error(fmt) ? -1 : pcm_frame_bytes(*fmt); }

int emspec_pcm_decode_device(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames,
                             int64_t src_stride_bytes, float* pcm, void* hip_stream) {
    if (!e) return fail(e, EMSPEC_ERR_INVALID_ARG, "null engine");
    if (const char* why = pcm_format_error(fmt)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (sources < 0 || frames < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "sources and frames must be >= 0");
    if (sources == 0 || frames == 0) return EMSPEC_OK;
    if (!src || !pcm) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    const int fb = pcm_frame_bytes(*fmt), ss = fb / fmt->channels == 3 ? 1 : fb / fmt->channels;
    if (frames > INT64_MAX / fb || src_stride_bytes < frames * fb)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "src_stride_bytes is smaller than a row of frames");
    if (reinterpret_cast<uintptr_t>(src) % ss || src_stride_bytes % ss)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the source pointer and stride must be multiples of the sample size");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, pcm_decode(src, *fmt, sources, frames, src_stride_bytes, pcm, frames, reinterpret_cast<hipStream_t>(hip_stream)));
    return EMSPEC_OK;
}

// (the unit function of emspec_batch / emspec_batch_packed: the full-rate emspec_batch_device on the decoded streams)
static HostRun pcm_batch_run(emspec_engine* e, int n, int hop, int reassign) {
    return [=](const float* pcm, int sc, int64_t samples, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
        return batch_device_full(e, pcm, sc, samples, n, hop, reassign, db, rgba, index, st);
    };
}

static int pcm_batch_check(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames,
                           int32_t n, int32_t hop) {
    if (!e || !src) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (const char* why = pcm_format_error(fmt)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    const int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (sources < 1 || frames < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need at least one source of at least fft-size frames");
    if ((int64_t)sources * fmt->views > 0x7fffffff) return fail(e, EMSPEC_ERR_INVALID_ARG, "too many streams (sources * views)");
    return EMSPEC_OK;
}

int emspec_batch_pcm(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames, int32_t n,
                     int32_t hop, int32_t reassign, const emspec_out* out) {
    if (!out) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = pcm_batch_check(e, src, fmt, sources, frames, n, hop);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    if (!out->db && !out->rgba && !out->index) return EMSPEC_OK;
    const bool post = e->smoothing > 0.0f || e->agc > 0.0f;   // (whole streams then, as in emspec_batch)
    HostJob job;
    job.src = src, job.S = sources, job.L = frames, job.n = n, job.hop = hop, job.dec = fmt;
    job.whole_streams = post, job.halo_D = latency(n, hop, reassign);
    job.out = out;
    job.run = pcm_batch_run(e, n, hop, reassign);
    return host_batch(e, job);
}

int emspec_batch_pcm_packed(emspec_engine* e, const void* src, const emspec_pcm_format* fmt, int32_t sources, int64_t frames,
                            int32_t n, int32_t hop, int32_t reassign, uint8_t* wire, int64_t wire_capacity, int64_t* offsets) {
    if (!wire || !offsets || wire_capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = pcm_batch_check(e, src, fmt, sources, frames, n, hop);
    if (rc) return rc;
    if ((uint64_t)reduced_columns(emspec_num_columns(frames, n, hop), e->time_reduce) * (uint64_t)e->cfg.rows >= (1ull << 32))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "at most 2^32 cells per stream");
    if (e->cfg.rows % 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "the wire image needs rows % 4 == 0");
    HIPCHK(e, hipSetDevice(e->device));
    const PackedOut pk{wire, wire_capacity, offsets};
    HostJob job;
    job.src = src, job.S = sources, job.L = frames, job.n = n, job.hop = hop, job.dec = fmt;
    job.whole_streams = true;
    job.pk = &pk;
    job.run = pcm_batch_run(e, n, hop, reassign);
    return host_batch(e, job);
}

}  // extern "C"
