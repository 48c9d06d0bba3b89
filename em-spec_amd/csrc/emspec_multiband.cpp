// emspec_multiband.cpp — the multi-band batch (include/emspec.h: emspec_batch_multiband*): two to four FFT sizes,
// each for its own band of rows, on the longest FFT's column grid, and the multi-resolution batch (emspec_batch_multires*, §3.8): its
// two-band case under rules of its own.  Each band is an ordinary batch of its own band plan (get_band_plan) through the same run
// functions as emspec_batch_device, into an engine workspace; multiband.hip.inc's kernel composes them into the caller's layout.
// What is accepted, the shifts, the row ranges and the workspace layout: emspec_band_plan.h.
#include "emspec_engine.h"

#include <string>

using namespace emspec;

namespace emspec {

// shape, split row and stream count of the two-band form: the batch and the live session (emspec_live.cpp) accept the same
int multires_check(emspec_engine* e, int32_t S, int32_t n_low, int32_t n_high, int32_t hop, int32_t split_row) {
    if (const char* why = multires_shape_error(n_low, n_high, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (const char* why = multires_split_error(split_row, e->cfg.rows)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (S < 1 || S > 65535) return fail(e, EMSPEC_ERR_INVALID_ARG, "need 1..65535 streams");
    return EMSPEC_OK;
}

}  // namespace emspec

namespace {

int multires_check(emspec_engine* e, int32_t S, int64_t L, int32_t n_low, int32_t n_high, int32_t hop, int32_t split_row) {
    if (int rc = emspec::multires_check(e, S, n_low, n_high, hop, split_row)) return rc;
    if (L < n_low) return fail(e, EMSPEC_ERR_INVALID_ARG, "need at least n_low samples per stream");
    return EMSPEC_OK;
}

int multiband_check(emspec_engine* e, int32_t S, int64_t L, int32_t bands, const int32_t* n, const int32_t* split, int32_t hop) {
    if (const char* why = band_shape_error(bands, n, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (const char* why = band_split_error(bands, split, e->cfg.rows)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (S < 1 || S > 65535) return fail(e, EMSPEC_ERR_INVALID_ARG, "need 1..65535 streams");
    if (L < n[0]) return fail(e, EMSPEC_ERR_INVALID_ARG, "need at least n[0] samples per stream");
    return EMSPEC_OK;
}

// S device-resident streams -> composed columns; streams in chunks so that the band workspace stays bounded (the records path's
// budget rule).  Per chunk: band k's C + 2 shift[k] columns of its rows, then the composition (with the display post-process on:
// into a raw plane, then launch_postprocess over whole streams).
int multiband_run(emspec_engine* e, const float* pcm, int32_t S, int64_t L, const BandPlan& bp, int32_t hop, int32_t reassign,
                  float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
    int rc;
    const int R = e->cfg.rows, K = bp.bands;
    const int64_t C = emspec_num_columns(L, bp.n[0], hop);
    Plan* pl[kMaxBands];
    for (int k = 0; k < K; ++k)
        if ((rc = get_band_plan(e, bp.n[k], bp.lo[k], bp.rows_of(k), &pl[k]))) return rc;
    const bool post = e->smoothing > 0.0f || e->agc > 0.0f;
    const BandLayout lay = band_layout(bp, C, R, post);
    const size_t col_cells = (size_t)C * R;
    // the dB -> index map: only lo / inv_range / gate are read, which every n shares (EXACT mode: its own rounding of lo)
    DbMap dm = db_map(e, bp.n[0]);
    if (e->exact()) {
        const ExactDbMap xm = exact_db_map(e, bp.n[0], exact_plan_dev(e, *pl[0], hop, reassign));
        dm.lo = xm.lo; dm.inv_range = xm.inv_range; dm.gate = xm.gate;
    }
    return for_stream_chunks(e, (void**)&e->d_mres, &e->mres_bytes, lay.per_stream, kBandPad, (size_t)4 << 30, S, [&](int s0, int sc, int chunk) -> int {
        int rc;
        if (post && s0 == 0) {   // the post-process workspaces of a chunk, in front of the first one
            if ((rc = grow(e, (void**)&e->d_peak, &e->peak_bytes, (size_t)chunk * C * 8 + 16))) return rc;
            if (!db && (rc = grow(e, (void**)&e->d_post, &e->post_bytes, (size_t)chunk * col_cells * 4))) return rc;
        }
        char* base = (char*)e->d_mres;
        const float* in = pcm + (size_t)s0 * L;
        BandSrc src;
        for (int k = 0; k < kMaxBands; ++k) {
            const bool used = k < K;
            src.plane[k] = (const float*)(base + lay.chunk_offset(used ? k : 0, chunk));
            src.shift[k] = used ? bp.shift[k] : 0;
            src.rows[k] = used ? bp.rows_of(k) : 0;
            src.q0[k] = used ? bp.lo[k] / 4 : R / 4;
            if (used && (rc = run_plan_columns(e, *pl[k], in, sc, L, hop, reassign, C + 2 * (int64_t)bp.shift[k], (float*)src.plane[k],
                                               nullptr, nullptr, st))) return rc;
        }
        const size_t o = (size_t)s0 * col_cells;
        if (!post) {
            HIPCHK(e, launch_multiband_compose(src, sc, C, R, dm, e->d_lut, db ? db + o : nullptr, rgba ? rgba + 4 * o : nullptr,
                                               index ? index + o : nullptr, st));
            return EMSPEC_OK;
        }
        float* wraw = (float*)(base + lay.chunk_offset(K, chunk));
        HIPCHK(e, launch_multiband_compose(src, sc, C, R, dm, e->d_lut, wraw, nullptr, nullptr, st));
        HIPCHK(e, launch_postprocess(wraw, db ? db + o : e->d_post, rgba ? rgba + 4 * o : nullptr, index ? index + o : nullptr, sc,
                                     C, R, e->smoothing, e->agc, e->cfg.db_top, db_map(e, bp.n[0]), e->d_lut, e->d_peak,
                                     e->d_peak + (size_t)sc * C, st));
        return EMSPEC_OK;
    });
}

// the device entries behind their checks: nothing wanted, else the run - under time reduction through reduce_streams
int multiband_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, const BandPlan& bp, int32_t hop, int32_t reassign,
                     float* db_dev, uint8_t* rgba_dev, uint8_t* index_dev, void* hip_stream) {
    HIPCHK(e, hipSetDevice(e->device));
    if (!db_dev && !rgba_dev && !index_dev) return EMSPEC_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    if (e->time_reduce == 1) return multiband_run(e, pcm_dev, S, L, bp, hop, reassign, db_dev, rgba_dev, index_dev, st);
    // time reduction: the composed full-rate columns of a chunk of streams into the engine workspace, reduced from there
    return reduce_streams(e, S, emspec_num_columns(L, bp.n[0], hop), db_dev, rgba_dev, index_dev, st, [=](int s0, int sc, float* fdb, uint8_t* fidx) {
        return multiband_run(e, pcm_dev + (size_t)s0 * L, sc, L, bp, hop, reassign, fdb, nullptr, fidx, st);
    });
}

// the host entries behind their checks: the host-buffer pipeline of emspec_batch (emspec_host.cpp) over whole streams - the bands'
// halos differ - of at least four per unit (two bands, 16 streams x 2^22 samples, index out, FAST: one stream per unit 26.3 ms,
// two 20.9, four 19.1)
int multiband_host(emspec_engine* e, const float* pcm, int32_t S, int64_t L, const BandPlan& bp, int32_t hop, int32_t reassign,
                   const emspec_out* out) {
    HIPCHK(e, hipSetDevice(e->device));
    if (!out->db && !out->rgba && !out->index) return EMSPEC_OK;
    HostJob job;
    job.src = pcm, job.S = S, job.L = L, job.n = bp.n[0], job.hop = hop;
    job.whole_streams = true, job.min_streams = 4;
    job.out = out;
    job.run = [=](const float* d_pcm, int sc, int64_t samples, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
        return multiband_run(e, d_pcm, sc, samples, bp, hop, reassign, db, rgba, index, st);
    };
    return host_batch(e, job);
}

// the two bands of an accepted multi-resolution call
BandPlan two_band_plan(const emspec_engine* e, int32_t n_low, int32_t n_high, int32_t hop, int32_t split_row) {
    const int32_t n[2] = {n_low, n_high};
    return band_plan(2, n, &split_row, hop, e->cfg.rows);
}

}  // namespace

extern "C" {

int32_t emspec_multires_shift(int32_t n_low, int32_t n_high, int32_t hop) {
    if (multires_shape_error(n_low, n_high, hop)) return -1;
    return (n_low - n_high) / (2 * hop);
}

int64_t emspec_multires_columns(int64_t L, int32_t n_low, int32_t n_high, int32_t hop) {
    if (multires_shape_error(n_low, n_high, hop)) return -1;
    return emspec_num_columns(L, n_low, hop);
}

int emspec_batch_multires_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n_low, int32_t n_high,
                                 int32_t hop, int32_t split_row, int32_t reassign, float* db_dev, uint8_t* rgba_dev,
                                 uint8_t* index_dev, void* hip_stream) {
    if (!e || !pcm_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (int rc = multires_check(e, S, L, n_low, n_high, hop, split_row)) return rc;
    return multiband_device(e, pcm_dev, S, L, two_band_plan(e, n_low, n_high, hop, split_row), hop, reassign, db_dev, rgba_dev,
                            index_dev, hip_stream);
}

int emspec_batch_multires(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n_low, int32_t n_high, int32_t hop,
                          int32_t split_row, int32_t reassign, const emspec_out* out) {
    if (!e || !pcm || !out) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (int rc = multires_check(e, S, L, n_low, n_high, hop, split_row)) return rc;
    return multiband_host(e, pcm, S, L, two_band_plan(e, n_low, n_high, hop, split_row), hop, reassign, out);
}

int emspec_multiband_shifts(int32_t bands, const int32_t* n, int32_t hop, int32_t* shifts_out) {
    if (band_shape_error(bands, n, hop)) return -1;
    for (int k = 0; shifts_out && k < bands; ++k) shifts_out[k] = (n[0] - n[k]) / (2 * hop);
    return 0;
}

int64_t emspec_multiband_columns(int64_t L, int32_t bands, const int32_t* n, int32_t hop) {
    if (band_shape_error(bands, n, hop)) return -1;
    return emspec_num_columns(L, n[0], hop);
}

int emspec_batch_multiband_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t bands, const int32_t* n,
                                  const int32_t* split_rows, int32_t hop, int32_t reassign, float* db_dev, uint8_t* rgba_dev,
                                  uint8_t* index_dev, void* hip_stream) {
    if (!e || !pcm_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (int rc = multiband_check(e, S, L, bands, n, split_rows, hop)) return rc;
    return multiband_device(e, pcm_dev, S, L, band_plan(bands, n, split_rows, hop, e->cfg.rows), hop, reassign, db_dev, rgba_dev,
                            index_dev, hip_stream);
}

int emspec_batch_multiband(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t bands, const int32_t* n,
                           const int32_t* split_rows, int32_t hop, int32_t reassign, const emspec_out* out) {
    if (!e || !pcm || !out) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (int rc = multiband_check(e, S, L, bands, n, split_rows, hop)) return rc;
    return multiband_host(e, pcm, S, L, band_plan(bands, n, split_rows, hop, e->cfg.rows), hop, reassign, out);
}

}  // extern "C"
