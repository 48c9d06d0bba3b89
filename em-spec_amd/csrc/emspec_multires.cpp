// emspec_multires.cpp — the multi-resolution batch (include/emspec.h: emspec_batch_multires*): a long FFT
// for the rows below split_row, a short one above, on the long FFT's column grid.  Each band is an ordinary batch of its own
// band plan (a slice of the engine's row table, get_band_plan) through the same run functions as emspec_batch_device, into an
// engine workspace; multires.hip.inc's kernel composes the two into the caller's layout.
#include "emspec_engine.h"

#include <algorithm>
#include <string>

using namespace emspec;

namespace emspec {

// null when (n_low, n_high, hop) is an accepted shape, else the rule it breaks
const char* multires_shape_error(int n_low, int n_high, int hop) {
    if (n_low != 8192 && n_low != 16384) return "n_low must be 8192 or 16384";
    if (n_high != 1024 && n_high != 2048 && n_high != 4096) return "n_high must be 1024, 2048 or 4096";
    if (hop < 1 || hop > n_high) return "hop must be in [1, n_high]";
    if ((n_low - n_high) % (2 * hop)) return "(n_low - n_high) / (2 hop) must be an integer";
    return nullptr;
}

// shape, split row and stream count: the batch and the live session (emspec_live.cpp) accept the same
int multires_check(emspec_engine* e, int32_t S, int32_t n_low, int32_t n_high, int32_t hop, int32_t split_row) {
    if (const char* why = multires_shape_error(n_low, n_high, hop)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (split_row % 4 || split_row < 64 || split_row > e->cfg.rows - 64)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "split_row must be a multiple of 4 in [64, rows - 64]");
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

// S device-resident streams -> composed columns; streams in chunks so that the band workspace stays bounded (the records
// path's budget rule).  Per chunk: the low band's C columns of rows [0, split), the high band's C + 2 shift columns of rows
// [split, R), the composition (with the display post-process on: into a raw plane, then launch_postprocess over whole streams).
int multires_run(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n_low, int32_t n_high, int32_t hop,
                 int32_t split, int32_t reassign, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
    int rc;
    const int R = e->cfg.rows, Rh = R - split, shift = (n_low - n_high) / (2 * hop);
    const int64_t C = emspec_num_columns(L, n_low, hop), Ch = emspec_num_columns(L, n_high, hop);   // Ch = C + 2 shift
    Plan *pl, *ph;
    if ((rc = get_band_plan(e, n_low, 0, split, &pl))) return rc;
    if ((rc = get_band_plan(e, n_high, split, Rh, &ph))) return rc;
    const bool post = e->smoothing > 0.0f || e->agc > 0.0f;
    const size_t col_cells = (size_t)C * R, lo_s = (size_t)C * split * 4, hi_s = (size_t)Ch * Rh * 4, raw_s = post ? col_cells * 4 : 0;
    // the dB -> index map: only lo / inv_range / gate are read, which every n shares (EXACT mode: its own rounding of lo)
    DbMap dm = db_map(e, n_low);
    if (e->exact()) {
        const ExactDbMap xm = exact_db_map(e, n_low, exact_plan_dev(e, *pl, hop, reassign));
        dm.lo = xm.lo; dm.inv_range = xm.inv_range; dm.gate = xm.gate;
    }
    return for_stream_chunks(e, (void**)&e->d_mres, &e->mres_bytes, lo_s + hi_s + raw_s, 1024, (size_t)4 << 30, S, [&](int s0, int sc, int chunk) -> int {
        int rc;
        if (post && s0 == 0) {   // the post-process workspaces of a chunk, in front of the first one
            if ((rc = grow(e, (void**)&e->d_peak, &e->peak_bytes, (size_t)chunk * C * 8 + 16))) return rc;
            if (!db && (rc = grow(e, (void**)&e->d_post, &e->post_bytes, (size_t)chunk * col_cells * 4))) return rc;
        }
        float* wlo = e->d_mres;
        float* whi = (float*)((char*)wlo + al(lo_s * chunk));
        float* wraw = (float*)((char*)whi + al(hi_s * chunk));
        const float* in = pcm + (size_t)s0 * L;
        if ((rc = run_plan_columns(e, *pl, in, sc, L, hop, reassign, C, wlo, nullptr, nullptr, st))) return rc;
        if ((rc = run_plan_columns(e, *ph, in, sc, L, hop, reassign, Ch, whi, nullptr, nullptr, st))) return rc;
        const size_t o = (size_t)s0 * col_cells;
        if (!post) {
            HIPCHK(e, launch_multires_compose(wlo, whi, sc, C, R, split, shift, dm, e->d_lut, db ? db + o : nullptr,
                                              rgba ? rgba + 4 * o : nullptr, index ? index + o : nullptr, st));
            return EMSPEC_OK;
        }
        HIPCHK(e, launch_multires_compose(wlo, whi, sc, C, R, split, shift, dm, e->d_lut, wraw, nullptr, nullptr, st));
        HIPCHK(e, launch_postprocess(wraw, db ? db + o : e->d_post, rgba ? rgba + 4 * o : nullptr, index ? index + o : nullptr, sc,
                                     C, R, e->smoothing, e->agc, e->cfg.db_top, db_map(e, n_low), e->d_lut, e->d_peak,
                                     e->d_peak + (size_t)sc * C, st));
        return EMSPEC_OK;
    });
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
    int rc = multires_check(e, S, L, n_low, n_high, hop, split_row);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    if (!db_dev && !rgba_dev && !index_dev) return EMSPEC_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    if (e->time_reduce == 1) return multires_run(e, pcm_dev, S, L, n_low, n_high, hop, split_row, reassign, db_dev, rgba_dev, index_dev, st);
    // time reduction: the composed full-rate columns of a chunk of streams into the engine workspace, reduced from there
    return reduce_streams(e, S, emspec_num_columns(L, n_low, hop), db_dev, rgba_dev, index_dev, st, [=](int s0, int sc, float* fdb, uint8_t* fidx) {
        return multires_run(e, pcm_dev + (size_t)s0 * L, sc, L, n_low, n_high, hop, split_row, reassign, fdb, nullptr, fidx, st);
    });
}

// host buffers: the host-buffer pipeline of emspec_batch (emspec_host.cpp) over whole streams - the two bands' halos differ -
// of at least four per unit (16 streams x 2^22 samples, index out, FAST: one stream per unit 26.3 ms, two 20.9, four 19.1)
int emspec_batch_multires(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n_low, int32_t n_high, int32_t hop,
                          int32_t split_row, int32_t reassign, const emspec_out* out) {
    if (!e || !pcm || !out) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = multires_check(e, S, L, n_low, n_high, hop, split_row);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    if (!out->db && !out->rgba && !out->index) return EMSPEC_OK;
    HostJob job;
    job.src = pcm, job.S = S, job.L = L, job.n = n_low, job.hop = hop;
    job.whole_streams = true, job.min_streams = 4;
    job.out = out;
    job.run = [=](const float* d_pcm, int sc, int64_t samples, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
        return multires_run(e, d_pcm, sc, samples, n_low, n_high, hop, split_row, reassign, db, rgba, index, st);
    };
    return host_batch(e, job);
}

}  // extern "C"
