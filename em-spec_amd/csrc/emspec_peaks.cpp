// emspec_peaks.cpp — spectral peaks (include/emspec.h: emspec_peaks_*, emspec_batch_peaks*, emspec_position_hz; DESIGN.md
// §3.11, §4.12): the k loudest local maxima of every finished column, as (position in row units, dB) pairs.  The device form is
// peaks.hip.inc's kernel on any [columns][rows] dB array; the batch forms run it behind emspec_batch_device's kernels on an
// engine workspace (device entry) or inside each unit's staging set of the host pipeline (emspec_host.cpp), so that only
// the peak lists leave the device; the host form is the same definition in plain C++.
#include "emspec_engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>

using namespace emspec;

namespace {

// null, or the rule the arguments break (what the device and the host form share)
const char* peaks_arg_error(int64_t columns, int32_t rows, int32_t k, float min_db) {
    if (columns < 0) return "columns must not be negative";
    if (rows % 4 || rows < 4 || rows > 4096) return "peaks need rows % 4 == 0 and 4 <= rows <= 4096";
    if (k < 1 || k > 32) return "k must be in [1, 32]";
    if (min_db != min_db) return "min_db must not be NaN";
    return nullptr;
}

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// the order of the selection: dB descending by float comparison, ties by ascending row
struct Cand { float db; int row; };
bool before(const Cand& a, const Cand& b) { return a.db > b.db || (a.db == b.db && a.row < b.row); }

// what the batch entries check in front of their work
int batch_peaks_check(emspec_engine* e, const void* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t k, float min_db,
                      const void* peaks, int max_streams) {
    if (!e || !pcm || !peaks) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (S < 1 || S > max_streams || L < n)
        return fail(e, EMSPEC_ERR_INVALID_ARG, max_streams == 65535 ? "need 1..65535 streams of at least fft-size samples"
                                                                    : "need at least one stream of at least fft-size samples");
    if (const char* why = peaks_arg_error(0, e->cfg.rows, k, min_db)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (!aligned(peaks, 8)) return fail(e, EMSPEC_ERR_INVALID_ARG, "peaks must be 8-byte aligned");
    if (e->time_reduce > 1)
        return fail(e, EMSPEC_ERR_STATE, "peaks are those of full-rate columns: not available while a time reduction is set (emspec_set_time_reduce(e, 1) turns it off)");
    return EMSPEC_OK;
}

}  // namespace

extern "C" {

int emspec_peaks_device(emspec_engine* e, const float* db_dev, int64_t columns, int32_t rows, int32_t k, float min_db,
                        emspec_peak* peaks_dev, void* hip_stream) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (const char* why = peaks_arg_error(columns, rows, k, min_db)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    if (columns == 0) return EMSPEC_OK;
    if (!db_dev || !peaks_dev) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(db_dev, 16)) return fail(e, EMSPEC_ERR_INVALID_ARG, "db_dev must be 16-byte aligned");
    if (!aligned(peaks_dev, 8)) return fail(e, EMSPEC_ERR_INVALID_ARG, "peaks_dev must be 8-byte aligned");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_peaks(db_dev, columns, rows, k, min_db, peaks_dev, (hipStream_t)hip_stream));
    return EMSPEC_OK;
}

int emspec_peaks_host(const float* db, int64_t columns, int32_t rows, int32_t k, float min_db, emspec_peak* peaks_out) {
    if (const char* why = peaks_arg_error(columns, rows, k, min_db)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, why);
    if (columns == 0) return EMSPEC_OK;
    if (!db || !peaks_out) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!aligned(db, 4) || !aligned(peaks_out, 4)) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "db and peaks_out must be 4-byte aligned");
    const float ninf = -std::numeric_limits<float>::infinity();
    Cand top[32];
    for (int64_t col = 0; col < columns; ++col) {
        const float* x = db + (size_t)col * (size_t)rows;
        int have = 0;
        for (int r = 0; r < rows; ++r) {
            const float l = r > 0 ? x[r - 1] : ninf, rn = r + 1 < rows ? x[r + 1] : ninf;
            if (!(x[r] >= min_db && x[r] > l && x[r] >= rn)) continue;
            // insertion into the k best so far (rows arrive in ascending order: an equal dB goes behind)
            const Cand c{x[r], r};
            if (have == k && !before(c, top[k - 1])) continue;
            int at = have < k ? have++ : k - 1;
            for (; at > 0 && before(c, top[at - 1]); --at) top[at] = top[at - 1];
            top[at] = c;
        }
        emspec_peak* out = peaks_out + (size_t)col * (size_t)k;
        for (int t = 0; t < k; ++t) {
            if (t >= have) { out[t].pos = -1.0f; out[t].db = ninf; continue; }
            const int r = top[t].row;
            const float b = x[r];
            float d = 0.0f;
            if (r > 0 && r < rows - 1) {
                const float a = x[r - 1], c = x[r + 1];
                const float tt = a - c;
                const float u = (a - b) + (c - b);
                d = (0.5f * tt) / u;
                if (d > 0.5f) d = 0.5f;
                if (d < -0.5f) d = -0.5f;
                if (d != d) d = 0.0f;
            }
            out[t].pos = ((float)r + 0.5f) + d;
            std::memcpy(&out[t].db, &x[r], 4);   // the cell's own bits
        }
    }
    return EMSPEC_OK;
}

int emspec_batch_peaks_device(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign,
                              int32_t k, float min_db, emspec_peak* peaks_dev, void* hip_stream) {
    int rc = batch_peaks_check(e, pcm_dev, S, L, n, hop, k, min_db, peaks_dev, 65535);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const int R = e->cfg.rows;
    const int64_t C = emspec_num_columns(L, n, hop);
    // the dB of a chunk of streams goes to the engine workspace the time reduction's device entries use (never both: see the
    // check above), sized by the records path's budget rule; the kernel reads it from there, in stream order behind the batch
    return for_stream_chunks(e, (void**)&e->d_full, &e->full_bytes, (size_t)C * R * 4, 256, (size_t)4 << 30, S, [&](int s0, int sc, int) -> int {
        float* wdb = reinterpret_cast<float*>(e->d_full);
        if (int rc = batch_device_full(e, pcm_dev + (size_t)s0 * L, sc, L, n, hop, reassign, wdb, nullptr, nullptr, st)) return rc;
        HIPCHK(e, launch_peaks(wdb, (int64_t)sc * C, R, k, min_db, peaks_dev + (size_t)s0 * C * k, st));
        return EMSPEC_OK;
    });
}

int emspec_batch_peaks(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign, int32_t k,
                       float min_db, emspec_peak* peaks_out) {
    int rc = batch_peaks_check(e, pcm, S, L, n, hop, k, min_db, peaks_out, 0x7fffffff);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    const PeaksOut pko{peaks_out, k, min_db};
    HostJob job;
    job.src = pcm, job.S = S, job.L = L, job.n = n, job.hop = hop;
    // units as emspec_batch cuts them: runs of a stream's columns when there are few streams, whole streams for the display
    // post-process, which walks a stream in time order
    job.whole_streams = e->smoothing > 0.0f || e->agc > 0.0f, job.halo_D = latency(n, hop, reassign);
    job.pko = &pko;
    job.run = [=](const float* p, int sc, int64_t samples, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
        return batch_device_full(e, p, sc, samples, n, hop, reassign, db, rgba, index, st);
    };
    return host_batch(e, job);
}

int emspec_position_hz(emspec_engine* e, float pos, double* hz) {
    if (!e || !hz) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    const int R = e->cfg.rows;
    if (!(pos >= 0.0f && pos <= (float)R)) return fail(e, EMSPEC_ERR_INVALID_ARG, "pos must be in [0, rows]");
    std::vector<float> edge((size_t)R + 1);
    const int rc = emspec_get_row_edges_hz(e, edge.data(), R + 1);
    if (rc) return rc;
    const int i = std::min(std::max((int)std::floor(pos), 0), R - 1);
    const double lo = (double)edge[i], hi = (double)edge[i + 1];
    *hz = lo * std::pow(hi / lo, (double)pos - (double)i);
    return EMSPEC_OK;
}

}  // extern "C"
