// emspec_api.cpp — the C ABI of libemspec (include/emspec.h): engine, plan
// cache, streaming state, host<->device staging.  Compiled with hipcc.
//
// No reference FFI exists to mirror (reference source is private,
// /root/reference/README.md:73); the contract is SURVEY.md §8(b).
// There is deliberately NO CPU path here: without a gfx950 device
// emspec_create fails.
#include "emspec_engine.h"
#ifdef EMSPEC_DIAG
#pragma GCC visibility push(default)
#include "../../include/emspec_debug.h"
#pragma GCC visibility pop
#endif
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

using namespace emspec;

namespace {
thread_local std::string g_create_error = "";
}  // namespace

namespace emspec {
int fail(const emspec_engine* e, int code, const std::string& msg) {
    if (e) e->err = msg; else g_create_error = msg;
    return code;
}
int grow(emspec_engine* e, void** ptr, size_t* have, size_t want) {
    if (*have >= want) return EMSPEC_OK;
    if (*ptr) { HIPCHK(e, hipFree(*ptr)); *ptr = nullptr; *have = 0; }
    HIPCHK(e, hipMalloc(ptr, want));   // (hipErrorOutOfMemory -> EMSPEC_ERR_OUT_OF_MEMORY; *ptr stays null, *have 0)
    *have = want;
    return EMSPEC_OK;
}
}  // namespace emspec

namespace emspec {   // (internal linkage is not needed: the library exports only what emspec.map lists; emspec_live.cpp uses these)

int check_shape(const emspec_engine* e, int n, int hop) {
    if (!supported_fft(n)) return fail(e, EMSPEC_ERR_INVALID_ARG, "fft size must be a power of two in [256,16384]");
    if (hop < 1 || hop > n) return fail(e, EMSPEC_ERR_INVALID_ARG, "hop must be in [1, fft size]");
    return EMSPEC_OK;
}

// The shape's tables (emspec_tables.h; DESIGN.md §3 "Tables"), built on the host and uploaded.
int get_plan(emspec_engine* e, int n, Plan** out) {
    auto it = e->plans.find(n);
    if (it != e->plans.end()) { *out = &it->second; return EMSPEC_OK; }
    Plan p;
    p.n = n;
    const int R = p.rows = e->cfg.rows;
    p.h_tw = twiddles32(n);
    p.h_ebin64 = edges_bin64(axis_of(e->cfg, e->custom_edges_hz), n);
    p.h_ebin = edges_bin32(p.h_ebin64);
    if (const char* why = edges_error(p.h_ebin)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
    HIPCHK(e, hipMalloc(&p.d_tw, sizeof(float) * n));
    HIPCHK(e, hipMalloc(&p.d_ebin, sizeof(float) * (R + 1)));
    HIPCHK(e, hipMemcpy(p.d_tw, p.h_tw.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(p.d_ebin, p.h_ebin.data(), sizeof(float) * (R + 1), hipMemcpyHostToDevice));
    if (e->exact()) {   // the same tables in binary64
        if (const char* why = edges_error(p.h_ebin64)) return fail(e, EMSPEC_ERR_INVALID_ARG, why);
        const std::vector<double> tw = twiddles64(n);
        HIPCHK(e, hipMalloc(&p.d_tw64, sizeof(double) * n));
        HIPCHK(e, hipMalloc(&p.d_ebin64, sizeof(double) * (R + 1)));
        HIPCHK(e, hipMemcpy(p.d_tw64, tw.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(p.d_ebin64, p.h_ebin64.data(), sizeof(double) * (R + 1), hipMemcpyHostToDevice));
    }
    auto ins = e->plans.emplace(n, std::move(p));
    *out = &ins.first->second;
    return EMSPEC_OK;
}

// A band of the table for the multi-resolution batch: rows [row0, row0 + rows) as a SLICE of the full plan's edge tables (float32
// and binary64) - recomputing a band's table from its own ends would differ in the last bit and move bins across edges.  The
// twiddles are the full plan's (both plans live until drop_plans, which drops them together).
int get_band_plan(emspec_engine* e, int n, int row0, int rows, Plan** out) {
    const auto key = std::make_tuple(n, row0, rows);
    auto it = e->band_plans.find(key);
    if (it != e->band_plans.end()) { *out = &it->second; return EMSPEC_OK; }
    Plan* full;
    int rc;
    if ((rc = get_plan(e, n, &full))) return rc;
    if (row0 < 0 || rows < 1 || row0 + rows > full->rows) return fail(e, EMSPEC_ERR_INVALID_ARG, "band outside the row table");
    Plan p;
    p.n = n;
    p.row0 = row0;
    p.rows = rows;
    p.d_tw = full->d_tw;
    p.d_tw64 = full->d_tw64;
    p.h_ebin.assign(full->h_ebin.begin() + row0, full->h_ebin.begin() + row0 + rows + 1);
    p.h_ebin64.assign(full->h_ebin64.begin() + row0, full->h_ebin64.begin() + row0 + rows + 1);
    HIPCHK(e, hipMalloc(&p.d_ebin, sizeof(float) * (rows + 1)));
    HIPCHK(e, hipMemcpy(p.d_ebin, p.h_ebin.data(), sizeof(float) * (rows + 1), hipMemcpyHostToDevice));
    if (e->exact()) {
        HIPCHK(e, hipMalloc(&p.d_ebin64, sizeof(double) * (rows + 1)));
        HIPCHK(e, hipMemcpy(p.d_ebin64, p.h_ebin64.data(), sizeof(double) * (rows + 1), hipMemcpyHostToDevice));
    }
    auto ins = e->band_plans.emplace(key, std::move(p));
    *out = &ins.first->second;
    return EMSPEC_OK;
}

// log_rows: the configured log axis, wide enough in every row for the float32 log2 hint (a narrower one is searched)
static bool plan_log_rows(const emspec_engine* e, const Plan& p) {
    return e->custom_edges_hz.empty() && hint_rows_ok(p.h_ebin64.front(), p.h_ebin64.back(), p.rows);
}
static PlanScalars scalars_of(const emspec_engine* e, const Plan& p, int hop, int reassign) {
    return plan_scalars(e->cfg, p.rows, plan_log_rows(e, p), p.n, hop, reassign);
}
PlanDev plan_dev(const emspec_engine* e, const Plan& p, int hop, int reassign) {
    const PlanScalars c = scalars_of(e, p, hop, reassign);
    PlanDev d;
    d.tw = p.d_tw;
    d.ebin = p.d_ebin;
    d.rows = c.rows;
    d.log_rows = c.log_rows;
    d.D = c.D;
    d.reassign = c.reassign;
    d.hop = c.hop;
    d.tscale = c.tscale32;
    d.pfloor_abs = c.pfloor_abs;
    // "shared" = 1: other kernels take CUs while a fused launch runs (a communicator with other ranks: RCCL transfers, the
    // gather's pack / expand) -> the shared-device segment plan.  2: this engine's own two-lane host pipeline (emspec_batch
    // runs neighbouring stream-chunks on two HIP streams): two fused launches share the chip, so segments are capped at
    // 1,024 columns (a one-round plan of very long workgroups would degenerate into two rounds); the chunks of that pipeline
    // are small (96 MB of staging), so their segments are short anyway and keep the exclusive plan's low halo.
    d.shared = comm_shares_device(e) ? 1 : 0;
    return d;
}

// EXACT mode: the plan and the dB map in binary64
ExactPlanDev exact_plan_dev(const emspec_engine* e, const Plan& p, int hop, int reassign) {
    const PlanScalars c = scalars_of(e, p, hop, reassign);
    const ExactScalars x = exact_scalars(p.n, c.rows, c.pfloor, p.h_ebin64.front(), p.h_ebin64.back());
    ExactPlanDev d;
    d.tw = p.d_tw64;
    d.ebin = p.d_ebin64;
    d.rows = c.rows;
    d.log_rows = c.log_rows;
    d.D = c.D;
    d.reassign = c.reassign;
    d.hop = c.hop;
    d.tscale = c.tscale;
    d.pfloor = c.pfloor;
    d.pmax = x.pmax;
    d.qscale = x.qscale;
    d.pfloor64 = x.pfloor64;
    d.pmax64 = x.pmax64;
    d.qscale64 = x.qscale64;
    d.e0 = p.h_ebin64.front();
    d.eR = p.h_ebin64.back();
    d.l2e0 = x.l2e0;
    d.rscale = x.rscale;
    return d;
}
ExactDbMap exact_db_map(const emspec_engine* e, int n, const ExactPlanDev& pd) {
    const DbScalars m = exact_db_scalars(e->cfg, n, pd.qscale);
    return ExactDbMap{m.scale, m.lo, m.inv_range, m.gate};
}
DbMap db_map(const emspec_engine* e, int n) {
    const DbScalars m = db_scalars(e->cfg, n);
    return DbMap{m.scale, m.lo, m.inv_range, m.gate};
}

}  // namespace emspec

static void drop_plans(emspec_engine* e);

extern "C" {

int emspec_default_config(emspec_config* c) {
    if (!c) return EMSPEC_ERR_INVALID_ARG;
    std::memset(c, 0, sizeof(*c));
    c->abi_version = EMSPEC_ABI_VERSION;
    c->device = 0;
    c->rows = 1024;
    c->sample_rate = 48000.0f;
    c->fmin_hz = 20.0f;
    c->fmax_hz = 24000.0f;
    c->gain = 1.0f;
    c->db_top = 0.0f;
    c->db_range = 80.0f;
    c->gate_db = -80.0f;
    c->power_floor = 1e-14f;
    return EMSPEC_OK;
}

int emspec_create(const emspec_config* cfg, emspec_engine** out) {
    if (!cfg || !out) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (cfg->abi_version != EMSPEC_ABI_VERSION) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "abi_version mismatch");
    if (cfg->rows < 64 || cfg->rows > 4096 || cfg->rows % 4) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "rows must be a multiple of 4 in [64,4096]");
    if (cfg->mode != EMSPEC_MODE_FAST && cfg->mode != EMSPEC_MODE_EXACT) return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "mode must be EMSPEC_MODE_FAST or EMSPEC_MODE_EXACT");
    if (!(cfg->sample_rate > 0) || !(cfg->fmin_hz > 0) || !(cfg->fmax_hz > cfg->fmin_hz) || !(cfg->db_range > 0) ||
        !(cfg->gain > 0) || !(cfg->power_floor >= 0))
        return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "bad sample_rate/fmin/fmax/db_range/gain/power_floor");
    if (cfg->fmax_hz > 0.5f * cfg->sample_rate)
        return fail(nullptr, EMSPEC_ERR_INVALID_ARG, "fmax_hz must not exceed sample_rate/2");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, EMSPEC_ERR_NO_DEVICE, "no HIP device available (libemspec has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, EMSPEC_ERR_NO_DEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return fail(nullptr, EMSPEC_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, EMSPEC_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    emspec_engine* e = new (std::nothrow) emspec_engine();
    if (!e) return fail(nullptr, EMSPEC_ERR_OUT_OF_MEMORY, "out of host memory");
    e->cfg = *cfg;
    e->device = cfg->device;
    e->arch = prop.gcnArchName;
    int rc = EMSPEC_OK;
    do {
        if (hipSetDevice(e->device) != hipSuccess) { rc = fail(nullptr, EMSPEC_ERR_HIP, "hipSetDevice failed"); break; }
        if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(nullptr, EMSPEC_ERR_HIP, "hipStreamCreate failed"); break; }
        // the copy streams of the host-buffer pipeline, created with the engine: which copy engine a HIP stream's transfers run on
        // follows from the order streams are made in, and two that are made late in a process full of other streams can land on
        // ONE engine - H2D and D2H then take turns (measured: index out 3.4e7 instead of 4.4e7 columns/s)
        if (hipStreamCreateWithFlags(&e->stream_in, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&e->stream_out, hipStreamNonBlocking) != hipSuccess) { rc = fail(nullptr, EMSPEC_ERR_HIP, "hipStreamCreate failed"); break; }
        if (hipMalloc(&e->d_lut, 1024 + 64) != hipSuccess) { rc = fail(nullptr, EMSPEC_ERR_OUT_OF_MEMORY, "hipMalloc(lut) failed"); break; }
        uint8_t lut[1024];
        default_lut(lut);
        if (hipMemcpy(e->d_lut, lut, 1024, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(nullptr, EMSPEC_ERR_HIP, "lut upload failed"); break; }
    } while (0);
    if (rc != EMSPEC_OK) { emspec_destroy(e); return rc; }
    *out = e;
    return EMSPEC_OK;
}

void emspec_destroy(emspec_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->stream_in) (void)hipStreamSynchronize(e->stream_in);
    if (e->stream_out) (void)hipStreamSynchronize(e->stream_out);
    comm_destroy(e);
    live_destroy(e);
    stereo_destroy(e);
    drop_plans(e);
    (void)hipFree(e->d_xlow);
    if (e->xlow_event) (void)hipEventDestroy(e->xlow_event);
    (void)hipFree(e->d_lut); (void)hipFree(e->d_hist); (void)hipFree(e->d_stage);
    (void)hipFree(e->d_raw); (void)hipFree(e->d_post); (void)hipFree(e->d_peak); (void)hipFree(e->d_mres);
    (void)hipFree(e->d_full);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->stream_in) (void)hipStreamDestroy(e->stream_in);
    if (e->stream_out) (void)hipStreamDestroy(e->stream_out);
    for (auto& ev : e->pipe_ev) if (ev) (void)hipEventDestroy(ev);
    if (e->h_hdr) (void)hipHostFree(e->h_hdr);
    (void)hipFree(e->d_packscratch);
    delete e;
}

const char* emspec_last_error(const emspec_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }
int32_t emspec_mode(const emspec_engine* e) { return e ? e->cfg.mode : -1; }
#ifndef EMSPEC_SOURCES_SHA
#define EMSPEC_SOURCES_SHA "unknown"
#endif
#define EMSPEC_STR2(x) #x
#define EMSPEC_STR(x) EMSPEC_STR2(x)
const char* emspec_build_info(void) { return "emspec abi=" EMSPEC_STR(EMSPEC_ABI_VERSION) " sources=" EMSPEC_SOURCES_SHA " arch=gfx950"; }
int emspec_device_status(emspec_engine* e) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipDeviceSynchronize());
    const int w = read_kernel_error(true);
    if (w != 0) return fail(e, EMSPEC_ERR_HIP, w < 0 ? "the device's kernel error word could not be read"
                                                  : "a kernel's bounded wait timed out (protocol error): the results of the launches since the last check are invalid");
    return EMSPEC_OK;
}
const char* emspec_device_arch(const emspec_engine* e) { return e ? e->arch.c_str() : ""; }
}  // extern "C"
// EXACT mode: the kernel family that serves plan p of this engine (the shape, and for the no-parking kernel the axis)
static Route exact_route_of(const emspec_engine* e, int n, const ExactPlanDev& pd, int row0 = 0) {
    return exact_route(n, pd, row0, axis_of(e->cfg, e->custom_edges_hz));
}
extern "C" {
int emspec_uses_fused(const emspec_engine* e, int32_t n, int32_t hop, int32_t reassign) {
    if (!e || n < 1 || hop < 1) return 0;
    if (e->exact()) {   // only the shape and the axis decide (the route reads rows and D)
        ExactPlanDev pd{};
        pd.rows = e->cfg.rows;
        pd.D = latency(n, hop, reassign);
        return is_records(exact_route_of(e, n, pd)) ? 0 : 1;
    }
    return fused_supported(n, hop, e->cfg.rows, reassign) ? 1 : 0;
}

static void drop_plans(emspec_engine* e) {
    for (auto& kv : e->band_plans) { (void)hipFree(kv.second.d_ebin); (void)hipFree(kv.second.d_ebin64); }   // (twiddles: the full plans')
    e->band_plans.clear();
    for (auto& kv : e->plans) {
        (void)hipFree(kv.second.d_tw); (void)hipFree(kv.second.d_ebin);
        (void)hipFree(kv.second.d_tw64); (void)hipFree(kv.second.d_ebin64);
    }
    e->plans.clear();
}

int emspec_set_row_edges_hz(emspec_engine* e, const float* edges_hz, int32_t count) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (live_pending(e)) return fail(e, EMSPEC_ERR_STATE, "columns are pending; flush or reset before changing the row edges");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (!edges_hz) {   // back to the configured log axis
        e->custom_edges_hz.clear();
        drop_plans(e);
        return EMSPEC_OK;
    }
    if (count != e->cfg.rows + 1) return fail(e, EMSPEC_ERR_INVALID_ARG, "need rows+1 edges");
    for (int r = 0; r <= e->cfg.rows; ++r) {
        const float f = edges_hz[r];
        if (!(f > 0.0f) || !(f <= 0.5f * e->cfg.sample_rate) || (r > 0 && !(f > edges_hz[r - 1])))
            return fail(e, EMSPEC_ERR_INVALID_ARG, "row edges must be strictly increasing in (0, sample_rate/2]");
    }
    e->custom_edges_hz.assign(edges_hz, edges_hz + count);
    drop_plans(e);
    return EMSPEC_OK;
}

int emspec_warped_edges_hz(int32_t rows, float fmin_hz, float fmax_hz, float low_end_boost, float freq_scale,
                           float* out) {
    if (!out || rows < 1 || !(fmin_hz > 0.0f) || !(fmax_hz > fmin_hz) || !(low_end_boost > 0.0f) || !(freq_scale > 0.0f))
        return EMSPEC_ERR_INVALID_ARG;
    warped_edges_hz(rows, fmin_hz, fmax_hz, low_end_boost, freq_scale, out);
    return EMSPEC_OK;
}

int emspec_make_colormap(float brightness, uint8_t* out) {
    if (!out || !(brightness >= 0.0f)) return EMSPEC_ERR_INVALID_ARG;
    make_colormap(brightness, out);
    return EMSPEC_OK;
}

int emspec_get_row_edges_hz(emspec_engine* e, float* edges_hz, int32_t count) {
    if (!e || !edges_hz) return EMSPEC_ERR_INVALID_ARG;
    if (count != e->cfg.rows + 1) return fail(e, EMSPEC_ERR_INVALID_ARG, "need room for rows+1 edges");
    const Axis axis = axis_of(e->cfg, e->custom_edges_hz);
    for (int r = 0; r <= axis.rows; ++r) edges_hz[r] = (float)edge_hz(axis, r);
    return EMSPEC_OK;
}

int emspec_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return EMSPEC_ERR_INVALID_ARG;
    *out = nullptr;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return EMSPEC_ERR_OUT_OF_MEMORY; }
    return EMSPEC_OK;
}
void emspec_host_free(void* p) { if (p) (void)hipHostFree(p); }

int emspec_set_colormap(emspec_engine* e, const uint8_t* rgba) {
    if (!e || !rgba) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(e->d_lut, rgba, 1024, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return EMSPEC_OK;
}

int64_t emspec_num_columns(int64_t L, int32_t n, int32_t hop) {
    if (n <= 0 || hop <= 0 || L < n) return 0;
    return (L - n) / hop + 1;
}

int32_t emspec_latency_columns(int32_t n, int32_t hop, int32_t reassign) {
    if (n <= 0 || hop <= 0) return 0;
    return latency(n, hop, reassign);
}

int emspec_get_tables(emspec_engine* e, int32_t n, float* edges, float* tw) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    int rc = check_shape(e, n, 1);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    Plan* p;
    if ((rc = get_plan(e, n, &p))) return rc;
    // read back what the kernels actually see
    if (edges) HIPCHK(e, hipMemcpy(edges, p->d_ebin, sizeof(float) * (e->cfg.rows + 1), hipMemcpyDeviceToHost));
    if (tw) HIPCHK(e, hipMemcpy(tw, p->d_tw, sizeof(float) * n, hipMemcpyDeviceToHost));
    return EMSPEC_OK;
}

}  // extern "C"

bool emspec::host_pinned(const void* p) {
    if (!p) return true;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

// Per-bin record workspaces (the shapes without a fused kernel): streams are processed in chunks so that the workspace
// stays bounded.  The budget follows the device: a quarter of what is free (counting what this engine already holds),
// at least 256 MiB, at most `cap` - a chunk only has to cover enough streams to fill the CUs, so a few GiB cost nothing
// measurable, and a fixed 12 GiB (round 3) pinned that much HBM per EXACT engine for its lifetime.  When the allocation
// fails all the same, the chunk is halved and tried again; one stream that does not fit is an out-of-memory error.
// (grow_chunked: the same rule for any engine workspace *ptr; the multi-resolution batch sizes its band workspace by it)
int emspec::grow_chunked(emspec_engine* e, void** ptr, size_t* have, size_t per_stream, size_t extra, size_t cap, int S, int* chunk_out) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = cap * 4; }
    int64_t budget_mb = -1;
#ifdef EMSPEC_DIAG
    if (const char* ev = getenv("EMSPEC_RECORD_BUDGET_MB")) budget_mb = atol(ev);   // test hook: force several stream-chunks
#endif
    // the budget, the first chunk and the halving: emspec_kernel_plan.h
    for (ChunkPlan cp = first_chunk(free_b, *have, per_stream, extra, cap, S, budget_mb);; cp = next_chunk(cp, per_stream, extra)) {
        const int rc = grow(e, ptr, have, cp.bytes);
        if (rc == EMSPEC_OK) { *chunk_out = cp.chunk; return EMSPEC_OK; }
        (void)hipGetLastError();
        if (rc != EMSPEC_ERR_OUT_OF_MEMORY || cp.chunk == 1) return rc;
    }
}
static int grow_record_workspace(emspec_engine* e, size_t per_stream, size_t extra, size_t cap, int S, int* chunk_out) {
    return grow_chunked(e, (void**)&e->d_hist, &e->hist_bytes, per_stream, extra, cap, S, chunk_out);
}

// columns of S device-resident streams -> dB / RGBA / index, no display post-process
static int run_columns(emspec_engine* e, const PlanDev& pd, const DbMap& m, const float* pcm, int32_t S, int64_t L,
                       int32_t n, int32_t hop, int32_t reassign, int64_t C, float* db, uint8_t* rgba, uint8_t* index,
                       hipStream_t st) {
    int rc;
    if (fused_supported(n, hop, pd.rows, reassign)) {
        HIPCHK(e, launch_fused(n, pd, m, e->d_lut, pcm, L, S, C, db, rgba, index, st));
        return EMSPEC_OK;
    }
    // generic path: per-bin records (frames_kernel) -> 32-column LDS tiles (tile_scatter_kernel),
    // in chunks of streams so the record workspace stays bounded
    int chunk = 1;
    if ((rc = grow_record_workspace(e, f32_record_bytes(n, C), 0, (size_t)4 << 30, S, &chunk))) return rc;
    const size_t col_cells = (size_t)C * pd.rows;
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int sc = (S - s0 < chunk) ? S - s0 : chunk;
        FrameSinks sk;
        sk.records = reinterpret_cast<uint2*>(e->d_hist);
        HIPCHK(e, launch_frames(n, pd, pcm + (size_t)s0 * L, L, sc, 0, C, sk, st));
        HIPCHK(e, launch_tile_scatter(sk.records, n, pd, m, e->d_lut, sc, C, db ? db + s0 * col_cells : nullptr,
                                      rgba ? rgba + 4 * s0 * col_cells : nullptr,
                                      index ? index + s0 * col_cells : nullptr, st));
    }
    return EMSPEC_OK;
}

// The low-row scratch of the EXACT kernels, `need` bytes: grown on demand; a launch on another HIP stream than the previous
// one waits for it (one scratch per engine: two launches must not run side by side on it)
static int xlow_prepare(emspec_engine* e, size_t need, hipStream_t st) {
    int rc;
    if (need > e->xlow_bytes) {
        if (e->xlow_used) HIPCHK(e, hipEventSynchronize(e->xlow_event));      // the old buffer may still be in use
        if ((rc = grow(e, (void**)&e->d_xlow, &e->xlow_bytes, need))) return rc;
    }
    if (!e->xlow_event) HIPCHK(e, hipEventCreateWithFlags(&e->xlow_event, hipEventDisableTiming));
    if (e->xlow_used) HIPCHK(e, hipStreamWaitEvent(st, e->xlow_event, 0));
    e->xlow_used = true;
    return EMSPEC_OK;
}
// (the no-parking kernel's: exact_fused_lr.hip.inc)
static int exact_lr_prepare(emspec_engine* e, int n, const ExactPlanDev& pd, int rl, int S, int64_t C, hipStream_t st) {
    return rl <= 0 ? EMSPEC_OK : xlow_prepare(e, exact_fused_lr_scratch_bytes(n, pd, rl, S, C), st);
}

// EXACT mode: per-bin (q, key) records (exact_frames_kernel) -> u64 LDS tiles (exact_tile_scatter_kernel), in chunks of
// streams so the record workspace stays bounded
static int run_columns_exact(emspec_engine* e, const Plan& p, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop,
                             int32_t reassign, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
    int rc;
    const ExactPlanDev pd = exact_plan_dev(e, p, hop, reassign);
    const ExactDbMap m = exact_db_map(e, n, pd);
    const Route route = exact_route_of(e, n, pd, p.row0);
    if (route.kind == RouteKind::exact_lr) {   // one kernel, no records, no parking (exact_fused_lr.hip.inc)
        const int rl = route.rl;
        if ((rc = exact_lr_prepare(e, n, pd, rl, S, C, st))) return rc;
        HIPCHK(e, launch_exact_fused_lr(n, pd, m, e->d_lut, pcm, L, S, C, rl, e->d_xlow, e->xlow_bytes, db, rgba, index, st));
        if (rl > 0) HIPCHK(e, hipEventRecord(e->xlow_event, st));
        return EMSPEC_OK;
    }
    if (route.kind == RouteKind::exact_parked) {   // one kernel with the ring parked under the planes (exact_fused.hip.inc): any axis
        HIPCHK(e, launch_exact_fused(n, pd, m, e->d_lut, pcm, L, S, C, db, rgba, index, st));
        return EMSPEC_OK;
    }
    const ExactRecords rec = exact_record_bytes(n, C);
    int chunk = 1;
    // (8 GiB here, 4 GiB for the float32 records: the walking scatter reads a 2D-frame halo per segment, and a stream-chunk's
    // segments get longer with the streams it holds - five streams of configs[4] per chunk: 23 % halo, ten: 12 %; 67.5 -> 66.1 ms per step, and 16 GiB measured 67.0)
    if ((rc = grow_record_workspace(e, rec.per_stream, kChunkPad, (size_t)8 << 30, S, &chunk))) return rc;
    const size_t col_cells = (size_t)C * pd.rows;
    // the scatter's low-row scratch (exact.hip.inc: a ring too large for LDS is walked with its sparse low rows in global
    // memory); cleared once per batch - the kernel leaves it zero, this only guards against a launch that was cut short
    const float* ebin_host = p.h_ebin.data();
    // (the last chunk may hold fewer streams, and fewer streams are cut into more segments: size for both)
    const size_t low_need = std::max(exact_scatter_scratch_bytes(n, pd, chunk, C, ebin_host),
                                     S % chunk ? exact_scatter_scratch_bytes(n, pd, S % chunk, C, ebin_host) : (size_t)0);
    if (low_need) {
        if ((rc = xlow_prepare(e, low_need, st))) return rc;
        HIPCHK(e, hipMemsetAsync(e->d_xlow, 0, low_need, st));
    }
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int sc = (S - s0 < chunk) ? S - s0 : chunk;
        ExactSinks sk;
        sk.rec_q = reinterpret_cast<long long*>(e->d_hist);
        sk.rec_key = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(e->d_hist) + second_array_offset(rec.q_per_stream, chunk));
        HIPCHK(e, launch_exact_frames(n, pd, pcm + (size_t)s0 * L, L, sc, 0, C, sk, st));
        HIPCHK(e, launch_exact_tile_scatter(sk.rec_q, sk.rec_key, n, pd, m, e->d_lut, sc, C, db ? db + s0 * col_cells : nullptr,
                                            rgba ? rgba + 4 * s0 * col_cells : nullptr,
                                            index ? index + s0 * col_cells : nullptr, st, low_need ? ebin_host : nullptr,
                                            low_need ? e->d_xlow : nullptr, low_need));   // (only what was cleared above: the buffer may be larger)
    }
    if (low_need) HIPCHK(e, hipEventRecord(e->xlow_event, st));
    return EMSPEC_OK;
}

namespace emspec {
int run_plan_columns(emspec_engine* e, const Plan& p, const float* pcm, int32_t S, int64_t L, int32_t hop, int32_t reassign,
                     int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
    if (e->exact()) return run_columns_exact(e, p, pcm, S, L, p.n, hop, reassign, C, db, rgba, index, st);
    return run_columns(e, plan_dev(e, p, hop, reassign), db_map(e, p.n), pcm, S, L, p.n, hop, reassign, C, db, rgba, index, st);
}
}  // namespace emspec

// Time reduction of a device entry: the full-rate columns of a chunk of streams - dB when the caller wants dB,
// the palette index when it wants index or RGBA - go to the engine workspace d_full, sized by the records path's budget rule,
// and one launch of reduce.hip.inc's kernel writes that chunk's reduced columns into the caller's arrays.
int emspec::reduce_streams(emspec_engine* e, int32_t S, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st,
                           const FullRun& full) {
    const int R = e->cfg.rows, f = e->time_reduce;
    const size_t cells = (size_t)C * R, rcells = (size_t)reduced_columns(C, f) * R;
    const size_t db_s = db ? cells * 4 : 0, idx_s = (index || rgba) ? cells : 0;   // (cells is a multiple of 4: both stay 16-byte aligned ...
    return for_stream_chunks(e, (void**)&e->d_full, &e->full_bytes, db_s + idx_s, kChunkPad, (size_t)4 << 30, S, [&](int s0, int sc, int chunk) -> int {
        float* wdb = db ? reinterpret_cast<float*>(e->d_full) : nullptr;
        uint8_t* widx = idx_s ? reinterpret_cast<uint8_t*>(e->d_full) + second_array_offset(db_s, chunk) : nullptr;   // ... and this 256)
        if (int rc = full(s0, sc, wdb, widx)) return rc;
        const size_t o = (size_t)s0 * rcells;
        HIPCHK(e, launch_reduce_columns(wdb, widx, sc, C, R, f, cells, rcells, e->d_lut, db ? db + o : nullptr,
                                        index ? index + o : nullptr, rgba ? rgba + 4 * o : nullptr, st));
        return EMSPEC_OK;
    });
}

int emspec::batch_device_full(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign,
                              float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
    int rc;
    if (S < 1 || S > 65535 || L < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need 1..65535 streams of at least fft-size samples");
    Plan* p;
    if ((rc = get_plan(e, n, &p))) return rc;
    const PlanDev pd = plan_dev(e, *p, hop, reassign);
    const DbMap m = db_map(e, n);
    const int64_t C = emspec_num_columns(L, n, hop);
    if (!db && !rgba && !index) return EMSPEC_OK;
    if (e->smoothing > 0.0f || e->agc > 0.0f) {
        // raw dB columns into a workspace, then AGC + temporal smoothing into the caller's buffers
        const size_t cells = (size_t)S * C * e->cfg.rows;
        if ((rc = grow(e, (void**)&e->d_raw, &e->raw_bytes, cells * 4))) return rc;
        if ((rc = grow(e, (void**)&e->d_peak, &e->peak_bytes, (size_t)S * C * 8 + 16))) return rc;
        float* outdb = db;
        if (!outdb) { if ((rc = grow(e, (void**)&e->d_post, &e->post_bytes, cells * 4))) return rc; outdb = e->d_post; }
        if ((rc = e->exact() ? run_columns_exact(e, *p, pcm, S, L, n, hop, reassign, C, e->d_raw, nullptr, nullptr, st)
                             : run_columns(e, pd, m, pcm, S, L, n, hop, reassign, C, e->d_raw, nullptr, nullptr, st))) return rc;
        HIPCHK(e, launch_postprocess(e->d_raw, outdb, rgba, index, S, C, e->cfg.rows, e->smoothing, e->agc,
                                     e->cfg.db_top, m, e->d_lut, e->d_peak, e->d_peak + (size_t)S * C, st));
        return EMSPEC_OK;
    }
    if (e->exact()) return run_columns_exact(e, *p, pcm, S, L, n, hop, reassign, C, db, rgba, index, st);
    return run_columns(e, pd, m, pcm, S, L, n, hop, reassign, C, db, rgba, index, st);
}

extern "C" {

int emspec_batch_device(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop,
                        int32_t reassign, float* db, uint8_t* rgba, uint8_t* index, void* hip_stream) {
    if (!e || !pcm) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (S < 1 || S > 65535 || L < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need 1..65535 streams of at least fft-size samples");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;   // NULL = the HIP default stream
    if (!db && !rgba && !index) {   // (the shape's tables are still built: a row table that cannot be is reported)
        Plan* p;
        return get_plan(e, n, &p);
    }
    if (e->time_reduce == 1) return batch_device_full(e, pcm, S, L, n, hop, reassign, db, rgba, index, st);
    return reduce_streams(e, S, emspec_num_columns(L, n, hop), db, rgba, index, st, [=](int s0, int sc, float* fdb, uint8_t* fidx) {
        return batch_device_full(e, pcm + (size_t)s0 * L, sc, L, n, hop, reassign, fdb, nullptr, fidx, st);
    });
}

#ifdef EMSPEC_DIAG   // diagnostic entry points (include/emspec_debug.h): libemspec_diag.so only
// Diagnostic: enqueue a kernel that keeps `groups` workgroups resident for ~usec microseconds on hip_stream.
int emspec_debug_occupy(emspec_engine* e, int32_t groups, int32_t usec, void* hip_stream) {
    if (!e || groups < 1 || groups > 4096 || usec < 1 || usec > 2000000) return fail(e, EMSPEC_ERR_INVALID_ARG, "bad argument");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_occupy(groups, usec, reinterpret_cast<unsigned*>(e->d_lut) + 256, (hipStream_t)hip_stream));   // (a spare word behind the palette)
    return EMSPEC_OK;
}

// Diagnostic (tests only): evaluate the fused kernels' row lookup as the plan of fft size n would run it (hinted, or searched
// where hint_rows_ok refuses the axis) and the generic binary search on `count` host values of k-hat.
int emspec_debug_row_lookup(emspec_engine* e, int32_t n, const float* kh, int64_t count, int32_t* out_hint,
                            int32_t* out_exact) {
    if (!e || !kh || !out_hint || !out_exact || count < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = check_shape(e, n, 1);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    Plan* p;
    if ((rc = get_plan(e, n, &p))) return rc;
    float* d_kh = nullptr; int32_t *d_a = nullptr, *d_b = nullptr;
    hipError_t r = hipMalloc(&d_kh, count * 4 + 4);
    if (r == hipSuccess) r = hipMalloc(&d_a, count * 4 + 4);
    if (r == hipSuccess) r = hipMalloc(&d_b, count * 4 + 4);
    if (r == hipSuccess) r = hipMemcpyAsync(d_kh, kh, count * 4, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = launch_row_lookup_probe(p->d_ebin, e->cfg.rows, plan_log_rows(e, *p) ? 1 : 0, d_kh, count, d_a, d_b, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(out_hint, d_a, count * 4, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(out_exact, d_b, count * 4, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    (void)hipFree(d_kh); (void)hipFree(d_a); (void)hipFree(d_b);
    HIPCHK(e, r);
    return EMSPEC_OK;
}

int emspec_debug_recip(emspec_engine* e, const float* d, int64_t count, float* out_short, float* out_ieee) {
    if (!e || !d || !out_short || !out_ieee || count < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    HIPCHK(e, hipSetDevice(e->device));
    float *d_in = nullptr, *d_a = nullptr, *d_b = nullptr;
    hipError_t r = hipMalloc(&d_in, count * 4 + 4);
    if (r == hipSuccess) r = hipMalloc(&d_a, count * 4 + 4);
    if (r == hipSuccess) r = hipMalloc(&d_b, count * 4 + 4);
    if (r == hipSuccess) r = hipMemcpyAsync(d_in, d, count * 4, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = launch_recip_probe(d_in, count, d_a, d_b, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(out_short, d_a, count * 4, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(out_ieee, d_b, count * 4, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    (void)hipFree(d_in); (void)hipFree(d_a); (void)hipFree(d_b);
    HIPCHK(e, r);
    return EMSPEC_OK;
}

int emspec_debug_recip64(emspec_engine* e, const double* d, int64_t count, double* out_short, double* out_ieee) {
    if (!e || !d || !out_short || !out_ieee || count < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    HIPCHK(e, hipSetDevice(e->device));
    double *d_in = nullptr, *d_a = nullptr, *d_b = nullptr;
    hipError_t r = hipMalloc(&d_in, count * 8 + 8);
    if (r == hipSuccess) r = hipMalloc(&d_a, count * 8 + 8);
    if (r == hipSuccess) r = hipMalloc(&d_b, count * 8 + 8);
    if (r == hipSuccess) r = hipMemcpyAsync(d_in, d, count * 8, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = launch_recip64_probe(d_in, count, d_a, d_b, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(out_short, d_a, count * 8, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(out_ieee, d_b, count * 8, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    (void)hipFree(d_in); (void)hipFree(d_a); (void)hipFree(d_b);
    HIPCHK(e, r);
    return EMSPEC_OK;
}

// Diagnostic (not part of the product path): run the stamped build of the fused kernel and
// return, per workgroup and wave, the cycles spent in each barrier-delimited phase.
// cycles: [groups][waves][8 slots] uint64 on the HOST; *groups receives the workgroup count and
// *waves the waves per workgroup (call with cycles == NULL first to size the buffer).
int emspec_debug_phase_cycles(emspec_engine* e, const float* pcm_dev, int32_t S, int64_t L, int32_t n, int32_t hop,
                              int32_t reassign, float* db_dev, uint8_t* index_dev, uint64_t* cycles, int64_t* groups,
                              int32_t* waves) {
    if (!e || !pcm_dev || !groups) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    HIPCHK(e, hipSetDevice(e->device));
    Plan* p;
    int rc;
    if ((rc = get_plan(e, n, &p))) return rc;
    // sizing call (stamps null: *groups), allocate, stamped launch, copy back, free
    auto stamped = [&](int wpg, auto&& launch) -> int {
        HIPCHK(e, launch(nullptr));
        if (waves) *waves = wpg;
        if (!cycles) return EMSPEC_OK;
        unsigned long long* d = nullptr;
        const size_t bytes = (size_t)(*groups) * wpg * 8 * sizeof(unsigned long long);
        HIPCHK(e, hipMalloc(&d, bytes));
        hipError_t r = launch(d);
        if (r == hipSuccess) r = hipMemcpyAsync(cycles, d, bytes, hipMemcpyDeviceToHost, e->stream);
        if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
        (void)hipFree(d);
        HIPCHK(e, r);
        return EMSPEC_OK;
    };
    const int64_t C = emspec_num_columns(L, n, hop);
    if (e->exact()) {   // the stamped builds of the two EXACT fused kernels (waves: 16; slots: exact_fused.hip.inc, exact_fused_lr.hip.inc)
        const ExactPlanDev xpd = exact_plan_dev(e, *p, hop, reassign);
        const ExactDbMap xm = exact_db_map(e, n, xpd);
        const Route route = exact_route_of(e, n, xpd);
        if (route.kind == RouteKind::exact_lr) {
            const int xrl = route.rl;
            if ((rc = exact_lr_prepare(e, n, xpd, xrl, S, C, e->stream))) return rc;
            return stamped(16, [&](unsigned long long* stamps) {
                hipError_t r = launch_exact_fused_lr(n, xpd, xm, e->d_lut, pcm_dev, L, S, C, xrl, e->d_xlow, e->xlow_bytes, db_dev, nullptr, index_dev, e->stream, stamps, groups);
                if (r == hipSuccess && xrl > 0) r = hipEventRecord(e->xlow_event, e->stream);   // (every launch on the scratch: later ones on other streams wait for it)
                return r;
            });
        }
        if (route.kind != RouteKind::exact_parked) return fail(e, EMSPEC_ERR_INVALID_ARG, "no fused exact kernel for this shape");
        return stamped(16, [&](unsigned long long* stamps) {
            return launch_exact_fused(n, xpd, xm, e->d_lut, pcm_dev, L, S, C, db_dev, nullptr, index_dev, e->stream, stamps, groups);
        });
    }
    if (!fused_supported(n, hop, e->cfg.rows, reassign)) return fail(e, EMSPEC_ERR_INVALID_ARG, "no fused kernel for this shape");
    const PlanDev pd = plan_dev(e, *p, hop, reassign);
    const DbMap m = db_map(e, n);
    return stamped(16, [&](unsigned long long* stamps) {
        return launch_fused(n, pd, m, e->d_lut, pcm_dev, L, S, C, db_dev, nullptr, index_dev, e->stream, stamps, groups);
    });
}
#endif  // EMSPEC_DIAG

}  // extern "C"

// the host-buffer entries run emspec_batch_device on each unit of the driver's pipeline (emspec_host.cpp)
static HostRun batch_run(emspec_engine* e, int n, int hop, int reassign) {
    return [=](const float* pcm, int sc, int64_t samples, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st) {
        return batch_device_full(e, pcm, sc, samples, n, hop, reassign, db, rgba, index, st);
    };
}

extern "C" {

int emspec_batch(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign,
                 const emspec_out* out) {
    if (!e || !pcm || !out) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (S < 1 || L < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need at least one stream of at least fft-size samples");
    HIPCHK(e, hipSetDevice(e->device));
    if (!out->db && !out->rgba && !out->index) return EMSPEC_OK;
    // With fewer than sixteen streams the units are runs of a stream's columns (pipe_items) - but the display post-process walks
    // a stream in time order: whole streams there
    const bool post = e->smoothing > 0.0f || e->agc > 0.0f;
    HostJob job;
    job.src = pcm, job.S = S, job.L = L, job.n = n, job.hop = hop;
    job.whole_streams = post, job.halo_D = latency(n, hop, reassign);
    job.out = out;
    job.run = batch_run(e, n, hop, reassign);
    return host_batch(e, job);
}

int emspec_batch_packed(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop, int32_t reassign,
                        uint8_t* wire, int64_t wire_capacity, int64_t* offsets) {
    if (!e || !pcm || !wire || !offsets || wire_capacity < 0) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (S < 1 || L < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need at least one stream of at least fft-size samples");
    if ((uint64_t)reduced_columns(emspec_num_columns(L, n, hop), e->time_reduce) * (uint64_t)e->cfg.rows >= (1ull << 32))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "at most 2^32 cells per stream");
    if (e->cfg.rows % 4) return fail(e, EMSPEC_ERR_INVALID_ARG, "the wire image needs rows % 4 == 0");
    HIPCHK(e, hipSetDevice(e->device));
    const PackedOut pk{wire, wire_capacity, offsets};
    // (an image is one stream's whole run of columns: whole streams)
    HostJob job;
    job.src = pcm, job.S = S, job.L = L, job.n = n, job.hop = hop;
    job.whole_streams = true;
    job.pk = &pk;
    job.run = batch_run(e, n, hop, reassign);
    return host_batch(e, job);
}

int emspec_wire_unpack_host(const uint8_t* wire, int64_t wire_bytes, int64_t columns, int32_t rows, uint8_t* index_out) {
    if (!wire || !index_out || columns < 1 || rows < 1) return EMSPEC_ERR_INVALID_ARG;
    return wire_unpack_host(wire, wire_bytes, columns, rows, index_out) ? EMSPEC_OK : EMSPEC_ERR_INVALID_ARG;
}

int emspec_parity_dump_device(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop,
                              int32_t reassign, int64_t frame0, int64_t nframes, float* power, int32_t* col,
                              int32_t* row, void* hip_stream) {
    if (!e || !pcm || !power || !col || !row) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (e->exact()) return fail(e, EMSPEC_ERR_STATE, "engine is in EXACT mode: use emspec_parity_dump_exact");
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    const int64_t C = emspec_num_columns(L, n, hop);
    if (S < 1 || S > 65535 || frame0 < 0 || nframes < 0 || frame0 + nframes > C)
        return fail(e, EMSPEC_ERR_INVALID_ARG, "frame range outside the stream");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;   // NULL = the HIP default stream
    Plan* p;
    if ((rc = get_plan(e, n, &p))) return rc;
    const PlanDev pd = plan_dev(e, *p, hop, reassign);
    FrameSinks sk;
    sk.power = power; sk.col = col; sk.row = row;
    HIPCHK(e, launch_frames(n, pd, pcm, L, S, frame0, nframes, sk, st));
    return EMSPEC_OK;
}

int emspec_parity_dump(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop,
                       int32_t reassign, int64_t frame0, int64_t nframes, float* power, int32_t* col, int32_t* row) {
    if (!e || !pcm || !power || !col || !row) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (e->exact()) return fail(e, EMSPEC_ERR_STATE, "engine is in EXACT mode: use emspec_parity_dump_exact");
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (S < 1 || S > 65535 || L < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need 1..65535 streams of at least fft-size samples");
    if (frame0 < 0 || nframes < 0 || frame0 + nframes > emspec_num_columns(L, n, hop))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "frame range outside the stream");
    HIPCHK(e, hipSetDevice(e->device));
    const size_t nb = (size_t)S * nframes * (n / 2 + 1);
    const size_t b_pcm = (size_t)S * L * sizeof(float);
    const DumpStage ds = dump_stage(b_pcm, nb, false);
    if ((rc = grow(e, (void**)&e->d_stage, &e->stage_bytes, ds.bytes))) return rc;
    char* base = e->d_stage;
    float* d_pcm = (float*)(base + ds.pcm);
    float* d_pw = (float*)(base + ds.power);
    int32_t* d_col = (int32_t*)(base + ds.col);
    int32_t* d_row = (int32_t*)(base + ds.row);
    HIPCHK(e, hipMemcpyAsync(d_pcm, pcm, b_pcm, hipMemcpyHostToDevice, e->stream));
    if ((rc = emspec_parity_dump_device(e, d_pcm, S, L, n, hop, reassign, frame0, nframes, d_pw, d_col, d_row, e->stream))) return rc;
    HIPCHK(e, hipMemcpyAsync(power, d_pw, nb * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(col, d_col, nb * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(row, d_row, nb * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return EMSPEC_OK;
}

int emspec_parity_dump_exact(emspec_engine* e, const float* pcm, int32_t S, int64_t L, int32_t n, int32_t hop,
                             int32_t reassign, int64_t frame0, int64_t nframes, double* power, int32_t* col, int32_t* row,
                             int64_t* q) {
    if (!e || !pcm || !power || !col || !row) return fail(e, EMSPEC_ERR_INVALID_ARG, "null argument");
    if (!e->exact()) return fail(e, EMSPEC_ERR_STATE, "engine is in FAST mode: use emspec_parity_dump");
    int rc = check_shape(e, n, hop);
    if (rc) return rc;
    if (S < 1 || S > 65535 || L < n) return fail(e, EMSPEC_ERR_INVALID_ARG, "need 1..65535 streams of at least fft-size samples");
    if (frame0 < 0 || nframes < 0 || frame0 + nframes > emspec_num_columns(L, n, hop))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "frame range outside the stream");
    HIPCHK(e, hipSetDevice(e->device));
    Plan* p;
    if ((rc = get_plan(e, n, &p))) return rc;
    const ExactPlanDev pd = exact_plan_dev(e, *p, hop, reassign);
    const size_t nb = (size_t)S * nframes * (n / 2 + 1);
    const size_t b_pcm = (size_t)S * L * sizeof(float);
    const DumpStage ds = dump_stage(b_pcm, nb, true);
    if ((rc = grow(e, (void**)&e->d_stage, &e->stage_bytes, ds.bytes))) return rc;
    char* base = e->d_stage;
    float* d_pcm = (float*)(base + ds.pcm);
    ExactSinks sk;
    sk.power = (double*)(base + ds.power);
    sk.q = (long long*)(base + ds.q);
    sk.col = (int32_t*)(base + ds.col);
    sk.row = (int32_t*)(base + ds.row);
    HIPCHK(e, hipMemcpyAsync(d_pcm, pcm, b_pcm, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, launch_exact_frames(n, pd, d_pcm, L, S, frame0, nframes, sk, e->stream));
    HIPCHK(e, hipMemcpyAsync(power, sk.power, nb * 8, hipMemcpyDeviceToHost, e->stream));
    if (q) HIPCHK(e, hipMemcpyAsync(q, sk.q, nb * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(col, sk.col, nb * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(row, sk.row, nb * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return EMSPEC_OK;
}

int emspec_set_display(emspec_engine* e, float smoothing, float agc_strength) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (!(smoothing >= 0.0f && smoothing <= 0.95f) || !(agc_strength >= 0.0f && agc_strength <= 1.0f))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "smoothing must be in [0,0.95], agc_strength in [0,1]");
    e->smoothing = smoothing;
    e->agc = agc_strength;
    return EMSPEC_OK;
}

int emspec_set_time_reduce(emspec_engine* e, int32_t factor) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    if (factor < 1 || factor > 65536) return fail(e, EMSPEC_ERR_INVALID_ARG, "the time reduction factor must be in [1, 65536]");
    if (live_pending(e)) return fail(e, EMSPEC_ERR_STATE, "columns are pending; flush or reset before changing the time reduction");
    e->time_reduce = factor;
    return EMSPEC_OK;
}
int32_t emspec_time_reduce(const emspec_engine* e) { return e ? e->time_reduce : -1; }
int64_t emspec_reduced_columns(int64_t columns, int32_t factor) {
    if (columns < 0 || factor < 1 || factor > 65536) return -1;
    return columns / factor + (columns % factor != 0);
}

int emspec_reset(emspec_engine* e) {
    if (!e) return EMSPEC_ERR_INVALID_ARG;
    live_reset(e);   // both streaming sessions: the single-stream calls' and the live multi-stream one (buffers are kept)
    return EMSPEC_OK;
}

// (the streaming calls - emspec_column, emspec_column_flush, emspec_push_samples, emspec_push_columns and the live multi-stream
// session - live in emspec_live.cpp)

}  // extern "C"
