// emspec_host.cpp — the host-buffer path (include/emspec.h: emspec_batch, emspec_batch_packed, emspec_batch_multires): S
// streams in host memory -> columns in host memory, or one packed wire image per stream, through staging sets on the device.
// One driver, host_batch, serves all three entries; each hands it the function that computes a unit on the device.
#include "emspec_engine.h"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

using namespace emspec;

namespace {

// A three-stage pipeline over units of the batch.  H2D copies on their own HIP stream, every kernel on the engine's compute
// stream (so the per-engine workspaces - EXACT records / low-row scratch, display post-process - are used by one launch at a
// time, and no two fused launches share the chip), D2H copies on a third stream; kPipeSets staging sets, events between the
// stages.  PCIe is full duplex: the H2D of unit k+1, the kernels of unit k and the D2H of unit k-1 are in flight together.
// With `pk` the palette-index columns leave the device as the gather's lossless wire image (pack.hip.inc: ~186 B instead of
// 1,024 B per column on the bench input), one image per stream, tightly packed into the caller's buffer in stream order; the
// host learns each image's size from its 32-byte header, which is copied out behind the pack, so the D2H stage of a unit is
// enqueued kPipeLag units after its kernels.  A batch of one unit has nothing to overlap: its three stages run in order on
// the compute stream.
constexpr int kPipeSets = 3, kPipeLag = 2;

// One unit of the host pipelines: `sc` whole streams from stream s0 on - or, when the batch has fewer streams than the pipeline
// needs units (BASELINE configs[1] is ONE stream), a run of columns [c0, c0 + cn) of one stream, computed as a batch of its own
// from the frames that reach those columns: D more on either side (a bin moves at most D columns), whose own columns - `skip` in
// front, the rest behind - are computed and left on the device.  Every frame that adds to a kept column is in the run and no
// other frame can reach it, so the kept columns are the whole batch's (EXACT mode: the same bytes; float32: the same sums in
// another order, as between any two launches).
struct PipeItem { int s0, sc; int64_t c0, cn, first_sample, samples, skip, cols; };

// How many units a batch is cut into.  A unit costs ~0.2 ms (EXACT: 0.4) on the compute stream whatever its size: a launch of
// the fused kernel takes 0.11-0.18 ms however few columns it has - a workgroup WALKS its segment, 2 D halo frames and the ring's
// start-up before the first column leaves (emspec_batch_device on 49 columns: 113 us on the GPU, 5 us to enqueue) - the units'
// kernels run one after the other, and each unit adds ~40 us of event waits and copy start-up.  Behind that, three stages
// overlap: with u units a call takes about
//     max(u x 0.2 ms,  M + (sum - M) / u),   M = the longest of [bytes in / 45 GB/s, kernel time, bytes out / 45 GB/s].
// Until late round 6 the count was fixed (sixteen, or one per stream below that): 8 streams x 2^18 samples took 1.65 ms - eight
// units - for 0.5 ms of copies and kernels.  The kernel rates are the bench line's, rounded; at most sixteen units.
int pipe_units(bool exact, int n, int64_t columns, size_t bytes_in, size_t bytes_out) {
    const double rate = (n <= 1024 ? 3.4e8 : n <= 2048 ? 2.2e8 : n <= 4096 ? 1.15e8 : n <= 8192 ? 5e7 : 2.2e7) / (exact ? (n > 4096 ? 2.8 : 2.1) : 1.0);
    const double t_in = (double)bytes_in / 45e9, t_out = (double)bytes_out / 45e9, t_k = (double)columns / rate;
    const double longest = std::max(t_in, std::max(t_k, t_out)), sum = t_in + t_k + t_out, per_unit = exact ? 0.4e-3 : 0.2e-3;
    int best = 1;
    double best_t = sum + per_unit;
    for (int u = 2; u <= 16; ++u) {
        const double t = std::max(u * per_unit, longest + (sum - longest) / u);
        if (t < best_t * 0.995) { best = u; best_t = t; }   // (not one unit more for nothing)
    }
#ifdef EMSPEC_DIAG
    if (const char* ev = getenv("EMSPEC_PIPE_CHUNKS")) { const int v = atoi(ev); if (v >= 1) best = v; }   // A/B aid
#endif
    return best;
}

// (f: the engine's time reduction.  A run starts on a multiple of f, so that every group of f columns lies in one unit - the
// lengths are then multiples of f but for the stream's last run - and a batch of fewer than two groups per stream is not cut)
std::vector<PipeItem> pipe_items(int S, int64_t L, int64_t C, int n, int hop, int D, size_t per_stream_bytes, bool by_time, int target, int f) {
    std::vector<PipeItem> items;
    // runs of columns: when there are fewer than `target` streams; at least 16,384 columns per run - a unit costs ~0.2 ms
    // (pipe_units) whatever its size, and 16 MB each way over PCIe take 0.35 ms (measured with 2,048-column runs: one stream
    // of 2^22 samples 1.49 ms instead of 0.84 in one piece)
    const int64_t pieces = by_time && S < target ? std::min<int64_t>((target + S - 1) / S, std::min(C / 16384, C / f)) : 1;
    if (pieces > 1) {
        for (int s = 0; s < S; ++s)
            for (int64_t t = 0; t < pieces; ++t) {
                PipeItem it;
                it.s0 = s; it.sc = 1;
                it.c0 = C * t / pieces / f * f;
                it.cn = (t + 1 < pieces ? C * (t + 1) / pieces / f * f : C) - it.c0;
                const int64_t f0 = std::max<int64_t>(it.c0 - D, 0), f1 = std::min<int64_t>(it.c0 + it.cn + D, C);   // frames [f0, f1)
                it.first_sample = f0 * hop;
                it.samples = (f1 - f0 - 1) * hop + n;
                it.skip = it.c0 - f0;
                it.cols = f1 - f0;
                items.push_back(it);
            }
        return items;
    }
    // chunks of streams: about `target` per batch (pipe_units), bounded by 1 GiB of staging per set; a chunk of a few streams
    // still fills the chip (segments are cut per launch)
    int chunk = (S + target - 1) / target;
    const int fit = (int)(((size_t)1 << 30) / per_stream_bytes);
    chunk = chunk > fit ? fit : chunk;
    chunk = chunk < 1 ? 1 : chunk;
    for (int s0 = 0; s0 < S; s0 += chunk) items.push_back(PipeItem{s0, std::min(chunk, S - s0), 0, C, 0, L, 0, C});
    return items;
}

size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

// (db / rgba / idx: what the unit's kernels write; odb / orgba / oidx: what is delivered - the same arrays, or with a time
// reduction the reduced columns beside them)
// (peaks: the unit's peak lists, emspec_batch_peaks)
struct Set { float* pcm; float* db; uint8_t* rgba; uint8_t* idx; uint8_t* wire; char* raw; float* odb; uint8_t* orgba; uint8_t* oidx; emspec_peak* peaks; };

// The staging set: every array at the size the largest unit needs (the wire images: one slot of `wire` bytes per stream).
struct Stage {
    size_t in = 0, db = 0, rgba = 0, idx = 0, wire = 0;
    size_t raw = 0;  // PCM entries: the unit's raw frames, which the decode kernel turns into `in`
    size_t rdb = 0, rrgba = 0, ridx = 0;   // time reduction: the unit's reduced columns (db / idx then hold the full-rate ones)
    bool reduced = false;
    size_t peaks = 0;   // emspec_batch_peaks: k (pos, dB) pairs per kept column of the unit
    int chunk = 1;   // streams in the largest unit
    size_t bytes() const { return in + db + rgba + idx + wire * chunk + raw + rdb + rrgba + ridx + peaks; }
    Set at(char* stage, int b) const {
        char* base = stage + (size_t)b * bytes();
        Set q{(float*)base, db ? (float*)(base + in) : nullptr, rgba ? (uint8_t*)(base + in + db) : nullptr,
              idx ? (uint8_t*)(base + in + db + rgba) : nullptr, wire ? (uint8_t*)(base + in + db + rgba + idx) : nullptr,
              raw ? base + in + db + rgba + idx + wire * chunk : nullptr, nullptr, nullptr, nullptr, nullptr};
        char* r = base + in + db + rgba + idx + wire * chunk + raw;
        q.odb = reduced ? (rdb ? (float*)r : nullptr) : q.db;
        q.orgba = reduced ? (rrgba ? (uint8_t*)(r + rdb) : nullptr) : q.rgba;
        q.oidx = reduced ? (ridx ? (uint8_t*)(r + rdb + rrgba) : nullptr) : q.idx;
        q.peaks = peaks ? (emspec_peak*)(r + rdb + rrgba + ridx) : nullptr;
        return q;
    }
};

// (V streams per unit of PipeItem::sc, frame_bytes of raw input each: 1 and 0 for the float entries, whose units are streams)
// (f > 1: dB and / or index at full rate - the index also when only RGBA is wanted - and the delivered arrays at the reduced rate)
// (peaks_k > 0: a region of peaks_k pairs per kept column)
Stage stage_layout(const std::vector<PipeItem>& items, int R, bool db, bool rgba, bool idx, size_t wire_s, int V, int frame_bytes, int f, int peaks_k) {
    Stage g;
    size_t cells = 0, rcells = 0;
    for (const PipeItem& it : items) {
        rcells = std::max(rcells, (size_t)((it.cn + f - 1) / f) * R * it.sc * V);
        g.in = std::max(g.in, al((size_t)it.samples * 4 * it.sc * V));
        g.raw = std::max(g.raw, frame_bytes ? al((size_t)it.samples * frame_bytes * it.sc) : 0);
        cells = std::max(cells, (size_t)it.cols * R * it.sc * V);
        g.chunk = std::max(g.chunk, it.sc * V);
        g.peaks = std::max(g.peaks, al((size_t)it.cn * it.sc * V * peaks_k * sizeof(emspec_peak)));
    }
    g.reduced = f > 1;
    g.db = db ? al(cells * 4) : 0;
    g.rgba = rgba && !g.reduced ? al(cells * 4) : 0;
    g.idx = idx || (rgba && g.reduced) ? al(cells) : 0;
    g.wire = al(wire_s);
    if (g.reduced) {
        g.rdb = db ? al(rcells * 4) : 0;
        g.rrgba = rgba ? al(rcells * 4) : 0;
        g.ridx = idx ? al(rcells) : 0;
    }
    return g;
}

// Where a unit's kept columns come from in its set and go in the caller's arrays: cell offsets and count.  A unit of whole
// streams is one span; a run of columns is one span per stream (V > 1: the views of the unit's source).
// (C: the columns a stream is computed at; f: the time reduction - Cr = ceil(C / f) columns of it are delivered, a run's
// ceil(cn / f) from column c0 / f on, out of the unit's reduced array, which holds the kept columns only)
struct Span { size_t from, to, cells; };
int spans_of(const PipeItem& it, int64_t C, int V) { return it.cn == C ? 1 : it.sc * V; }
Span span_of(const PipeItem& it, int64_t C, int R, int V, int k, int f) {
    if (f == 1) {
        if (it.cn == C) return Span{0, (size_t)it.s0 * V * C * R, (size_t)it.cn * R * it.sc * V};
        return Span{((size_t)k * it.cols + (size_t)it.skip) * R, (((size_t)it.s0 * V + k) * C + (size_t)it.c0) * R, (size_t)it.cn * R};
    }
    const size_t Cr = (size_t)((C + f - 1) / f), crn = (size_t)((it.cn + f - 1) / f);
    if (it.cn == C) return Span{0, (size_t)it.s0 * V * Cr * R, crn * R * it.sc * V};
    return Span{(size_t)k * crn * R, (((size_t)it.s0 * V + k) * Cr + (size_t)(it.c0 / f)) * R, crn * R};
}

}  // namespace

bool emspec::host_pinned(const void* p) {
    if (!p) return true;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

int emspec::host_batch(emspec_engine* e, const void* pcm, int S, int64_t L, int n, int hop, int halo_D, int min_streams,
                       const emspec_out* out, const PackedOut* pk, const HostRun& run, const emspec_pcm_format* dec, const PeaksOut* pko) {
    if (!e->stream_in) HIPCHK(e, hipStreamCreateWithFlags(&e->stream_in, hipStreamNonBlocking));
    if (!e->stream_out) HIPCHK(e, hipStreamCreateWithFlags(&e->stream_out, hipStreamNonBlocking));
    for (hipEvent_t& ev : e->pipe_ev)
        if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const int64_t C = emspec_num_columns(L, n, hop);
    const int R = e->cfg.rows, f = e->time_reduce;
    const int64_t Cr = reduced_columns(C, f);   // columns per stream that are delivered (C are computed)
    int rc;
    // dec: the S rows are SOURCES of interleaved frames (emspec_batch_pcm): fb bytes per frame in, V streams each out
    const int V = dec ? dec->views : 1, fb = dec ? pcm_frame_bytes(*dec) : (int)sizeof(float);
    const size_t col_cells = (size_t)C * R, out_cells = (size_t)Cr * R, in_s = (size_t)L * fb;
    // (pko: the dB columns are staged for the peaks kernel and stay on the device; only the peak lists are delivered)
    const int pkk = pko ? pko->k : 0;
    const bool want_db = out && out->db, stage_db = want_db || pko, want_rgba = out && out->rgba, want_idx = (out && out->index) || pk;
    const size_t wire_s = pk ? (size_t)wire_bound_bytes(Cr, R) : 0;
    size_t per_stream = al(in_s) + (dec ? al((size_t)L * 4 * V) : 0) +
                        V * (al(stage_db ? col_cells * 4 : 0) + al(want_rgba ? col_cells * 4 : 0) + al(want_idx ? col_cells : 0) + al(wire_s) +
                             al((size_t)C * pkk * sizeof(emspec_peak)));
    if (f > 1)   // full-rate dB / index (no full-rate RGBA) and the reduced arrays
        per_stream = al(in_s) + (dec ? al((size_t)L * 4 * V) : 0) +
                     V * (al(want_db ? col_cells * 4 : 0) + al(want_idx || want_rgba ? col_cells : 0) + al(wire_s) +
                          al(want_db ? out_cells * 4 : 0) + al(want_rgba ? out_cells * 4 : 0) + al(want_idx ? out_cells : 0));
    int units = pipe_units(e->exact(), n, (int64_t)S * V * C, (size_t)S * in_s,
                           pk ? (size_t)S * V * out_cells / 5 : (size_t)S * V * out_cells * ((want_db ? 4 : 0) + (want_rgba ? 4 : 0) + (want_idx ? 1 : 0)) +
                                (size_t)S * V * C * pkk * sizeof(emspec_peak));
    if (halo_D < 0) units = std::min(units, std::max(S / min_streams, 1));   // whole streams: at least min_streams per unit
    const std::vector<PipeItem> items = pipe_items(S, L, C, n, hop, halo_D, per_stream, halo_D >= 0, units, f);
    const int nu = (int)items.size();
    const bool one = nu == 1;
    const Stage g = stage_layout(items, R, stage_db, want_rgba, want_idx, wire_s, V, dec ? fb : 0, f, pkk);
    if ((rc = grow(e, (void**)&e->d_stage, &e->stage_bytes, std::min(nu, kPipeSets) * g.bytes() + 1024))) return rc;
    if (pk) {
        if ((rc = grow(e, (void**)&e->d_packscratch, &e->packscratch_bytes, wire_scratch_bytes(Cr)))) return rc;
        const size_t hb = (size_t)kPipeSets * g.chunk * 32;
        if (hb > e->h_hdr_bytes) {
            if (e->h_hdr) (void)hipHostFree(e->h_hdr);
            e->h_hdr = nullptr; e->h_hdr_bytes = 0;
            HIPCHK(e, hipHostMalloc((void**)&e->h_hdr, hb, hipHostMallocDefault));
            e->h_hdr_bytes = hb;
        }
        pk->offsets[0] = 0;
    }
    const hipStream_t s_in = one ? e->stream : e->stream_in, s_out = one ? e->stream : e->stream_out;
    hipEvent_t *ev_in = e->pipe_ev, *ev_comp = ev_in + kPipeSets, *ev_out = ev_comp + kPipeSets;   // per staging set
    const int tr = f;   // (the lambdas below count units with `f`)
    // the only D2H copies of columns: unit f's kept columns into the caller's arrays, on `st` behind the unit's kernels
    auto copy_out = [&](int f, hipStream_t st) {
        const Set q = g.at(e->d_stage, f % kPipeSets);
        hipError_t r = st == e->stream ? hipSuccess : hipStreamWaitEvent(st, ev_comp[f % kPipeSets], 0);
        for (int k = 0; k < spans_of(items[f], C, V); ++k) {
            const Span sp = span_of(items[f], C, R, V, k, tr);
            if (r == hipSuccess && want_db) r = hipMemcpyAsync(out->db + sp.to, q.odb + sp.from, sp.cells * 4, hipMemcpyDeviceToHost, st);
            if (r == hipSuccess && want_rgba) r = hipMemcpyAsync(out->rgba + 4 * sp.to, q.orgba + 4 * sp.from, sp.cells * 4, hipMemcpyDeviceToHost, st);
            if (r == hipSuccess && want_idx) r = hipMemcpyAsync(out->index + sp.to, q.oidx + sp.from, sp.cells, hipMemcpyDeviceToHost, st);
            // (peak lists: the set holds the unit's kept columns only, span after span)
            if (r == hipSuccess && pko) r = hipMemcpyAsync(pko->peaks + sp.to / R * pkk, q.peaks + (size_t)k * (sp.cells / R) * pkk,
                                                           sp.cells / R * pkk * sizeof(emspec_peak), hipMemcpyDeviceToHost, st);
        }
        return r;
    };

    // Host buffers in ORDINARY (pageable) memory.  The runtime serves such copies itself (it pins the pages and streams them:
    // ~45 GB/s one way on this box) but the call returns only when the copy is done, so from one host thread the samples in, the
    // kernels and the columns out run one after the other.  A second host thread, the drainer, then does nothing but the copies
    // out: in, compute and out overlap as they do from page-locked memory (round 6: 2.15e7 -> 4.3e7 columns/s on the bench
    // shape; pinning the caller's buffers per call instead costs more than it saves: 49 ms vs 27 ms for 670 MB).
    std::mutex mu;
    std::condition_variable cv;
    int launched = 0, drained = 0;      // units whose kernels are enqueued / whose columns are in the caller's memory
    bool stop = false;
    hipError_t herr_out = hipSuccess;
    // A caller that allocates its result per call (np.empty, new Uint8Array) hands over pages that were never touched: the runtime's
    // copy then takes a page fault per 4 KB on its one thread (1 GB of palette indices: 90 ms of a 114 ms call).  kTouchers threads
    // write one byte into every page of a unit's destination before the drainer copies the unit there (every byte of the outputs
    // is overwritten by the call anyway); on resident pages that costs nothing measurable.
    constexpr int kTouchers = 3;
    int touched[kTouchers] = {};
    auto touch_all = [&](int t) {
        auto touch = [&](void* base, size_t bytes) {
            if (!base || !bytes) return;
            volatile char* p = reinterpret_cast<volatile char*>(base);
            const size_t lo = bytes * (size_t)t / kTouchers, hi = bytes * (size_t)(t + 1) / kTouchers;
            for (size_t a = lo; a < hi; a += 4096) p[a] = 0;
            if (t == kTouchers - 1) p[bytes - 1] = 0;
        };
        for (int f = 0; f < nu; ++f) {
            for (int k = 0; k < spans_of(items[f], C, V); ++k) {
                const Span sp = span_of(items[f], C, R, V, k, tr);
                if (want_db) touch(out->db + sp.to, sp.cells * 4);
                if (want_rgba) touch(out->rgba + 4 * sp.to, sp.cells * 4);
                if (want_idx) touch(out->index + sp.to, sp.cells);
                if (pko) touch(pko->peaks + sp.to / R * pkk, sp.cells / R * pkk * sizeof(emspec_peak));
            }
            std::lock_guard<std::mutex> lk(mu);
            touched[t] = f + 1;
            cv.notify_all();
            if (stop) break;
        }
    };
    auto ready = [&](int f) {   // unit f's kernels are enqueued and its destination touched (under mu)
        bool r = launched > f;
        for (int t = 0; t < kTouchers; ++t) r = r && touched[t] > f;
        return r;
    };
    auto drain_all = [&] {
        hipError_t r = hipSetDevice(e->device);
        for (int f = 0; f < nu && r == hipSuccess; ++f) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return ready(f) || stop; });
                if (!ready(f)) break;
            }
            r = copy_out(f, e->stream_out);
            if (r == hipSuccess) r = hipStreamSynchronize(e->stream_out);
            std::lock_guard<std::mutex> lk(mu);
            drained = f + 1;
            cv.notify_all();
        }
        std::lock_guard<std::mutex> lk(mu);
        herr_out = r;
        stop = true;
        cv.notify_all();
    };
    std::thread drainer, touchers[kTouchers];
    bool threaded = !pk && nu >= 2 && !(host_pinned(pcm) && (!out || (host_pinned(out->db) && host_pinned(out->rgba) && host_pinned(out->index))) &&
                                        (!pko || host_pinned(pko->peaks)));
    try {
        if (threaded) drainer = std::thread(drain_all);
    } catch (const std::exception&) {   // no thread to be had: the caller's thread drains (its copies block it)
        threaded = false;
    }
    for (int t = 0; threaded && t < kTouchers; ++t) {
        try {
            touchers[t] = std::thread(touch_all, t);
        } catch (const std::exception&) {   // (its share counts as touched: the runtime takes those faults itself)
            std::lock_guard<std::mutex> lk(mu);
            touched[t] = nu;
            cv.notify_all();
        }
    }

    hipError_t herr = hipSuccess;
    // the D2H stage of unit f on the caller's thread (its kernels are enqueued; with pk: wait for them, then the images' sizes
    // are known)
    auto drain = [&](int f) {
        const PipeItem& it = items[f];
        const int b = f % kPipeSets;
        if (!pk) {
            herr = copy_out(f, s_out);
        } else {
            const Set q = g.at(e->d_stage, b);
            herr = hipEventSynchronize(ev_comp[b]);
            for (int i = 0; i < it.sc * V && herr == hipSuccess && rc == EMSPEC_OK; ++i) {
                const uint32_t* h = reinterpret_cast<const uint32_t*>(e->h_hdr + ((size_t)b * g.chunk + i) * 32);
                const uint64_t hcols = (uint64_t)h[2] | ((uint64_t)h[3] << 32), hpay = (uint64_t)h[4] | ((uint64_t)h[5] << 32);
                if (h[0] != 0x32574D45u || (int32_t)h[1] != R || hcols != (uint64_t)Cr || hpay > (uint64_t)out_cells) {
                    rc = fail(e, EMSPEC_ERR_HIP, "the packed image of a stream carries a bad header");
                    break;
                }
                const int64_t bytes = wire_fixed_bytes(Cr, R) + (int64_t)((hpay + 15) & ~(uint64_t)15);
                const int64_t at = pk->offsets[it.s0 * V + i];
                if (at + bytes > pk->capacity) {
                    rc = fail(e, EMSPEC_ERR_INVALID_ARG, "wire buffer too small (emspec_wire_bound(columns, rows) per stream always suffices)");
                    break;
                }
                herr = hipMemcpyAsync(pk->wire + at, q.wire + (size_t)i * g.wire, (size_t)bytes, hipMemcpyDeviceToHost, s_out);
                // every image STARTS on a 16-byte boundary: the fixed part (32 + 4 C (1 + R/32) bytes) is a multiple of 4 only, so
                // up to 12 bytes of slack follow an image (stream s occupies [offsets[s], offsets[s+1]), slack included; the
                // unpackers take the image's real size from its header).  The slack is cleared: the bytes of wire[0 .. offsets[S])
                // are then the same whatever the caller's buffer held before, as an image's own pad is (pack.hip.inc)
                const int64_t end = (at + bytes + 15) & ~(int64_t)15;
                if (std::min(end, pk->capacity) > at + bytes) std::memset(pk->wire + at + bytes, 0, (size_t)(std::min(end, pk->capacity) - (at + bytes)));
                pk->offsets[it.s0 * V + i + 1] = end;
            }
        }
        if (herr == hipSuccess && rc == EMSPEC_OK && !one) herr = hipEventRecord(ev_out[b], s_out);
    };
    int enqueued = 0;   // units whose copies out the caller's thread has enqueued
    for (int ci = 0; ci < nu && rc == EMSPEC_OK && herr == hipSuccess; ++ci) {
        const PipeItem& it = items[ci];
        const int b = ci % kPipeSets;
        const Set q = g.at(e->d_stage, b);
        // 1. the set is free once unit ci - kPipeSets has left it: its input once its kernels are done, its outputs once they
        //    are copied out
        if (ci >= kPipeSets && threaded) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return drained > ci - kPipeSets || stop; });
            if (drained <= ci - kPipeSets) break;
        } else if (ci >= kPipeSets) {
            herr = hipStreamWaitEvent(s_in, ev_comp[b], 0);
            if (herr == hipSuccess) herr = hipStreamWaitEvent(e->stream, ev_out[b], 0);
        }
        // 2. samples in (PCM entries: the raw frames, from a byte offset that is a multiple of the sample size only)
        if (herr == hipSuccess)
            herr = hipMemcpyAsync(dec ? (void*)q.raw : (void*)q.pcm, static_cast<const char*>(pcm) + ((size_t)it.s0 * L + (size_t)it.first_sample) * fb,
                                  (size_t)it.samples * fb * it.sc, hipMemcpyHostToDevice, s_in);
        if (herr == hipSuccess && !one) herr = hipEventRecord(ev_in[b], s_in);
        if (herr == hipSuccess && !one) herr = hipStreamWaitEvent(e->stream, ev_in[b], 0);
        if (herr != hipSuccess) break;
        // 3. kernels (PCM entries: the decode kernel first, raw frames -> the unit's sc * V float streams)
        if (dec && (herr = pcm_decode(q.raw, *dec, it.sc, it.samples, it.samples * fb, q.pcm, it.samples, e->stream)) != hipSuccess) break;
        if ((rc = run(q.pcm, it.sc * V, it.samples, q.db, q.rgba, q.idx, e->stream))) break;
        // 3b. time reduction: the unit's kept columns (a run: from column `skip` of its it.cols) -> the set's reduced arrays
        if (f > 1 && (herr = launch_reduce_columns(q.db ? q.db + (size_t)it.skip * R : nullptr, q.idx ? q.idx + (size_t)it.skip * R : nullptr,
                                                   it.sc * V, it.cn, R, f, (size_t)it.cols * R, (size_t)((it.cn + f - 1) / f) * R, e->d_lut,
                                                   q.odb, q.oidx, q.orgba, e->stream)) != hipSuccess) break;
        // 3c. peaks: the k loudest local maxima of every kept column (peaks.hip.inc), span after span into the set's peak lists
        for (int k = 0; pko && k < spans_of(it, C, V) && herr == hipSuccess; ++k) {
            const Span sp = span_of(it, C, R, V, k, 1);
            herr = launch_peaks(q.db + sp.from, (int64_t)(sp.cells / R), R, pkk, pko->min_db, q.peaks + (size_t)k * (sp.cells / R) * pkk, e->stream);
        }
        if (herr != hipSuccess) break;
        // 4. packed: each stream's image, its header to the host behind it
        for (int i = 0; pk && i < it.sc * V && herr == hipSuccess; ++i) {
            uint8_t* w = q.wire + (size_t)i * g.wire;
            herr = launch_wire_pack(q.oidx + (size_t)i * out_cells, Cr, R, w, e->d_packscratch, e->stream);
            if (herr == hipSuccess) herr = hipMemcpyAsync(e->h_hdr + ((size_t)b * g.chunk + i) * 32, w, 32, hipMemcpyDeviceToHost, e->stream);
        }
        // 5. computed
        if (herr == hipSuccess && (pk || !one)) herr = hipEventRecord(ev_comp[b], e->stream);
        if (threaded) {
            std::lock_guard<std::mutex> lk(mu);
            if (herr == hipSuccess) launched = ci + 1;
            cv.notify_all();
            continue;
        }
        // 6. copies out, kPipeLag units behind when the host has to read the images' sizes first
        while (herr == hipSuccess && rc == EMSPEC_OK && enqueued <= ci - (pk ? kPipeLag : 0)) drain(enqueued++);
    }
    if (threaded) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (launched < nu) stop = true;   // an error: the drainer finishes what was launched and leaves
            cv.notify_all();
        }
        drainer.join();
        for (auto& th : touchers)
            if (th.joinable()) th.join();
    }
    while (!threaded && herr == hipSuccess && rc == EMSPEC_OK && enqueued < nu) drain(enqueued++);
    const hipError_t s1 = hipStreamSynchronize(s_in), s2 = one ? hipSuccess : hipStreamSynchronize(e->stream),
                     s3 = one ? hipSuccess : hipStreamSynchronize(s_out);
    if (rc != EMSPEC_OK) return rc;
    HIPCHK(e, herr);
    HIPCHK(e, herr_out);
    HIPCHK(e, s1);
    HIPCHK(e, s2);
    HIPCHK(e, s3);
    if (read_kernel_error(true) > 0) return fail(e, EMSPEC_ERR_HIP, "a kernel's bounded wait timed out (protocol error): results invalid");
    return EMSPEC_OK;
}
