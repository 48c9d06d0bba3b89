// emspec_host.cpp — the host-buffer path (include/emspec.h: emspec_batch, _packed, _multires, _pcm, _peaks, _pcm_stereo): S streams
// in host memory -> columns in host memory, or one packed wire image per stream, peak lists or the stereo image of each source,
// through staging sets on the device.  One driver, host_batch, serves every entry: each hands it a HostJob (emspec_engine.h).  It
// is three parts around one Pipe: plan_pipe (the plan, emspec_pipe_plan.h, and the workspaces), the background delivery
// (deliver_start / _finish) and the unit loop (run_units).
#include "emspec_engine.h"
#include "emspec_pipe_plan.h"

#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

using namespace emspec;

namespace {

// A three-stage pipeline over units of the batch ("Host buffers").  H2D copies on their own HIP stream, every kernel
// on the engine's compute stream (so the per-engine workspaces are used by one launch at a time, and no two fused launches share
// the chip), D2H copies on a third stream; kPipeSets staging sets, events between the stages.  With `pk` the index columns leave
// as one wire image per stream (pack.hip.inc), packed into the caller's buffer in stream order; the host learns an image's size
// from its 32-byte header, copied out behind the pack, so the D2H stage of a unit is enqueued kPipeLag units after its kernels.
// A batch of one unit has nothing to overlap: its stages run in order on the compute stream.
constexpr int kPipeSets = 3, kPipeLag = 2, kTouchers = 3;

struct Pipe {   // what the three parts of host_batch share
    emspec_engine* e; const HostJob& j;
    // the plan: C columns per stream are computed, Cr delivered (f: the time reduction); a source of fb bytes per frame gives V
    // streams; nu units, a lone one on the compute stream throughout; outs: ONE table of what is delivered, a row per array
    int64_t C = 0, Cr = 0; int R = 0, f = 1, V = 1, fb = 4, nu = 0; bool one = false;
    OutRow outs[kOutRows] = {}; std::vector<PipeItem> items; Stage g;
    hipStream_t s_in = nullptr, s_out = nullptr; hipEvent_t *ev_in = nullptr, *ev_comp = nullptr, *ev_out = nullptr;   // (per staging set)
    // the background delivery, under mu: units whose kernels are enqueued / that are copied out / that toucher t has been through
    bool threaded = false, stop = false; std::mutex mu; std::condition_variable cv;
    int launched = 0, drained = 0, touched[kTouchers] = {}; hipError_t herr_out = hipSuccess;
    std::thread drainer, touchers[kTouchers];
    // the unit loop: its first failure, and the units whose copies out the caller's thread has enqueued
    hipError_t herr = hipSuccess; int rc = EMSPEC_OK, enqueued = 0;
    bool ok() const { return herr == hipSuccess && rc == EMSPEC_OK; }
};

// Part 1: the plan and the workspaces.
int plan_pipe(Pipe& p) {
    emspec_engine* e = p.e;
    const HostJob& j = p.j;
    p.R = e->cfg.rows; p.f = e->time_reduce;
    p.C = emspec_num_columns(j.L, j.n, j.hop); p.Cr = reduced_columns(p.C, p.f);
    // dec: the S rows are SOURCES of interleaved frames (emspec_batch_pcm): fb bytes per frame in, V streams each out
    p.V = j.dec ? j.dec->views : 1; p.fb = j.dec ? pcm_frame_bytes(*j.dec) : (int)sizeof(float);
    // the array of a setting that is on holds an item per stream (cross: per source) and delivered column
    auto room = [&](const void* set, int64_t rows, int64_t capacity, const char* too_small) {
        return set && rows * p.Cr > capacity ? fail(e, EMSPEC_ERR_INVALID_ARG, too_small) : (int)EMSPEC_OK;
    };
    if (int rc = room(e->wave_out, (int64_t)j.S * p.V, e->wave_capacity, "the envelope set with emspec_set_wave_out is too small: it needs streams x delivered columns pairs")) return rc;
    if (int rc = room(e->level_out, (int64_t)j.S * p.V, e->level_capacity, "the array set with emspec_set_level_out is too small: it needs streams x delivered columns records")) return rc;
    if (e->cross_out && !j.dec)
        return fail(e, EMSPEC_ERR_STATE, "cross records are of a PCM source's views: not available on float streams while emspec_set_cross_out is set (NULL clears it)");
    if (e->cross_out && (e->cross_a >= p.V || e->cross_b >= p.V))
        return fail(e, EMSPEC_ERR_INVALID_ARG, "the channels a and b set with emspec_set_cross_out must be in 0 .. views - 1 of the call's format");
    if (int rc = room(e->cross_out, (int64_t)j.S, e->cross_capacity, "the array set with emspec_set_cross_out is too small: it needs sources x delivered columns records")) return rc;
    if (!e->stream_in) HIPCHK(e, hipStreamCreateWithFlags(&e->stream_in, hipStreamNonBlocking));
    if (!e->stream_out) HIPCHK(e, hipStreamCreateWithFlags(&e->stream_out, hipStreamNonBlocking));
    for (hipEvent_t& ev : e->pipe_ev) if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    // what is delivered (pk: the index is staged for the images; pko: the dB columns are staged for the peaks kernel and stay
    // on the device, only the peak lists are delivered)
    const emspec_out none{}, &o = j.out ? *j.out : none;
    p.outs[kDb] = OutRow{(char*)o.db, o.db ? (size_t)4 : 0};
    p.outs[kRgba] = OutRow{(char*)o.rgba, o.rgba ? (size_t)4 : 0};
    p.outs[kIdx] = OutRow{(char*)o.index, o.index || j.pk ? (size_t)1 : 0};
    p.outs[kPeaks] = OutRow{j.pko ? (char*)j.pko->peaks : nullptr, j.pko ? j.pko->k * sizeof(emspec_peak) : 0};
    p.outs[kWave] = OutRow{(char*)e->wave_out, e->wave_out ? sizeof(emspec_wave) : 0};   // (beside any of them: emspec_set_wave_out)
    p.outs[kLevel] = OutRow{(char*)e->level_out, e->level_out ? sizeof(emspec_level) : 0};   // (likewise: emspec_set_level_out, _cross_out)
    p.outs[kCross] = OutRow{(char*)e->cross_out, e->cross_out ? sizeof(emspec_cross) : 0};
    if (const StereoHostOut* so = j.stereo) {   // (the dB columns are staged for the compose kernel and stay on the device)
        p.outs[kSLevel] = OutRow{(char*)so->level, so->level ? (size_t)4 : 0};
        p.outs[kSIdx] = OutRow{(char*)so->index, so->index ? (size_t)1 : 0};
        p.outs[kSPan] = OutRow{(char*)so->pan, so->pan ? (size_t)1 : 0};
        p.outs[kSRgba] = OutRow{(char*)so->rgba, so->rgba ? (size_t)4 : 0};
    }
    const size_t wire_s = j.pk ? (size_t)wire_bound_bytes(p.Cr, p.R) : 0, in_s = (size_t)j.L * p.fb;
    const size_t per_stream = per_stream_bytes(p.outs, in_s, j.dec ? (size_t)j.L * 4 * p.V : 0, p.V, p.C, p.Cr, p.R, wire_s, p.f);
    const size_t bytes_out = j.stereo ? stereo_bytes_out(p.outs, (size_t)j.S, p.C, p.R) : bytes_out_estimate(p.outs, j.pk != nullptr, (size_t)j.S * p.V, p.C, p.Cr, p.R);
    int units = pipe_units(e->exact(), j.n, (int64_t)j.S * p.V * p.C, (size_t)j.S * in_s, bytes_out);
#ifdef EMSPEC_DIAG
    if (const char* ev = getenv("EMSPEC_PIPE_CHUNKS")) { const int v = atoi(ev); if (v >= 1) units = v; }   // A/B aid
#endif
    if (j.whole_streams) units = std::min(units, std::max(j.S / j.min_streams, 1));   // at least min_streams per unit
    p.items = pipe_items(j.S, j.L, p.C, j.n, j.hop, j.halo_D, per_stream, !j.whole_streams, units, p.f);
    p.nu = (int)p.items.size();
    p.one = p.nu == 1;
    p.g = stage_layout(p.items, p.R, p.outs, wire_s, p.V, j.dec ? p.fb : 0, p.f);
    if (int rc = grow(e, (void**)&e->d_stage, &e->stage_bytes, std::min(p.nu, kPipeSets) * p.g.bytes() + 1024)) return rc;
    if (j.pk) {
        if (int rc = grow(e, (void**)&e->d_packscratch, &e->packscratch_bytes, wire_scratch_bytes(p.Cr))) return rc;
        const size_t hb = (size_t)kPipeSets * p.g.chunk * kWireHeader;
        if (hb > e->h_hdr_bytes) {
            if (e->h_hdr) (void)hipHostFree(e->h_hdr);
            e->h_hdr = nullptr; e->h_hdr_bytes = 0;
            HIPCHK(e, hipHostMalloc((void**)&e->h_hdr, hb, hipHostMallocDefault));
            e->h_hdr_bytes = hb;
        }
        j.pk->offsets[0] = 0;
    }
    p.s_in = p.one ? e->stream : e->stream_in; p.s_out = p.one ? e->stream : e->stream_out;
    p.ev_in = e->pipe_ev; p.ev_comp = p.ev_in + kPipeSets; p.ev_out = p.ev_comp + kPipeSets;
    return EMSPEC_OK;
}

// What unit u delivers: fn(where in the caller's array, byte offset in the unit's set, bytes) for every span of every row that
// is copied out.  (The peak lists count in columns, and a set holds those of the unit's kept columns only, span after span; so
// do the envelope's pairs and the level meters' records, in delivered columns: wave_span_of, cross_span_of.)
template <class F>
void for_pieces(const Pipe& p, int u, F&& fn) {
    for (int k = 0; k < spans_of(p.items[u], p.C, p.V); ++k) {
        const Span sp = span_of(p.items[u], p.C, p.R, p.V, k, p.f), ws = wave_span_of(p.items[u], p.C, p.V, k, p.f);
        static_assert(kWave == 4 && kWave + 1 == kSLevel && kSRgba + 1 == kLevel && kCross + 1 == kOutRows, "a new row is served by no loop of for_pieces");
        for (int w : {kDb, kRgba, kIdx, kPeaks, kWave, kLevel}) {   // every row in front of the stereo rows, and the level records
            const OutRow& o = p.outs[w];
            const size_t cols = sp.cells / p.R, off = p.g.out_off(w);
            if (!o.host) continue;
            if (w == kWave || w == kLevel) fn(o.host + ws.to * o.unit, off + ws.from * o.unit, ws.cells * o.unit);   // the envelope's pairs, the level records
            else if (w == kPeaks) fn(o.host + sp.to / p.R * o.unit, off + k * cols * o.unit, cols * o.unit);
            else fn(o.host + sp.to * o.unit, off + sp.from * o.unit, sp.cells * o.unit);
        }
    }
    if (const OutRow& o = p.outs[kCross]; o.host) {   // beside them the cross records: one span of sources' delivered columns per unit
        const Span cs = cross_span_of(p.items[u], p.C, p.f);
        fn(o.host + cs.to * o.unit, p.g.out_off(kCross) + cs.from * o.unit, cs.cells * o.unit);
    }
    // the stereo image: one span of pair cells per unit
    const Span ss = stereo_span_of(p.items[u], p.C, p.R);
    for (int w = kSLevel; w <= kSRgba; ++w)
        if (const OutRow& o = p.outs[w]; o.host) fn(o.host + ss.to * o.unit, p.g.out_off(w) + ss.from * o.unit, ss.cells * o.unit);
}
// the only D2H copies of columns: unit u's kept columns into the caller's arrays, on `st` behind the unit's kernels
hipError_t copy_out(const Pipe& p, int u, hipStream_t st, bool computed = false) {   // (computed: the host has waited for the kernels)
    const char* set = p.e->d_stage + (size_t)(u % kPipeSets) * p.g.bytes();
    hipError_t r = st == p.e->stream || computed ? hipSuccess : hipStreamWaitEvent(st, p.ev_comp[u % kPipeSets], 0);
    for_pieces(p, u, [&](char* to, size_t from, size_t bytes) {
        if (r == hipSuccess) r = hipMemcpyAsync(to, set + from, bytes, hipMemcpyDeviceToHost, st);
    });
    return r;
}

// Part 2: the background delivery, for host buffers in ORDINARY (pageable) memory ("Pageable buffers").  The runtime's
// copy of such memory blocks the calling thread, so a second host thread, the drainer, does nothing but the copies out: in, compute
// and out overlap as from page-locked memory.  Untouched pages of a fresh result array cost that copy a page fault per 4 KB: kTouchers
// threads write one byte into every page of a unit's destination ahead of the drainer (every byte is overwritten anyway).
void touch_all(Pipe& p, int t) {
    for (int u = 0; u < p.nu; ++u) {
        for_pieces(p, u, [t](volatile char* d, size_t, size_t bytes) {
            for (size_t a = bytes * (size_t)t / kTouchers; a < bytes * (size_t)(t + 1) / kTouchers; a += 4096) d[a] = 0;
            if (bytes && t == kTouchers - 1) d[bytes - 1] = 0;
        });
        std::lock_guard<std::mutex> lk(p.mu);
        p.touched[t] = u + 1;
        p.cv.notify_all();
        if (p.stop) break;
    }
}
bool ready(const Pipe& p, int u) {   // unit u's kernels are enqueued and its destination touched (under mu)
    return p.launched > u && std::all_of(p.touched, p.touched + kTouchers, [u](int t) { return t > u; });
}
void drain_all(Pipe& p) {
    hipError_t r = hipSetDevice(p.e->device);
    for (int u = 0; u < p.nu && r == hipSuccess; ++u) {
        {
            std::unique_lock<std::mutex> lk(p.mu);
            p.cv.wait(lk, [&] { return ready(p, u) || p.stop; });
            if (!ready(p, u)) break;
        }
        r = copy_out(p, u, p.e->stream_out);
        if (r == hipSuccess) r = hipStreamSynchronize(p.e->stream_out);
        std::lock_guard<std::mutex> lk(p.mu);
        p.drained = u + 1;
        p.cv.notify_all();
    }
    std::lock_guard<std::mutex> lk(p.mu);
    p.herr_out = r;
    p.stop = true;
    p.cv.notify_all();
}
void deliver_start(Pipe& p) {
    const bool many = !p.j.pk && p.nu >= 2;
    bool pinned = many && host_pinned(p.j.src);
    for (const OutRow& o : p.outs) pinned = pinned && host_pinned(o.host);
    p.threaded = many && !pinned;   // (page-locked buffers throughout: the caller's thread enqueues everything)
    try {
        if (p.threaded) p.drainer = std::thread(drain_all, std::ref(p));
    } catch (const std::exception&) {   // no thread to be had: the caller's thread drains (its copies block it)
        p.threaded = false;
    }
    for (int t = 0; p.threaded && t < kTouchers; ++t) {
        try {
            p.touchers[t] = std::thread(touch_all, std::ref(p), t);
        } catch (const std::exception&) {   // (its share counts as touched: the runtime takes those faults itself)
            std::lock_guard<std::mutex> lk(p.mu);
            p.touched[t] = p.nu;
            p.cv.notify_all();
        }
    }
}
void deliver_finish(Pipe& p) {
    if (!p.threaded) return;
    {
        std::lock_guard<std::mutex> lk(p.mu);
        if (p.launched < p.nu) p.stop = true;   // an error: the drainer finishes what was launched and leaves
        p.cv.notify_all();
    }
    p.drainer.join();
    for (auto& th : p.touchers) if (th.joinable()) th.join();
}

// Part 3: the unit loop; first the D2H stage of unit u on the caller's thread (with pk: wait for its kernels, then the images'
// sizes are known)
void drain(Pipe& p, int u) {
    emspec_engine* e = p.e; const PackedOut* pk = p.j.pk;
    const PipeItem& it = p.items[u]; const int b = u % kPipeSets;
    if (!pk) {
        p.herr = copy_out(p, u, p.s_out);
    } else {
        const uint8_t* wire = p.g.at(e->d_stage, b).wire;
        p.herr = hipEventSynchronize(p.ev_comp[b]);
        for (int i = 0; i < it.sc * p.V && p.ok(); ++i) {
            const WireHeader h = wire_header(e->h_hdr + ((size_t)b * p.g.chunk + i) * kWireHeader);
            if (!wire_header_matches(h, p.Cr, p.R)) {
                p.rc = fail(e, EMSPEC_ERR_HIP, "the packed image of a stream carries a bad header");
                break;
            }
            const int64_t bytes = wire_padded_bytes(p.Cr, p.R, h.payload);
            const int64_t at = pk->offsets[it.s0 * p.V + i];
            if (at + bytes > pk->capacity) {
                p.rc = fail(e, EMSPEC_ERR_INVALID_ARG, "wire buffer too small (emspec_wire_bound(columns, rows) per stream always suffices)");
                break;
            }
            p.herr = hipMemcpyAsync(pk->wire + at, wire + (size_t)i * p.g.wire, (size_t)bytes, hipMemcpyDeviceToHost, p.s_out);
            // every image STARTS on a 16-byte boundary: the fixed part is a multiple of 4 only, so up to 12 bytes of slack follow
            // an image (stream s occupies [offsets[s], offsets[s+1]), slack included; include/emspec.h).  The slack is cleared, as
            // an image's own pad is: the bytes of wire[0 .. offsets[S]) are the same whatever the caller's buffer held before
            const int64_t end = (at + bytes + 15) & ~(int64_t)15;
            if (std::min(end, pk->capacity) > at + bytes) std::memset(pk->wire + at + bytes, 0, (size_t)(std::min(end, pk->capacity) - (at + bytes)));
            pk->offsets[it.s0 * p.V + i + 1] = end;
        }
        // (the index has no host array with pk: what is left to copy out is the envelope's pairs, beside the images)
        if (p.ok()) p.herr = copy_out(p, u, p.s_out, true);
    }
    if (p.ok() && !p.one) p.herr = hipEventRecord(p.ev_out[b], p.s_out);
}
void run_units(Pipe& p) {
    emspec_engine* e = p.e;
    const HostJob& j = p.j;
    hipError_t& herr = p.herr;
    const int R = p.R, V = p.V, f = p.f; const bool one = p.one;
    for (int u = 0; u < p.nu && p.ok(); ++u) {
        const PipeItem& it = p.items[u];
        const int b = u % kPipeSets;
        const Set q = p.g.at(e->d_stage, b);
        // 1. the set is free once unit u - kPipeSets has left it: its input with its kernels, its outputs once copied out
        if (u >= kPipeSets && p.threaded) {
            std::unique_lock<std::mutex> lk(p.mu);
            p.cv.wait(lk, [&] { return p.drained > u - kPipeSets || p.stop; });
            if (p.drained <= u - kPipeSets) break;
        } else if (u >= kPipeSets) {
            herr = hipStreamWaitEvent(p.s_in, p.ev_comp[b], 0);
            if (herr == hipSuccess) herr = hipStreamWaitEvent(e->stream, p.ev_out[b], 0);
        }
        // 2. samples in (PCM entries: the raw frames, from a byte offset that is a multiple of the sample size only)
        if (herr == hipSuccess)
            herr = hipMemcpyAsync(j.dec ? (void*)q.raw : (void*)q.pcm, static_cast<const char*>(j.src) + ((size_t)it.s0 * j.L + (size_t)it.first_sample) * p.fb,
                                  (size_t)it.samples * p.fb * it.sc, hipMemcpyHostToDevice, p.s_in);
        if (herr == hipSuccess && !one) herr = hipEventRecord(p.ev_in[b], p.s_in);
        if (herr == hipSuccess && !one) herr = hipStreamWaitEvent(e->stream, p.ev_in[b], 0);
        if (herr != hipSuccess) break;
        // 3. kernels (PCM entries: the decode kernel first, raw frames -> the unit's sc * V float streams)
        if (j.dec && (herr = pcm_decode(q.raw, *j.dec, it.sc, it.samples, it.samples * p.fb, q.pcm, it.samples, e->stream)) != hipSuccess) break;
        if ((p.rc = j.run(q.pcm, it.sc * V, it.samples, q.db, q.rgba, q.idx, e->stream))) break;
        // 3b. time reduction: the unit's kept columns (a run: from column `skip` of its it.cols) -> the set's reduced arrays
        if (f > 1 && (herr = launch_reduce_columns(q.db ? q.db + (size_t)it.skip * R : nullptr, q.idx ? q.idx + (size_t)it.skip * R : nullptr,
                                                   it.sc * V, it.cn, R, f, (size_t)it.cols * R, (size_t)((it.cn + f - 1) / f) * R, e->d_lut,
                                                   q.odb, q.oidx, q.orgba, e->stream)) != hipSuccess) break;
        // 3c. peaks: the k loudest local maxima of every kept column (peaks.hip.inc), span after span into the set's peak lists
        for (int k = 0; j.pko && k < spans_of(it, p.C, V) && herr == hipSuccess; ++k) {
            const Span sp = span_of(it, p.C, R, V, k, 1);
            herr = launch_peaks(q.db + sp.from, (int64_t)(sp.cells / R), R, j.pko->k, j.pko->min_db, q.peaks + (size_t)k * (sp.cells / R) * j.pko->k, e->stream);
        }
        // 3d. envelope and level meters: the samples under the unit's kept columns, in groups of f (window.hip.inc) - a pair and
        // a level record per stream, a cross record per source - into the set's arrays
        if ((q.wave || q.level || q.cross) && herr == hipSuccess) {
            const WaveRun wr = wave_run_of(it, j.n, j.hop, f);
            if (q.wave) herr = launch_wave(q.pcm, it.sc * V, it.samples, wr.first, wr.cols, j.hop, f, q.wave, wr.pairs, e->stream);
            if (q.level && herr == hipSuccess)
                herr = launch_level(q.pcm, it.sc * V, it.samples, wr.first, wr.cols, j.hop, f, q.level, wr.pairs, e->stream);
            if (q.cross && herr == hipSuccess)
                herr = launch_cross(q.pcm, it.sc, V, e->cross_a, e->cross_b, it.samples, wr.first, wr.cols, j.hop, f, q.cross, wr.pairs, e->stream);
        }
        // 3e. stereo image: the unit's sc sources are sc pairs of V streams, composed over all the unit's columns (stereo.hip.inc)
        if (j.stereo && herr == hipSuccess) {
            StereoCompose sc;
            sc.db = q.db, sc.views = V, sc.a = j.stereo->a, sc.b = j.stereo->b, sc.cells = (long long)it.cols * R;
            sc.law = j.stereo->law, sc.pal = reinterpret_cast<const uint32_t*>(e->d_stereo_pal);
            sc.out = StereoOut{q.slevel, q.sidx, q.span, reinterpret_cast<uint32_t*>(q.srgba)};
            herr = launch_stereo_compose(sc, it.sc, e->stream);
        }
        if (herr != hipSuccess) break;
        // 4. packed: each stream's image, its header to the host behind it
        for (int i = 0; j.pk && i < it.sc * V && herr == hipSuccess; ++i) {
            uint8_t* w = q.wire + (size_t)i * p.g.wire;
            herr = launch_wire_pack(q.oidx + (size_t)i * p.Cr * R, p.Cr, R, w, e->d_packscratch, e->stream);
            if (herr == hipSuccess) herr = hipMemcpyAsync(e->h_hdr + ((size_t)b * p.g.chunk + i) * kWireHeader, w, kWireHeader, hipMemcpyDeviceToHost, e->stream);
        }
        // 5. computed
        if (herr == hipSuccess && (j.pk || !one)) herr = hipEventRecord(p.ev_comp[b], e->stream);
        if (p.threaded) {
            std::lock_guard<std::mutex> lk(p.mu);
            if (herr == hipSuccess) p.launched = u + 1;
            p.cv.notify_all();
            continue;
        }
        // 6. copies out, kPipeLag units behind when the host has to read the images' sizes first
        while (p.ok() && p.enqueued <= u - (j.pk ? kPipeLag : 0)) drain(p, p.enqueued++);
    }
}

}  // namespace

int emspec::host_batch(emspec_engine* e, const HostJob& job) {
    Pipe p{e, job};
    if (int rc = plan_pipe(p)) return rc;
    deliver_start(p);
    run_units(p);
    deliver_finish(p);
    while (!p.threaded && p.ok() && p.enqueued < p.nu) drain(p, p.enqueued++);
    const hipError_t s1 = hipStreamSynchronize(p.s_in), s2 = p.one ? hipSuccess : hipStreamSynchronize(e->stream),
                     s3 = p.one ? hipSuccess : hipStreamSynchronize(p.s_out);
    if (p.rc != EMSPEC_OK) return p.rc;
    HIPCHK(e, p.herr); HIPCHK(e, p.herr_out);
    HIPCHK(e, s1); HIPCHK(e, s2); HIPCHK(e, s3);
    if (read_kernel_error(true) > 0) return fail(e, EMSPEC_ERR_HIP, "a kernel's bounded wait timed out (protocol error): results invalid");
    return EMSPEC_OK;
}
