// live.hip.inc — device side of the live multi-stream streaming calls (emspec_columns / emspec_push_samples_multi;
// include/emspec.h).  BASELINE configs[2] is "64 concurrent 48 kHz streams" and the renderer's call is per frame
// (north_star: computeSpectrogramColumn): here S streams advance by one hop (or one block of samples) each in ONE launch.
// No reference file:line exists (the reference source is private, /root/reference/README.md:73); the stages are those of
// SURVEY.md §8(a), the streaming glue is §8(f) row 4.  Included by kernels.hip before the frame kernels; the per-frame
// kernels (frames_kernel, ex::exact_frames_kernel, ex::exact_frames16384_kernel) call into it from their run-time sink form.
//
// Launch shape: grid = (M + 1, S), M = the largest number of frames any stream has in this launch.
//   workgroup (f, s), f < streams[s].frames : frame j0 + f of stream s -> device-scope atomics into the stream's column ring
//                                             [slots][rows]; then takes a ticket; the last one finalises (live_finalize)
//   workgroup (M, s)                        : moves the stream's new samples from the staging block into its sample ring
// Samples: absolute sample a of stream s is fresh[s][a - newbase] when a >= newbase (page-locked host memory, read over
// PCIe by the kernel - no copy engine, no second launch) and sring[s][a & ring_mask] otherwise.  The ring holds at least
// n + (the staging block's capacity) samples, so what this launch's ingest overwrites is older than anything its frames read.
#pragma once

namespace emspec {

// Diagnostic build: thread 0 of a stream's first frame workgroup stamps the 100 MHz wall clock at phase k (0: entry, 1: descriptor
// read, 2: samples in registers, 3: transform done, 4: bins + scatter issued, 5: ticket taken, 6: finalised).
__device__ __forceinline__ void live_stamp(const LiveSinks& lv, int s, int f, int k) {
#ifdef EMSPEC_DIAG
    if (lv.stamps && f == 0 && threadIdx.x == 0) lv.stamps[s * 8 + k] = wall_clock64();
#endif
}

__device__ __forceinline__ void live_stamp_after(const LiveSinks& lv, int s, int f, int k, float dep) {
#ifdef EMSPEC_DIAG
    asm volatile("" ::"v"(dep));   // the stamp is taken once `dep` has arrived
    live_stamp(lv, s, f, k);
#endif
}

struct LiveBlock {
    LiveStream d;   // the stream's descriptor as the host wrote it (the long band's frame count: what the finalize emits)
    long long bj0;  // this band's first frame in the launch ...
    int bframes;    // ... and how many (they differ from d.j0 / d.frames for the short band of a multi-resolution session only)
    int s;          // stream
    int f;          // frame within the launch
    long long a0;   // absolute index of the frame's first sample
    long long jc0;  // column of the band's first frame in the launch: the ring is indexed by the emitted column
    const float* fresh;
    const float* ring;
    int mask;
    // (returns false when this workgroup has nothing to transform: it is the ingest workgroup, or beyond the stream's frames)
    __device__ __forceinline__ bool init(const LiveSinks& lv, int hop, int nthreads) {
        s = (int)blockIdx.y;
        f = (int)blockIdx.x;
        live_stamp(lv, s, f, 0);
        // every stream in the same state (the usual case): the descriptor travels in the kernel arguments - one PCIe round trip less
        d = lv.uniform ? lv.uni : lv.streams[s];
        if (d.frames >= 0) live_stamp(lv, s, f, 1);   // (depends on the descriptor: stamped when it has arrived)
        mask = lv.ring_mask;
        fresh = lv.fresh + (size_t)s * (size_t)lv.fresh_stride;
        ring = lv.sring ? lv.sring + (size_t)s * (size_t)(mask + 1) : nullptr;
        // short band of a multi-resolution session: frame_shift frames ahead, and frames 0 .. frame_shift with the first one
        bj0 = d.j0 == 0 ? 0 : d.j0 + lv.frame_shift;
        bframes = (d.j0 == 0 && d.frames > 0) ? d.frames + lv.frame_shift : d.frames;
        if (f == (int)gridDim.x - 1) {
            if (lv.sring && !lv.no_ingest) {
                float* w = lv.sring + (size_t)s * (size_t)(mask + 1);
                for (int i = (int)threadIdx.x; i < d.newcount; i += nthreads) w[(d.newbase + i) & mask] = fresh[i];
            }
            return false;
        }
        if (f >= bframes) return false;
        a0 = (bj0 + f) * (long long)hop;
        jc0 = bj0 - lv.col_shift;
        return true;
    }
    __device__ __forceinline__ float sample(int n) const {
        const long long a = a0 + n, rel = a - d.newbase;
        return rel >= 0 ? fresh[rel] : ring[a & mask];
    }
    __device__ __forceinline__ long long column() const { return jc0 + f; }
};

// Ring slot of column jcol + dcol, |dcol| <= D < slots, from the slot of jcol: no 64-bit modulo per bin.
__device__ __forceinline__ int live_slot(int slot_j, int dcol, int slots) {
    int sl = slot_j + dcol;
    sl = sl < 0 ? sl + slots : sl;
    return sl >= slots ? sl - slots : sl;
}

// After a frame's atomics: true on every thread of the stream's LAST workgroup (which then finalises).  The counter returns
// to zero for the next launch.  lds_word: any word of the kernel's dynamic LDS - the frame's spectrum is dead once every wave
// has passed the first barrier below (a static __shared__ word would lower the 160 KB the frame kernels may ask for).
__device__ __forceinline__ bool live_last_arrival(const LiveSinks& lv, int s, int frames, void* lds_word) {
    if (lv.defer_finalize) return false;   // live_finalize_kernel follows on the stream: the kernel boundary orders the scatter before it
    unsigned* const tk = reinterpret_cast<unsigned*>(lds_word);
    if (frames == 1) {
        // The stream's only workgroup of this launch (the live case: one hop per call).  Its scatter - device-scope atomics,
        // performed at the memory side - is complete once every wave has waited for the acknowledgement of its own
        // (s_waitcnt vmcnt(0): a workgroup-scope fence alone compiles to no wait - the ISA showed a bare s_barrier - and a
        // finalising load of another wave could then overtake an add to the column that leaves, i.e. a bin with dcol = -D) and
        // passed the barrier; the finalising loads are device-scope too.  No ticket, and no agent-scope fence: that one also
        // writes the L2 back (~2 us), which the end of the kernel does anyway.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __threadfence_block();
        __syncthreads();
        live_stamp(lv, s, (int)blockIdx.x, 4);
        live_stamp(lv, s, (int)blockIdx.x, 5);
        return true;
    }
    __threadfence();        // the scatter's atomics are performed at device scope; this orders them before the ticket
    __syncthreads();
    live_stamp(lv, s, (int)blockIdx.x, 4);
    if (threadIdx.x == 0) *tk = atomicAdd(lv.done + s, 1u);
    __syncthreads();
    const unsigned ticket = *tk;
    live_stamp(lv, s, (int)blockIdx.x, 5);
    const bool last = ticket + 1u == (unsigned)frames;
    if (last) {
        if (threadIdx.x == 0) __hip_atomic_store(lv.done + s, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
    }
    return last;
}

// Finalise the i-th of the columns this launch completed for stream s: column j0 - D + i (i < frames; flush form: i < flush).
// Columns below 0 are skipped - or, in the per-frame form, emitted as the empty column.  CELL: float (FAST) or unsigned long long
// (EXACT); conv(cell, db, index) is the mode's "dB + colour" stage.
// rows: the launch's band (ring stride, loop bound); it fills rows [lv.row0, lv.row0 + rows) of the output column of lv.out_rows
// rows in place - the other band of a multi-resolution session writes the rest of the same column from its own ring.
// D: the latency of the EMITTED column (the long band's; the frame kernels pass their plan's D + lv.lat_extra).
template <class CELL, class CONV>
__device__ __forceinline__ void live_finalize_column(const LiveSinks& lv, const LiveStream& d, int s, int i, CELL* ring_all, int slots,
                                                     int rows, int D, int nthreads, const CONV& conv) {
    const long long c = d.j0 - D + i;
    if (c < 0 && !lv.empty_col) return;
    // its slot in the stream's output block: out_at + the columns emitted before it (those below 0 are not, without empty_col)
    const long long below = d.j0 - D < 0 ? D - d.j0 : 0;
    const int oc = d.out_at + (lv.empty_col ? i : i - (int)(below < i ? below : i));
    CELL* ring = ring_all + (size_t)s * (size_t)slots * (size_t)rows;
    const size_t oat = ((size_t)s * (size_t)lv.out_cols + (size_t)oc) * (size_t)lv.out_rows + (size_t)lv.row0;
    float* odb = lv.out_db ? lv.out_db + oat : nullptr;
    uint32_t* orgba = lv.out_rgba ? lv.out_rgba + oat : nullptr;
    CELL* cells = c >= 0 ? ring + (size_t)(c % slots) * (size_t)rows : nullptr;
    // FIN rows of a thread in flight at once: each load is a round trip to the memory side (~2 us), and issued one per
    // loop iteration they were 4 serial round trips of the finalising workgroup (9.8 us of a 31 us kernel)
    constexpr int FIN = 8;
    for (int r0 = (int)threadIdx.x; r0 < rows; r0 += nthreads * FIN) {
        CELL e[FIN];
#pragma unroll
        for (int u = 0; u < FIN; ++u) {
            const int r = r0 + u * nthreads;
            e[u] = (cells && r < rows) ? __hip_atomic_load(cells + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : CELL(0);
        }
#pragma unroll
        for (int u = 0; u < FIN; ++u) {
            const int r = r0 + u * nthreads;
            if (cells && r < rows) __hip_atomic_store(cells + r, CELL(0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int u = 0; u < FIN; ++u) {
            const int r = r0 + u * nthreads;
            if (r >= rows) break;
            float db;
            int idx;
            conv(e[u], db, idx);
            if (odb) odb[r] = db;
            if (orgba) orgba[r] = lv.lut[idx];
        }
    }
}
// ... all of them, by one workgroup (the stream's last one of a frame launch).  A launch that completes many columns per stream
// (a long block of samples) defers them to live_finalize_kernel instead, one workgroup per column (lv.defer_finalize).
template <class CELL, class CONV>
__device__ __forceinline__ void live_finalize(const LiveSinks& lv, const LiveStream& d, int s, CELL* ring_all, int slots, int rows,
                                              int D, int nthreads, const CONV& conv) {
    const int ncol = d.flush ? d.flush : d.frames;
    for (int i = 0; i < ncol; ++i) live_finalize_column<CELL>(lv, d, s, i, ring_all, slots, rows, D, nthreads, conv);
}

struct LiveConvF32 {
    DbMap m;
    __device__ __forceinline__ void operator()(float e, float& db, int& idx) const {
        db = cell_db(m, e);
        idx = cell_index(m, db);
    }
};

}  // namespace emspec
