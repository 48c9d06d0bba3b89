// live_history.hip.inc — the live history (include/emspec.h: emspec_set_live_history, emspec_history_view; DESIGN.md §3.14,
// §4.16): a ring of the dB columns the streaming calls deliver, W per stream, and views that read it back reduced by a factor
// and coloured by a law of the caller's.  Two kernels: the store goes behind a live launch's last kernel, where the overlay
// kernel goes (live_overlay.hip.inc), and reads the same LiveSinks descriptors; the view is the time reduction of reduce.hip.inc
// (DESIGN.md §3.10) with the ring as its input and cell_index + LUT behind it.  The arithmetic of slots, held ranges and groups:
// emspec_history_plan.h.  Included by kernels.hip behind live_overlay.hip.inc.
namespace emspec {

// Grid (units, S), units = the most frames (flush form: columns) any stream has in the launch: workgroup (i, s) serves the
// launch's i-th column of stream s, c = j0 - D + i, which the frame / flush / post kernels left in slot live_out_slot(..) of the
// device block h.db (laid out like the launch's output).  It loads the column with 16-byte loads, writes it to the caller's
// out_db when the overlay kernel does not (h.fill_out), and stores it in ring slot c mod W - unless c is the empty column of
// the per-frame form (c < 0: delivered, not a column) or the launch emits more than W columns of the stream and c is not among
// the last W (history_keep_from: no two workgroups of a launch write one slot).  Workgroup (0, s) records the stream's new
// column count for the view kernel.  All global offsets are 64-bit; plain vector stores only.
__global__ __launch_bounds__(256) void live_history_store_kernel(LiveSinks lv, LiveHistory h) {
    const int s = (int)blockIdx.y, i = (int)blockIdx.x;
    const LiveStream d = lv.uniform ? lv.uni : lv.streams[s];
    const int ncol = d.flush ? d.flush : d.frames;
    if (i >= ncol) return;
    const long long c = d.j0 - h.D + i, cend = d.j0 - h.D + ncol, c0 = d.j0 - h.D < 0 ? 0 : d.j0 - h.D;
    if (i == 0 && threadIdx.x == 0 && cend > 0) h.ends[s] = cend;
    const int oc = live_out_slot(d.j0, d.out_at, h.D, i, lv.empty_col != 0);
    if (oc < 0) return;
    const bool keep = c >= 0 && c >= history_keep_from(c0, cend - c0, h.W);
    float* odb = h.fill_out && lv.out_db ? lv.out_db + ((size_t)s * (size_t)lv.out_cols + (size_t)oc) * (size_t)h.rows : nullptr;
    if (!keep && !odb) return;
    const int Q = h.rows >> 2;
    const float4* src = reinterpret_cast<const float4*>(h.db + ((size_t)s * (size_t)lv.out_cols + (size_t)oc) * (size_t)h.rows);
    float4* dst = keep ? reinterpret_cast<float4*>(h.ring + ((size_t)s * (size_t)h.W + (size_t)history_slot(c, h.W)) * (size_t)h.rows) : nullptr;
    const bool aligned = (reinterpret_cast<uintptr_t>(odb) & 15) == 0;
    for (int q = (int)threadIdx.x; q < Q; q += 256) {
        const float4 v = src[q];
        if (dst) dst[q] = v;
        if (odb) {
            if (aligned) reinterpret_cast<float4*>(odb)[q] = v;
            else { odb[4 * q] = v.x; odb[4 * q + 1] = v.y; odb[4 * q + 2] = v.z; odb[4 * q + 3] = v.w; }
        }
    }
}

// lv: the launch's sinks with out_db / out_cols the CALLER's dB destination (null: not wanted) and the stride of h.db;
// units: the most frames (flush form: columns) of any stream.  rows % 4 == 0, 1 <= W.
hipError_t launch_live_history_store(const LiveSinks& lv, const LiveHistory& h, int S, int units, hipStream_t st) {
    if (S <= 0 || units <= 0) return hipSuccess;
    if (S > 65535 || !h.db || !h.ring || !h.ends || h.W < 1 || h.rows < 4 || h.rows % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(live_history_store_kernel, dim3((unsigned)units, (unsigned)S), dim3(256), 0, st, lv, h);
    return hipGetLastError();
}

// ---- the view ----
__device__ __forceinline__ void history_hold(float4& m, const float4& x) {   // (reduce.hip.inc: hold, on a row quad)
    hold(m.x, x.x); hold(m.y, x.y); hold(m.z, x.z); hold(m.w, x.w);
}
// Columns j0 .. j1 - 1 of a group whose first column sits in slot `slot0` of the stream's ring `col` ([W][Q] quads), row quad q,
// held into m in column order: four columns' 16-byte loads in flight, the slot advanced by one per column and wrapped by one
// compare (past the end: the run's last column again, which changes nothing).
__device__ __forceinline__ void history_walk(const float4* __restrict__ col, int Q, int W, int slot0, int j0, int j1, int q, float4& m) {
    int slot = slot0 + j0;
    slot = slot >= W ? slot - W : slot;
    for (int j = j0; j < j1; j += 4) {
        float4 v[4];
        int sl = slot;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = col[(size_t)sl * (size_t)Q + (size_t)q];
            if (j + k + 1 < j1) sl = history_next_slot(sl, W);
        }
        slot = sl;   // (the slot of column j + 4 when the run has one)
#pragma unroll
        for (int k = 0; k < 4; ++k) history_hold(m, v[k]);
    }
}

// One pass.  A thread owns row quad q of group g of stream v.stream0 + blockIdx.y; (g, q) = blockIdx.x * 64 * (SPLIT ? 1 : 4) +
// its index in that run, q fastest, so a wave reads consecutive 16-byte pieces of one stored column.
//   SPLIT = false: 256 threads, each walks its whole group.
//   SPLIT = true: blockDim = (64, P): the P waves of a workgroup serve the SAME 64 (g, q) and cut the group's columns into P
//     consecutive runs; wave 0 starts from the group's first column as the definition does, the others from -inf (which no
//     column's value fails to replace unless it is -inf itself, or a NaN, which the definition skips behind the first
//     column too), and wave 0 holds their results in run order out of LDS.  A maximum taken in the definition's order over
//     runs in order: the split changes no byte.  For views of few wide groups (one group of W columns per stream).
// Then cell_index of dB + shift under the view's law, and the LUT: per row quad one 16-byte dB store, one 4-byte index word,
// one 16-byte RGBA store (each only when asked for).
template <bool SPLIT>
__global__ __launch_bounds__(SPLIT ? 1024 : 256) void history_view_kernel(HistoryView v) {
    __shared__ float4 part[SPLIT ? 15 * 64 : 1];
    const int Q = v.rows >> 2;
    const unsigned t = SPLIT ? blockIdx.x * 64u + threadIdx.x : blockIdx.x * 256u + threadIdx.x;
    const int p = SPLIT ? (int)threadIdx.y : 0, P = SPLIT ? (int)blockDim.y : 1;
    const int sv = (int)blockIdx.y, s = v.stream0 + sv;
    const bool live = t < (unsigned)v.groups * (unsigned)Q;
    const unsigned g = live ? t / (unsigned)Q : 0u;
    const int q = live ? (int)(t - g * (unsigned)Q) : 0;
    const HistoryGroup grp = history_group(v.first, v.f, (long long)g, v.ends[s]);
    long long n64 = grp.c1 - grp.c0;
    n64 = n64 < 1 ? 1 : (n64 > v.W ? v.W : n64);   // (a view that fits has 1 .. min(f, W) columns in every group)
    const int n = (int)n64;
    const float4* col = reinterpret_cast<const float4*>(v.ring + (size_t)s * (size_t)v.W * (size_t)v.rows);
    const int slot0 = history_group_slot(v.slot_first, (int)(g * (unsigned)v.f), v.W);
    const int run = (n + P - 1) / P, j0 = p * run < n ? p * run : n, j1 = j0 + run < n ? j0 + run : n;
    const float ninf = -__builtin_inff();
    float4 m = make_float4(ninf, ninf, ninf, ninf);
    if (p == 0) {
        m = col[(size_t)slot0 * (size_t)Q + (size_t)q];
        history_walk(col, Q, v.W, slot0, 1, j1, q, m);
    } else {
        history_walk(col, Q, v.W, slot0, j0, j1, q, m);
    }
    if constexpr (SPLIT) {
        if (p > 0) part[(p - 1) * 64 + threadIdx.x] = m;
        __syncthreads();
        if (p > 0) return;
        for (int k = 1; k < P; ++k) history_hold(m, part[(k - 1) * 64 + threadIdx.x]);
    }
    if (!live) return;
    const size_t cell = ((size_t)sv * (size_t)v.groups + (size_t)g) * (size_t)v.rows + (size_t)q * 4;
    if (v.db) *reinterpret_cast<float4*>(v.db + cell) = m;
    if (v.index || v.rgba) {
        const uint32_t ix = (uint32_t)cell_index(v.map, m.x + v.shift), iy = (uint32_t)cell_index(v.map, m.y + v.shift);
        const uint32_t iz = (uint32_t)cell_index(v.map, m.z + v.shift), iw = (uint32_t)cell_index(v.map, m.w + v.shift);
        if (v.index) *reinterpret_cast<uint32_t*>(v.index + cell) = ix | (iy << 8) | (iz << 16) | (iw << 24);
        if (v.rgba) *reinterpret_cast<uint4*>(v.rgba + cell) = make_uint4(v.lut[ix], v.lut[iy], v.lut[iz], v.lut[iw]);
    }
}

// The split form when the plain one's streams x groups x rows / 4 threads are fewer than two waves per SIMD of the device and
// the groups are wide enough to cut: P = the waves that fill it, at most 16, each with at least 16 columns.
int history_view_split(int streams, int64_t groups, int rows, int f) {
    const int64_t threads = (int64_t)streams * groups * (rows / 4), want = (int64_t)device_cus() * 512;
    if (threads >= want || f < 32) return 1;
    const int64_t p = std::min<int64_t>(std::min<int64_t>((want + threads - 1) / threads, 16), f / 16);
    return p < 2 ? 1 : (int)p;
}

// v: the view (emspec_launch.h); streams: how many from v.stream0 on.  The caller has validated the view against every
// addressed stream (emspec_history_plan.h: history_view_check) - the kernel reads v.ends only for the last group's length.
// rows % 4 == 0; db / rgba 16-byte and index 4-byte aligned; groups <= W.
hipError_t launch_history_view(const HistoryView& v, int streams, hipStream_t st) {
    if (streams <= 0 || v.groups <= 0) return hipSuccess;
    if (!v.db && !v.index && !v.rgba) return hipSuccess;
    if (streams > 65535 || !v.ring || !v.ends || v.W < 1 || v.groups > v.W || v.rows < 4 || v.rows % 4 || v.f < 1 || v.slot_first < 0 ||
        v.slot_first >= v.W || (int64_t)(v.groups - 1) * v.f >= v.W || ((v.index || v.rgba) && !v.lut))
        return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(v.db) | reinterpret_cast<uintptr_t>(v.rgba)) % 16 || reinterpret_cast<uintptr_t>(v.index) % 4)
        return hipErrorInvalidValue;
    const int64_t work = (int64_t)v.groups * (v.rows / 4);   // (<= 2^20 x 2^10)
    const int P = history_view_split(streams, v.groups, v.rows, v.f);
    if (P > 1)
        hipLaunchKernelGGL(history_view_kernel<true>, dim3((unsigned)((work + 63) / 64), (unsigned)streams), dim3(64, (unsigned)P), 0, st, v);
    else
        hipLaunchKernelGGL(history_view_kernel<false>, dim3((unsigned)((work + 255) / 256), (unsigned)streams), dim3(256), 0, st, v);
    return hipGetLastError();
}

}  // namespace emspec
