// stereo.hip.inc — the stereo image (include/emspec.h: emspec_stereo_device, emspec_batch_stereo_device,
// emspec_history_view_stereo*; DESIGN.md §3.16, §4.18): one picture of a channel pair, brightness from the louder channel,
// hue from the balance of the two.  Two kernels: the compose kernel on any dB array [pairs * views][cells], and the stereo
// history view, which is history_view_kernel's walk (live_history.hip.inc) over the rings of both channels.  Both end in the
// same per-quad stage; the per-cell arithmetic is emspec_stereo_plan.h's, which the host twin runs too.  Included by kernels.hip
// behind live_history.hip.inc.
namespace emspec {

// One row quad of a pair: xa / xb the two channels' dB, `cell` the quad's first cell in the outputs.  Per requested output one
// 16-byte level store, one 4-byte index word, one 4-byte pan word, one 16-byte RGBA store (the palette read from global memory).
__device__ __forceinline__ void stereo_quad(const StereoLaw& w, const uint32_t* __restrict__ pal, const StereoOut& o, size_t cell,
                                            const float4& xa, const float4& xb) {
    const StereoCell c0 = stereo_cell(w, xa.x, xb.x), c1 = stereo_cell(w, xa.y, xb.y);
    const StereoCell c2 = stereo_cell(w, xa.z, xb.z), c3 = stereo_cell(w, xa.w, xb.w);
    if (o.level) *reinterpret_cast<float4*>(o.level + cell) = make_float4(c0.level, c1.level, c2.level, c3.level);
    if (o.index)
        *reinterpret_cast<uint32_t*>(o.index + cell) = (uint32_t)c0.index | ((uint32_t)c1.index << 8) | ((uint32_t)c2.index << 16) | ((uint32_t)c3.index << 24);
    if (o.pan)
        *reinterpret_cast<uint32_t*>(o.pan + cell) = (uint32_t)c0.pan | ((uint32_t)c1.pan << 8) | ((uint32_t)c2.pan << 16) | ((uint32_t)c3.pan << 24);
    if (o.rgba)
        *reinterpret_cast<uint4*>(o.rgba + cell) = make_uint4(pal[c0.pan * 256 + c0.index], pal[c1.pan * 256 + c1.index],
                                                              pal[c2.pan * 256 + c2.index], pal[c3.pan * 256 + c3.index]);
}

// Grid (ceil(cells / 4 / 256), pairs): a thread owns row quad blockIdx.x * 256 + threadIdx.x of pair blockIdx.y - two 16-byte
// loads, channel A from stream pair * views + a and channel B from stream pair * views + b.  64-bit offsets; plain vector
// stores only, no LDS, no scratch.
__global__ __launch_bounds__(256) void stereo_compose_kernel(StereoCompose s) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)(s.cells >> 2)) return;
    const size_t pair = blockIdx.y, cells = (size_t)s.cells;
    const float4 xa = reinterpret_cast<const float4*>(s.db + (pair * (size_t)s.views + (size_t)s.a) * cells)[q];
    const float4 xb = reinterpret_cast<const float4*>(s.db + (pair * (size_t)s.views + (size_t)s.b) * cells)[q];
    stereo_quad(s.law, s.pal, s.out, pair * cells + q * 4, xa, xb);
}

// cells % 4 == 0; db, level, rgba 16-byte and index, pan 4-byte aligned; 0 <= a, b < views; pairs <= 65535.
hipError_t launch_stereo_compose(const StereoCompose& s, int pairs, hipStream_t st) {
    if (pairs <= 0 || s.cells <= 0) return hipSuccess;
    if (!s.out.level && !s.out.index && !s.out.pan && !s.out.rgba) return hipSuccess;
    const int64_t blocks = (s.cells / 4 + 255) / 256;
    if (pairs > 65535 || s.cells % 4 || blocks > 0x7fffffff || !s.db || s.views < 2 || s.a < 0 || s.a >= s.views || s.b < 0 || s.b >= s.views ||
        (s.out.rgba && !s.pal))
        return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(s.db) | reinterpret_cast<uintptr_t>(s.out.level) | reinterpret_cast<uintptr_t>(s.out.rgba)) % 16 ||
        (reinterpret_cast<uintptr_t>(s.out.index) | reinterpret_cast<uintptr_t>(s.out.pan)) % 4)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(stereo_compose_kernel, dim3((unsigned)blocks, (unsigned)pairs), dim3(256), 0, st, s);
    return hipGetLastError();
}

// ---- the stereo history view ----
// The peak hold of row quad q of group g of one stream's ring, as history_view_kernel takes it: wave p of P walks its run of the
// group's n columns (wave 0 from the group's first column, the others from -inf).
__device__ __forceinline__ float4 stereo_hold_run(const float4* __restrict__ col, int Q, int W, int slot0, int n, int p, int P, int q) {
    const int run = (n + P - 1) / P, j0 = p * run < n ? p * run : n, j1 = j0 + run < n ? j0 + run : n;
    const float ninf = -__builtin_inff();
    float4 m = make_float4(ninf, ninf, ninf, ninf);
    if (p == 0) {
        m = col[(size_t)slot0 * (size_t)Q + (size_t)q];
        history_walk(col, Q, W, slot0, 1, j1, q, m);
    } else {
        history_walk(col, Q, W, slot0, j0, j1, q, m);
    }
    return m;
}

// A thread owns row quad q of group g of pair blockIdx.y, (g, q) indexed as in history_view_kernel; the two channels' rings are
// those of streams stream0 + pair * views + a / + b.  SPLIT as there: blockDim = (64, P), the P waves cut each channel's group
// into runs and wave 0 holds the partial maxima in run order out of LDS (2 x 15 x 64 quads), which changes no byte.  Then the
// per-quad stage on the two maxima.
template <bool SPLIT>
__global__ __launch_bounds__(SPLIT ? 1024 : 256) void stereo_view_kernel(StereoView v) {
    __shared__ float4 part[SPLIT ? 2 * 15 * 64 : 1];
    const int Q = v.rows >> 2;
    const unsigned t = SPLIT ? blockIdx.x * 64u + threadIdx.x : blockIdx.x * 256u + threadIdx.x;
    const int p = SPLIT ? (int)threadIdx.y : 0, P = SPLIT ? (int)blockDim.y : 1;
    const int pair = (int)blockIdx.y, sa = v.stream0 + pair * v.views + v.a, sb = v.stream0 + pair * v.views + v.b;
    const bool live = t < (unsigned)v.groups * (unsigned)Q;
    const unsigned g = live ? t / (unsigned)Q : 0u;
    const int q = live ? (int)(t - g * (unsigned)Q) : 0;
    const int slot0 = history_group_slot(v.slot_first, (int)(g * (unsigned)v.f), v.W);
    float4 m[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const int s = ch ? sb : sa;
        const HistoryGroup grp = history_group(v.first, v.f, (long long)g, v.ends[s]);
        long long n64 = grp.c1 - grp.c0;
        n64 = n64 < 1 ? 1 : (n64 > v.W ? v.W : n64);   // (a view that fits has 1 .. min(f, W) columns in every group)
        const float4* col = reinterpret_cast<const float4*>(v.ring + (size_t)s * (size_t)v.W * (size_t)v.rows);
        m[ch] = stereo_hold_run(col, Q, v.W, slot0, (int)n64, p, P, q);
    }
    if constexpr (SPLIT) {
        if (p > 0) {
            part[(p - 1) * 64 + threadIdx.x] = m[0];
            part[(15 + p - 1) * 64 + threadIdx.x] = m[1];
        }
        __syncthreads();
        if (p > 0) return;
        for (int k = 1; k < P; ++k) {
            history_hold(m[0], part[(k - 1) * 64 + threadIdx.x]);
            history_hold(m[1], part[(15 + k - 1) * 64 + threadIdx.x]);
        }
    }
    if (!live) return;
    const size_t cell = ((size_t)pair * (size_t)v.groups + (size_t)g) * (size_t)v.rows + (size_t)q * 4;
    stereo_quad(v.law, v.pal, v.out, cell, m[0], m[1]);
}

// v: the view (emspec_launch.h); the caller has validated it against every stream of every pair (history_view_check).
// rows % 4 == 0; level / rgba 16-byte and index / pan 4-byte aligned; groups <= W.  The split as the mono view of the pairs'
// 2 x pairs streams takes it.
hipError_t launch_stereo_view(const StereoView& v, int pairs, hipStream_t st) {
    if (pairs <= 0 || v.groups <= 0) return hipSuccess;
    if (!v.out.level && !v.out.index && !v.out.pan && !v.out.rgba) return hipSuccess;
    if (pairs > 65535 || !v.ring || !v.ends || v.W < 1 || v.groups > v.W || v.rows < 4 || v.rows % 4 || v.f < 1 || v.slot_first < 0 ||
        v.slot_first >= v.W || (int64_t)(v.groups - 1) * v.f >= v.W || v.views < 2 || v.a < 0 || v.a >= v.views || v.b < 0 || v.b >= v.views ||
        v.stream0 < 0 || (v.out.rgba && !v.pal))
        return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(v.out.level) | reinterpret_cast<uintptr_t>(v.out.rgba)) % 16 ||
        (reinterpret_cast<uintptr_t>(v.out.index) | reinterpret_cast<uintptr_t>(v.out.pan)) % 4)
        return hipErrorInvalidValue;
    const int64_t work = (int64_t)v.groups * (v.rows / 4);
    const int P = history_view_split(2 * pairs, v.groups, v.rows, v.f);
    if (P > 1)
        hipLaunchKernelGGL(stereo_view_kernel<true>, dim3((unsigned)((work + 63) / 64), (unsigned)pairs), dim3(64, (unsigned)P), 0, st, v);
    else
        hipLaunchKernelGGL(stereo_view_kernel<false>, dim3((unsigned)((work + 255) / 256), (unsigned)pairs), dim3(256), 0, st, v);
    return hipGetLastError();
}

}  // namespace emspec
