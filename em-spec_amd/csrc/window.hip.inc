// window.hip.inc — the reductions over the samples under each delivered column (DESIGN.md §3.12, §3.17, §4.13, §4.19;
// include/emspec.h: emspec_wave_device, emspec_level_device, emspec_cross_device, emspec_set_wave_out, _level_out, _cross_out):
// ONE walk over the windows with three reducers (emspec_window_plan.h) - the envelope's pair (lo, hi), the level record (sum of
// k^2 in two limbs, peak |k|, count of NaN and saturated samples) and, per pair of streams, the cross record (sum of k_A k_B in
// two limbs).  Integer minima, maxima and sums only: a result is a function of the window's bits, whatever the order and the
// split.  One HBM-bound pass: every sample of a window is read once, with 16-byte loads between the window's first and last
// 16-byte boundary and per element outside (window_scan).  Included by kernels.hip after peaks.hip.inc.
#include "emspec_window_plan.h"

namespace emspec {

// ---- what a reducer needs of the device beside the plan header: the xor butterfly's step (the Acc of the lane m away, combined
// into this lane's) and the atomic merge of a piece's Acc into the window's slot, which holds the start value or other pieces.
__device__ __forceinline__ uint32_t window_shfl(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
__device__ __forceinline__ uint64_t window_shfl(uint64_t v, int m) {
    return ((uint64_t)window_shfl((uint32_t)(v >> 32), m) << 32) | window_shfl((uint32_t)v, m);
}
__device__ __forceinline__ void window_mix(WaveKeys& r, int m) { EnvelopeRed::combine(r, WaveKeys{window_shfl(r.lo, m), window_shfl(r.hi, m)}); }
__device__ __forceinline__ void window_mix(emspec_level& r, int m) {
    LevelRed::combine(r, emspec_level{window_shfl(r.sq_lo, m), window_shfl(r.sq_hi, m), window_shfl(r.peak, m), window_shfl(r.odd, m)});
}
__device__ __forceinline__ void window_mix(emspec_cross& r, int m) {
    CrossRed::combine(r, emspec_cross{window_shfl(r.lo, m), (int64_t)window_shfl((uint64_t)r.hi, m)});
}
// the envelope: integer minimum and maximum of keys; the records: 64-bit integer sums (the high limb of a cross record adds as
// its two's complement) and the peak's maximum
__device__ __forceinline__ void window_merge(WaveKeys* o, const WaveKeys& r) {
    atomicMin(&o->lo, r.lo);
    atomicMax(&o->hi, r.hi);
}
__device__ __forceinline__ void window_merge(emspec_level* o, const emspec_level& r) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sq_lo), (unsigned long long)r.sq_lo);
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sq_hi), (unsigned long long)r.sq_hi);
    atomicMax(&o->peak, r.peak);
    atomicAdd(&o->odd, r.odd);
}
__device__ __forceinline__ void window_merge(emspec_cross* o, const emspec_cross& r) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->lo), (unsigned long long)r.lo);
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->hi), (unsigned long long)r.hi);
}

// The geometry of a launch.  Window w = (s, g): group g of f columns of hop samples, from `first` samples into the stream on
// (window_of).  Row s reads stream s and, for a cross record, streams s views + a and s views + b.
struct WindowGeom { const uint32_t* x; int64_t stride, first, cols; int hop, f; int64_t Cr; int views, a, b; };
// Row s's stream(s), from the first window's first sample on: the windows are then window_of(g, f, cols, hop, 0).  (`first`
// rides in the pointers and a one-stream row has no multiply by views: measured, profiles/window_rate.txt - with `first` in
// the indices the cross team kernel was scheduled differently and ran 1.2 % slower at factor 64.)
struct WindowSrc { const uint32_t* xa; const uint32_t* xb; };
template <class Red> __device__ __forceinline__ WindowSrc window_src(const WindowGeom& G, int64_t s) {
    if constexpr (Red::kStreams == 2) return WindowSrc{G.x + (s * G.views + G.a) * G.stride + G.first, G.x + (s * G.views + G.b) * G.stride + G.first};
    else return WindowSrc{G.x + s * G.stride + G.first, nullptr};
}

// Windows of at most kWindowSplit samples: a team of T lanes (window_team: a power of two, 1 .. 64, the same for the whole
// launch) per window, 256 / T windows per workgroup and step of the grid's stride - down to one thread per window, so that
// hop = 1 is not a wave per sample.  The team's lanes combine over the xor butterfly; its first lane stores the result.
template <class Red>
__global__ __launch_bounds__(kWindowBlock) void window_kernel(WindowGeom G, int64_t windows, int T, typename Red::Acc* __restrict__ out, int64_t out_stride) {
    const int l = threadIdx.x & (T - 1);
    const int64_t per = kWindowBlock / T;
    for (int64_t w = (int64_t)blockIdx.x * per + threadIdx.x / T; w < windows; w += (int64_t)gridDim.x * per) {
        const int64_t s = w / G.Cr, g = w % G.Cr;
        const WindowSpan ws = window_of(g, G.f, G.cols, G.hop, 0);
        typename Red::Acc r = Red::start();
        const WindowSrc src = window_src<Red>(G, s);
        window_scan<Red>(src.xa, src.xb, ws.a, ws.b, l, T, r);
        for (int m = T >> 1; m >= 1; m >>= 1) window_mix(r, m);
        if (l == 0) {
            if constexpr (Red::kFinish) r = Red::finish(r);
            out[s * out_stride + g] = r;
        }
    }
}

// Longer windows: a workgroup per piece of kWindowPiece samples, `ppw` pieces per window (those past a short last window's end
// do nothing).  The pieces of a window meet in its slot of the output: window_fill_kernel writes the start value in front of
// this launch and every workgroup adds its piece with integer atomics.  (Integer minima, maxima and sums are associative and
// commutative: the slot does not depend on the order of arrival.)  The envelope's slot holds KEYS until window_finish_kernel
// turns them into the samples' bits behind this launch; the records need no pass behind.
template <class Red>
__global__ __launch_bounds__(kWindowBlock) void window_split_kernel(WindowGeom G, int64_t ppw, int64_t items, typename Red::Acc* __restrict__ out, int64_t out_stride) {
    __shared__ typename Red::Acc part[kWindowBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {   // (uniform in the workgroup, so its barriers are)
        const int64_t w = it / ppw, s = w / G.Cr, g = w % G.Cr;
        const WindowSpan ps = window_piece(window_of(g, G.f, G.cols, G.hop, 0), it % ppw);
        if (ps.a >= ps.b) continue;
        typename Red::Acc r = Red::start();
        const WindowSrc src = window_src<Red>(G, s);
        window_scan<Red>(src.xa, src.xb, ps.a, ps.b, threadIdx.x, kWindowBlock, r);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) window_mix(r, m);
        if (lane == 0) part[wv] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 1; k < kWindowBlock / 64; ++k) Red::combine(r, part[k]);
            window_merge(out + (s * out_stride + g), r);
        }
        __syncthreads();   // the next item overwrites part[]
    }
}
// every slot of the launch := the reducer's start value, `words` 8-byte words of `value` each (the envelope: one word of start
// keys; the records: zeros)
__global__ __launch_bounds__(kWindowBlock) void window_fill_kernel(uint64_t* __restrict__ out, int64_t out_stride, int64_t Cr, int64_t windows, int words,
                                                                    uint64_t value) {
    for (int64_t i = (int64_t)blockIdx.x * kWindowBlock + threadIdx.x; i < windows * words; i += (int64_t)gridDim.x * kWindowBlock) {
        const int64_t w = i / words;
        out[((w / Cr) * out_stride + w % Cr) * words + i % words] = value;
    }
}
// every slot of the launch: keys -> the samples' bits (the envelope behind the split)
template <class Red>
__global__ __launch_bounds__(kWindowBlock) void window_finish_kernel(typename Red::Acc* __restrict__ out, int64_t out_stride, int64_t Cr, int64_t windows) {
    for (int64_t w = (int64_t)blockIdx.x * kWindowBlock + threadIdx.x; w < windows; w += (int64_t)gridDim.x * kWindowBlock) {
        typename Red::Acc* o = out + (w / Cr) * out_stride + w % Cr;
        *o = Red::finish(*o);
    }
}

// pcm: rows x views streams, `stride` samples apart, 4-byte aligned; row s's windows start `first` samples into its stream(s)
// and cover `cols` columns of `hop` samples in groups of f: ceil(cols / f) results per row into out (8-byte aligned),
// out_stride results apart.  `first` makes a unit of the host pipeline that is a run of columns of a longer stream servable
// (emspec_host.cpp).  The caller guarantees first + cols hop <= the samples of a stream, and f hop <= 2^30.  All offsets are
// 64-bit; the grids stride.
template <class Red>
static hipError_t launch_window(const float* pcm, int rows, int views, int a, int b, int64_t stride, int64_t first, int64_t cols, int hop, int f,
                                void* out, int64_t out_stride, hipStream_t st) {
    using Acc = typename Red::Acc;
    static_assert(sizeof(Acc) % 8 == 0 && alignof(Acc) == 8, "a slot is 8-byte words");
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (!pcm || !out || hop < 1 || f < 1 || first < 0 || views < 1 || a < 0 || a >= views || b < 0 || b >= views ||
        reinterpret_cast<uintptr_t>(pcm) % 4 || reinterpret_cast<uintptr_t>(out) % 8)
        return hipErrorInvalidValue;
    const WindowGeom G{reinterpret_cast<const uint32_t*>(pcm), stride, first, cols, hop, f, (cols + f - 1) / f, views, a, b};
    const int64_t windows = (int64_t)rows * G.Cr, longest = window_longest(f, cols, hop);
    auto grid = [](int64_t blocks) { return dim3((unsigned)(blocks < kWindowGridCap ? blocks : kWindowGridCap)); };
    const dim3 block(kWindowBlock);
    Acc* o = static_cast<Acc*>(out);
    if (longest <= kWindowSplit) {
        const int T = window_team(longest);
        hipLaunchKernelGGL(window_kernel<Red>, grid((windows + kWindowBlock / T - 1) / (kWindowBlock / T)), block, 0, st, G, windows, T, o, out_stride);
        return hipGetLastError();
    }
    const int words = (int)(sizeof(Acc) / 8);
    const Acc none = Red::start();
    uint64_t value;   // (every word of a start value is its first)
    __builtin_memcpy(&value, &none, 8);
    const int64_t ppw = window_pieces(longest), items = windows * ppw;
    hipLaunchKernelGGL(window_fill_kernel, grid((windows * words + kWindowBlock - 1) / kWindowBlock), block, 0, st, reinterpret_cast<uint64_t*>(out),
                       out_stride, G.Cr, windows, words, value);
    hipLaunchKernelGGL(window_split_kernel<Red>, grid(items), block, 0, st, G, ppw, items, o, out_stride);
    if constexpr (Red::kFinish)
        hipLaunchKernelGGL(window_finish_kernel<Red>, grid((windows + kWindowBlock - 1) / kWindowBlock), block, 0, st, o, out_stride, G.Cr, windows);
    return hipGetLastError();
}

// (contracts: emspec_launch.h)
hipError_t launch_wave(const float* pcm, int S, int64_t stride, int64_t first, int64_t cols, int hop, int f, void* out, int64_t out_stride,
                       hipStream_t st) {
    return launch_window<EnvelopeRed>(pcm, S, 1, 0, 0, stride, first, cols, hop, f, out, out_stride, st);
}
hipError_t launch_level(const float* pcm, int S, int64_t stride, int64_t first, int64_t cols, int hop, int f, void* out, int64_t out_stride,
                        hipStream_t st) {
    return launch_window<LevelRed>(pcm, S, 1, 0, 0, stride, first, cols, hop, f, out, out_stride, st);
}
hipError_t launch_cross(const float* pcm, int pairs, int views, int a, int b, int64_t stride, int64_t first, int64_t cols, int hop, int f,
                        void* out, int64_t out_stride, hipStream_t st) {
    return launch_window<CrossRed>(pcm, pairs, views, a, b, stride, first, cols, hop, f, out, out_stride, st);
}

}  // namespace emspec
