// level.hip.inc — the level meters of the samples under each delivered column (DESIGN.md §3.17, §4.19; include/emspec.h:
// emspec_level_device, emspec_cross_device, emspec_set_level_out, emspec_set_cross_out): per stream and window of samples the
// record (sum of k^2 in two limbs, peak |k|, count of NaN and saturated samples), per pair of streams and window the sum of
// k_A k_B in two limbs; k = the sample in units of 2^-24 (emspec_level_plan.h: level_magnitude, level_take, cross_take).
// Integer sums and maxima only: a record is a function of the window's bits, whatever the order and the split.
// The walk is the envelope's (wave.hip.inc): every sample of a window is read once, with 16-byte loads between the window's
// first and last 16-byte boundary and per element outside.  Included by kernels.hip after wave.hip.inc.
#include "emspec_level_plan.h"

namespace emspec {

constexpr int kLevelBlock = 256;
constexpr int64_t kLevelPiece = 65536;   // samples of a long window that one workgroup reduces
constexpr int64_t kLevelSplit = 16384;   // windows longer than this are cut into pieces over workgroups

template <bool CROSS> using LevelRec = std::conditional_t<CROSS, emspec_cross, emspec_level>;
// The samples of a window: stream A's from xa[0] on, and for a cross record stream B's from xb[0] on (the same indices).
struct LevelSrc { const uint32_t* xa; const uint32_t* xb; };
// Four of B's samples where A's lie on a 16-byte boundary: B is 4-byte aligned only
struct __attribute__((aligned(4))) LevelQuadB { uint32_t x, y, z, w; };
template <bool CROSS> struct LevelQuad;
template <> struct LevelQuad<false> { uint4 a; };
template <> struct LevelQuad<true> { uint4 a; LevelQuadB b; };

template <bool CROSS> __device__ __forceinline__ void level_take1(const LevelSrc& src, int64_t i, LevelRec<CROSS>& r) {
    if constexpr (CROSS) cross_take(r, src.xa[i], src.xb[i]);
    else level_take(r, src.xa[i]);
}
template <bool CROSS> __device__ __forceinline__ LevelQuad<CROSS> level_load4(const LevelSrc& src, int64_t i) {   // xa + i: 16-byte aligned
    LevelQuad<CROSS> q;
    q.a = *reinterpret_cast<const uint4*>(src.xa + i);
    if constexpr (CROSS) q.b = *reinterpret_cast<const LevelQuadB*>(src.xb + i);
    return q;
}
template <bool CROSS> __device__ __forceinline__ void level_take4(const LevelQuad<CROSS>& q, LevelRec<CROSS>& r) {
    if constexpr (CROSS) { cross_take(r, q.a.x, q.b.x); cross_take(r, q.a.y, q.b.y); cross_take(r, q.a.z, q.b.z); cross_take(r, q.a.w, q.b.w); }
    else { level_take(r, q.a.x); level_take(r, q.a.y); level_take(r, q.a.z); level_take(r, q.a.w); }
}

// Lane l of a team of T lanes takes its share of the samples [a, b) of src: the elements in front of A's first 16-byte boundary
// and behind its last one singly, the quads between them T apart, four loads in flight.  Unlike a minimum, a sum cannot take a
// quad twice: a quad past the end is not loaded.  Nothing outside [a, b) is read.
template <bool CROSS>
__device__ __forceinline__ void level_scan(const LevelSrc& src, int64_t a, int64_t b, int l, int T, LevelRec<CROSS>& r) {
    int64_t A = a + (int64_t)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(src.xa + a) >> 2) & 3u)) & 3u);
    if (A > b) A = b;
    const int64_t nq = (b - A) >> 2, B = A + 4 * nq;
    for (int64_t i = a + l; i < A; i += T) level_take1<CROSS>(src, i, r);
    for (int64_t i = B + l; i < b; i += T) level_take1<CROSS>(src, i, r);
    int64_t j = l;
    for (; j + 3 * (int64_t)T < nq; j += 4 * (int64_t)T) {
        const LevelQuad<CROSS> v0 = level_load4<CROSS>(src, A + 4 * j), v1 = level_load4<CROSS>(src, A + 4 * (j + T)),
                               v2 = level_load4<CROSS>(src, A + 4 * (j + 2 * (int64_t)T)), v3 = level_load4<CROSS>(src, A + 4 * (j + 3 * (int64_t)T));
        level_take4<CROSS>(v0, r); level_take4<CROSS>(v1, r); level_take4<CROSS>(v2, r); level_take4<CROSS>(v3, r);
    }
    for (; j < nq; j += T) level_take4<CROSS>(level_load4<CROSS>(src, A + 4 * j), r);
}

__device__ __forceinline__ uint64_t level_shfl(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}
// the record of the lane m away, combined into this lane's (the xor butterfly's step)
__device__ __forceinline__ void level_mix(emspec_level& r, int m) {
    emspec_level o;
    o.sq_lo = level_shfl(r.sq_lo, m); o.sq_hi = level_shfl(r.sq_hi, m);
    o.peak = (uint32_t)__shfl_xor((int)r.peak, m, 64); o.odd = (uint32_t)__shfl_xor((int)r.odd, m, 64);
    level_combine(r, o);
}
__device__ __forceinline__ void level_mix(emspec_cross& r, int m) {
    emspec_cross o;
    o.lo = level_shfl(r.lo, m); o.hi = (int64_t)level_shfl((uint64_t)r.hi, m);
    cross_combine(r, o);
}
// a piece's record into the window's, which level_zero_kernel cleared: 64-bit integer atomics (the high limb of a cross record
// adds as its two's complement)
__device__ __forceinline__ void level_merge(emspec_level* o, const emspec_level& r) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sq_lo), (unsigned long long)r.sq_lo);
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->sq_hi), (unsigned long long)r.sq_hi);
    atomicMax(&o->peak, r.peak);
    atomicAdd(&o->odd, r.odd);
}
__device__ __forceinline__ void level_merge(emspec_cross* o, const emspec_cross& r) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->lo), (unsigned long long)r.lo);
    atomicAdd(reinterpret_cast<unsigned long long*>(&o->hi), (unsigned long long)r.hi);
}

// The geometry of a launch.  Window w = (s, g): group g of f columns of hop samples, from `first` samples into the stream on.
// A level record's stream is s; a cross record's are s views + a and s views + b.
struct LevelGeom { const uint32_t* x; int64_t stride, first, cols; int hop, f; int64_t Cr; int views, a, b; };
template <bool CROSS> __device__ __forceinline__ LevelSrc level_src(const LevelGeom& G, int64_t s) {
    if constexpr (CROSS) return LevelSrc{G.x + (s * G.views + G.a) * G.stride + G.first, G.x + (s * G.views + G.b) * G.stride + G.first};
    else return LevelSrc{G.x + s * G.stride + G.first, nullptr};
}

// Windows of at most kLevelSplit samples: a team of T lanes (a power of two, 1 .. 64, the same for the whole launch) per window,
// 256 / T windows per workgroup and step of the grid's stride.  The team's lanes combine their records over the xor butterfly;
// its first lane stores the record.
template <bool CROSS>
__global__ __launch_bounds__(kLevelBlock) void level_kernel(LevelGeom G, int64_t windows, int T, LevelRec<CROSS>* __restrict__ out, int64_t out_stride) {
    const int l = threadIdx.x & (T - 1);
    const int64_t per = kLevelBlock / T;
    for (int64_t w = (int64_t)blockIdx.x * per + threadIdx.x / T; w < windows; w += (int64_t)gridDim.x * per) {
        const int64_t s = w / G.Cr, g = w % G.Cr;
        const int64_t c0 = g * G.f, c1 = c0 + G.f < G.cols ? c0 + G.f : G.cols;
        LevelRec<CROSS> r = {};
        level_scan<CROSS>(level_src<CROSS>(G, s), c0 * G.hop, c1 * G.hop, l, T, r);
        for (int m = T >> 1; m >= 1; m >>= 1) level_mix(r, m);
        if (l == 0) out[s * out_stride + g] = r;
    }
}

// Longer windows: a workgroup per piece of kLevelPiece samples, `ppw` pieces per window (those past a short last window's end
// do nothing).  The pieces of a window meet in its record, which level_zero_kernel clears in front of this launch: every
// workgroup adds its piece with integer atomics.  (Integer sums and maxima are associative and commutative: the record does not
// depend on the order of arrival, and needs no pass behind.)
template <bool CROSS>
__global__ __launch_bounds__(kLevelBlock) void level_split_kernel(LevelGeom G, int64_t ppw, int64_t items, LevelRec<CROSS>* __restrict__ out, int64_t out_stride) {
    __shared__ LevelRec<CROSS> part[kLevelBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {   // (uniform in the workgroup, so its barriers are)
        const int64_t p = it % ppw, w = it / ppw, s = w / G.Cr, g = w % G.Cr;
        const int64_t c0 = g * G.f, c1 = c0 + G.f < G.cols ? c0 + G.f : G.cols;
        const int64_t a = c0 * G.hop + p * kLevelPiece, end = c1 * G.hop;
        if (a >= end) continue;
        const int64_t b = a + kLevelPiece < end ? a + kLevelPiece : end;
        LevelRec<CROSS> r = {};
        level_scan<CROSS>(level_src<CROSS>(G, s), a, b, threadIdx.x, kLevelBlock, r);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) level_mix(r, m);
        if (lane == 0) part[wv] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 1; k < kLevelBlock / 64; ++k) {
                if constexpr (CROSS) cross_combine(r, part[k]);
                else level_combine(r, part[k]);
            }
            level_merge(out + (s * out_stride + g), r);
        }
        __syncthreads();   // the next item overwrites part[]
    }
}
// every record of the launch := that of no sample (all zero), in 8-byte words
__global__ __launch_bounds__(kLevelBlock) void level_zero_kernel(uint64_t* __restrict__ out, int64_t out_stride, int64_t Cr, int64_t windows, int words) {
    for (int64_t i = (int64_t)blockIdx.x * kLevelBlock + threadIdx.x; i < windows * words; i += (int64_t)gridDim.x * kLevelBlock) {
        const int64_t w = i / words;
        out[((w / Cr) * out_stride + w % Cr) * words + i % words] = 0;
    }
}

template <bool CROSS>
static hipError_t launch_level_any(const LevelGeom& G, int S, void* out, int64_t out_stride, hipStream_t st) {
    using Rec = LevelRec<CROSS>;
    const int64_t windows = (int64_t)S * G.Cr, longest = (int64_t)(G.f < G.cols ? G.f : G.cols) * G.hop;
    const int64_t cap = 8 * 256 * 8;   // workgroups: a few per CU, then stride
    if (longest <= kLevelSplit) {
        int T = 1;   // about 16 samples or more per lane
        while (T < 64 && (int64_t)T * 32 <= longest) T *= 2;
        const int64_t blocks = (windows + kLevelBlock / T - 1) / (kLevelBlock / T);
        hipLaunchKernelGGL(level_kernel<CROSS>, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kLevelBlock), 0, st, G, windows, T,
                           reinterpret_cast<Rec*>(out), out_stride);
        return hipGetLastError();
    }
    const int words = (int)(sizeof(Rec) / 8);
    const int64_t ppw = (longest + kLevelPiece - 1) / kLevelPiece, items = windows * ppw, kb = (windows * words + kLevelBlock - 1) / kLevelBlock;
    hipLaunchKernelGGL(level_zero_kernel, dim3((unsigned)(kb < cap ? kb : cap)), dim3(kLevelBlock), 0, st, reinterpret_cast<uint64_t*>(out),
                       out_stride, G.Cr, windows, words);
    hipLaunchKernelGGL(level_split_kernel<CROSS>, dim3((unsigned)(items < cap ? items : cap)), dim3(kLevelBlock), 0, st, G, ppw, items,
                       reinterpret_cast<Rec*>(out), out_stride);
    return hipGetLastError();
}

// pcm: S streams, `stride` samples apart, 4-byte aligned; stream s's windows start `first` samples into it and cover `cols`
// columns of `hop` samples in groups of f: ceil(cols / f) records per stream into out (8-byte aligned), out_stride records apart.
// The caller guarantees first + cols hop <= the samples of a stream, and f hop <= 2^30.  All offsets are 64-bit; the grids stride.
hipError_t launch_level(const float* pcm, int S, int64_t stride, int64_t first, int64_t cols, int hop, int f, void* out, int64_t out_stride,
                        hipStream_t st) {
    if (S <= 0 || cols <= 0) return hipSuccess;
    if (!pcm || !out || hop < 1 || f < 1 || first < 0 || reinterpret_cast<uintptr_t>(pcm) % 4 || reinterpret_cast<uintptr_t>(out) % 8)
        return hipErrorInvalidValue;
    const LevelGeom G{reinterpret_cast<const uint32_t*>(pcm), stride, first, cols, hop, f, (cols + f - 1) / f, 1, 0, 0};
    return launch_level_any<false>(G, S, out, out_stride, st);
}
// ... and the cross records of `pairs` pairs: pair p's streams are p views + a and p views + b of pcm's pairs * views streams
hipError_t launch_cross(const float* pcm, int pairs, int views, int a, int b, int64_t stride, int64_t first, int64_t cols, int hop, int f,
                        void* out, int64_t out_stride, hipStream_t st) {
    if (pairs <= 0 || cols <= 0) return hipSuccess;
    if (!pcm || !out || hop < 1 || f < 1 || first < 0 || views < 1 || a < 0 || a >= views || b < 0 || b >= views ||
        reinterpret_cast<uintptr_t>(pcm) % 4 || reinterpret_cast<uintptr_t>(out) % 8)
        return hipErrorInvalidValue;
    const LevelGeom G{reinterpret_cast<const uint32_t*>(pcm), stride, first, cols, hop, f, (cols + f - 1) / f, views, a, b};
    return launch_level_any<true>(G, pairs, out, out_stride, st);
}

}  // namespace emspec
