// wave.hip.inc — the waveform envelope of the samples under each delivered column (DESIGN.md §3.12, §4.13; include/emspec.h:
// emspec_wave_device, emspec_set_wave_out): per stream and window of samples the pair (lo, hi).
//   key(u) = (u & 0x80000000) ? ~u : (u | 0x80000000)      u: the sample's 32 bits; the total order of the floats, -0.0 < +0.0
//   lo = the sample with the smallest key, hi = the one with the largest, each with its own bits; NaN samples are skipped;
//   a window without a sample that is not NaN gives (+inf, -inf)
// Integer minima and maxima of keys only: the pair is a function of the window's bits, whatever the order and the split.
// One HBM-bound pass: every sample of a window is read once, with 16-byte loads between the window's first and last 16-byte
// boundary and per element outside.  Included by kernels.hip after peaks.hip.inc.
namespace emspec {

// The keys of the samples that are not NaN lie in [key(-inf), key(+inf)].  A NaN counts as key(+inf) for the minimum and as
// key(-inf) for the maximum, which are also the values a reduction starts from: it changes nothing, and a window without a
// sample decodes to (+inf, -inf).
constexpr uint32_t kWaveLoNone = 0xff800000u, kWaveHiNone = 0x007fffffu;
constexpr int kWaveBlock = 256;
constexpr int64_t kWavePiece = 65536;   // samples of a long window that one workgroup reduces (256 KB)
constexpr int64_t kWaveSplit = 16384;   // windows longer than this are cut into pieces over workgroups

__device__ __forceinline__ void wave_take(uint32_t u, uint32_t& lo, uint32_t& hi) {
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    const bool nan = (u & 0x7fffffffu) > 0x7f800000u;
    const uint32_t kl = nan ? kWaveLoNone : key, kh = nan ? kWaveHiNone : key;
    lo = kl < lo ? kl : lo;
    hi = kh > hi ? kh : hi;
}
__device__ __forceinline__ void wave_take4(const uint4& v, uint32_t& lo, uint32_t& hi) {
    wave_take(v.x, lo, hi); wave_take(v.y, lo, hi); wave_take(v.z, lo, hi); wave_take(v.w, lo, hi);
}
__device__ __forceinline__ uint32_t wave_bits(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// Lane l of a team of T lanes takes its share of the samples x[a .. b): the elements in front of the first 16-byte boundary
// and behind the last one singly, the quads between them T apart, four loads in flight (a quad past the end: the lane's
// first quad again, which changes nothing).  x is 4-byte aligned only; nothing outside [a, b) is read.
__device__ __forceinline__ void wave_scan(const uint32_t* __restrict__ x, int64_t a, int64_t b, int l, int T, uint32_t& lo, uint32_t& hi) {
    int64_t A = a + (int64_t)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(x + a) >> 2) & 3u)) & 3u);
    if (A > b) A = b;
    const int64_t nq = (b - A) >> 2, B = A + 4 * nq;
    for (int64_t i = a + l; i < A; i += T) wave_take(x[i], lo, hi);
    for (int64_t i = B + l; i < b; i += T) wave_take(x[i], lo, hi);
    const uint4* q = reinterpret_cast<const uint4*>(x + A);
    for (int64_t j = l; j < nq; j += 4 * (int64_t)T) {
        const int64_t j1 = j + T, j2 = j + 2 * (int64_t)T, j3 = j + 3 * (int64_t)T;
        const uint4 v0 = q[j], v1 = q[j1 < nq ? j1 : j], v2 = q[j2 < nq ? j2 : j], v3 = q[j3 < nq ? j3 : j];
        wave_take4(v0, lo, hi); wave_take4(v1, lo, hi); wave_take4(v2, lo, hi); wave_take4(v3, lo, hi);
    }
}

// Windows of at most kWaveSplit samples: a team of T lanes (a power of two, 1 .. 64, the same for the whole launch) per window,
// 256 / T windows per workgroup and step of the grid's stride - down to one thread per window, so that hop = 1 is not a wave
// per sample.  Window w = (stream s, group g) covers x[s stride + first + g f hop ..) up to column min((g + 1) f, cols).
// The team's lanes combine their keys with integer min / max over the xor butterfly; its first lane stores the pair.
__global__ __launch_bounds__(kWaveBlock) void wave_kernel(const uint32_t* __restrict__ x, int64_t stride, int64_t first, int64_t cols,
                                                          int hop, int f, int64_t Cr, int64_t windows, int T, uint2* __restrict__ out,
                                                          int64_t out_stride) {
    const int l = threadIdx.x & (T - 1);
    const int64_t per = kWaveBlock / T;
    for (int64_t w = (int64_t)blockIdx.x * per + threadIdx.x / T; w < windows; w += (int64_t)gridDim.x * per) {
        const int64_t s = w / Cr, g = w % Cr;
        const int64_t c0 = g * f, c1 = c0 + f < cols ? c0 + f : cols;
        const int64_t base = s * stride + first;
        uint32_t lo = kWaveLoNone, hi = kWaveHiNone;
        wave_scan(x, base + c0 * hop, base + c1 * hop, l, T, lo, hi);
        for (int m = T >> 1; m >= 1; m >>= 1) {
            const uint32_t ol = (uint32_t)__shfl_xor((int)lo, m, 64), oh = (uint32_t)__shfl_xor((int)hi, m, 64);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        if (l == 0) out[s * out_stride + g] = make_uint2(wave_bits(lo), wave_bits(hi));
    }
}

// Longer windows: a workgroup per piece of kWavePiece samples, `ppw` pieces per window (those past a short last window's end
// do nothing).  The pieces of a window meet in its output pair, which holds KEYS during this launch: wave_keys_kernel writes
// the start values in front of it, every workgroup adds its piece with one integer atomic minimum and one maximum, and
// wave_keys_kernel turns the keys into the samples' bits behind it.  (Integer min / max are associative and commutative: the
// pair does not depend on the order of arrival.)
__global__ __launch_bounds__(kWaveBlock) void wave_split_kernel(const uint32_t* __restrict__ x, int64_t stride, int64_t first, int64_t cols,
                                                                int hop, int f, int64_t Cr, int64_t ppw, int64_t items,
                                                                uint32_t* __restrict__ out, int64_t out_stride) {
    __shared__ uint32_t part[2][kWaveBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {   // (uniform in the workgroup, so its barriers are)
        const int64_t p = it % ppw, w = it / ppw, s = w / Cr, g = w % Cr;
        const int64_t c0 = g * f, c1 = c0 + f < cols ? c0 + f : cols;
        const int64_t base = s * stride + first, a = base + c0 * hop + p * kWavePiece, end = base + c1 * hop;
        if (a >= end) continue;
        const int64_t b = a + kWavePiece < end ? a + kWavePiece : end;
        uint32_t lo = kWaveLoNone, hi = kWaveHiNone;
        wave_scan(x, a, b, threadIdx.x, kWaveBlock, lo, hi);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t ol = (uint32_t)__shfl_xor((int)lo, m, 64), oh = (uint32_t)__shfl_xor((int)hi, m, 64);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        if (lane == 0) { part[0][wv] = lo; part[1][wv] = hi; }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 1; k < kWaveBlock / 64; ++k) {
                lo = part[0][k] < lo ? part[0][k] : lo;
                hi = part[1][k] > hi ? part[1][k] : hi;
            }
            uint32_t* o = out + 2 * (s * out_stride + g);
            atomicMin(o, lo);
            atomicMax(o + 1, hi);
        }
        __syncthreads();   // the next item overwrites part[]
    }
}
// decode == 0: every pair of the launch := the start keys;  decode != 0: keys -> the samples' bits
__global__ __launch_bounds__(kWaveBlock) void wave_keys_kernel(uint2* __restrict__ out, int64_t out_stride, int64_t Cr, int64_t windows, int decode) {
    for (int64_t w = (int64_t)blockIdx.x * kWaveBlock + threadIdx.x; w < windows; w += (int64_t)gridDim.x * kWaveBlock) {
        uint2* o = out + (w / Cr) * out_stride + w % Cr;
        if (decode) { const uint2 k = *o; *o = make_uint2(wave_bits(k.x), wave_bits(k.y)); }
        else *o = make_uint2(kWaveLoNone, kWaveHiNone);
    }
}

// pcm: S streams, `stride` samples apart, 4-byte aligned; stream s's windows start `first` samples into it and cover `cols`
// columns of `hop` samples in groups of f: ceil(cols / f) pairs per stream into out (8-byte aligned), out_stride pairs apart.
// `first` makes a unit of the host pipeline that is a run of columns of a longer stream servable (emspec_host.cpp).  The
// caller guarantees first + cols hop <= the samples of a stream.  All offsets are 64-bit; the grids stride.
hipError_t launch_wave(const float* pcm, int S, int64_t stride, int64_t first, int64_t cols, int hop, int f, void* out, int64_t out_stride,
                       hipStream_t st) {
    if (S <= 0 || cols <= 0) return hipSuccess;
    if (!pcm || !out || hop < 1 || f < 1 || first < 0 || reinterpret_cast<uintptr_t>(pcm) % 4 || reinterpret_cast<uintptr_t>(out) % 8)
        return hipErrorInvalidValue;
    const uint32_t* x = reinterpret_cast<const uint32_t*>(pcm);
    const int64_t Cr = (cols + f - 1) / f, windows = (int64_t)S * Cr, longest = (int64_t)(f < cols ? f : cols) * hop;
    const int64_t cap = 8 * 256 * 8;   // workgroups: a few per CU, then stride
    if (longest <= kWaveSplit) {
        int T = 1;   // about 16 samples or more per lane
        while (T < 64 && (int64_t)T * 32 <= longest) T *= 2;
        const int64_t blocks = (windows + kWaveBlock / T - 1) / (kWaveBlock / T);
        hipLaunchKernelGGL(wave_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kWaveBlock), 0, st, x, stride, first, cols, hop, f,
                           Cr, windows, T, reinterpret_cast<uint2*>(out), out_stride);
        return hipGetLastError();
    }
    const int64_t ppw = (longest + kWavePiece - 1) / kWavePiece, items = windows * ppw, kb = (windows + kWaveBlock - 1) / kWaveBlock;
    const dim3 kgrid((unsigned)(kb < cap ? kb : cap));
    hipLaunchKernelGGL(wave_keys_kernel, kgrid, dim3(kWaveBlock), 0, st, reinterpret_cast<uint2*>(out), out_stride, Cr, windows, 0);
    hipLaunchKernelGGL(wave_split_kernel, dim3((unsigned)(items < cap ? items : cap)), dim3(kWaveBlock), 0, st, x, stride, first, cols, hop, f,
                       Cr, ppw, items, reinterpret_cast<uint32_t*>(out), out_stride);
    hipLaunchKernelGGL(wave_keys_kernel, kgrid, dim3(kWaveBlock), 0, st, reinterpret_cast<uint2*>(out), out_stride, Cr, windows, 1);
    return hipGetLastError();
}

}  // namespace emspec
