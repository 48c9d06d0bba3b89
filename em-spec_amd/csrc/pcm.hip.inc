// pcm.hip.inc — the PCM front end's decode kernel (DESIGN.md §3.9, §4.10; include/emspec.h: emspec_pcm_decode_device,
// emspec_batch_pcm, emspec_push_samples_pcm): interleaved s16 / s24 / s32 / f32 frames -> the float32 streams every other
// kernel reads.  Included by kernels.hip after pack.hip.inc.
namespace emspec {

// The aligned dword at q, of which only the bytes inside [lo, hi) may be touched: whole when it lies inside, else put
// together from byte loads of the bytes that do (a row's at most 3 leading / trailing bytes), 0 when none does.
// (offsets relative to `base`, a pointer into global memory: q may be negative by up to 3)
__device__ __forceinline__ uint32_t pcm_edge_dword(const uint8_t* __restrict__ base, long long q, long long lo, long long hi) {
    if (q >= lo && q + 4 <= hi) return *reinterpret_cast<const uint32_t*>(base + q);
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (q + b >= lo && q + b < hi) v |= (uint32_t)base[q + b] << (8 * b);
    return v;
}

// A lane decodes FOUR consecutive frames of one source - 4 * CH samples, a whole number of dwords for every sample type -
// for all views, and a wave 256 consecutive frames: the input is read once, as aligned dwords (the lane's bytes are
// contiguous; a 16-bit stereo frame quad is one 16-byte load per lane, consecutive across the wave), and every view gets one
// 16-byte store per lane.  A row that does not start on a dword (s16 at an odd sample, packed s24 anywhere) is read through
// the aligned dwords around the lane's bytes and realigned with v_alignbyte_b32; only a dword that straddles the row's first
// or last byte is put together from byte loads.  No LDS, no scratch.  Arithmetic: DESIGN.md §3.9 - conversion, then
// acc = mix[v][0] * x_0, acc = acc + mix[v][c] * x_c in ascending c, every product and sum rounded to binary32 (the library
// is built with -ffp-contract=off).
// src: row of source i at src + i * src_stride (bytes); out: stream i * views + v at out + (i * views + v) * out_stride.
// vec: out and out_stride allow 16-byte stores.
template <int TYPE, int CH>
__global__ __launch_bounds__(256) void pcm_decode_kernel(const uint8_t* __restrict__ src, long long src_stride, int sources,
                                                         long long frames, PcmMix mix, int views, float* __restrict__ out,
                                                         long long out_stride, int vec) {
    constexpr int BPS = TYPE == kPcmS16 ? 2 : TYPE == kPcmS24 ? 3 : 4;
    constexpr int FB = BPS * CH;   // bytes per frame = dwords per four frames
    const long long t0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= frames) return;
    const int nf = frames - t0 < 4 ? (int)(frames - t0) : 4;
    for (int i = (int)blockIdx.y; i < sources; i += (int)gridDim.y) {
        // byte offsets from src: the row, the lane's four frames, and the aligned dword they start in
        const long long row = (long long)i * src_stride, row_end = row + frames * FB, a = row + t0 * FB;
        const unsigned sh = (unsigned)((reinterpret_cast<uintptr_t>(src) + (uintptr_t)a) & 3);
        const long long p = a - sh;
        uint32_t d[FB + 1];
        if (p >= row && p + 4 * (FB + 1) <= row_end) {   // (every lane but a row's first and last)
            const uint32_t* __restrict__ pd = static_cast<const uint32_t*>(__builtin_assume_aligned(src + p, 4));
#pragma unroll
            for (int k = 0; k <= FB; ++k) d[k] = pd[k];
        } else {
#pragma unroll
            for (int k = 0; k <= FB; ++k) d[k] = pcm_edge_dword(src, p + 4 * k, row, row_end);
        }
        uint32_t w[FB];
#pragma unroll
        for (int k = 0; k < FB; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
        float x[4][CH];
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int j = f * CH + c;
                if (TYPE == kPcmS16) {
                    const int s = (int)(int16_t)(w[j / 2] >> (16 * (j & 1)));
                    x[f][c] = (float)s * 0x1p-15f;
                } else if (TYPE == kPcmS24) {
                    const int k = (3 * j) / 4, o = (3 * j) % 4;
                    const uint32_t u = o <= 1 ? w[k] >> (8 * o) : __builtin_amdgcn_alignbyte(w[k + 1 < FB ? k + 1 : k], w[k], (unsigned)o);
                    const int s = (int)(u << 8) >> 8;
                    x[f][c] = (float)s * 0x1p-23f;
                } else if (TYPE == kPcmS32) {
                    x[f][c] = (float)(int)w[j] * 0x1p-31f;
                } else {
                    x[f][c] = __uint_as_float(w[j]);
                }
            }
        for (int v = 0; v < views; ++v) {
            const float* m = mix.w + v * kPcmMaxChannels;
            float acc[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                acc[f] = m[0] * x[f][0];
#pragma unroll
                for (int c = 1; c < CH; ++c) acc[f] = acc[f] + m[c] * x[f][c];
            }
            float* o = out + ((long long)i * views + v) * out_stride + t0;
            if (vec && nf == 4) {
                *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int f = 0; f < 4; ++f)
                    if (f < nf) o[f] = acc[f];
            }
        }
    }
}

template <int TYPE>
static hipError_t pcm_decode_type(int ch, dim3 grid, hipStream_t st, const uint8_t* src, long long src_stride, int sources,
                                  long long frames, const PcmMix& mix, int views, float* out, long long out_stride, int vec) {
#define EMSPEC_PCM_CASE(C)                                                                                                    \
    case C:                                                                                                                   \
        hipLaunchKernelGGL((pcm_decode_kernel<TYPE, C>), grid, dim3(256), 0, st, src, src_stride, sources, frames, mix, views, \
                           out, out_stride, vec);                                                                             \
        break;
    switch (ch) {
        EMSPEC_PCM_CASE(1) EMSPEC_PCM_CASE(2) EMSPEC_PCM_CASE(3) EMSPEC_PCM_CASE(4)
        EMSPEC_PCM_CASE(5) EMSPEC_PCM_CASE(6) EMSPEC_PCM_CASE(7) EMSPEC_PCM_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef EMSPEC_PCM_CASE
    return hipGetLastError();
}

// (the format has passed pcm_format_error, emspec_pcm.cpp)  The kernel's mix rows are padded to kPcmMaxChannels weights.
hipError_t launch_pcm_decode(const void* src, int sample_type, int channels, int views, const float* w, int sources, int64_t frames,
                             int64_t src_stride_bytes, float* out, int64_t out_stride, hipStream_t st) {
    if (sources <= 0 || frames <= 0) return hipSuccess;
    if (views < 1 || views > kPcmMaxViews || channels < 1 || channels > kPcmMaxChannels) return hipErrorInvalidValue;
    PcmMix mix{};
    for (int v = 0; v < views; ++v)
        for (int c = 0; c < channels; ++c) mix.w[v * kPcmMaxChannels + c] = w[v * channels + c];
    const int64_t quads = (frames + 3) / 4, bx = (quads + 255) / 256;
    if (bx > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)bx, (unsigned)(sources > 65535 ? 65535 : sources));
    const int vec = (reinterpret_cast<uintptr_t>(out) % 16 == 0 && out_stride % 4 == 0) ? 1 : 0;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(src);
    switch (sample_type) {
        case kPcmS16: return pcm_decode_type<kPcmS16>(channels, grid, st, s, src_stride_bytes, sources, frames, mix, views, out, out_stride, vec);
        case kPcmS24: return pcm_decode_type<kPcmS24>(channels, grid, st, s, src_stride_bytes, sources, frames, mix, views, out, out_stride, vec);
        case kPcmS32: return pcm_decode_type<kPcmS32>(channels, grid, st, s, src_stride_bytes, sources, frames, mix, views, out, out_stride, vec);
        case kPcmF32: return pcm_decode_type<kPcmF32>(channels, grid, st, s, src_stride_bytes, sources, frames, mix, views, out, out_stride, vec);
    }
    return hipErrorInvalidValue;
}

}  // namespace emspec
