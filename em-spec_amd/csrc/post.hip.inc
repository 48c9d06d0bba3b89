// post.hip.inc — display post-process over finished dB columns (SURVEY.md §8(f) item 2):
// "Adaptive brightness" (AGC, README.md:14) and "Temporal smoothing" (README.md:50).
// The reference documents neither law; this is the [BUILD-DEFINED] one (DESIGN.md §3.6):
//   m_c   = max_r dB[c][r]                                   column peak
//   p_c   = p_{c-1} + k (m_c - p_{c-1}),  k = 0.25 rising, 0.02 falling,  p_{-1} = m_0
//   g_c   = clamp(agc * (db_top - p_c), -40, 40)             gain in dB
//   y_c   = s * y_{c-1} + (1-s) * (dB_c + g_c),   y_{-1} = dB_0 + g_0     per row
// Outputs: y as dB, and palette index / RGBA from y.  Included by kernels.hip.
namespace emspec {

constexpr float AGC_UP = 0.25f, AGC_DOWN = 0.02f, AGC_MAX_GAIN = 40.0f;
constexpr int POST_CHUNK = 1024, POST_WARM = 512;   // s^512 < 1e-11 for s <= 0.95: chunks are exact to float

// column peaks: one wave per column (R floats, 16-byte loads), grid-stride over S*C columns
__global__ __launch_bounds__(256) void column_max_kernel(const float* __restrict__ db, int64_t ncols, int R,
                                                         float* __restrict__ peak) {
    const int lane = threadIdx.x & 63;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < ncols; c += (int64_t)gridDim.x * 4) {
        const float4* p = reinterpret_cast<const float4*>(db + (size_t)c * R);
        float m = -3.0e38f;
        for (int q = lane; q < R / 4; q += 64) {
            const float4 v = p[q];
            m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) peak[c] = m;
    }
}

// AGC recurrence: one thread per stream, sequential in time (C steps of a few flops)
__global__ void agc_scan_kernel(const float* __restrict__ peak, int S, int64_t C, float agc, float db_top,
                                float* __restrict__ gain) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const float* m = peak + (size_t)s * C;
    float* g = gain + (size_t)s * C;
    float p = m[0];
    for (int64_t c = 0; c < C; ++c) {
        const float d = m[c] - p;
        p = p + (d > 0.0f ? AGC_UP : AGC_DOWN) * d;
        float gg = agc * (db_top - p);
        gg = gg < -AGC_MAX_GAIN ? -AGC_MAX_GAIN : (gg > AGC_MAX_GAIN ? AGC_MAX_GAIN : gg);
        g[c] = gg;
    }
}

// apply gain + IIR along time: thread = (stream, chunk of columns, quad of rows); a chunk warms its
// state up over the POST_WARM columns before it (exact to float precision), 4 loads kept in flight
__global__ __launch_bounds__(256) void smooth_apply_kernel(float* __restrict__ db, const float* __restrict__ gain,
                                                           int S, int64_t C, int R, float sm, DbMap dm,
                                                           const uint32_t* __restrict__ lut, uint32_t* __restrict__ rgba,
                                                           uint8_t* __restrict__ index, float* __restrict__ out) {
    const int qpc = R / 4;
    const int64_t nchunk = (C + POST_CHUNK - 1) / POST_CHUNK;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(gid % qpc);
    const int64_t rest = gid / qpc;
    const int64_t ch = rest % nchunk;
    const int s = (int)(rest / nchunk);
    if (s >= S) return;
    const int64_t c_out = ch * POST_CHUNK;
    const int64_t c_end = (c_out + POST_CHUNK < C) ? c_out + POST_CHUNK : C;
    const int64_t c_beg = (sm > 0.0f && c_out > POST_WARM) ? c_out - POST_WARM : (sm > 0.0f ? 0 : c_out);
    const float* g = gain ? gain + (size_t)s * C : nullptr;
    const size_t base = (size_t)s * C * R + (size_t)q * 4;
    auto load = [&](int64_t c) {
        float4 v = *reinterpret_cast<const float4*>(db + base + (size_t)c * R);
        const float gg = g ? g[c] : 0.0f;
        return make_float4(v.x + gg, v.y + gg, v.z + gg, v.w + gg);
    };
    float4 y = load(c_beg);
    const float a = 1.0f - sm;
    for (int64_t c = c_beg; c < c_end; c += 4) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = (c + u < c_end) ? load(c + u) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t cc = c + u;
            if (cc >= c_end) break;
            if (cc > c_beg || c_beg > 0) {   // the very first column of a stream passes through (y_{-1} = x_0)
                y.x = sm * y.x + a * x[u].x; y.y = sm * y.y + a * x[u].y;
                y.z = sm * y.z + a * x[u].z; y.w = sm * y.w + a * x[u].w;
            } else {
                y = x[u];
            }
            if (cc >= c_out) {
                const size_t o = base + (size_t)cc * R;
                *reinterpret_cast<float4*>(out + o) = y;
                if (rgba || index) {
                    const int i0 = cell_index(dm, y.x), i1 = cell_index(dm, y.y), i2 = cell_index(dm, y.z), i3 = cell_index(dm, y.w);
                    store_colour4(lut, i0, i1, i2, i3, o, rgba, index);
                }
            }
        }
    }
}

// in: db [S][C][R] (raw columns); out_db may alias db only when sm == 0 (chunks re-read their warm-up
// columns); peak/gain: workspaces of S*C floats (gain unused when agc == 0)
hipError_t launch_postprocess(const float* db, float* out_db, uint8_t* rgba, uint8_t* index, int S, int64_t C, int R,
                              float sm, float agc, float db_top, const DbMap& dm, const uint8_t* lut, float* peak,
                              float* gain, hipStream_t st) {
    if (S <= 0 || C <= 0) return hipSuccess;
    const float* gptr = nullptr;
    if (agc > 0.0f) {
        const int64_t ncols = (int64_t)S * C;
        int64_t blocks = (ncols + 3) / 4;
        blocks = blocks > 8192 ? 8192 : blocks;
        hipLaunchKernelGGL(column_max_kernel, dim3((unsigned)blocks), dim3(256), 0, st, db, ncols, R, peak);
        hipLaunchKernelGGL(agc_scan_kernel, dim3((S + 63) / 64), dim3(64), 0, st, peak, S, C, agc, db_top, gain);
        gptr = gain;
    }
    const int64_t nchunk = (C + POST_CHUNK - 1) / POST_CHUNK;
    const int64_t threads = (int64_t)S * nchunk * (R / 4);
    hipLaunchKernelGGL(smooth_apply_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st,
                       const_cast<float*>(db), gptr, S, C, R, sm, dm, reinterpret_cast<const uint32_t*>(lut),
                       reinterpret_cast<uint32_t*>(rgba), index, out_db);
    return hipGetLastError();
}

// streaming form: one finished column (raw dB in[R]) -> post-processed (out_db and/or rgba; out_db may be `in`), state
// carried in st[0] = AGC level p, st[1] = 1 once initialised, yprev[R] = previous smoothed column.  256 threads; red: 4 floats
// of LDS.  Ends on a barrier: callers run it column after column.
__device__ __forceinline__ void post_column_body(const float* in, float* out_db, uint32_t* rgba, int R, float sm, float agc,
                                                 float db_top, const DbMap& dm, const uint32_t* __restrict__ lut,
                                                 float* __restrict__ state, float* __restrict__ yprev, float* red) {
    float m = -3.0e38f;
    for (int r = threadIdx.x; r < R; r += 256) m = fmaxf(m, in[r]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const bool first = state[1] == 0.0f;
    float p = first ? m : state[0];
    const float d = m - p;
    p = p + (d > 0.0f ? AGC_UP : AGC_DOWN) * d;
    float g = agc * (db_top - p);
    g = g < -AGC_MAX_GAIN ? -AGC_MAX_GAIN : (g > AGC_MAX_GAIN ? AGC_MAX_GAIN : g);
    if (agc <= 0.0f) g = 0.0f;
    __syncthreads();
    for (int r = threadIdx.x; r < R; r += 256) {
        const float x = in[r] + g;
        const float y = first ? x : sm * yprev[r] + (1.0f - sm) * x;
        yprev[r] = y;
        if (out_db) out_db[r] = y;
        if (rgba) rgba[r] = lut[cell_index(dm, y)];
    }
    if (threadIdx.x == 0) { state[0] = p; state[1] = 1.0f; }
    __syncthreads();
}

}  // namespace emspec
