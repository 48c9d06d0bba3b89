// reduce.hip.inc — the time reduction of finished columns (DESIGN.md §3.10, §4.11; include/emspec.h: emspec_set_time_reduce):
// groups of `f` consecutive columns of a stream collapse into one by maximum (peak hold), the last group may be short.
//   db   [s][g][r] = m,  m = in[s][g f][r];  then for c = g f + 1 .. in order:  if (in[s][c][r] > m) m = in[s][c][r]
//   index[s][g][r] = max over the group of in_index[s][c][r]   (unsigned bytes)
//   rgba [s][g][r] = LUT[index[s][g][r]]
// One HBM-bound pass: every full-rate cell is read once (1 byte when no dB is asked for, 5 with dB), the reduced cells are
// written once.  Included by kernels.hip after pack.hip.inc.
namespace emspec {

// per-byte unsigned maximum of two packed words
__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const uint32_t x = (a >> k) & 255u, y = (b >> k) & 255u;
        r |= (x > y ? x : y) << k;
    }
    return r;
}
__device__ __forceinline__ void hold(float& m, float x) { if (x > m) m = x; }   // (as the definition: a NaN holds only in front)

// Thread = (stream, reduced column g, run of U rows), rows fastest: the threads of a wave read consecutive 16-byte pieces of one
// full-rate column (U = 16: one uint4 of indices, four float4 of dB; U = 4, for rows % 16 != 0: one word of indices, one float4),
// column after column of the group with four columns' loads in flight.  in_stride / out_stride: cells between two streams of
// the input / output (a unit of the host pipeline reduces a run of columns out of a longer staged stream).  All offsets 64-bit.
template <int U, bool DB, bool IDX>
__global__ __launch_bounds__(256) void reduce_columns_kernel(const float* __restrict__ db_in, const uint8_t* __restrict__ idx_in,
                                                             int S, int64_t C, int64_t Cr, int R, int f, size_t in_stride,
                                                             size_t out_stride, const uint32_t* __restrict__ lut,
                                                             float* __restrict__ db_out, uint8_t* __restrict__ idx_out,
                                                             uint32_t* __restrict__ rgba_out) {
    constexpr int W = U / 4;   // words of indices = float4s of dB per thread and column
    const int upc = R / U;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int u = (int)(gid % upc);
    const int64_t rest = gid / upc;
    const int64_t g = rest % Cr;
    const int64_t s = rest / Cr;
    if (s >= S) return;
    const int64_t c0 = g * f, c1 = (c0 + f < C) ? c0 + f : C;
    const size_t in0 = (size_t)s * in_stride + (size_t)c0 * R + (size_t)u * U;
    const size_t out0 = (size_t)s * out_stride + (size_t)g * R + (size_t)u * U;
    float4 m[W];
    uint32_t x[W];
    auto load_db = [&](int64_t c, float4* v) {
        const float4* p = reinterpret_cast<const float4*>(db_in + in0 + (size_t)(c - c0) * R);
#pragma unroll
        for (int w = 0; w < W; ++w) v[w] = p[w];
    };
    auto load_idx = [&](int64_t c, uint32_t* v) {
        if constexpr (W == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(idx_in + in0 + (size_t)(c - c0) * R);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = *reinterpret_cast<const uint32_t*>(idx_in + in0 + (size_t)(c - c0) * R);
        }
    };
    if constexpr (DB) load_db(c0, m);
    if constexpr (IDX) load_idx(c0, x);
    for (int64_t c = c0 + 1; c < c1; c += 4) {
        float4 v[4][W];
        uint32_t y[4][W];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t cc = c + k < c1 ? c + k : c1 - 1;   // (past the end: the group's last column again, which changes nothing)
            if constexpr (DB) load_db(cc, v[k]);
            if constexpr (IDX) load_idx(cc, y[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if constexpr (DB) { hold(m[w].x, v[k][w].x); hold(m[w].y, v[k][w].y); hold(m[w].z, v[k][w].z); hold(m[w].w, v[k][w].w); }
                if constexpr (IDX) x[w] = max_u8x4(x[w], y[k][w]);
            }
    }
    if constexpr (DB) {
        float4* p = reinterpret_cast<float4*>(db_out + out0);
#pragma unroll
        for (int w = 0; w < W; ++w) p[w] = m[w];
    }
    if constexpr (IDX) {
        if (idx_out) {
            if constexpr (W == 4) *reinterpret_cast<uint4*>(idx_out + out0) = make_uint4(x[0], x[1], x[2], x[3]);
            else *reinterpret_cast<uint32_t*>(idx_out + out0) = x[0];
        }
        if (rgba_out) {
            uint4* p = reinterpret_cast<uint4*>(rgba_out + out0);
#pragma unroll
            for (int w = 0; w < W; ++w)
                p[w] = make_uint4(lut[x[w] & 255u], lut[(x[w] >> 8) & 255u], lut[(x[w] >> 16) & 255u], lut[x[w] >> 24]);
        }
    }
}

// db_in / idx_in: [S] streams of C full-rate columns of R cells, in_stride cells apart (either may be null: not reduced);
// outputs: [S] streams of ceil(C / f) columns, out_stride cells apart (rgba + [4]); db_out goes with db_in, idx_out and / or
// rgba_out with idx_in.  R % 4 == 0; every pointer and stride keeps a 4-row piece aligned (16 bytes of dB, 4 of indices) - the
// 16-row form is taken when rows, strides and pointers allow 16-byte index loads.
hipError_t launch_reduce_columns(const float* db_in, const uint8_t* idx_in, int S, int64_t C, int R, int f, size_t in_stride,
                                 size_t out_stride, const uint8_t* lut, float* db_out, uint8_t* idx_out, uint8_t* rgba_out,
                                 hipStream_t st) {
    if (S <= 0 || C <= 0) return hipSuccess;
    const bool want_db = db_out != nullptr, want_idx = idx_out || rgba_out;
    if (R % 4 || f < 1 || (want_db && !db_in) || (want_idx && !idx_in)) return hipErrorInvalidValue;
    if (!want_db && !want_idx) return hipSuccess;
    const int64_t Cr = (C + f - 1) / f;
    const bool wide = R % 16 == 0 && in_stride % 16 == 0 && out_stride % 16 == 0 &&
                      (reinterpret_cast<uintptr_t>(idx_in) | reinterpret_cast<uintptr_t>(idx_out)) % 16 == 0;
    const int U = wide ? 16 : 4;
    const int64_t threads = (int64_t)S * Cr * (R / U), blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const uint32_t* l = reinterpret_cast<const uint32_t*>(lut);
    uint32_t* rg = reinterpret_cast<uint32_t*>(rgba_out);
    const dim3 grid((unsigned)blocks), block(256);
#define EMSPEC_REDUCE(UU)                                                                                                       \
    do {                                                                                                                        \
        if (want_db && want_idx)                                                                                                \
            hipLaunchKernelGGL((reduce_columns_kernel<UU, true, true>), grid, block, 0, st, db_in, idx_in, S, C, Cr, R, f,      \
                               in_stride, out_stride, l, db_out, idx_out, rg);                                                  \
        else if (want_db)                                                                                                       \
            hipLaunchKernelGGL((reduce_columns_kernel<UU, true, false>), grid, block, 0, st, db_in, idx_in, S, C, Cr, R, f,     \
                               in_stride, out_stride, l, db_out, idx_out, rg);                                                  \
        else                                                                                                                    \
            hipLaunchKernelGGL((reduce_columns_kernel<UU, false, true>), grid, block, 0, st, db_in, idx_in, S, C, Cr, R, f,     \
                               in_stride, out_stride, l, db_out, idx_out, rg);                                                  \
    } while (0)
    if (wide) EMSPEC_REDUCE(16); else EMSPEC_REDUCE(4);
#undef EMSPEC_REDUCE
    return hipGetLastError();
}

}  // namespace emspec
