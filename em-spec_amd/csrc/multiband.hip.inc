// multiband.hip.inc — the composition stage of the multi-band batch (DESIGN.md §3.13, §4.14; emspec_multiband.cpp): up to four
// bands' raw dB, each of its own FFT size, stitched on the longest FFT's column grid.  Included by kernels.hip after post.hip.inc.
namespace emspec {

// One wave per (stream, column), grid-stride over S * C of them.  Band k's plane is [S][C + 2 shift[k]][rows_k] raw dB; column c takes
// band k's column c + shift[k] for the rows [4 q0[k], 4 q0[k + 1]).  A lane moves a quad of rows (16-byte loads and stores, the wave
// covers 256 consecutive rows per step; every seam is a multiple of 4, so a quad never straddles one).  The descriptor comes by
// value - no runtime-indexed copy of it, no scratch.  What belongs to the column is the wave's own and is worked out on the scalar
// unit: band 0's source column (band 0 starts at row 0 with shift 0) and, for the other bands, how many quads their source column -
// moved back by the band's first row - lies from it (the planes are one allocation, less than 2^31 quads long: the launcher checks).
// A lane then picks its band's distance with three compares and selects on 32-bit values, unrolled over the slots.
// Outputs [S][C][R] (rgba + [4]), any of them null: dB as read, the palette index by cell_index - the function every finalize
// stage uses, so the bytes are those of the single-resolution batches - and RGBA = LUT[index].
// (amdgpu_waves_per_eu: the scalar work would otherwise take more than 100 SGPRs, which costs the eighth wave per SIMD - measured
// +11 % on the kernel, profiles/multiband_rate.txt)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void multiband_compose_kernel(BandSrc b, int S, int64_t C, int R, DbMap dm,
                                                                const uint32_t* __restrict__ lut, float* __restrict__ db,
                                                                uint32_t* __restrict__ rgba, uint8_t* __restrict__ index) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the same in every lane: the column loop is scalar
    const int qall = R / 4;
    const int64_t ncols = (int64_t)S * C;
    for (int64_t sc = (int64_t)blockIdx.x * 4 + wave; sc < ncols; sc += (int64_t)gridDim.x * 4) {
        const int64_t s = sc / C, c = sc - s * C;
        const float4* base = reinterpret_cast<const float4*>(b.plane[0] + sc * (int64_t)b.rows[0]);
        int dist[kMaxBands];   // quads from `base` to band k's source column moved back by its first row
#pragma unroll
        for (int k = 1; k < kMaxBands; ++k) {
            const int64_t off = (s * (C + 2 * (int64_t)b.shift[k]) + c + b.shift[k]) * (int64_t)b.rows[k] - 4 * (int64_t)b.q0[k];
            dist[k] = (int)(((b.plane[k] - b.plane[0]) + off - sc * (int64_t)b.rows[0]) >> 2);
        }
        const size_t o = (size_t)sc * R;
        for (int q = lane; q < qall; q += 64) {
            int d = 0;
#pragma unroll
            for (int k = 1; k < kMaxBands; ++k) d = q >= b.q0[k] ? dist[k] : d;
            const float4 v = base[(int64_t)(d + q)];
            if (db) *reinterpret_cast<float4*>(db + o + 4 * q) = v;
            if (rgba || index) {
                const int i0 = cell_index(dm, v.x), i1 = cell_index(dm, v.y), i2 = cell_index(dm, v.z), i3 = cell_index(dm, v.w);
                store_colour4(lut, i0, i1, i2, i3, o + 4 * q, rgba, index);
            }
        }
    }
}

hipError_t launch_multiband_compose(const BandSrc& b, int S, int64_t C, int R, const DbMap& dm, const uint8_t* lut, float* db,
                                    uint8_t* rgba, uint8_t* index, hipStream_t st) {
    if (S <= 0 || C <= 0) return hipSuccess;
    // the kernel addresses every band from band 0's plane with 32-bit quad distances
    if (b.q0[0] != 0 || b.shift[0] != 0) return hipErrorInvalidValue;
    for (int k = 1; k < kMaxBands; ++k) {
        const int64_t first = b.plane[k] - b.plane[0], quads = (int64_t)S * (C + 2 * (int64_t)b.shift[k]) * b.rows[k] / 4;
        if (first % 4 || first / 4 + quads >= ((int64_t)1 << 31) || first / 4 - (int64_t)S * C * b.rows[0] / 4 - b.q0[k] <= -((int64_t)1 << 31))
            return hipErrorInvalidValue;
    }
    const int64_t ncols = (int64_t)S * C;
    int64_t blocks = (ncols + 3) / 4;
    blocks = blocks > 16384 ? 16384 : blocks;
    hipLaunchKernelGGL(multiband_compose_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b, S, C, R, dm,
                       reinterpret_cast<const uint32_t*>(lut), db, reinterpret_cast<uint32_t*>(rgba), index);
    return hipGetLastError();
}

}  // namespace emspec
