// multires.hip.inc — the composition stage of the multi-resolution batch (DESIGN.md §3.8, §4.9; emspec_multires.cpp):
// the long FFT's raw dB for rows [0, split), the short FFT's for rows [split, R), on the long FFT's column grid.
// Included by kernels.hip after post.hip.inc.
namespace emspec {

// One wave per (stream, column), grid-stride over S * C of them.  lo: [S][C][split] raw dB of the low band, hi: [S][C + 2 shift]
// [R - split] of the high band; column c takes the low band's column c and the high band's column c + shift (which starts
// shift * (R - split) floats after the high band's column c).  A lane moves a quad of rows (16-byte loads and stores, the wave
// covers 256 consecutive rows per step; split and R are multiples of 4, so a quad never straddles the seam).  Outputs [S][C][R]
// (rgba + [4]), any of them null: dB as read, the palette index by cell_index - the function every finalize stage uses, so the
// bytes are those of the single-resolution batches - and RGBA = LUT[index].
__global__ __launch_bounds__(256) void multires_compose_kernel(const float* __restrict__ lo, const float* __restrict__ hi,
                                                               int S, int64_t C, int R, int split, int shift, DbMap dm,
                                                               const uint32_t* __restrict__ lut, float* __restrict__ db,
                                                               uint32_t* __restrict__ rgba, uint8_t* __restrict__ index) {
    const int lane = threadIdx.x & 63;
    const int qlo = split / 4, qall = R / 4, Rh = R - split;
    const int64_t Ch = C + 2 * (int64_t)shift, ncols = (int64_t)S * C;
    for (int64_t sc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); sc < ncols; sc += (int64_t)gridDim.x * 4) {
        const int64_t s = sc / C, c = sc - s * C;
        const float4* pl = reinterpret_cast<const float4*>(lo + (size_t)sc * split);
        const float4* ph = reinterpret_cast<const float4*>(hi + ((size_t)s * Ch + c + shift) * Rh);
        const size_t o = (size_t)sc * R;
        for (int q = lane; q < qall; q += 64) {
            const float4 v = q < qlo ? pl[q] : ph[q - qlo];
            if (db) *reinterpret_cast<float4*>(db + o + 4 * q) = v;
            if (rgba || index) {
                const int i0 = cell_index(dm, v.x), i1 = cell_index(dm, v.y), i2 = cell_index(dm, v.z), i3 = cell_index(dm, v.w);
                store_colour4(lut, i0, i1, i2, i3, o + 4 * q, rgba, index);
            }
        }
    }
}

hipError_t launch_multires_compose(const float* lo, const float* hi, int S, int64_t C, int R, int split, int shift,
                                   const DbMap& dm, const uint8_t* lut, float* db, uint8_t* rgba, uint8_t* index,
                                   hipStream_t st) {
    if (S <= 0 || C <= 0) return hipSuccess;
    const int64_t ncols = (int64_t)S * C;
    int64_t blocks = (ncols + 3) / 4;
    blocks = blocks > 16384 ? 16384 : blocks;
    hipLaunchKernelGGL(multires_compose_kernel, dim3((unsigned)blocks), dim3(256), 0, st, lo, hi, S, C, R, split, shift, dm,
                       reinterpret_cast<const uint32_t*>(lut), db, reinterpret_cast<uint32_t*>(rgba), index);
    return hipGetLastError();
}

}  // namespace emspec
