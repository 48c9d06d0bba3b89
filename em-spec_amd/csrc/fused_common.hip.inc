// fused_common.hip.inc — the straight-line arithmetic every batch kernel runs between its FFT and the output arrays, stated
// once.  Included by kernels.hip before the first kernel that scatters or finalises (the tile / walk scatter, then
// fused.hip.inc, post.hip.inc, multiband.hip.inc).  A file of its own rather than a section of emspec_device.h: that header is
// also the EXACT-mode and live kernels', which use none of this, and these helpers know the fused kernels' ring layout.
//
// The kernels differ in their SCHEDULE (who runs which FFT pass when, barriers, s_setprio points, where the ring lives) and
// keep all of that; what is here has no barrier, no priority change and no launder in it.  Everything is
// __device__ __forceinline__ and written as the same expression tree, in the same order, as the kernels spelled it before
// (DESIGN.md §3: the arithmetic order is the specification); profiles/refactor_fused_common_isa.txt holds the kernel-by-kernel
// comparison of the generated code.
namespace emspec {

// The RGBA and palette-index stores of four neighbouring cells (either pointer may be null); o = the cells' linear offset.
__device__ __forceinline__ void store_colour4(const uint32_t* lut, int i0, int i1, int i2, int i3, size_t o,
                                              uint32_t* rgba, uint8_t* index) {
    if (rgba) *reinterpret_cast<uint4*>(rgba + o) = make_uint4(lut[i0], lut[i1], lut[i2], lut[i3]);
    if (index) *reinterpret_cast<uint32_t*>(index + o) =
        (uint32_t)i0 | ((uint32_t)i1 << 8) | ((uint32_t)i2 << 16) | ((uint32_t)i3 << 24);
}

// Stage "dB + colour" of four neighbouring cells: energies -> dB -> palette index, and the three optional stores.
// FASTDB: cell_db_fast (the fused kernels) instead of cell_db (the record scatters).
template <bool FASTDB>
__device__ __forceinline__ void store_cells4(const DbMap& dm, const uint32_t* lut, const float4 e4, const size_t o,
                                             float* db, uint32_t* rgba, uint8_t* index) {
    const float d0 = FASTDB ? cell_db_fast(dm, e4.x) : cell_db(dm, e4.x), d1 = FASTDB ? cell_db_fast(dm, e4.y) : cell_db(dm, e4.y);
    const float d2 = FASTDB ? cell_db_fast(dm, e4.z) : cell_db(dm, e4.z), d3 = FASTDB ? cell_db_fast(dm, e4.w) : cell_db(dm, e4.w);
    const int i0 = cell_index(dm, d0), i1 = cell_index(dm, d1), i2 = cell_index(dm, d2), i3 = cell_index(dm, d3);
    if (db) *reinterpret_cast<float4*>(db + o) = make_float4(d0, d1, d2, d3);
    store_colour4(lut, i0, i1, i2, i3, o, rgba, index);
}

// A finished quad of the fused kernels' column ring [slots][R], cells cell .. cell + 3 of slot sl: read it, clear it for the
// slot's next column, finalise it to the linear output offset o.  (24-bit multiply: full rate)
__device__ __forceinline__ void finalize_ring_quad(float* ring, int sl, int R, int cell, const DbMap& dm, const uint32_t* lut,
                                                   const size_t o, float* db, uint32_t* rgba, uint8_t* index) {
    float4* quad = reinterpret_cast<float4*>(ring + __umul24((unsigned)sl, (unsigned)R) + cell);
    const float4 e4 = *quad;
    *quad = make_float4(0.f, 0.f, 0.f, 0.f);
    store_cells4<true>(dm, lut, e4, o, db, rgba, index);
}

// The spectrum at a thread's six positions, F(i) = Z[4g-1+i] at fb[fpos[i]] and M(i) = Z[N-4g+1-i] at fb[mpos[i]], split
// into Y = Z + conj W and T = -j (Z - conj W) (ur = -Ti).  All twelve reads are issued before the first use: left alone
// the compiler reads them two at a time into the same registers, a full LDS round trip per pair.
__device__ __forceinline__ void read_split6(const float2* fb, const int (&fpos)[6], const int (&mpos)[6],
                                            float (&yr)[6], float (&yi)[6], float (&ur)[6], float (&tr)[6]) {
    float2 f[6], m[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) { f[i] = fb[fpos[i]]; m[i] = fb[mpos[i]]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        yr[i] = f[i].x + m[i].x; yi[i] = f[i].y - m[i].y; ur[i] = f[i].x - m[i].x; tr[i] = f[i].y + m[i].y;
    }
}

}  // namespace emspec
