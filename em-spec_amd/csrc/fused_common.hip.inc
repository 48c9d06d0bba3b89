// fused_common.hip.inc — the straight-line arithmetic every batch kernel runs between its FFT and the output arrays, stated
// once.  Included by kernels.hip before the first kernel that scatters or finalises (the tile / walk scatter, then
// fused.hip.inc, post.hip.inc, multires.hip.inc).  A file of its own rather than a section of emspec_device.h: that header is
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

// The per-bin stage of bins 4g .. 4g+3 from the split spectra at positions 4g-1 .. 4g+4: spectral Hann identities, power
// gate, time and frequency reassignment, row lookup, segment test, ring slot; then runs of bins that share a cell are
// summed in registers (a lane's consecutive bins often do), so okv[] marks one accumulate per distinct cell.
// This is the second statement of reassign_core / reassign_core_fast (emspec_device.h): same results bit for bit, other
// operand layout - the six positions arrive as arrays instead of three YT records, T's imaginary part is carried negated
// (ur = -Ti, exact, hence -(Ui * Ai)), and the outcome is a ring cell and a predicate instead of a BinOut.  Branch-free and
// unrolled so the four bins' dependency chains (reassign -> edge-table read -> accumulate) overlap.
// kf0 = (float)(4g); sbase = ring slot of column j - dmax; jrel = j - c0; span = c1 - c0; dmax = the ring's reach (a
// compile-time constant of the kernel, or pl.D), slots = its slot count (likewise); Df = (float)pl.D.
// The accumulates, and the s_setprio steps between them, stay in each kernel: they are schedule.
template <bool FAST>
__device__ __forceinline__ void bins4(const float pfloor_abs, const int reassign, const float tscale, const HintLookup& lk,
                                      const float (&yr)[6], const float (&yi)[6], const float (&ur)[6], const float (&tr)[6],
                                      const float kf0, const int sbase,
                                      const int jrel, const unsigned span, const float Df, float* ring, const int R,
                                      const int dmax, const int slots, float* (&cellp)[4], float (&pw)[4], bool (&okv)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float Ar = twice_minus(yr[e + 1], yr[e] + yr[e + 2]), Ai = twice_minus(yi[e + 1], yi[e] + yi[e + 2]);
        const float Br = twice_minus(tr[e + 1], tr[e] + tr[e + 2]), Ui = twice_minus(ur[e + 1], ur[e] + ur[e + 2]);
        const float Dr = yr[e] - yr[e + 2], Di = yi[e] - yi[e + 2];
        const float den = __builtin_fmaf(Ar, Ar, Ai * Ai);
        const float P = den * 0.015625f;
        bool ok = (P >= pfloor_abs) && (P <= kPowerMax);
        const float kf = kf0 + (float)e;
        float kh = kf;
        int d = dmax;
        if (FAST || reassign) {
            const float numT = __builtin_fmaf(Br, Ar, -(Ui * Ai));
            const float numF = __builtin_fmaf(Dr, Ar, Di * Ai);
            const float inv = FAST ? recip_normal(den) : 1.0f / den;
            const float cf = __builtin_floorf(__builtin_fmaf(numT * inv, tscale, 0.5f));
            ok = ok && (__builtin_fabsf(cf) <= Df);
            d = (int)cf + dmax;
            kh = kf + numF * inv;
        }
        const int rr = FAST ? lk.row_signed_log(kh) : lk.row_signed(kh);   // -1 / R when k-hat is off the frequency axis
        ok = ok && ((unsigned)rr < (unsigned)R);
        ok = ok && ((unsigned)(jrel + d - dmax) < span);
        unsigned sl = (unsigned)(sbase + d);   // garbage when !ok: the cell is then never touched
        sl = min(sl, sl - (unsigned)slots);
        cellp[e] = ring + __umul24(sl, (unsigned)R) + rr;   // 24-bit multiply: full rate (v_mul_lo_u32 is quarter rate)
        pw[e] = P;
        okv[e] = ok;
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const bool same = okv[e] && okv[e + 1] && (cellp[e] == cellp[e + 1]);
        pw[e + 1] = same ? pw[e + 1] + pw[e] : pw[e + 1];
        okv[e] = okv[e] && !same;
    }
}

}  // namespace emspec
