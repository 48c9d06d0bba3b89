// fused_pp.hip.inc — fused batch kernel for N = 4096 (hop 256, 512 or 1024), the two 8-wave teams HALF AN ITERATION
// APART.  The product path since round 3; in its present form (spectrum reads in role 0) since round 4.
// Included by fused.hip.inc after fused_r8.hip.inc (same LDS images, swizzle and FFT helpers: namespace f8).  The arithmetic
// between the FFT and the output arrays is the one definition of fused_common.hip.inc (finalize_ring_quad, read_split6); the
// four-bin stage is spelled out in each kernel (here, fused_n8192, fused_small, diag/fused_pp4), the same text in the same
// order: per bin the spectral Hann identities, the power gate, time and frequency reassignment, the row lookup, the segment
// test and the ring slot; then runs of a lane's consecutive bins that share a cell are summed in registers, so okv[] marks
// one accumulate per distinct cell.  It is the second statement of reassign_core / reassign_core_fast (emspec_device.h):
// same results bit for bit, other operand layout (six positions as arrays, ur = -Ti carried negated, a ring cell and a
// predicate instead of a BinOut).  A shared function for it (bins4, until it lost its last caller) rescheduled these kernels
// (profiles/refactor_fused_common_isa.txt), so sharing it waits for an A/B measurement per kernel.
//
// The lock-step kernel this one replaced (fused4096_r8_kernel, docs/HISTORY.md "Retired kernel forms") ran its two frames
// together: all 16 waves stream LDS in the FFT passes, then all 16 waves
// issue VALU in the per-bin stage, with three workgroup barriers per two frames - and a timing-only build without those
// barriers runs 21 % faster (docs/HISTORY.md §4.1e): what the barriers cost is not the instruction but the coupling of
// sixteen waves to the slowest one three times per iteration, and the loss of overlap between LDS-bound and VALU-bound
// phases.  Here team h = 0 (waves 0-7, even frames) and team 1 (odd frames) alternate roles every half-iteration k:
//     role 0 (k + h even): passes B, C, D of frame j0 + k | arrive | finalise column j0 + k - 2 - D (the team's first four
//                          waves) | wait for the team | the 12 spectrum reads of the thread's bins + conjugate split
//     role 1 (k + h odd) : per-bin stage of frame j0 + k - 1 FROM REGISTERS, scatter, pass A of frame j0 + k + 1 and its write
// so every SIMD always holds two waves of each kind.  One workgroup barrier per half-iteration orders write -> pass B (the
// team leaving role 1) and spectrum reads -> pass-A write (the team leaving role 0: its buffer is free the moment it enters
// role 1).  The third ordering, pass D -> spectrum reads, is inside role 0 of one team: an arrival counter in LDS (one
// ds_add per wave after its pass-D stores, one poll before its reads; the finalize sits between the two; every wave of the
// team arrives before it polls, so the wait always ends - the spin is bounded all the same).
// The split spectra (24 floats: Y and T at the thread's six positions) cross the barrier in registers.  The loop body is one
// (role 0, role 1) pair per team - team 1 enters through one extra barrier, team 0 leaves through one - so that array is
// local to the body and nothing is carried around the loop for it (119 VGPRs, no scratch).
// Round 3's form read the spectra at the start of role 1 (arrival counter between those reads and the pass-A write): role 1
// was the long role (5.4 k cycles against 4.4 k), and its first instructions were twelve LDS reads queued behind the other
// team's passes.  Moving the reads - not more: handing over the stencils or the dot products instead (24 or 12 floats)
// measured 9.14 / 9.15 ms against 9.04 - A/B on one box: 9.32 -> 9.02 ms, bit-identical palette indices
// (the old form was A/B variant "pp3" until it was retired, docs/HISTORY.md "Retired kernel forms").
// Passes B, C and D issue their stores as their data is ready (f8::pass8_store_as_you_go, fused_r8.hip.inc): two ds_write_b64
// behind each pair of the last stage instead of the four to eight back to back the compiler otherwise leaves at a pass's end,
// in front of the next pass's reads.  The same instructions in another order: 9.06 -> 8.93 ms, A/B on one box;
// diag/fused_pp4.hip.inc keeps the stores-at-the-end form as variant "pp4".  Pass A's write in role 1 stays clustered in front
// of the barrier: spreading it as well measured no gain alone (9.05) and 8.97 together with the others (docs/HISTORY.md §20).
// Ring: at half-iteration k the column j0 + k - 2 - D is finalised by the role-0 team (its last contributor, frame
// j0 + k - 2, was scattered by that team at k - 1) while the role-1 team scatters frame j0 + k - 1, which reaches no
// lower than column j0 + k - 1 - D: 2D + 2 slots, as in the lock-step kernel.
// Measured and not kept (rounds 3-4, on the round-3 form): pass A of the OTHER team's next frame at the end of role 0
// (9.78 vs 9.15 ms); the finished column's cells two per thread over all eight waves of the role-0 team (9.55 vs 9.15 ms - the
// first four waves finish passes B, C, D ahead of the other four anyway, so the finalize fills their lead); deferring a
// thread's fourth accumulate to its team's next role with a 2D + 3 slot ring (no change - the wait is the VARIANCE of the
// slowest of sixteen waves, not the difference of the means); the halo spectra by DPP: not built - with the lanes of a wave
// 32 bins apart (worth 4.6 %, fused_r8) the neighbouring group lives in another WAVE.
namespace emspec {

// stamped (diagnostic) build, slots: 0 finalize | 1 passes B C D | 2 bins | 3 scatter + next pass A | 4 spectrum reads +
// split | 5 team wait | 6 pass-A write + the two barrier waits | 7 accumulate rounds (low word), 100 MHz ticks (high word)
#define EMSPEC_STAMP(slot)                                                        \
    if constexpr (STAMP) {                                                        \
        const unsigned long long now_ = __builtin_readcyclecounter();             \
        acc_[slot] += now_ - last_;                                               \
        last_ = now_;                                                             \
    }
template <int HOP, bool STAMP, bool FAST = false>
__global__ __launch_bounds__(1024, 4) void fused4096_pp_kernel(
    PlanDev pl, DbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, float* __restrict__ db, uint32_t* __restrict__ rgba, uint8_t* __restrict__ index,
    unsigned long long* __restrict__ stamps) {
    using namespace f8;
    constexpr int DMAX = Geo<HOP>::DMAX, SLOTS = Geo<HOP>::SLOTS, SH = Geo<HOP>::SH;
    unsigned long long acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last_ = 0;
    extern __shared__ float4 smem4[];
    const int R = pl.rows, D = pl.D;
    float2* fbuf = reinterpret_cast<float2*>(smem4);            // [2][4096] complex
    float* ring = reinterpret_cast<float*>(fbuf + 2 * N);        // [SLOTS][R]
    float* seb = ring + SLOTS * R;                                // [R+1] (+3 pad)
    uint32_t* slut = reinterpret_cast<uint32_t*>(seb + R + 4);   // [256]
    float2* stwB = reinterpret_cast<float2*>(slut + 256);        // [7][64] pass-B twiddles
    float2* stwC = stwB + 7 * 64;                                 // [7][8]  pass-C twiddles
    unsigned* arrive = reinterpret_cast<unsigned*>(stwC + 7 * 8);   // [2] per-team arrival counters (+ 2 words unused)

    const int tid = threadIdx.x, h = tid >> 9, t = tid & 511;
    float2* fb = fbuf + h * N;
    int s;
    int64_t c0, c1;
    if (!seg_of_block(sp, C, s, c0, c1)) return;
    const int64_t j0 = (c0 - D > 0 ? c0 - D : 0) & ~(int64_t)1;
    const int64_t jstop = c1 + D;
    const float* x0 = pcm + (size_t)s * L;

    // ---- workgroup set-up
    for (int q = tid; q < SLOTS * R / 4; q += 1024) reinterpret_cast<float4*>(ring)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = tid; r <= R; r += 1024) seb[r] = pl.ebin[r];
    if (tid < 256) slut[tid] = lut[tid];
    if (tid < 7 * 64) stwB[tid] = pl.tw[tw_index8<3>(tid >> 6, tid & 63)];
    else if (tid < 7 * 64 + 7 * 8) stwC[tid - 7 * 64] = pl.tw[tw_index8<6>((tid - 7 * 64) >> 3, (tid - 7 * 64) & 7)];
    else if (tid < 7 * 64 + 7 * 8 + 4) arrive[tid - (7 * 64 + 7 * 8)] = 0u;
    float2 twA[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) twA[e] = pl.tw[tw_index8<0>(e, t)];
    float xs[8];
    {
        const int64_t j = j0 + h;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t idx = j * HOP + t + 512 * i;
            xs[i] = idx < L ? x0[idx] : 0.0f;
        }
    }
    const float r0 = (float)(t - N / 2) * (2.0f / (float)N);   // ramp of register 0; register i adds i/4 (exact)
    HintLookup lk;
    lk.init(seb, pl.ebin, R, pl.log_rows);
    int posB[8], posC[8];     // in-place positions of this thread's pass-B / pass-C points
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        posB[i] = swz(((t >> 6) << 9) + (t & 63) + (i << 6));
        posC[i] = swz(((t >> 3) << 6) + (t & 7) + (i << 3));
    }
    // bin groups: the lanes of one wave-instruction sit 32 bins apart (see fused_r8.hip.inc)
    const int bg = ((t & 63) << 3) | (t >> 6);
    int fpos[6], mpos[6];     // positions of Z[4g-1+i] and Z[N-4g+1-i] in the in-place buffer
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        fpos[i] = zpos((4 * bg - 1 + i) & (N - 1));
        mpos[i] = zpos((N - 4 * bg + 1 - i) & (N - 1));
    }
    // both teams write pass A of their first frame (j0 + h) before the loop
    {
        float2 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.25f * (float)i));
        stages8(v, TwRegsSym{twA});
        const int64_t j = j0 + h;
        if (j < C && j < jstop) {
            float2* const w0 = fb + swz(t);
            float2* const w1 = fb + (swz(t) ^ 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) ((i & 1) ? w1 : w0)[T * i] = v[i];
        }
    }
    // Half-iterations k = 0 .. klast: the last column c1-1 is finalised at klast = c1 - 1 + 2 + D - j0.  Team h runs the
    // pairs (k, k + 1) for k = h, h + 2, ..: P pairs and 2P + 1 workgroup barriers for both teams (team 1's half-iteration 0
    // has nothing to do: one barrier in front; team 0 closes with one).  The half-iterations past klast that this adds
    // find their frames and columns outside the segment and do nothing.
    const int klast = (int)(c1 + 1 + D - j0);
    const int P = (klast + 2) >> 1;
    // Column bookkeeping in 32 bits, relative to the segment's first frame j0 (the launcher refuses a segment whose walk
    // does not fit: fused_pp_walk_ok, emspec_seg_plan.h - every difference below is at most seglen + 2D + 3, and the
    // samples a segment walks stay far inside an int).  What is the same for both teams is carried per pair in scalar
    // registers; the team's h is added.  As 64-bit vector arithmetic per half-iteration (j against C and jstop, the column
    // against c0 and c1, the prefetch's sample index against L, the output offset by two multiplies and a 64-bit
    // multiply-add) the same tests cost 14 more VALU per pair, several at quarter rate: 8.86 -> 8.76 ms, A/B on one box
    // (docs/HISTORY.md §22; diag/fused_pp4.hip.inc keeps the 64-bit form).
    const int kact = (int)((C < jstop ? C : jstop) - j0);   // frame j0 + k is walked for k < kact
    const int kfin = (int)(c0 + 2 + D - j0);                // column c0 is finalised at half-iteration kfin, c0 + i at kfin + i
    const unsigned span = (unsigned)(c1 - c0);
    const int jrel0 = (int)(j0 - c0);
    int sk0 = (int)(j0 % SLOTS);         // ring slot of column j0 + 2p: even, so the team's + h never wraps
    // the finalize's output offset of column j0 + 2p - 2 - D, cell 0 (wraps below column 0, where it is not used)
    size_t ocol = ((size_t)s * (size_t)C + (size_t)(j0 - 2 - D)) * (size_t)R;
    // the sample prefetch of frame j0 + 2p + 2 + h: a row pointer and the samples that remain from it, counted in int
    // (clamped: a count that large stays above every offset for the whole walk), and the thread's offset from it
    const float* xrow = x0 + (j0 + 2) * HOP;
    const int64_t rem0 = L - (j0 + 2) * HOP;
    int xrem = rem0 < 0x7fffffff ? (int)rem0 : 0x7fffffff;
    unsigned arrivals = 0;               // role-0 visits of this team so far x 8 waves = the counter's target
    __syncthreads();
    unsigned long long real0_ = 0;
    if constexpr (STAMP) { last_ = __builtin_readcyclecounter(); real0_ = __builtin_amdgcn_s_memrealtime(); }
    if (h) __syncthreads();
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        // Launder t once per pair: every LDS address below is then recomputed (1-3 VALU each) instead of being hoisted
        // out of the loop, which would pin ~50 VGPRs.
        int tt = t;
        asm volatile("" : "+v"(tt));
        const int k = 2 * p + h;             // this team's half-iteration in role 0: frame j = j0 + k
        const int sk = sk0 + h;              // ring slot of column j
        const bool active = k < kact;
        float yr[6], yi[6], ur[6], tr[6];   // Y = Z + conj W, T = -j (Z - conj W) at the six positions (ur = -Ti): role 0 -> role 1
        // ================= role 0 at half-iteration k: passes B, C, D of frame j, finalise column j-2-D, spectrum reads
        if (active) {
            float2 v[8];
            // pass B = stages 3..5 : p = hi*512 + i*64 + lo
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[posB[i]];
            pass8_store_as_you_go(bfly8(v, TwLdsSym<64>{stwB + (tt & 63)}), [&](int i) { fb[posB[i]] = v[i]; });
            wave_lds_sync();
            // pass C = stages 6..8 : p = hi*64 + i*8 + lo   (same wave's sub-FFT)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[posC[i]];
            pass8_store_as_you_go(bfly8(v, TwLdsSym<8>{stwC + (tt & 7)}), [&](int i) { fb[posC[i]] = v[i]; });
            wave_lds_sync();
            // pass D = stages 9..11 : p = 8*t + i, in place; Z[k] ends at position bitrev12(k)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz((tt << 3) + i)];
            pass8_store_as_you_go(BflyD{v}, [&](int i) { fb[swz((tt << 3) + i)] = v[i]; });
        }
        // this wave's pass-D stores are issued (the LDS pipe serves one wave's operations in order, so the counter moves
        // after them): tell the team
        asm volatile("" ::: "memory");
        if ((tt & 63) == 0) __hip_atomic_fetch_add(arrive + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm volatile("" ::: "memory");
        arrivals += 8;
        EMSPEC_STAMP(1)
        {
            const int qpc = R >> 2;   // float4 quads per column
            if (t < qpc && (unsigned)(k - kfin) < span) {   // column j - 2 - D lies in [c0, c1)
                const int cell = t << 2;
                int sl = sk - 2 - D;
                sl += sl < 0 ? SLOTS : 0;
                finalize_ring_quad(ring, sl, R, cell, dm, slut, ocol + (unsigned)(h * R + cell), db, rgba, index);
            }
        }
        EMSPEC_STAMP(0)
        // the spectrum is complete once all eight waves of the team have stored their pass D
        // (bounded: 2^16 polls is ~2 ms, far beyond any legitimate wait - a protocol error must fail a test, not hang)
        for (unsigned spins = 0; (int)(__hip_atomic_load(arrive + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - arrivals) < 0; ++spins) {
            if (spins >= (1u << 16)) { g_kernel_error = 1; break; }   // reported by emspec_device_status: the results are invalid
            __builtin_amdgcn_s_sleep(1);
        }
        asm volatile("" ::: "memory");
        EMSPEC_STAMP(5)
        read_split6(fb, fpos, mpos, yr, yi, ur, tr);   // all twelve reads issued before the first use
        EMSPEC_STAMP(4)
        __syncthreads();
        EMSPEC_STAMP(6)
        // ================= role 1 at half-iteration k + 1: bins + scatter of frame j, pass A of frame j + 2 and its write
        {
            const int xo = h * HOP + t + 512 * (8 - SH);       // first new sample register of frame jn = j + 2, from xrow
            float xn[SH];
#pragma unroll
            for (int q = 0; q < SH; ++q) xn[q] = (xo + 512 * q < xrem) ? xrow[xo + 512 * q] : 0.0f;
            if (active) {
                __builtin_amdgcn_s_setprio(2);
                float* cellp[4];
                float pw[4];
                bool okv[4];
                int sbase = sk - DMAX;                 // ring slot of column j-DMAX
                sbase += sbase < 0 ? SLOTS : 0;
                const int jrel = jrel0 + k;            // j - c0
                const float Df = (float)D;
                const float kf0 = (float)(4 * (((tt & 63) << 3) | (tt >> 6)));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float Ar = twice_minus(yr[e + 1], yr[e] + yr[e + 2]), Ai = twice_minus(yi[e + 1], yi[e] + yi[e + 2]);
                    const float Br = twice_minus(tr[e + 1], tr[e] + tr[e + 2]), Ui = twice_minus(ur[e + 1], ur[e] + ur[e + 2]);
                    const float Dr = yr[e] - yr[e + 2], Di = yi[e] - yi[e + 2];
                    const float den = __builtin_fmaf(Ar, Ar, Ai * Ai);
                    const float Pw = den * 0.015625f;
                    bool ok = (Pw >= pl.pfloor_abs) && (Pw <= kPowerMax);
                    const float kf = kf0 + (float)e;
                    float kh = kf;
                    int d = DMAX;
                    if (FAST || pl.reassign) {
                        const float numT = __builtin_fmaf(Br, Ar, -(Ui * Ai));
                        const float numF = __builtin_fmaf(Dr, Ar, Di * Ai);
                        const float inv = FAST ? recip_normal(den) : 1.0f / den;
                        const float cf = __builtin_floorf(__builtin_fmaf(numT * inv, pl.tscale, 0.5f));
                        ok = ok && (__builtin_fabsf(cf) <= Df);
                        d = (int)cf + DMAX;
                        kh = kf + numF * inv;
                    }
                    const int rr = FAST ? lk.row_signed_log(kh) : lk.row_signed(kh);   // -1 / R when k-hat is off the frequency axis
                    ok = ok && ((unsigned)rr < (unsigned)R);
                    ok = ok && ((unsigned)(jrel + d - DMAX) < span);
                    unsigned sl = (unsigned)(sbase + d);   // garbage when !ok: the cell is then never touched
                    sl = min(sl, sl - (unsigned)SLOTS);
                    cellp[e] = ring + __umul24(sl, (unsigned)R) + rr;
                    pw[e] = Pw;
                    okv[e] = ok;
                }
                // a lane's consecutive bins often share a cell: sum such runs in registers first
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const bool same = okv[e] && okv[e + 1] && (cellp[e] == cellp[e + 1]);
                    pw[e + 1] = same ? pw[e + 1] + pw[e] : pw[e + 1];
                    okv[e] = okv[e] && !same;
                }
                EMSPEC_STAMP(2)
                if constexpr (STAMP) {   // diagnostic build: slot 7 counts accumulate rounds (4 calls per frame)
                    acc_[7] += lds_accumulate_counted(cellp[0], pw[0], okv[0]);
                    acc_[7] += lds_accumulate_counted(cellp[1], pw[1], okv[1]);
                    acc_[7] += lds_accumulate_counted(cellp[2], pw[2], okv[2]);
                    acc_[7] += lds_accumulate_counted(cellp[3], pw[3], okv[3]);
                } else {
                    lds_accumulate(cellp[0], pw[0], okv[0]);
                    lds_accumulate(cellp[1], pw[1], okv[1]);
                    __builtin_amdgcn_s_setprio(1);
                    lds_accumulate(cellp[2], pw[2], okv[2]);
                    lds_accumulate(cellp[3], pw[3], okv[3]);
                }
                __builtin_amdgcn_s_setprio(0);
            }
            // next frame of this team: shift the sample registers by one (two hops), run its pass A in registers
#pragma unroll
            for (int i = 0; i < 8 - SH; ++i) xs[i] = xs[i + SH];
#pragma unroll
            for (int q = 0; q < SH; ++q) xs[8 - SH + q] = xn[q];
            float2 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.25f * (float)i));
            stages8(v, TwRegsSym{twA});
            EMSPEC_STAMP(3)
            if (k + 2 < kact) {   // frame j + 2 is walked; the team read this buffer's spectra before the barrier above: it is free
                float2* const w0 = fb + swz(tt);
                float2* const w1 = fb + (swz(tt) ^ 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) ((i & 1) ? w1 : w0)[T * i] = v[i];
            }
        }
        __syncthreads();
        EMSPEC_STAMP(6)
        sk0 += 2;
        sk0 -= sk0 >= SLOTS ? SLOTS : 0;
        ocol += 2 * (size_t)R;
        xrow += 2 * HOP;
        xrem -= 2 * HOP;
    }
    if (!h) __syncthreads();
    if constexpr (STAMP) {
        if ((tid & 63) == 0) {
            unsigned long long* o = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (tid >> 6)) * 8;
            acc_[7] = (acc_[7] & 0xFFFFFFFFull) | ((__builtin_amdgcn_s_memrealtime() - real0_) << 32);
            for (int i = 0; i < 8; ++i) o[i] = acc_[i];
        }
    }
}
#undef EMSPEC_STAMP
// (dynamic LDS: fused_pp_lds_bytes, emspec_kernel_plan.h)

}  // namespace emspec
