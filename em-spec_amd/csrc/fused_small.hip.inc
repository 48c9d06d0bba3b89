// fused_small.hip.inc — the fused batch kernel for N = 2048 and N = 1024 (and, as S = 0, for N = 4096 at the hops
// fused_pp.hip.inc is not built for) on the 4096-point carrier network of fused_r8.hip.inc.  Included by kernels.hip after
// fused_r8.hip.inc (reuses f8::swz / zpos / tw_index8 / TwLdsSym); the finalize and the spectrum split are
// fused_common.hip.inc's, the four-bin stage is spelled out in the order fused_pp.hip.inc describes.
//
// A 4096-point radix-2 DIF network whose first S stages are skipped is 2^S independent
// (4096 >> S)-point networks side by side, and its twiddles are the small network's own
// (tw_n[q] == tw4096[q << S]: the double argument is identical).  So each 512-thread team runs
// FPT = 2^S consecutive frames through its 4096-point buffer at once — S = 1: two 2048-point
// frames, S = 2: four 1024-point frames — with pass A reduced to stages S..2 and passes B, C, D
// unchanged.  Frame slot fs of a team lives in buffer part fs, and its spectrum sample Z[m] ends at
// zpos((m << S) | bitrev_S(fs)).  The hop is a run-time value: samples are reloaded for every block (consecutive
// frames overlap, so the loads hit L1/L2), and the ring has 2D + 2 FPT column slots, whatever fits in LDS.
// (The lock-step form of this kernel, fused_small_kernel, was the product until round 3 and an A/B form after it:
// docs/HISTORY.md "Retired kernel forms".)
namespace emspec {

namespace fsm {
// three-minus-U0 radix-2 DIF stages on 8 registers (the tail of f8::stages8)
template <int U0, class W>
__device__ __forceinline__ void stages8_from(float2 (&v)[8], const W& w) {
#pragma unroll
    for (int u = U0; u < 3; ++u) {
        const int mloc = 4 >> u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i & mloc) continue;
            const float2 a = v[i], b = v[i + mloc];
            v[i] = cadd(a, b);
            v[i + mloc] = cmul_tw(csub(a, b), w(8 - 2 * mloc + (i & (mloc - 1))));
        }
    }
}
template <int S> __device__ __forceinline__ int brev_s(int x);
template <> __device__ __forceinline__ int brev_s<0>(int x) { return x; }
template <> __device__ __forceinline__ int brev_s<1>(int x) { return x; }
template <> __device__ __forceinline__ int brev_s<2>(int x) { return ((x & 1) << 1) | (x >> 1); }
}  // namespace fsm

// The two teams run HALF AN ITERATION APART (the schedule of fused_pp.hip.inc, DESIGN.md
// §4.1, with FPT frames per team and half-iteration instead of one; like it with the spectrum reads in role 0 since round 4).
// Team h takes the blocks b = k of FPT consecutive frames with (k + h) even; at half-iteration k
//     role 0 (k + h even): passes B, C, D of block k | arrive | finalise the FPT columns no later block reaches | wait for the
//                          team | the 12 spectrum reads of the thread's bins + conjugate split               (LDS-heavy)
//     role 1 (k + h odd) : bins (from registers) + scatter of block k - 1, samples + pass A of block k + 1 and its write
// One workgroup barrier per half-iteration; the team-internal ordering pass D -> spectrum reads is the arrival counter of
// fused_pp; the loop body is one (role 0, role 1) pair per team, team 1 one barrier behind.  A team's 512 threads take the
// FPT x (512 >> S) groups of 4 bins of its own buffer: wave w of the team takes frame slot w mod FPT, its lanes sit
// (8 >> S) groups apart (the swizzle's conflict-free read pattern).
// Ring: at k the role-0 team finalises columns j0 + (k-2) FPT - D .. + FPT - 1 (last contributor: block k - 2, scattered
// by that team at k - 1) while the role-1 team scatters block k - 1, which reaches no lower than column
// j0 + (k-1) FPT - D, and no higher than j0 + k FPT - 1 + D: 2 D + 2 FPT slots.
template <int S, bool FAST = false>   // FAST: reassignment ON + log-spaced edges known at compile time (fused_r8.hip.inc)
__global__ __launch_bounds__(1024, 4) void fused_small_pp_kernel(
    PlanDev pl, DbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, int slots, float* __restrict__ db, uint32_t* __restrict__ rgba, uint8_t* __restrict__ index) {
    using namespace f8;   // the 4096-point carrier network: swz, zpos, tw_index8, TwRegsSym, TwLdsSym
    constexpr int NS = 4096 >> S;          // FFT size
    constexpr int FPT = 1 << S;            // frames per team and half-iteration
    constexpr int RPF = 8 >> S;            // sample registers per frame (512 samples each)
    extern __shared__ float4 smem4[];
    const int R = pl.rows, D = pl.D, HOP = pl.hop, SLOTS = slots;
    float2* fbuf = reinterpret_cast<float2*>(smem4);            // [2][4096] complex
    float* ring = reinterpret_cast<float*>(fbuf + 2 * 4096);     // [SLOTS][R]
    float* seb = ring + SLOTS * R;                                // [R+1] (+3 pad)
    uint32_t* slut = reinterpret_cast<uint32_t*>(seb + R + 4);   // [256]
    float2* stwB = reinterpret_cast<float2*>(slut + 256);        // [7][64] pass-B twiddles
    float2* stwC = stwB + 7 * 64;                                 // [7][8]  pass-C twiddles
    unsigned* arrive = reinterpret_cast<unsigned*>(stwC + 7 * 8);   // [2] per-team arrival counters

    const int tid = threadIdx.x, h = tid >> 9, t = tid & 511;
    float2* fb = fbuf + h * 4096;
    int s;
    int64_t c0, c1;
    if (!seg_of_block(sp, C, s, c0, c1)) return;
    const int64_t j0 = c0 - D > 0 ? c0 - D : 0;
    const int64_t jstop = c1 + D < C ? c1 + D : C;              // frames j0 .. jstop-1 can reach this segment
    const float* x0 = pcm + (size_t)s * L;

    // ---- workgroup set-up (pl.tw is the NS-point table: carrier index >> S)
    for (int q = tid; q < SLOTS * R / 4; q += 1024) reinterpret_cast<float4*>(ring)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = tid; r <= R; r += 1024) seb[r] = pl.ebin[r];
    if (tid < 256) slut[tid] = lut[tid];
    if (tid < 7 * 64) stwB[tid] = pl.tw[tw_index8<3>(tid >> 6, tid & 63) >> S];
    else if (tid < 7 * 64 + 7 * 8) stwC[tid - 7 * 64] = pl.tw[tw_index8<6>((tid - 7 * 64) >> 3, (tid - 7 * 64) & 7) >> S];
    else if (tid < 7 * 64 + 7 * 8 + 2) arrive[tid - (7 * 64 + 7 * 8)] = 0u;
    float2 twA[7];   // only the slots of stages S..2 are used
#pragma unroll
    for (int e = 0; e < 7; ++e) twA[e] = (e >= (S == 0 ? 0 : (S == 1 ? 4 : 6))) ? pl.tw[tw_index8<0>(e, t) >> S] : make_float2(0.f, 0.f);
    const float r0 = (float)(t - NS / 2) * (2.0f / (float)NS);   // ramp of a frame's register 0; register ii adds ii*1024/NS
    HintLookup lk;
    lk.init(seb, pl.ebin, R, pl.log_rows);
    // this thread's bins: frame slot bf of its team's block, group bg of 4 bins
    const int bf = (t >> 6) & (FPT - 1);
    const int bg = ((t & 63) << (3 - S)) | (t >> (6 + S));
    const int bpart = fsm::brev_s<S>(bf);                          // low bits of the carrier index
    int fpos[6], mpos[6];     // positions of Z[4g-1+i] and Z[NS-4g+1-i] of that frame
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        fpos[i] = zpos((((4 * bg - 1 + i) & (NS - 1)) << S) | bpart);
        mpos[i] = zpos((((NS - 4 * bg + 1 - i) & (NS - 1)) << S) | bpart);
    }
    // samples of block b (frames j0 + b FPT + f): register i holds sample tq + 512 (i mod RPF) of frame f = i / RPF
    auto load_block = [&](int64_t b, float (&x)[8], int tq) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t j = j0 + b * FPT + (i / RPF);
            const int64_t idx = j * HOP + tq + 512 * (i % RPF);
            x[i] = (j < jstop && idx < L) ? x0[idx] : 0.0f;
        }
    };
    auto pass_a = [&](float2 (&v)[8], const float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = make_float2(x[i], x[i] * (r0 + (float)(i % RPF) * (1024.0f / (float)NS)));
        fsm::stages8_from<S>(v, TwRegsSym{twA});
    };
    // both teams write pass A of their first block (block h) before the loop
    {
        float x[8];
        float2 v[8];
        load_block(h, x, t);
        pass_a(v, x);
        if (j0 + (int64_t)h * FPT < jstop) {
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(t) ^ cswz(512 * i)] = v[i];
        }
    }
    // q / qpc for the finalize loop as a multiply: m = ceil(2^20 / qpc) gives floor(q / qpc) = (q m) >> 20 for q (m qpc - 2^20)
    // < 2^20, i.e. for every q < 4096 here (qpc <= 256); hipcc's signed division is ~17 instructions, two of them quarter rate
    const unsigned qmagic = ((1u << 20) + (unsigned)(R >> 2) - 1u) / (unsigned)(R >> 2);
    // half-iterations k = 0 .. klast: column c1 - 1 leaves at the first k with j0 + (k-1) FPT - 1 - D >= c1 - 1.  Team h runs
    // the pairs (k, k + 1), k = h, h + 2, ..: P pairs and 2P + 1 workgroup barriers for both teams (fused_pp.hip.inc)
    const int klast = (int)((c1 + D - j0 + FPT - 1) / FPT) + 1;
    const int P = (klast + 2) >> 1;
    int sk = (int)((j0 + (int64_t)h * FPT) % SLOTS);   // ring slot of column j0 + k FPT
    unsigned arrivals = 0;                              // role-0 visits of this team so far x 8 waves = the counter's target
    __syncthreads();
    if (h) __syncthreads();
    int k = h;
#pragma unroll 1
    for (int p = 0; p < P; ++p, k += 2) {
        int tt = t;
        asm volatile("" : "+v"(tt));
        float yr[6], yi[6], ur[6], tr[6];   // the split spectra at the thread's six positions: role 0 -> role 1
        // ================= role 0 at half-iteration k: passes B, C, D of block k, finalise, spectrum reads
        if (j0 + (int64_t)k * FPT < jstop) {
            float2 v[8];
            // pass B = carrier stages 3..5 : p = hi*512 + i*64 + lo   (wave-local from here on)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz(((tt >> 6) << 9) + (tt & 63)) ^ cswz(i << 6)];
            stages8(v, TwLdsSym<64>{stwB + (tt & 63)});
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(((tt >> 6) << 9) + (tt & 63)) ^ cswz(i << 6)] = v[i];
            wave_lds_sync();
            // pass C = stages 6..8 : p = hi*64 + i*8 + lo
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz(((tt >> 3) << 6) + (tt & 7)) ^ cswz(i << 3)];
            stages8(v, TwLdsSym<8>{stwC + (tt & 7)});
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(((tt >> 3) << 6) + (tt & 7)) ^ cswz(i << 3)] = v[i];
            wave_lds_sync();
            // pass D = stages 9..11 of the carrier = the last three stages of the NS-point network
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz(tt << 3) ^ i];
            fft_stages<12 - S, 9 - S, 3>(v, 0, pl.tw);
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(tt << 3) ^ i] = v[i];
        }
        // this wave's pass-D stores are issued (in-order LDS pipe): tell the team
        asm volatile("" ::: "memory");
        if ((tt & 63) == 0) __hip_atomic_fetch_add(arrive + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm volatile("" ::: "memory");
        arrivals += 8;
        {   // columns j0+(k-2)FPT-D .. +FPT-1 can no longer be reached: finalise, store, clear
            const int qpc = R >> 2;   // float4 quads per column
            for (int q = tt; q < FPT * qpc; q += 512) {
                const int cc = (int)(__umul24((unsigned)q, qmagic) >> 20);   // q / qpc (exact: q <= 1024, see qmagic)
                const int cell = (q - cc * qpc) << 2;
                const int64_t col = j0 + (int64_t)(k - 2) * FPT - D + cc;
                if (col >= c0 && col < c1) {
                    int sl = sk - 2 * FPT - D + cc;
                    sl += sl < 0 ? SLOTS : 0;
                    finalize_ring_quad(ring, sl, R, cell, dm, slut, ((size_t)s * C + col) * R + cell, db, rgba, index);
                }
            }
        }
        // the block's spectra are complete once all eight waves of the team have stored their pass D
        // (bounded: 2^16 polls is ~2 ms, far beyond any legitimate wait - a protocol error must fail a test, not hang)
        for (unsigned spins = 0; (int)(__hip_atomic_load(arrive + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - arrivals) < 0; ++spins) {
            if (spins >= (1u << 16)) { g_kernel_error = 1; break; }   // reported by emspec_device_status: the results are invalid
            __builtin_amdgcn_s_sleep(1);
        }
        asm volatile("" ::: "memory");
        read_split6(fb, fpos, mpos, yr, yi, ur, tr);   // all twelve reads issued before the first use
        __syncthreads();
        // ================= role 1 at half-iteration k + 1: bins + scatter of block k, samples + pass A of block k + 2, its write
        {
            const int64_t j = j0 + (int64_t)k * FPT + bf;             // this thread's bins belong to frame j
            float xn[8];
            load_block(k + 2, xn, tt);
            if (j < jstop) {
                __builtin_amdgcn_s_setprio(2);
                int sbase = sk + bf - D;                   // ring slot of column j-D
                sbase -= sbase >= SLOTS ? SLOTS : 0;
                sbase += sbase < 0 ? SLOTS : 0;
                const int jrel = (int)(j - c0);
                const unsigned span = (unsigned)(c1 - c0);
                const float Df = (float)D;
                const float kf0 = (float)(4 * (((tt & 63) << (3 - S)) | (tt >> (6 + S))));
                float* cellp[4];
                float pw[4];
                bool okv[4];
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
                    int d = D;
                    if (FAST || pl.reassign) {
                        const float numT = __builtin_fmaf(Br, Ar, -(Ui * Ai));
                        const float numF = __builtin_fmaf(Dr, Ar, Di * Ai);
                        const float inv = FAST ? recip_normal(den) : 1.0f / den;
                        const float cf = __builtin_floorf(__builtin_fmaf(numT * inv, pl.tscale, 0.5f));
                        ok = ok && (__builtin_fabsf(cf) <= Df);
                        d = (int)cf + D;
                        kh = kf + numF * inv;
                    }
                    const int rr = FAST ? lk.row_signed_log(kh) : lk.row_signed(kh);   // -1 / R when k-hat is off the frequency axis
                    ok = ok && ((unsigned)rr < (unsigned)R);
                    ok = ok && ((unsigned)(jrel + d - D) < span);
                    unsigned sl = (unsigned)(sbase + d);   // garbage when !ok: the cell is then never touched
                    sl = min(sl, sl - (unsigned)SLOTS);
                    cellp[e] = ring + __umul24(sl, (unsigned)R) + rr;
                    pw[e] = Pw;
                    okv[e] = ok;
                }
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const bool same = okv[e] && okv[e + 1] && (cellp[e] == cellp[e + 1]);
                    pw[e + 1] = same ? pw[e + 1] + pw[e] : pw[e + 1];
                    okv[e] = okv[e] && !same;
                }
                lds_accumulate(cellp[0], pw[0], okv[0]);
                lds_accumulate(cellp[1], pw[1], okv[1]);
                __builtin_amdgcn_s_setprio(1);
                lds_accumulate(cellp[2], pw[2], okv[2]);
                lds_accumulate(cellp[3], pw[3], okv[3]);
                __builtin_amdgcn_s_setprio(0);
            }
            float2 v[8];
            pass_a(v, xn);                              // block k+2 of this team, in registers
            if (j0 + (int64_t)(k + 2) * FPT < jstop) {  // the team read this buffer's spectra before the barrier above: it is free
#pragma unroll
                for (int i = 0; i < 8; ++i) fb[swz(tt) ^ cswz(512 * i)] = v[i];
            }
        }
        __syncthreads();
        sk += 2 * FPT;
        sk -= sk >= SLOTS ? SLOTS : 0;
    }
    if (!h) __syncthreads();
}

// (ring slots the kernel needs for reach D, and the dynamic LDS that takes: fused_small_slots, fused_small_lds_bytes,
// emspec_kernel_plan.h)

}  // namespace emspec
