// diag/fused_pp3.hip.inc — the round-3 form of fused4096_pp_kernel (the product kernel of rounds 3 and 4 until the
// spectrum reads moved into role 0, fused_pp.hip.inc), kept as A/B variants "pp3" and - with per-team software barriers
// instead of the workgroup barrier - "ppt".  Same arithmetic, LDS images and ring schedule as the product kernel:
//     role 0 (k + h even): finalise one column, passes B, C, D of frame j0 + k        (LDS-heavy)
//     role 1 (k + h odd) : spectrum reads, bins + scatter of frame j0 + k - 1, pass A of frame j0 + k + 1 and its write
// One workgroup barrier per half-iteration; the ordering bins' reads -> the next frame's pass-A write into the same
// buffer is an arrival counter in LDS.  Measured against the product kernel (round 4, A/B on one box): 9.32 vs 9.02 ms.
namespace emspec {

#define EMSPEC_STAMP(slot)                                                        \
    if constexpr (STAMP) {                                                        \
        const unsigned long long now_ = __builtin_readcyclecounter();             \
        acc_[slot] += now_ - last_;                                               \
        last_ = now_;                                                             \
    }
template <int HOP, bool STAMP, bool FAST = false, bool TEAMSYNC = false>
__global__ __launch_bounds__(1024, 4) void fused4096_pp3_kernel(
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
    unsigned* arrive = reinterpret_cast<unsigned*>(stwC + 7 * 8);   // [2] per-team arrival counters
    unsigned* bar = arrive + 2;                                     // [2] per-team barrier counters (TEAMSYNC)

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
    int sk = (int)(j0 % SLOTS);          // ring slot of column j0 + k
    unsigned arrivals = 0;               // role-1 visits of this team so far (x 8 waves = the counter's target)
    __syncthreads();
    unsigned long long real0_ = 0;
    if constexpr (STAMP) { last_ = __builtin_readcyclecounter(); real0_ = __builtin_amdgcn_s_memrealtime(); }

    // half-iterations k = 0 .. klast: the last column c1-1 is finalised at k = c1 - 1 + 2 + D - j0
    const int klast = (int)(c1 + 1 + D - j0);
#pragma unroll 1
    for (int k = 0; k <= klast; ++k) {
        // Launder t once per half-iteration: every LDS address below is then recomputed (1-3 VALU each) instead of
        // being hoisted out of the loop, which would pin ~50 VGPRs.
        int tt = t;
        asm volatile("" : "+v"(tt));
        if (((k + h) & 1) == 0) {
            // ================= role 0: finalise column j0+k-2-D, passes B, C, D of frame j0+k
            const int64_t j = j0 + k;
            const bool active = j < C && j < jstop;
            {
                const int qpc = R >> 2;   // float4 quads per column
                const int64_t col = j - 2 - D;
                if (t < qpc && col >= c0 && col < c1) {
                    const int cell = t << 2;
                    int sl = sk - 2 - D;
                    sl += sl < 0 ? SLOTS : 0;
                    finalize_ring_quad(ring, sl, R, cell, dm, slut, ((size_t)s * C + col) * R + cell, db, rgba, index);
                }
            }
            EMSPEC_STAMP(0)
            if (active) {
                float2 v[8];
                // pass B = stages 3..5 : p = hi*512 + i*64 + lo
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = fb[posB[i]];
                stages8(v, TwLdsSym<64>{stwB + (tt & 63)});
#pragma unroll
                for (int i = 0; i < 8; ++i) fb[posB[i]] = v[i];
                wave_lds_sync();
                // pass C = stages 6..8 : p = hi*64 + i*8 + lo   (same wave's sub-FFT)
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = fb[posC[i]];
                stages8(v, TwLdsSym<8>{stwC + (tt & 7)});
#pragma unroll
                for (int i = 0; i < 8; ++i) fb[posC[i]] = v[i];
                wave_lds_sync();
                // pass D = stages 9..11 : p = 8*t + i, in place; Z[k] ends at position bitrev12(k)
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = fb[swz((tt << 3) + i)];
                fft_stages<LOG2N, 9, 3>(v, 0, pl.tw);
#pragma unroll
                for (int i = 0; i < 8; ++i) fb[swz((tt << 3) + i)] = v[i];
            }
            EMSPEC_STAMP(1)
        } else {
            // ================= role 1: bins + scatter of frame j0+k-1, pass A of frame j0+k+1 and its write
            const int64_t j = j0 + k - 1;                      // team 1 at k = 0: frame j0-1 does not exist
            const bool active = k >= 1 && j < C && j < jstop;
            const int64_t jn = j + 2;
            const bool next = k >= 1;                          // (team 1 wrote frame j0+1 before the loop)
            const int64_t nx = jn * HOP + t + 512 * (8 - SH);  // first new sample register of frame jn
            float xn[SH];
#pragma unroll
            for (int q = 0; q < SH; ++q) xn[q] = (next && nx + 512 * q < L) ? x0[nx + 512 * q] : 0.0f;
            float* cellp[4];
            float pw[4];
            bool okv[4] = {false, false, false, false};
            if (active) {
                // per-bin stages: bins 4g .. 4g+3 from F(i) = Z[4g-1+i], M(i) = Z[N-4g+1-i], i = 0..5 (fused_r8.hip.inc)
                __builtin_amdgcn_s_setprio(2);
                float yr[6], yi[6], ur[6], tr[6];
                read_split6(fb, fpos, mpos, yr, yi, ur, tr);   // all twelve reads issued before the first use
                // this wave's reads of the frame buffer are done (the LDS pipe serves one wave's operations in order, so
                // the counter moves after them): tell the team
                asm volatile("" ::: "memory");
                if ((tt & 63) == 0) __hip_atomic_fetch_add(arrive + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                asm volatile("" ::: "memory");
                int sbase = sk - 1 - DMAX;                 // ring slot of column j-DMAX
                sbase += sbase < 0 ? SLOTS : 0;
                const int jrel = (int)(j - c0);
                const unsigned span = (unsigned)(c1 - c0);
                const float Df = (float)D;
                const float kf0 = (float)(4 * (((tt & 63) << 3) | (tt >> 6)));
                bins4<FAST>(pl.pfloor_abs, pl.reassign, pl.tscale, lk, yr, yi, ur, tr, kf0, sbase, jrel, span, Df, ring, R, DMAX, SLOTS, cellp, pw, okv);   // fused_common.hip.inc
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
                EMSPEC_STAMP(3)
            } else {
                if ((tt & 63) == 0) __hip_atomic_fetch_add(arrive + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            arrivals += 8;
            if (next) {
                // next frame of this team: shift the sample registers by one (two hops), run its pass A in registers
#pragma unroll
                for (int i = 0; i < 8 - SH; ++i) xs[i] = xs[i + SH];
#pragma unroll
                for (int q = 0; q < SH; ++q) xs[8 - SH + q] = xn[q];
                float2 v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.25f * (float)i));
                stages8(v, TwRegsSym{twA});
                EMSPEC_STAMP(4)
                // the frame buffer may be overwritten once all eight waves of the team have read their bins
                // (bounded: 2^16 polls is ~2 ms, far beyond any legitimate wait - a protocol error must fail a test, not hang)
                for (unsigned spins = 0; (int)(__hip_atomic_load(arrive + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - arrivals) < 0; ++spins) {
                    if (spins >= (1u << 16)) { g_kernel_error = 1; break; }   // reported by emspec_device_status: the results are invalid
                    __builtin_amdgcn_s_sleep(1);
                }
                asm volatile("" ::: "memory");
                EMSPEC_STAMP(5)
                if (jn < C && jn < jstop) {
                    float2* const w0 = fb + swz(tt);
                    float2* const w1 = fb + (swz(tt) ^ 8);
#pragma unroll
                    for (int i = 0; i < 8; ++i) ((i & 1) ? w1 : w0)[T * i] = v[i];
                }
            }
        }
        if constexpr (TEAMSYNC) {
            // team barrier: this wave's LDS operations are issued (in-order pipe), so the counter moves after them; then
            // wait until the eight waves of the team have finished half-iteration k AND the other team has finished k - 1
            // (its scatter at k - 1 is the second-to-last contributor of the column this team may finalise at k + 1)
            asm volatile("" ::: "memory");
            if ((tt & 63) == 0) __hip_atomic_fetch_add(bar + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned mine = 8u * (unsigned)(k + 1), theirs = 8u * (unsigned)k;
            for (unsigned spins = 0; spins < (1u << 16); ++spins) {
                const unsigned a = __hip_atomic_load(bar + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const unsigned b = __hip_atomic_load(bar + (h ^ 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if ((int)(a - mine) >= 0 && (int)(b - theirs) >= 0) break;
                __builtin_amdgcn_s_sleep(1);
            }
            asm volatile("" ::: "memory");
        } else {
            __syncthreads();
        }
        EMSPEC_STAMP(6)
        sk += 1;
        sk -= sk >= SLOTS ? SLOTS : 0;
    }
    if constexpr (STAMP) {
        if ((tid & 63) == 0) {
            unsigned long long* o = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (tid >> 6)) * 8;
            acc_[7] = (acc_[7] & 0xFFFFFFFFull) | ((__builtin_amdgcn_s_memrealtime() - real0_) << 32);
            for (int i = 0; i < 8; ++i) o[i] = acc_[i];
        }
    }
}
#undef EMSPEC_STAMP

}  // namespace emspec
