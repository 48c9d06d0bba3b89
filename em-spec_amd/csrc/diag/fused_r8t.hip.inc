// fused_r8t.hip.inc — fused batch kernel, 1024 threads, DECOUPLED TEAMS.  Included by kernels.hip.
//
// Same arithmetic, data layout and LDS images as fused4096_r8_kernel (fused_r8.hip.inc), but the
// two 8-wave teams of the workgroup (team 0: even frames, team 1: odd frames) no longer share
// barriers.  Each team synchronises on its own LDS arrival counter (team_barrier), so while one
// team waits or streams LDS the other owns the VALU issue slots.  The teams meet only at the ring:
//   - team h finalises the column its own frame completes (column j-8) after the OTHER team has
//     finished scattering every frame that can reach it (wait on the other team's barrier count);
//   - a ring slot freed by the other team (column j-11) must be clear before this team scatters
//     frame j (wait on the other team's finalise count); slots freed by the team itself are ordered
//     by program order.
// Every wait is a bounded spin (s_sleep between polls); a timeout raises *errflag and the wave
// carries on, so a protocol bug shows up as a failed test, never as a hang.
namespace emspec {

namespace f8t {
constexpr unsigned SPIN_LIMIT = 1u << 18;   // ~0.03 s of polling: far beyond any legitimate wait
// wrap-safe "counter >= target"
__device__ __forceinline__ void wait_ge(const unsigned* ctr, unsigned target, int* errflag, bool& dead) {
    unsigned spins = 0;
    if (dead) return;     // after one timeout this wave stops waiting altogether: the launch drains quickly
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - target) < 0) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > SPIN_LIMIT) { *errflag = 1; dead = true; break; }
    }
}
// barrier among the 8 waves of one team: arrive (one lane per wave), then poll.  The LDS pipe is
// in-order per wave, so a wave's earlier LDS writes are performed before its arrival is.
__device__ __forceinline__ void team_barrier(unsigned* ctr, unsigned& target, int* errflag, bool& dead) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    target += 8;
    if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    wait_ge(ctr, target, errflag, dead);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
}  // namespace f8t

#define EMSPEC_STAMP(slot)                                                        \
    if constexpr (STAMP) {                                                        \
        const unsigned long long now_ = __builtin_readcyclecounter();             \
        acc_[slot] += now_ - last_;                                               \
        last_ = now_;                                                             \
    }
template <bool STAMP>
__global__ __launch_bounds__(1024, 4) void fused4096_r8t_kernel(
    PlanDev pl, DbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, float* __restrict__ db, uint32_t* __restrict__ rgba, uint8_t* __restrict__ index,
    unsigned long long* __restrict__ stamps, int* __restrict__ errflag) {
    using namespace f8;
    constexpr int HOP = 256, DMAX = Geo<HOP>::DMAX, SLOTS = Geo<HOP>::SLOTS;   // this variant: hop 256 only
    using namespace f8t;
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
    unsigned* ctrs = reinterpret_cast<unsigned*>(stwC + 7 * 8);   // [0..1] team barrier counts, [2..3] finalise counts

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
    if (tid < 4) ctrs[tid] = 0u;
    if (tid < 7 * 64) stwB[tid] = pl.tw[tw_index8<3>(tid >> 6, tid & 63)];
    else if (tid < 7 * 64 + 7 * 8) stwC[tid - 7 * 64] = pl.tw[tw_index8<6>((tid - 7 * 64) >> 3, (tid - 7 * 64) & 7)];
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
    // bin groups dealt to threads so the lanes of one instruction are 32 bins apart (see fused_r8.hip.inc)
    const int bg = ((t & 63) << 3) | (t >> 6);
    int fpos[6], mpos[6];     // positions of Z[4g-1+i] and Z[N-4g+1-i] in the in-place buffer
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        fpos[i] = zpos((4 * bg - 1 + i) & (N - 1));
        mpos[i] = zpos((N - 4 * bg + 1 - i) & (N - 1));
    }
    int sj_even = (int)(j0 % SLOTS);
    __syncthreads();      // the only workgroup-wide barrier: ring, tables and counters are ready
    if constexpr (STAMP) last_ = __builtin_readcyclecounter();
    unsigned* myBar = ctrs + h;             // arrivals at this team's barriers (3 per iteration, 8 waves each)
    unsigned* otherBar = ctrs + (1 - h);
    unsigned* myFin = ctrs + 2 + h;         // waves of this team that finished finalising (8 per iteration)
    unsigned* otherFin = ctrs + 2 + (1 - h);
    unsigned bar_target = 0, it = 0;
    bool dead = false;

    // pass A (pack z = x + j*ramp*x, stages 0..2) is software-pipelined: it is register-only, so it is
    // computed for the NEXT frame before the barrier that ends an iteration (filling barrier wait)
    float2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.25f * (float)i));
    stages8(v, TwRegs{twA});
#pragma unroll 1
    for (int64_t jb = j0; jb < jstop; jb += 2) {
        const int64_t j = jb + h;
        const bool active = j < C;
        const int64_t nx = (j + 16) * HOP + t;       // = (j+2)*HOP + t + 512*7
        // Launder t once per iteration: every LDS address below is then recomputed (1-3 VALU
        // each) instead of being hoisted out of the loop, which would pin ~50 VGPRs.
        int tt = t;
        asm volatile("" : "+v"(tt));
        const float xn = nx < L ? x0[nx] : 0.0f;

        if (active) {
            // pass A results were computed in registers before the previous iteration's last barrier
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(tt + T * i)] = v[i];
        }
        EMSPEC_STAMP(0)
        team_barrier(myBar, bar_target, errflag, dead);     // T1: pass A of this frame is in LDS
        EMSPEC_STAMP(1)
        if (active) {
            __builtin_amdgcn_s_setprio(3);   // progress-based priority: a wave that is behind outranks one ahead
            // pass B = stages 3..5 : p = hi*512 + i*64 + lo
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[posB[i]];
            stages8(v, TwLds<64>{stwB + (tt & 63)});
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[posB[i]] = v[i];
            wave_lds_sync();
        }
        EMSPEC_STAMP(2)
        if (active) {
            __builtin_amdgcn_s_setprio(2);
            // pass C = stages 6..8 : p = hi*64 + i*8 + lo   (same wave's sub-FFT)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[posC[i]];
            stages8(v, TwLds<8>{stwC + (tt & 7)});
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[posC[i]] = v[i];
            wave_lds_sync();
        }
        EMSPEC_STAMP(3)
        if (active) {
            __builtin_amdgcn_s_setprio(1);
            // pass D = stages 9..11 : p = 8*t + i, in place; Z[k] ends at position bitrev12(k)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz((tt << 3) + i)];
            fft_stages<LOG2N, 9, 3>(v, 0, pl.tw);
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz((tt << 3) + i)] = v[i];
            __builtin_amdgcn_s_setprio(0);
        }
        EMSPEC_STAMP(4)
        team_barrier(myBar, bar_target, errflag, dead);     // T2: the whole spectrum of this frame is in LDS
        // ring slot reuse: the slot of column j-11 (freed by the other team, at its frame j-3) is about
        // to be hit as column j+7; the other team must have finished that finalise
        {
            const unsigned need = h ? 8u * it : (it > 0 ? 8u * (it - 1) : 0u);
            wait_ge(otherFin, need, errflag, dead);
        }
        EMSPEC_STAMP(1)
        if (active) {
            // per-bin stages: bins 4t .. 4t+3 from F(i) = Z[4t-1+i], M(i) = Z[N-4t+1-i], i = 0..5
            // (positions hoisted out of the frame loop: they depend on t only).  Branch-free and
            // unrolled so the four bins' dependency chains (spectrum read -> reassign -> edge-table
            // read -> accumulate) overlap; one predicate per bin guards the accumulate.
            // The Nyquist bin k = N/2 is not visited: Y[N/2+1] = conj Y[N/2-1] makes its k-shift
            // exactly 0 in this arithmetic, so k-hat = N/2 >= ebin[R] (fmax <= fs/2 is enforced by
            // emspec_create) and it can never reach the histogram.  Skipping it keeps the 8 waves
            // of a frame at equal work.  (frames_kernel still reports it in the parity dump.)
            __builtin_amdgcn_s_setprio(3);
            float yr[6], yi[6], ur[6], tr[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const float2 f = fb[fpos[i]], m = fb[mpos[i]];
                yr[i] = f.x + m.x; yi[i] = f.y - m.y; ur[i] = f.x - m.x; tr[i] = f.y + m.y;   // ur = -Ti
            }
            int sbase = sj_even + h - DMAX;            // ring slot of column j-8
            sbase += sbase < 0 ? SLOTS : 0;
            const int jrel = (int)(j - c0);
            const unsigned span = (unsigned)(c1 - c0);
            const float Df = (float)D;
            const float kf0 = (float)(4 * (((tt & 63) << 3) | (tt >> 6)));
            float* cellp[4];
            float pw[4];
            bool okv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float Ar = (yr[e + 1] + yr[e + 1]) - (yr[e] + yr[e + 2]), Ai = (yi[e + 1] + yi[e + 1]) - (yi[e] + yi[e + 2]);
                const float Br = (tr[e + 1] + tr[e + 1]) - (tr[e] + tr[e + 2]), Ui = (ur[e + 1] + ur[e + 1]) - (ur[e] + ur[e + 2]);
                const float Dr = yr[e] - yr[e + 2], Di = yi[e] - yi[e + 2];
                const float den = __builtin_fmaf(Ar, Ar, Ai * Ai);
                const float P = den * 0.015625f;
                bool ok = (P >= pl.pfloor_abs) && (P <= kPowerMax);
                const float kf = kf0 + (float)e;
                float kh = kf;
                int d = DMAX;
                if (pl.reassign) {
                    const float numT = __builtin_fmaf(Br, Ar, -(Ui * Ai));
                    const float numF = __builtin_fmaf(Dr, Ar, Di * Ai);
                    const float inv = 1.0f / den;
                    const float cf = __builtin_floorf(__builtin_fmaf(numT * inv, pl.tscale, 0.5f));
                    ok = ok && (__builtin_fabsf(cf) <= Df);
                    d = (int)cf + DMAX;
                    kh = kf + numF * inv;
                }
                ok = ok && lk.in_range(kh);
                const int rr = lk.row_unchecked(kh);
                ok = ok && ((unsigned)(jrel + d - DMAX) < span);
                unsigned sl = (unsigned)(sbase + (ok ? d : 0));
                sl = min(sl, sl - (unsigned)SLOTS);
                cellp[e] = ring + __umul24(sl, (unsigned)R) + rr;   // 24-bit multiply: full rate (v_mul_lo_u32 is quarter rate)
                pw[e] = P;
                okv[e] = ok;
            }
            // a lane's consecutive bins often share a cell: sum such runs in registers first
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const bool same = okv[e] && okv[e + 1] && (cellp[e] == cellp[e + 1]);
                pw[e + 1] = same ? pw[e + 1] + pw[e] : pw[e + 1];
                okv[e] = okv[e] && !same;
            }
            lds_accumulate(cellp[0], pw[0], okv[0]);
            __builtin_amdgcn_s_setprio(2);
            lds_accumulate(cellp[1], pw[1], okv[1]);
            __builtin_amdgcn_s_setprio(1);
            lds_accumulate(cellp[2], pw[2], okv[2]);
            lds_accumulate(cellp[3], pw[3], okv[3]);
            __builtin_amdgcn_s_setprio(0);
        }
        // next frame of this half: shift the sample registers by one (two hops) and run its pass A
#pragma unroll
        for (int i = 0; i < 7; ++i) xs[i] = xs[i + 1];
        xs[7] = xn;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.25f * (float)i));
        stages8(v, TwRegs{twA});
        EMSPEC_STAMP(5)
        team_barrier(myBar, bar_target, errflag, dead);     // T3: this team's scatter of frame j is complete
        // ---- column j-D can no longer be reached once the other team has scattered every frame <= j:
        // team 0 (j = jb) needs the other team's previous iteration, team 1 (j = jb+1) team 0's current one
        wait_ge(otherBar, h ? 8u * (3u * it + 3u) : 8u * 3u * it, errflag, dead);
        EMSPEC_STAMP(1)
        {
            const int qpc = R >> 2;   // float4 quads per column
            const int64_t col = j - D;
            int sl = sj_even + h - D;
            sl += sl < 0 ? SLOTS : 0;
            sl -= sl >= SLOTS ? SLOTS : 0;
            if (col >= c0 && col < c1) {
                for (int q = tt; q < qpc; q += 512) {
                    const int cell = q << 2;
                    finalize_ring_quad(ring, sl, R, cell, dm, slut, ((size_t)s * C + col) * R + cell, db, rgba, index);
                }
            }
            // every wave reports, whether or not it had cells: 8 per iteration
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if ((tid & 63) == 0) __hip_atomic_fetch_add(myFin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        ++it;
        sj_even += 2;
        sj_even -= sj_even >= SLOTS ? SLOTS : 0;
        EMSPEC_STAMP(6)
    }
    if constexpr (STAMP) {
        if ((tid & 63) == 0) {
            unsigned long long* o = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (tid >> 6)) * 8;
            for (int i = 0; i < 8; ++i) o[i] = acc_[i];
        }
    }
}
#undef EMSPEC_STAMP

static size_t fused_r8t_lds_bytes(int rows) {
    return (size_t)2 * f8::N * sizeof(float2) + (size_t)f8::Geo<256>::SLOTS * rows * 4 + (size_t)(rows + 4) * 4 + 1024 +
           (size_t)(7 * 64 + 7 * 8) * sizeof(float2) + 64;
}

}  // namespace emspec
