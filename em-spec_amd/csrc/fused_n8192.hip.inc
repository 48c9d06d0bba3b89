// fused_n8192.hip.inc — fused batch kernel for N = 8192 on the skeleton of fused_r8.hip.inc.
// Included by kernels.hip after fused_r8.hip.inc (it reuses f8::swz / zpos / stages8 / TwLdsSym).  Its finalize and spectrum
// split are spelled out here, in the order of fused_common.hip.inc's finalize_ring_quad and read_split6, and its four-bin
// stage in the order fused_pp.hip.inc's header gives (Hann identities, power gate, reassignment, row lookup, segment test,
// ring slot, then the run sums).  Calling shared functions for them rescheduled this kernel
// (profiles/refactor_fused_common_isa.txt), so that waits for an A/B measurement.
//
// The first stage of the canonical radix-2 DIF network splits an 8192-point frame into two
// independent 4096-point transforms:
//     a[n] = z[n] + z[n+4096]                 -> the even bins  Z[2m]   = FFT4096(a)[m]
//     b[n] = (z[n] - z[n+4096]) * W8192^n     -> the odd bins   Z[2m+1] = FFT4096(b)[m]
// which are exactly the two team buffers of the N = 4096 kernel.  Team 0 (threads 0..511)
// transforms a, team 1 transforms b, both of the SAME frame; stages 1..12 of the 8192 network are
// stages 0..11 of a 4096 network whose twiddle table is every second entry of the 8192 table
// (tw8192[2q] and tw4096[q] are the same float: the double argument is identical), so the result
// is bit-identical to the generic kernel's and the oracle's network.  One frame per iteration;
// the per-bin stage runs on all 1024 threads (4 bins each) and reads even bins from buffer 0 and
// odd bins from buffer 1.  Ring: 2D+1 column slots (hop 512: 17, hop 1024: 9); hop 256 would
// need 33 slots and stays on the generic path.  Sample registers: x[j*hop + t + 512 i], i < 16;
// one hop is HOP/512 registers.
namespace emspec {

namespace f13 {
constexpr int N = 8192, M = 4096, T = 512;
template <int HOP>
struct Geo {
    static_assert(HOP == 512 || HOP == 1024, "a hop must be a whole number of 512-sample registers");
    static constexpr int DMAX = N / (2 * HOP), SLOTS = 2 * DMAX + 1;
    static constexpr int SH = HOP / 512;
};
// buffer offset (complex units, both team buffers) of spectrum sample Z[k]
__device__ __forceinline__ int zoff(int k) {
    k &= N - 1;
    return (k & 1) * M + f8::zpos(k >> 1);
}
}  // namespace f13

template <int HOP, bool FAST = false>   // FAST: reassignment ON + log-spaced edges known at compile time (fused_r8.hip.inc)
__global__ __launch_bounds__(1024, 4) void fused8192_kernel(
    PlanDev pl, DbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, float* __restrict__ db, uint32_t* __restrict__ rgba, uint8_t* __restrict__ index) {
    using namespace f8;   // the 4096-point sub-network: swz, zpos, stages8, tw_index8, TwRegsSym, TwLdsSym
    constexpr int N = f13::N, M = f13::M, T = f13::T;
    constexpr int DMAX = f13::Geo<HOP>::DMAX, SLOTS = f13::Geo<HOP>::SLOTS, SH = f13::Geo<HOP>::SH;
    extern __shared__ float4 smem4[];
    const int R = pl.rows, D = pl.D;
    float2* fbuf = reinterpret_cast<float2*>(smem4);            // [2][4096] complex: even bins, odd bins
    float* ring = reinterpret_cast<float*>(fbuf + 2 * M);        // [SLOTS][R]
    float* seb = ring + SLOTS * R;                                // [R+1] (+3 pad)
    uint32_t* slut = reinterpret_cast<uint32_t*>(seb + R + 4);   // [256]
    float2* stwB = reinterpret_cast<float2*>(slut + 256);        // [7][64] pass-B twiddles
    float2* stwC = stwB + 7 * 64;                                 // [7][8]  pass-C twiddles

    const int tid = threadIdx.x, h = tid >> 9, t = tid & 511;
    float2* fb = fbuf + h * M;
    const int hu = __builtin_amdgcn_readfirstlane(h);   // team index as a scalar: branches on it are wave-uniform
    int s;
    int64_t c0, c1;
    if (!seg_of_block(sp, C, s, c0, c1)) return;
    const int64_t j0 = c0 - D > 0 ? c0 - D : 0;
    const int64_t jstop = c1 + D;
    const float* x0 = pcm + (size_t)s * L;

    // ---- workgroup set-up (sub-network twiddles: every second entry of the 8192 table)
    for (int q = tid; q < SLOTS * R / 4; q += 1024) reinterpret_cast<float4*>(ring)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = tid; r <= R; r += 1024) seb[r] = pl.ebin[r];
    if (tid < 256) slut[tid] = lut[tid];
    if (tid < 7 * 64) stwB[tid] = pl.tw[2 * tw_index8<3>(tid >> 6, tid & 63)];
    else if (tid < 7 * 64 + 7 * 8) stwC[tid - 7 * 64] = pl.tw[2 * tw_index8<6>((tid - 7 * 64) >> 3, (tid - 7 * 64) & 7)];
    float2 twA[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) twA[e] = pl.tw[2 * tw_index8<0>(e, t)];
    float xs[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t idx = j0 * HOP + t + 512 * i;
        xs[i] = idx < L ? x0[idx] : 0.0f;
    }
    const float r0 = (float)(t - N / 2) * (2.0f / (float)N);   // ramp of register 0; register i adds i/8 (exact)
    HintLookup lk;
    lk.init(seb, pl.ebin, R, pl.log_rows);
    // Bin groups: 1024 groups of 4 bins over all 16 waves; the lanes of a wave are 16 groups = 64 bins apart
    // (same reasoning as in the N = 4096 kernel; in bit-reversed sub-transform order this is also the
    // conflict-free read pattern of the swizzle).
    const int bg = ((tid & 63) << 4) | (tid >> 6);
    int fpos[6], mpos[6];     // offsets of Z[4g-1+i] and Z[N-4g+1-i] in the two in-place buffers
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        fpos[i] = f13::zoff(4 * bg - 1 + i);
        mpos[i] = f13::zoff(N - 4 * bg + 1 - i);
    }
    int sj = (int)(j0 % SLOTS);   // ring slot of column j
    __syncthreads();

    // stage 0 + pass A (stages 1..3 of the 8192 network = 0..2 of the sub-network) are register-only
    // and are computed for the NEXT frame before the barrier that ends an iteration.
    float2 v[8];
    auto first_pass = [&](int tq) {
        if (hu == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float2 lo = make_float2(xs[i], xs[i] * (r0 + 0.125f * (float)i));
                const float2 hi = make_float2(xs[i + 8], xs[i + 8] * (r0 + 0.125f * (float)(i + 8)));
                v[i] = cadd(lo, hi);
            }
        } else {
            float2 w0[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) w0[i] = pl.tw[tq + 512 * i];   // W8192^n, n = t + 512 i  (L1/L2 resident)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float2 lo = make_float2(xs[i], xs[i] * (r0 + 0.125f * (float)i));
                const float2 hi = make_float2(xs[i + 8], xs[i + 8] * (r0 + 0.125f * (float)(i + 8)));
                v[i] = cmul_tw(csub(lo, hi), w0[i]);
            }
        }
        stages8(v, TwRegsSym{twA});
    };
    // stage "dB + colour" for a column no later frame reaches: dB, palette index, optional RGBA, slot cleared.  It runs one
    // iteration late, after the write barrier and beside the other waves' pass B (the slot is not touched again before
    // that iteration's scatter, which the pass-D barrier orders behind it): straight after the scatter barrier only 4 of
    // the 16 waves had work and the rest of the workgroup waited for them.
    auto finalize = [&](int64_t col, int slot_of_col, int tq) {
        const int qpc = R >> 2;   // float4 quads per column
        if (tq < qpc && col >= c0 && col < c1) {
            const int cell = tq << 2;
            int sl = slot_of_col;
            sl += sl < 0 ? SLOTS : 0;
            float4* cq = reinterpret_cast<float4*>(ring + __umul24((unsigned)sl, (unsigned)R) + cell);
            const float4 e4 = *cq;
            *cq = make_float4(0.f, 0.f, 0.f, 0.f);
            const float d0 = cell_db_fast(dm, e4.x), d1 = cell_db_fast(dm, e4.y);
            const float d2 = cell_db_fast(dm, e4.z), d3 = cell_db_fast(dm, e4.w);
            const int i0 = cell_index(dm, d0), i1 = cell_index(dm, d1), i2 = cell_index(dm, d2), i3 = cell_index(dm, d3);
            const size_t o = ((size_t)s * C + col) * R + cell;
            if (db) *reinterpret_cast<float4*>(db + o) = make_float4(d0, d1, d2, d3);
            if (rgba) *reinterpret_cast<uint4*>(rgba + o) = make_uint4(slut[i0], slut[i1], slut[i2], slut[i3]);
            if (index) *reinterpret_cast<uint32_t*>(index + o) =
                (uint32_t)i0 | ((uint32_t)i1 << 8) | ((uint32_t)i2 << 16) | ((uint32_t)i3 << 24);
        }
    };
    first_pass(t);
#pragma unroll 1
    for (int64_t j = j0; j < jstop; ++j) {
        const bool active = j < C;
        const int64_t nx = (j + 1) * HOP + t + 512 * (16 - SH);   // first new sample register of frame j+1
        // Launder the thread ids once per iteration: LDS addresses below are then cheap recomputations
        // instead of ~50 hoisted VGPRs (see fused_r8.hip.inc).
        int tt = t, tw_ = tid;
        asm volatile("" : "+v"(tt));
        asm volatile("" : "+v"(tw_));
        float xn[SH];
#pragma unroll
        for (int q = 0; q < SH; ++q) xn[q] = nx + 512 * q < L ? x0[nx + 512 * q] : 0.0f;

        if (active) {
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(tt) ^ cswz(T * i)] = v[i];   // swz(P + (i << b)) = swz(P) ^ cswz(i << b), fused_r8.hip.inc
        }
        __syncthreads();
        finalize(j - 1 - D, sj - 1 - D, tw_);          // the column the previous frame completed
        if (active) {
            __builtin_amdgcn_s_setprio(3);   // progress-based priority: a wave that is behind outranks one ahead
            // pass B = sub-network stages 3..5 : p = hi*512 + i*64 + lo   (wave-local from here on)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz(((tt >> 6) << 9) + (tt & 63)) ^ cswz(i << 6)];
            stages8(v, TwLdsSym<64>{stwB + (tt & 63)});
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(((tt >> 6) << 9) + (tt & 63)) ^ cswz(i << 6)] = v[i];
            wave_lds_sync();
            __builtin_amdgcn_s_setprio(2);
            // pass C = stages 6..8 : p = hi*64 + i*8 + lo
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz(((tt >> 3) << 6) + (tt & 7)) ^ cswz(i << 3)];
            stages8(v, TwLdsSym<8>{stwC + (tt & 7)});
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(((tt >> 3) << 6) + (tt & 7)) ^ cswz(i << 3)] = v[i];
            wave_lds_sync();
            __builtin_amdgcn_s_setprio(1);
            // pass D = stages 9..11 (10..12 of the 8192 network) : p = 8*t + i, in place
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fb[swz(tt << 3) ^ i];
            fft_stages<13, 10, 3>(v, 0, pl.tw);
#pragma unroll
            for (int i = 0; i < 8; ++i) fb[swz(tt << 3) ^ i] = v[i];
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        if (active) {
            // per-bin stages on all 1024 threads: bins 4g..4g+3 from F(i) = Z[4g-1+i], M(i) = Z[N-4g+1-i], i = 0..5.
            // The Nyquist bin is not visited (k-hat = N/2 >= ebin[R], see fused_r8.hip.inc).
            __builtin_amdgcn_s_setprio(3);
            float yr[6], yi[6], ur[6], tr[6];
            {
                float2 f[6], m[6];     // all twelve spectrum reads issued before the first use (fused_pp.hip.inc)
#pragma unroll
                for (int i = 0; i < 6; ++i) { f[i] = fbuf[fpos[i]]; m[i] = fbuf[mpos[i]]; }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    yr[i] = f[i].x + m[i].x; yi[i] = f[i].y - m[i].y; ur[i] = f[i].x - m[i].x; tr[i] = f[i].y + m[i].y;   // ur = -Ti
                }
            }
            int sbase = sj - DMAX;                     // ring slot of column j-DMAX
            sbase += sbase < 0 ? SLOTS : 0;
            const int jrel = (int)(j - c0);
            const unsigned span = (unsigned)(c1 - c0);
            const float Df = (float)D;
            const float kf0 = (float)(4 * (((tw_ & 63) << 4) | (tw_ >> 6)));
            float* cellp[4];
            float pw[4];
            bool okv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float Ar = twice_minus(yr[e + 1], yr[e] + yr[e + 2]), Ai = twice_minus(yi[e + 1], yi[e] + yi[e + 2]);
                const float Br = twice_minus(tr[e + 1], tr[e] + tr[e + 2]), Ui = twice_minus(ur[e + 1], ur[e] + ur[e + 2]);
                const float Dr = yr[e] - yr[e + 2], Di = yi[e] - yi[e + 2];
                const float den = __builtin_fmaf(Ar, Ar, Ai * Ai);
                const float P = den * 0.015625f;
                bool ok = (P >= pl.pfloor_abs) && (P <= kPowerMax);
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
        // next frame: shift the sample registers by one hop and run its stage 0 + pass A
#pragma unroll
        for (int i = 0; i < 16 - SH; ++i) xs[i] = xs[i + SH];
#pragma unroll
        for (int q = 0; q < SH; ++q) xs[16 - SH + q] = xn[q];
        first_pass(tt);
        __syncthreads();
        sj += 1;
        sj -= sj >= SLOTS ? SLOTS : 0;
    }
    finalize(jstop - 1 - D, sj - 1 - D, tid);          // the last frame's column (the loop's last barrier is behind us)
}

// (dynamic LDS: fused8192_lds_bytes, emspec_kernel_plan.h)

}  // namespace emspec
