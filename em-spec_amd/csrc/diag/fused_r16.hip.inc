// diag/fused_r16.hip.inc — DIAGNOSTIC BUILD ONLY (-DEMSPEC_DIAG, libemspec_diag.so).
// The first fused batch kernel (512 threads, radix-16, 2 waves per SIMD), kept as the A/B record of what
// occupancy is worth (0.56x the default kernel).  Not compiled into libemspec.so.
//
// fused4096_kernel: N = 4096, hop = 256.  One 512-thread workgroup walks a
// segment of ONE stream in time order, two frames per iteration (threads 0..255
// take frame jb, threads 256..511 frame jb+1, 16 points each):
//   - frame gather by register shift: thread t of a half owns the samples
//     pcm[(j+i)*256 + t], i = 0..15, so advancing two frames shifts the 16
//     registers by two and loads two new samples (coalesced, 4*hop bytes per
//     column from HBM — the algorithmic minimum);
//   - packed FFT: three radix-16 register passes (canonical radix-2 DIF
//     butterflies, twiddles of passes A/B held in registers for the whole walk),
//     two in-place LDS exchanges with an XOR bank swizzle (conflict-free on both
//     the write and the read side), then a natural-order rewrite;
//   - per-bin stages on 8 consecutive bins per thread (rolling 3-bin window),
//     log2-hinted exact row lookup, float LDS atomics into an 18-slot column
//     ring (2D+2 slots, D = 8);
//   - a column leaves the ring as soon as no later frame can reach it: dB,
//     palette index / RGBA computed in-kernel and written with 16-byte stores.
// Nothing but pcm is read from HBM and nothing but finished columns is written.
namespace emspec {

namespace fz {
constexpr int LOG2N = 12, N = 4096, T = 256, HOP = 256, SLOTS = 18, DMAX = 8;

// in-place exchange buffer: XOR swizzle of the low 5 bits (complex units)
__device__ __forceinline__ int swz(int p) {
    return p ^ ((((p >> 8) & 1) << 4) | (((p >> 7) & 1) << 3) | ((p >> 9) & 7));
}
// natural-order buffer (complex units): conflict-free both for the pass-C rewrite (lanes = consecutive k)
// and for the per-bin reads (lanes = k stepping by 8)
__device__ __forceinline__ int nidx(int k) { return k ^ ((k >> 5) & 7); }

template <int S0>
__device__ __forceinline__ void load_tw16(float2 (&w)[15], int lo, const float2* __restrict__ tw) {
    constexpr int B0 = LOG2N - S0 - 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int mloc = 8 >> u;
#pragma unroll
        for (int mm = 0; mm < mloc; ++mm) w[16 - 2 * mloc + mm] = tw[((mm << B0) + lo) << (S0 + u)];
    }
}
// four radix-2 DIF stages on 16 registers, twiddle slot e read from wl[e*16] (LDS table [15][16],
// column = t & 15 already folded into wl)
__device__ __forceinline__ void stages16_lds(float2 (&v)[16], const float2* wl) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int mloc = 8 >> u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i & mloc) continue;
            const float2 a = v[i], b = v[i + mloc];
            v[i] = cadd(a, b);
            v[i + mloc] = cmul_tw(csub(a, b), wl[(16 - 2 * mloc + (i & (mloc - 1))) * 16]);
        }
    }
}
// four radix-2 DIF stages on 16 registers with preloaded twiddles
__device__ __forceinline__ void stages16(float2 (&v)[16], const float2 (&w)[15]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int mloc = 8 >> u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i & mloc) continue;
            const float2 a = v[i], b = v[i + mloc];
            v[i] = cadd(a, b);
            v[i + mloc] = cmul_tw(csub(a, b), w[16 - 2 * mloc + (i & (mloc - 1))]);
        }
    }
}

}  // namespace fz

// STAMP = true is the diagnostic build (emspec_debug_phase_cycles): lane 0 of every wave sums the
// shader-clock cycles it spends in each barrier-delimited phase into `stamps`; it never runs in
// the product path and no output depends on it.
#define EMSPEC_STAMP(slot)                                                        \
    if constexpr (STAMP) {                                                        \
        const unsigned long long now_ = __builtin_readcyclecounter();             \
        acc_[slot] += now_ - last_;                                               \
        last_ = now_;                                                             \
    }
template <bool STAMP>
__global__ __launch_bounds__(512, 2) void fused4096_kernel(
    PlanDev pl, DbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, float* __restrict__ db, uint32_t* __restrict__ rgba, uint8_t* __restrict__ index,
    unsigned long long* __restrict__ stamps) {
    using namespace fz;
    unsigned long long acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last_ = 0;
    extern __shared__ float4 smem4[];
    const int R = pl.rows, D = pl.D;
    float2* fbuf = reinterpret_cast<float2*>(smem4);       // [2][4096] complex
    float* ring = reinterpret_cast<float*>(fbuf + 2 * N);   // [SLOTS][R]
    float* seb = ring + SLOTS * R;                           // [R+1]
    uint32_t* slut = reinterpret_cast<uint32_t*>(seb + R + 4);  // [256]
    float2* stwB = reinterpret_cast<float2*>(slut + 256);       // [15][16] pass-B twiddles

    const int tid = threadIdx.x, h = tid >> 8, t = tid & 255;
    float2* fb = fbuf + h * N;
    int s;
    int64_t c0, c1;
    if (!seg_of_block(sp, C, s, c0, c1)) return;
    const int64_t j0 = (c0 - D > 0 ? c0 - D : 0) & ~(int64_t)1;
    const int64_t jstop = c1 + D;            // frames/columns are walked up to here (frames >= C are idle)
    const float* x0 = pcm + (size_t)s * L;

    // ---- workgroup set-up: clear the ring, stage tables, hoist twiddles, prime the sample registers
    for (int q = tid; q < SLOTS * R / 4; q += 512) reinterpret_cast<float4*>(ring)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = tid; r <= R; r += 512) seb[r] = pl.ebin[r];
    if (tid < 256) slut[tid] = lut[tid];
    float2 twA[15];
    load_tw16<0>(twA, t, pl.tw);
    if (tid < 240) {
        // slot e = tid >> 4 of column lo = tid & 15: stage u, m = e - (16 - 2*mloc)
        const int e = tid >> 4, lo = tid & 15;
        const int u = e < 8 ? 0 : (e < 12 ? 1 : (e < 14 ? 2 : 3));
        const int mloc = 8 >> u, mm = e - (16 - 2 * mloc);
        stwB[tid] = pl.tw[((mm << 4) + lo) << (4 + u)];
    }
    float xs[16];
    {
        const int64_t j = j0 + h;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t idx = (j + i) * HOP + t;
            xs[i] = idx < L ? x0[idx] : 0.0f;
        }
    }
    const float r0 = (float)(t - N / 2) * (2.0f / (float)N);   // ramp of register 0; register i adds i/8 (exact)
    HintLookup lk;
    lk.init(seb, pl.ebin, R, pl.log_rows);
    int sj_even = (int)(j0 % SLOTS);
    __syncthreads();
    if constexpr (STAMP) last_ = __builtin_readcyclecounter();

#pragma unroll 1
    for (int64_t jb = j0; jb < jstop; jb += 2) {
        const int64_t j = jb + h;
        const bool active = j < C && j < jstop;
        // prefetch the two samples the next iteration needs
        const int64_t n0 = (j + 16) * HOP + t, n1 = (j + 17) * HOP + t;
        const float xn0 = n0 < L ? x0[n0] : 0.0f;
        const float xn1 = n1 < L ? x0[n1] : 0.0f;

        float2 v[16];
        if (active) {
            // pack z = x + j*ramp*x ; pass A = stages 0..3
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.125f * (float)i));
            stages16(v, twA);
#pragma unroll
            for (int i = 0; i < 16; ++i) fb[swz(t + T * i)] = v[i];
        }
        EMSPEC_STAMP(0)
        __syncthreads();
        EMSPEC_STAMP(1)
        if (active) {
            // pass B = stages 4..7, in place
            const int base = ((t >> 4) << 8) + (t & 15);
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = fb[swz(base + (i << 4))];
            stages16_lds(v, stwB + (t & 15));
#pragma unroll
            for (int i = 0; i < 16; ++i) fb[swz(base + (i << 4))] = v[i];
        }
        EMSPEC_STAMP(2)
        __syncthreads();
        EMSPEC_STAMP(1)
        if (active) {
            // pass C = stages 8..11 on group g = bitrev8(t): outputs are k = bitrev4(i)*256 + t
            const int g = (int)(__brev((unsigned)t) >> 24);
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = fb[swz((g << 4) + i)];
            fft_stages<LOG2N, 8, 4>(v, 0, pl.tw);
        }
        EMSPEC_STAMP(3)
        __syncthreads();
        EMSPEC_STAMP(1)
        if (active) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = (int)(__brev((unsigned)i) >> 28) * 256 + t;
                fb[nidx(k)] = v[i];
            }
        }
        EMSPEC_STAMP(4)
        __syncthreads();
        EMSPEC_STAMP(1)
        if (active) {
            // per-bin stages: bins 8t .. 8t+7 (+ Nyquist on t == 255), rolling window over
            // F(i) = Z[8t-1+i] and M(i) = Z[N-8t+1-i].  Branch-free: every lane evaluates every
            // stage, one predicate guards the LDS atomic.  Same operations as reassign_core
            // (Ti is carried negated: u = -Ti, exact).
            const int fk = 8 * t - 1, mk = N - 8 * t + 1;
            float2 f0 = fb[nidx(fk & (N - 1))], m0 = fb[nidx(mk & (N - 1))];
            float2 f1 = fb[nidx((fk + 1) & (N - 1))], m1 = fb[nidx((mk - 1) & (N - 1))];
            float ymr = f0.x + m0.x, ymi = f0.y - m0.y, umr = f0.x - m0.x, tmr = f0.y + m0.y;
            float ycr = f1.x + m1.x, yci = f1.y - m1.y, ucr = f1.x - m1.x, tcr = f1.y + m1.y;
            // ring slot of column (j - 8 + d), d = dcol + 8 in [0,16]:  (sbase + d) mod 18
            int sbase = sj_even + h - DMAX;
            sbase += sbase < 0 ? SLOTS : 0;
            const int jrel = (int)(j - c0);               // this frame's column relative to the segment
            const unsigned span = (unsigned)(c1 - c0);
            const float Df = (float)D;
            float kf = (float)(8 * t);
            // (the Nyquist bin is not visited: it can never reach the histogram, see fused_r8.hip.inc)
#pragma unroll 2
            for (int e = 0; e < 8; ++e) {
                const float2 f2 = fb[nidx((fk + 2 + e) & (N - 1))], m2 = fb[nidx((mk - 2 - e) & (N - 1))];
                const float ypr = f2.x + m2.x, ypi = f2.y - m2.y, upr = f2.x - m2.x, tpr = f2.y + m2.y;
                const float Ar = (ycr + ycr) - (ymr + ypr), Ai = (yci + yci) - (ymi + ypi);
                const float Br = (tcr + tcr) - (tmr + tpr), Ui = (ucr + ucr) - (umr + upr);   // Ui = -Bi
                const float Dr = ymr - ypr, Di = ymi - ypi;
                const float den = __builtin_fmaf(Ar, Ar, Ai * Ai);
                const float P = den * 0.015625f;
                bool ok = (P >= pl.pfloor_abs) && (P <= kPowerMax);
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
                const int r0 = lk.row_unchecked(kh);
                ok = ok && ((unsigned)(jrel + d - DMAX) < span);
                unsigned sl = (unsigned)(sbase + (ok ? d : 0));
                sl = min(sl, sl - (unsigned)SLOTS);
                if (ok) atomicAdd(ring + sl * R + r0, P);
                ymr = ycr; ymi = yci; umr = ucr; tmr = tcr;
                ycr = ypr; yci = ypi; ucr = upr; tcr = tpr;
                kf += 1.0f;
            }
        }
        EMSPEC_STAMP(5)
        __syncthreads();
        EMSPEC_STAMP(1)
        // ---- columns jb-D and jb-D+1 can no longer be reached: finalise, store, clear
        {
            const int qpc = R >> 2;   // float4 quads per column
            for (int q = tid; q < 2 * qpc; q += 512) {
                const int cc = q >= qpc ? 1 : 0;
                const int cell = (q - cc * qpc) << 2;
                const int64_t col = jb - D + cc;
                if (col >= c0 && col < c1) {
                    int sl = sj_even - D + cc;
                    sl += sl < 0 ? SLOTS : 0;
                    sl -= sl >= SLOTS ? SLOTS : 0;
                    finalize_ring_quad(ring, sl, R, cell, dm, slut, ((size_t)s * C + col) * R + cell, db, rgba, index);
                }
            }
        }
        // advance: shift the sample registers by two frames
#pragma unroll
        for (int i = 0; i < 14; ++i) xs[i] = xs[i + 2];
        xs[14] = xn0;
        xs[15] = xn1;
        sj_even += 2;
        sj_even -= sj_even >= SLOTS ? SLOTS : 0;
        // (the ring clear above and the next scatter are separated by the barriers of the next iteration)
        EMSPEC_STAMP(6)
    }
    if constexpr (STAMP) {
        if ((tid & 63) == 0) {
            unsigned long long* o = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (tid >> 6)) * 8;
            for (int i = 0; i < 8; ++i) o[i] = acc_[i];
        }
    }
}
#undef EMSPEC_STAMP

}  // namespace emspec
namespace emspec {
static size_t fused_lds_bytes(int rows) {
    return (size_t)2 * fz::N * sizeof(float2) + (size_t)fz::SLOTS * rows * 4 + (size_t)(rows + 4) * 4 + 1024 + 240 * 8;
}
}  // namespace emspec
