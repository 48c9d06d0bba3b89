// fused_r8.hip.inc — fused batch kernel, 1024-thread variant.  Included by kernels.hip.
//
// Same algorithm and arithmetic as fused4096_kernel (fused.hip.inc), arranged for
// occupancy: the LDS column ring limits a CU to one workgroup, so the workgroup is
// made 16 waves (4 per SIMD, <= 128 VGPRs) and each frame is spread over 512 threads
// with 8 points per thread: four radix-8 register passes (the same canonical radix-2
// DIF butterflies, stages 0-2 / 3-5 / 6-8 / 9-11) over one in-place LDS buffer.
// After pass A the transform is 8 independent 512-point sub-FFTs, and wave w of a frame
// owns sub-FFT w (64 lanes x 8 points): passes B, C and D are WAVE-LOCAL, ordered only by
// the in-order LDS pipe (no workgroup barrier).  The output stays in place (bit-reversed)
// and the per-bin stage reads it there.  One XOR swizzle makes all five access patterns
// (A write, B, C, D read/write, bit-reversed bin reads) bank-conflict-free.
// Barriers per 2-frame iteration: after pass A, after pass D, after the scatter.
// Threads 0..511 take frame jb, threads 512..1023 frame jb+1.  With hop = 256 the
// register stride (512 samples) is two hops, so advancing two frames shifts the eight
// sample registers by one and loads ONE new sample per thread (hop 512: two, hop 1024: four;
// the ring then needs 10 / 6 column slots instead of 18).
namespace emspec {

namespace f8 {
constexpr int LOG2N = 12, N = 4096, T = 512;
// ring geometry per hop: reach DMAX = N/(2*hop) columns either way, two frames per iteration
template <int HOP>
struct Geo {
    static_assert(HOP == 256 || HOP == 512 || HOP == 1024, "hop must keep two frames a whole number of sample registers apart");
    static constexpr int DMAX = N / (2 * HOP), SLOTS = 2 * DMAX + 2;
    static constexpr int SH = 2 * HOP / 512;   // sample registers (512 samples each) two frames are apart
};

// in-place buffer swizzle (complex units): low 5 bits ^= (p7^p8, p6^p9, p7, p6, p5).
// GF(2)-linear in p[9:5]; chosen so that every wave-instruction of every pass touches 32
// (reads) / 16 (writes) distinct bank positions:
//   A write / B read+write : lanes = p[5:0]                      (S constant per 32 lanes)
//   C read+write           : lanes = p[2:0] x p[8:6]             (needs S[4:3] ~ p[7:6])
//   D read+write           : lanes = p[8:3]                      (needs S[2:0] ~ p[7:5])
//   bin reads, bit-reversed: lanes = k[6:2] = p[9:5]             (needs S ~ p[9:5], full rank)
__device__ __forceinline__ int swz(int p) {
    const int s = ((p >> 5) & 7) | ((((p >> 6) ^ (p >> 9)) & 1) << 3) | ((((p >> 7) ^ (p >> 8)) & 1) << 4);
    return p ^ s;
}
// The swizzle is GF(2)-linear and reads bits 5..9 only, so for bit fields that do not overlap
//   swz(P + (i << b)) = swz(P) ^ swz(i << b):
// one thread-dependent base per pass and one XOR with a compile-time constant (cswz) per point.  The kernels that
// recompute their addresses every iteration (fused_n8192, fused_small) use it; here the pass-B / pass-C positions are
// hoisted (recomputing them, even this cheaply, measured slower: 10.41 vs 10.11 ms).
__device__ __forceinline__ constexpr int cswz(int p) {
    return p ^ (((p >> 5) & 7) | ((((p >> 6) ^ (p >> 9)) & 1) << 3) | ((((p >> 7) ^ (p >> 8)) & 1) << 4));
}
// position of spectrum sample Z[k] in the in-place (bit-reversed) buffer
__device__ __forceinline__ int zpos(int k) { return swz((int)(__brev((unsigned)k) >> 20)); }
template <int S0>
__device__ __forceinline__ int tw_index8(int e, int lo) {   // slot e in [0,7): stage u, butterfly mm
    constexpr int B0 = LOG2N - S0 - 3;
    const int u = e < 4 ? 0 : (e < 6 ? 1 : 2);
    const int mloc = 4 >> u, mm = e - (8 - 2 * mloc);
    return ((mm << B0) + lo) << (S0 + u);
}
// three radix-2 DIF stages on 8 registers; twiddle slot e comes from w(e)
template <class W>
__device__ __forceinline__ void stages8(float2 (&v)[8], const W& w) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
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
struct TwRegs { const float2* w; __device__ __forceinline__ float2 operator()(int e) const { return w[e]; } };
template <int STRIDE>
struct TwLds { const float2* base; __device__ __forceinline__ float2 operator()(int e) const { return base[e * STRIDE]; } };
// The seven slots of a radix-8 pass from FOUR values: within a stage the upper half of the slots lies a quarter turn beyond
// the lower half (slot mm + mloc/2: exponent + (mloc/2 << B0) << (S0 + u) = + N/4), and the table is quarter-turn
// symmetric, tw[q + N/4] = (tw[q].y, -tw[q].x) exactly (DESIGN.md §3.1; negation is exact): slots 2, 3 are slots 0, 1
// rotated, slot 5 is slot 4 rotated.  Bit-identical butterflies, 3 LDS reads (or 6 registers) fewer per pass.
__device__ __forceinline__ constexpr int sym8_src(int e) { return e < 2 ? e : (e < 4 ? e - 2 : (e == 5 ? 4 : e)); }
__device__ __forceinline__ constexpr bool sym8_rot(int e) { return e == 2 || e == 3 || e == 5; }
struct TwRegsSym {
    const float2* w;
    __device__ __forceinline__ float2 operator()(int e) const {
        const float2 x = w[sym8_src(e)];
        return sym8_rot(e) ? make_float2(x.y, -x.x) : x;
    }
};
template <int STRIDE>
struct TwLdsSym {
    const float2* base;
    __device__ __forceinline__ float2 operator()(int e) const {
        const float2 x = base[sym8_src(e) * STRIDE];
        return sym8_rot(e) ? make_float2(x.y, -x.x) : x;
    }
};

// ---- store-as-you-go form of a radix-8 pass (fused4096_pp_kernel's passes B, C, D only; stages8 and fft_stages keep their
// schedules).  A ds_write_b64 costs the LDS store path about 6 cycles per wave-instruction and a wave's LDS operations issue
// in order, so a pass that ends in eight stores back to back puts about 48 cycles of store path per wave in front of the
// next pass's reads, while the wave has nothing else to issue.  Here the pass's last stage
// runs pair by pair, each pair's two stores behind its own butterfly, and the second quad of the middle stage is sunk
// between the first quad's pairs: the stores are spread over the last ~48 VALU of the pass, two at a time.
// Same butterflies on the same operands as stages8 / fft_stages<12, 9, 3> (the butterflies of one stage are independent,
// so their order among themselves is free); the fences pin the order, which the scheduler otherwise undoes (it clusters stores).
// A fence lets scalar and global-memory instructions pass (0x4 | 0x10), nothing else.
struct Bfly8 {   // butterfly I of local stage U of stages8(v, w), the seven twiddle slots w(e) in registers
    float2 (&v)[8];
    float2 tw[7];
    template <int U, int I>
    __device__ __forceinline__ void run() const {
        constexpr int mloc = 4 >> U;
        const float2 a = v[I], b = v[I + mloc];
        v[I] = cadd(a, b);
        v[I + mloc] = cmul_tw(csub(a, b), tw[8 - 2 * mloc + (I & (mloc - 1))]);
    }
};
// The slots are read once, in front of the pass: a table read behind one of the pass's own stores could not be merged with
// the same slot's earlier read (the store may alias it), and the pass would read its LDS twiddles again and wait for them.
template <class W>
__device__ __forceinline__ Bfly8 bfly8(float2 (&v)[8], const W& w) {
    return Bfly8{v, {w(0), w(1), w(2), w(3), w(4), w(5), w(6)}};
}
struct BflyD {   // butterfly I of stage 9 + U of fft_stages<LOG2N, 9, 3>(v, 0, tw): the twiddles are compile-time constants
    float2 (&v)[8];
    template <int U, int I>
    __device__ __forceinline__ void run() const {
        constexpr int mloc = 4 >> U, q = (I & (mloc - 1)) << (9 + U);
        static_assert(q == 0 || q == N / 8 || q == N / 4 || q == 3 * (N / 8), "pass D has these four twiddles only");
        constexpr float kC8 = 0.70710677f;   // tw[N/8] = (c, -c), tw[3N/8] = (-c, -c): see fft_stages
        const float2 a = v[I], b = v[I + mloc];
        v[I] = cadd(a, b);
        const float2 d = csub(a, b);
        if constexpr (q == 0) v[I + mloc] = d;
        else if constexpr (q == N / 4) v[I + mloc] = make_float2(d.y, -d.x);
        else if constexpr (q == N / 8) v[I + mloc] = cmul_tw(d, make_float2(kC8, -kC8));
        else v[I + mloc] = cmul_tw(d, make_float2(-kC8, -kC8));
    }
};
#define EMSPEC_STORE_FENCE() __builtin_amdgcn_sched_barrier(0x4 | 0x10)
template <class B, class St>
__device__ __forceinline__ void pass8_store_as_you_go(const B& bf, const St& st) {   // st(i) stores register i
    bf.template run<0, 0>(); bf.template run<0, 1>(); bf.template run<0, 2>(); bf.template run<0, 3>();
    bf.template run<1, 0>(); bf.template run<1, 1>();
    bf.template run<2, 0>(); st(0); st(1);
    EMSPEC_STORE_FENCE();
    bf.template run<1, 4>();
    bf.template run<2, 2>(); st(2); st(3);
    EMSPEC_STORE_FENCE();
    bf.template run<1, 5>();
    bf.template run<2, 4>(); st(4); st(5);
    EMSPEC_STORE_FENCE();
    bf.template run<2, 6>(); st(6); st(7);
}
#undef EMSPEC_STORE_FENCE
}  // namespace f8

#define EMSPEC_STAMP(slot)                                                       \
    if constexpr (STAMP) {                                                        \
        const unsigned long long now_ = __builtin_readcyclecounter();             \
        acc_[slot] += now_ - last_;                                               \
        last_ = now_;                                                             \
    }
// FAST: reassignment ON and a log-spaced edge table are known at compile time (the launcher checks): the per-bin stage
// is then one basic block - without it the two wave-uniform run-time branches per bin (pl.reassign, the table kind)
// cut it into a dozen blocks, the scheduler cannot move code across them, and the four bins' dependent chains
// (divide -> log2 -> table read -> compares) run one after the other with a full LDS round trip each.
template <int HOP, bool STAMP, bool FAST = false>
__global__ __launch_bounds__(1024, 4) void fused4096_r8_kernel(
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
    // Bin groups are dealt to threads so that the lanes of one wave-instruction are 32 bins apart
    // (group g = 8*lane + wave owns bins 4g..4g+3): a log-frequency row is up to ~12 bins wide, and
    // lanes that share a cell in the same accumulate instruction serialise it (one LDS round each).
    const int bg = ((t & 63) << 3) | (t >> 6);
    int fpos[6], mpos[6];     // positions of Z[4g-1+i] and Z[N-4g+1-i] in the in-place buffer
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        fpos[i] = zpos((4 * bg - 1 + i) & (N - 1));
        mpos[i] = zpos((N - 4 * bg + 1 - i) & (N - 1));
    }
    int sj_even = (int)(j0 % SLOTS);
    __syncthreads();
    unsigned long long real0_ = 0;   // diagnostic build: constant 100 MHz clock beside the shader clock (in-kernel clock check)
    if constexpr (STAMP) { last_ = __builtin_readcyclecounter(); real0_ = __builtin_amdgcn_s_memrealtime(); }

    // pass A (pack z = x + j*ramp*x, stages 0..2) is software-pipelined: it is register-only, so it is
    // computed for the NEXT frame before the barrier that ends an iteration (filling barrier wait)
    float2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.25f * (float)i));
    stages8(v, TwRegs{twA});
#pragma unroll 1
    for (int64_t jb = j0; jb < jstop + 2; jb += 2) {   // one extra, empty iteration finalises the last two columns
        const int64_t j = jb + h;
        const bool active = j < C && j < jstop;
        const int64_t nx = (j + 2) * HOP + t + 512 * (8 - SH);   // first new sample register of frame j+2
        // Launder t once per iteration: every LDS address below is then recomputed (1-3 VALU
        // each) instead of being hoisted out of the loop, which would pin ~50 VGPRs.
        int tt = t;
        asm volatile("" : "+v"(tt));
        float xn[SH];
#pragma unroll
        for (int q = 0; q < SH; ++q) xn[q] = nx + 512 * q < L ? x0[nx + 512 * q] : 0.0f;

        if (active) {
            // pass A results were computed in registers before the previous iteration's last barrier
            // swz(tt + 512 i) = (swz(tt) ^ 8 (i & 1)) + 512 i: the swizzle touches the low five bits only and of the bits
            // it reads, i moves p9 alone - two address registers and immediate offsets instead of eight recomputed addresses
            float2* const w0 = fb + swz(tt);
            float2* const w1 = fb + (swz(tt) ^ 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) ((i & 1) ? w1 : w0)[T * i] = v[i];
        }
        EMSPEC_STAMP(0)
        __syncthreads();
        EMSPEC_STAMP(1)
        // ---- columns jb-2-D and jb-1-D were completed by the previous iteration: finalise, store, clear.  Done
        // here, beside the other waves' pass B, rather than right after the scatter barrier where the rest of the
        // workgroup would wait for it; their ring slots are reused only by this iteration's scatter (after the
        // next barrier).  Team h takes column jb-2-D+h, one float4 of cells per thread.
        {
            const int qpc = R >> 2;   // float4 quads per column
            const int64_t col = jb - 2 - D + h;
            if (t < qpc && col >= c0 && col < c1) {
                const int cell = t << 2;
                int sl = sj_even - 2 - D + h;
                sl += sl < 0 ? SLOTS : 0;
                finalize_ring_quad(ring, sl, R, cell, dm, slut, ((size_t)s * C + col) * R + cell, db, rgba, index);
            }
        }
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
        __syncthreads();
        EMSPEC_STAMP(1)
        if (active) {
            // per-bin stages: bins 4g .. 4g+3 (g = this thread's bin group) from F(i) = Z[4g-1+i], M(i) = Z[N-4g+1-i], i = 0..5
            // (positions hoisted out of the frame loop: they depend on t only).  Branch-free and
            // unrolled so the four bins' dependency chains (spectrum read -> reassign -> edge-table
            // read -> accumulate) overlap; one predicate per bin guards the accumulate.
            // The Nyquist bin k = N/2 is not visited: Y[N/2+1] = conj Y[N/2-1] makes its k-shift
            // exactly 0 in this arithmetic, so k-hat = N/2 >= ebin[R] (fmax <= fs/2 is enforced by
            // emspec_create) and it can never reach the histogram.  Skipping it keeps the 8 waves
            // of a frame at equal work.  (frames_kernel still reports it in the parity dump.)
            __builtin_amdgcn_s_setprio(3);
            float yr[6], yi[6], ur[6], tr[6];
            read_split6(fb, fpos, mpos, yr, yi, ur, tr);   // all twelve reads issued before the first use
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
            EMSPEC_STAMP(5)
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
        for (int i = 0; i < 8 - SH; ++i) xs[i] = xs[i + SH];
#pragma unroll
        for (int q = 0; q < SH; ++q) xs[8 - SH + q] = xn[q];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.25f * (float)i));
        stages8(v, TwRegs{twA});
        EMSPEC_STAMP(6)
        __syncthreads();
        EMSPEC_STAMP(1)
        sj_even += 2;
        sj_even -= sj_even >= SLOTS ? SLOTS : 0;
    }
    if constexpr (STAMP) {
        if ((tid & 63) == 0) {
            unsigned long long* o = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (tid >> 6)) * 8;
            // slot 7: low word = accumulate rounds (r8 kernel), high word = the walk's duration in 100 MHz ticks; the
            // shader clock it held = (sum of slots 0..6) / ticks * 100 MHz (MI355X_MICROARCH.md "DVFS give-back" item 6)
            acc_[7] = (acc_[7] & 0xFFFFFFFFull) | ((__builtin_amdgcn_s_memrealtime() - real0_) << 32);
            for (int i = 0; i < 8; ++i) o[i] = acc_[i];
        }
    }
}
#undef EMSPEC_STAMP
// (dynamic LDS: fused_r8_lds_bytes, emspec_kernel_plan.h)

}  // namespace emspec
