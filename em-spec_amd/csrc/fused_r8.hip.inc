// fused_r8.hip.inc — what the 1024-thread radix-8 fused kernels share (namespace f8): ring geometry, the in-place buffer's
// swizzle, the radix-8 register passes and their twiddle sources.  Included by fused.hip.inc before the kernels that use it
// (fused_pp, fused_n8192, fused_small, diag/fused_pp4; the EXACT kernels take the swizzle and tw_index8 from here too).
// The kernel this file used to hold, the lock-step fused4096_r8_kernel (the product of rounds 1-2, an A/B form after them),
// is retired: docs/HISTORY.md "Retired kernel forms".  What its text explained and other files point to is kept below.
//
// The layout: the LDS column ring limits a CU to one workgroup, so the workgroup is
// made 16 waves (4 per SIMD, <= 128 VGPRs) and each frame is spread over 512 threads
// with 8 points per thread: four radix-8 register passes (the same canonical radix-2
// DIF butterflies, stages 0-2 / 3-5 / 6-8 / 9-11) over one in-place LDS buffer.
// After pass A the transform is 8 independent 512-point sub-FFTs, and wave w of a frame
// owns sub-FFT w (64 lanes x 8 points): passes B, C and D are WAVE-LOCAL, ordered only by
// the in-order LDS pipe (no workgroup barrier).  The output stays in place (bit-reversed)
// and the per-bin stage reads it there.  One XOR swizzle makes all five access patterns
// (A write, B, C, D read/write, bit-reversed bin reads) bank-conflict-free.
// Threads 0..511 take one frame, threads 512..1023 the next.  With hop = 256 the
// register stride (512 samples) is two hops, so advancing two frames shifts the eight
// sample registers by one and loads ONE new sample per thread (hop 512: two, hop 1024: four;
// the ring then needs 10 / 6 column slots instead of 18).
//
// Notes the kernels refer to:
//  - Bin groups are dealt to threads so that the lanes of one wave-instruction are 32 bins apart (group g = 8*lane + wave
//    owns bins 4g..4g+3): a log-frequency row is up to ~12 bins wide, and lanes that share a cell in the same accumulate
//    instruction serialise it (one LDS round each).
//  - The Nyquist bin k = N/2 is not visited: Y[N/2+1] = conj Y[N/2-1] makes its k-shift exactly 0 in this arithmetic, so
//    k-hat = N/2 >= ebin[R] (emspec_tables.h: edges_bin64 ends the axis at min(e[R], N/2), in binary64 and so in float32; that
//    fmax <= fs/2 is enforced by emspec_create is not enough, the unclamped binary64 edge can round an ulp above N/2) and it
//    can never reach the histogram.  Skipping it keeps the 8 waves of a frame at equal work.  (frames_kernel still reports it in the parity dump.)
//  - The thread index is laundered once per iteration (asm volatile("" : "+v"(tt))): every LDS address is then recomputed
//    (1-3 VALU each) instead of being hoisted out of the frame loop, which would pin ~50 VGPRs.
//  - FAST (template parameter of every kernel here): reassignment ON and a log-spaced edge table are known at compile time
//    (the launcher checks): the per-bin stage is then one basic block - without it the two wave-uniform run-time branches
//    per bin (pl.reassign, the table kind) cut it into a dozen blocks, the scheduler cannot move code across them, and the
//    four bins' dependent chains (divide -> log2 -> table read -> compares) run one after the other with a full LDS round
//    trip each.
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
// recompute their addresses every iteration (fused_n8192, fused_small) use it; fused_pp hoists its pass-B / pass-C
// positions (recomputing them, even this cheaply, measured slower in the lock-step kernel: 10.41 vs 10.11 ms).
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

}  // namespace emspec
