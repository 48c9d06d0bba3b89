// fused_n16384.hip.inc — fused batch kernel for N = 16384 (BASELINE configs[4]: hop 512, "HBM-bound stress").
// Included by kernels.hip.
//
// Why this shape.  A 16384-point packed FFT needs 128 KB of LDS and the column ring of the reassignment
// scatter (2D+1 = 33 slots x 1024 rows x 4 B at hop 512) needs 132 KB: together they do not fit the CU's
// 160 KB, which is why round 1 ran this size as two kernels with a per-bin record array in HBM between them
// (138 KB of traffic per column against 7 KB algorithmic).  Here ONE workgroup walks a segment of one stream in
// time order and the two images TIME-SHARE the same LDS region:
//   - while a frame's FFT and per-bin stage own the region, the ring is parked in registers
//     (33 x 1024 floats / 1024 threads = 33 VGPRs per thread, moved as float4);
//   - the per-bin results (power, cell) of the thread's 8 consecutive bins wait in registers;
//   - then the ring is written back, the bins are accumulated (exchange-based float add, run-length pre-summed
//     per thread), the finished column leaves as dB / palette index / RGBA, and the ring is parked again.
// HBM sees the samples once (L2 absorbs the 32-fold frame overlap: 4*hop bytes per column + a 2D-frame halo per
// segment) and the finished columns once.  The arithmetic is frames_kernel's (same butterflies, same per-bin
// operation order), so results are bit-identical to the generic path and the oracle's bit model.
// The FFT itself is fft_rest<14,4> of kernels.hip: radix-16 register passes over the padded in-place buffer,
// wave-local middle pass, natural-order rewrite.
// Measured and not kept (round 4): "own-location" parking as in exact_fused4096_kernel - every thread parks the sixteen
// 8-byte places its own pass-1 results go to in the moment it stores them and restores them itself, the ring (34 slots)
// lying over exactly the padded buffer, the finished column converted one frame later beside the accumulates: five
// barriers per frame instead of six, no resident slot, no clearing selects, bit-identical output - 24.0 vs 23.7 ms.
// The barrier it saves is worth less than what sixteen 8-byte LDS accesses cost more than eight 16-byte ones, and the
// conversion costs 1 % beside the accumulates (0.25 ms) where it cost nothing visible in its own interval.  Timing-only
// builds of that form: without parking and restoring 22.0 ms - moving the ring out and in is 8 % of the frame, pure LDS
// bandwidth (2 x 128 KB per frame) that nothing overlaps; without the conversion 23.8 ms.
namespace emspec {

// (the f14:: sizes - the parked cells, the resident slot, where the ring starts in the transform's region - and the shapes and
// dynamic LDS that follow from them: emspec_kernel_plan.h)
static_assert(f14::FFT_BYTES == PaddedSize<f14::N>::value * (int)sizeof(float2), "the transform's region");

namespace f14 {
// (padded) position of spectrum sample Z[k] in the in-place buffer: bit-reversed
__device__ __forceinline__ int zpos14(int k) { return padi((int)(__brev((unsigned)k) >> 18)); }
// Z[k + e] for k a multiple of 8, 0 <= e < 8, sits zoff(e) slots after Z[k]: bitrev14(k + e) = bitrev14(k) +
// (bitrev3(e) << 11), and the padding p + (p >> 4) is additive over multiples of 16
__device__ __forceinline__ constexpr int zoff(int e) {
    const int b = ((e & 1) << 2) | (e & 2) | ((e >> 2) & 1);
    return (b << 11) + (b << 7);
}
__device__ __forceinline__ float2 rot_tw(float2 w) { return make_float2(w.y, -w.x); }   // table entry q + N/4 from entry q
// Stages 0..3 of the canonical DIF network on the 16 points n = lo + 1024 i a thread holds, with 8 loaded twiddles
// instead of 15: the table is quarter-turn symmetric, tw[q + N/4] = (tw[q].y, -tw[q].x) exactly (enforced where the
// table is built, DESIGN.md §3.1), and negation is exact, so this is bit-identical to fft_stages<14, 0, 4>.
//   stage 0: ta[i] = W^(lo + 1024 i), i < 4
__device__ __forceinline__ void pass1_stage0(float2 (&v)[16], const float2 (&ta)[4]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float2 a = v[i], b = v[i + 8];
        v[i] = cadd(a, b);
        v[i + 8] = cmul_tw(csub(a, b), i < 4 ? ta[i] : rot_tw(ta[i - 4]));
    }
}
// tb[0], tb[1] = W^(2 lo), W^(2 lo + 2048);  tb[2] = W^(4 lo);  tb[3] = W^(8 lo)
__device__ __forceinline__ void pass1_stage123(float2 (&v)[16], const float2 (&tb)[4]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i & 4) continue;
        const int m = i & 3;
        const float2 a = v[i], b = v[i + 4];
        v[i] = cadd(a, b);
        v[i + 4] = cmul_tw(csub(a, b), m < 2 ? tb[m] : rot_tw(tb[m - 2]));
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i & 2) continue;
        const float2 a = v[i], b = v[i + 2];
        v[i] = cadd(a, b);
        v[i + 2] = cmul_tw(csub(a, b), (i & 1) ? rot_tw(tb[2]) : tb[2]);
    }
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        const float2 a = v[i], b = v[i + 1];
        v[i] = cadd(a, b);
        v[i + 1] = cmul_tw(csub(a, b), tb[3]);
    }
}
}  // namespace f14

// STAMP = true is the diagnostic build (emspec_debug_phase_cycles, libemspec_diag.so only): lane 0 of every wave sums
// the shader-clock cycles it spends in each phase into `stamps`; no output depends on it.
#define EMSPEC_STAMP(slot)                                                        \
    if constexpr (STAMP) {                                                        \
        const unsigned long long now_ = __builtin_readcyclecounter();             \
        acc_[slot] += now_ - last_;                                               \
        last_ = now_;                                                             \
    }
// FAST: reassignment ON and a log-spaced edge table known at compile time - the per-bin stage is then one basic block
// (see fused_r8.hip.inc)
template <bool STAMP, bool FAST = false>
__global__ __launch_bounds__(1024) void fused16384_kernel(
    PlanDev pl, DbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, float* __restrict__ db, uint32_t* __restrict__ rgba, uint8_t* __restrict__ index,
    unsigned long long* __restrict__ stamps) {
    using namespace f14;
    unsigned long long acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last_ = 0;
    extern __shared__ float4 smem4[];
    float2* sm = reinterpret_cast<float2*>(smem4);                 // FFT buffer (padded), aliased by ...
    float* ring = reinterpret_cast<float*>(reinterpret_cast<char*>(smem4) + RING_OFF);   // ... the column ring [slots][R]
    float2* stw = reinterpret_cast<float2*>(reinterpret_cast<char*>(smem4) + FFT_BYTES + RES_BYTES);   // middle-pass twiddles
    float* seb = reinterpret_cast<float*>(stw + mid_tw_entries(LOG2N));   // [R+1] (+3 pad)
    uint32_t* slut = reinterpret_cast<uint32_t*>(seb + pl.rows + 4);      // [256]

    const int t = threadIdx.x;
    const int R = pl.rows, D = pl.D, slots = 2 * D + 1;
    const int nq4 = slots * (R >> 2);                              // float4 quads in the ring
    const bool fastring = R == 1024 && nq4 >= NQ * T;               // every parked quad is a ring cell, 256 quads per column
    int s;
    int64_t c0, c1;
    if (!seg_of_block(sp, C, s, c0, c1)) return;
    const int64_t jlo = c0 - D > 0 ? c0 - D : 0;
    const int64_t jhi = (c1 + D < C ? c1 + D : C) - 1;             // last frame that can reach this segment
    const float* x0 = pcm + (size_t)s * L;
    const unsigned span = (unsigned)(c1 - c0);

    for (int r = t; r <= R; r += T) seb[r] = pl.ebin[r];
    if (t < 256) slut[t] = lut[t];
    stage_mid_twiddles<LOG2N, 4>(stw, pl.tw, t, T);
    HintLookup lk;
    lk.init(seb, pl.ebin, R, pl.log_rows);

    float4 park[NQ];       // ring quads t + 1024 m (cells 0 .. 32767)
    const int ncell = slots * R;
    if (PARKED_CELLS + t < ncell) ring[PARKED_CELLS + t] = 0.0f;   // the resident cells (first touched after two barriers)
#pragma unroll
    for (int m = 0; m < NQ; ++m) park[m] = make_float4(0.f, 0.f, 0.f, 0.f);

    int sj = 0;                                                    // ring slot of column j - D
    const float rs = 2.0f / (float)N;
    const float Df = (float)D;
    // Pass 1 (stages 0..3) of the NEXT frame needs no LDS: it runs in registers in the scatter interval of the current
    // frame, where the accumulates leave the vector pipes idle (LDS round trips) - half of the waves of every SIMD run
    // it before their accumulates, the other half after, so each SIMD always has waves of both kinds - and its sixteen
    // results wait in registers until the ring has left the region again.  The samples are requested one interval
    // earlier (before the ring is written back), so their L2 latency is off the critical path.
    float xs[16];
    auto prefetch = [&](int64_t jf, int tl) {
        const float* x = x0 + jf * pl.hop;
#pragma unroll
        for (int i = 0; i < 16; ++i) xs[i] = x[tl + T * i];
    };
    float2 v[16];
    auto pass1 = [&](int tl) {
        const float r0 = (float)(tl - N / 2) * rs;             // ramp of point lo; point lo + 1024 i adds i/8 (exact)
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = make_float2(xs[i], xs[i] * (r0 + 0.125f * (float)i));   // ramp (n - N/2) * 2/N, exact
        // this thread's eight pass-1 twiddles (L1/L2 hits; holding them across the frame would cost 16 VGPRs), fetched
        // in two groups so that only the stage that needs them holds them: stage 0: W^(lo + 1024 i), i < 4; then
        // stage 1: W^(2 lo), W^(2 lo + 2048); stage 2: W^(4 lo); stage 3: W^(8 lo)
        float2 ta[4], tb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) ta[i] = pl.tw[i * 1024 + tl];
        pass1_stage0(v, ta);
        __builtin_amdgcn_sched_barrier(0);                     // keep the second group's loads behind stage 0
        tb[0] = pl.tw[2 * tl]; tb[1] = pl.tw[2048 + 2 * tl]; tb[2] = pl.tw[4 * tl]; tb[3] = pl.tw[8 * tl];
        pass1_stage123(v, tb);
    };
    prefetch(jlo, t);
    pass1(t);
    unsigned long long real0_ = 0;   // diagnostic build: constant 100 MHz clock beside the shader clock (in-kernel clock check)
    if constexpr (STAMP) { last_ = __builtin_readcyclecounter(); real0_ = __builtin_amdgcn_s_memrealtime(); }
#pragma unroll 1
    for (int64_t j = jlo; j <= jhi; ++j) {
        // Launder the thread id once per frame: every address below is then recomputed from it (1-3 VALU each)
        // instead of being hoisted out of the frame loop, which would pin dozens of VGPRs beside the parked ring.
        int tt = t;
        asm volatile("" : "+v"(tt));
        // ---- stages "Frame gather" .. "STFT": the FFT owns the LDS region; pass 1 of this frame is already in registers
#pragma unroll
        for (int i = 0; i < 16; ++i) sm[padi(tt) + (T + T / 16) * i] = v[i];   // padi(tt + T i) = padi(tt) + (T + T/16) i
        EMSPEC_STAMP(0)
        __syncthreads();
        EMSPEC_STAMP(1)
        // Issue arbitration is oldest-first, so without help waves 12-15 trail waves 0-3 by half a phase and the old
        // waves idle at the barriers.  Each wave lowers its priority as it advances through a barrier interval: a wave
        // that is behind outranks one that is ahead.
        __builtin_amdgcn_s_setprio(3);
        fft_rest<LOG2N, 4, true, true>(sm, stw, tt, pl.tw);        // in place: Z[k] at sm[padi(bitrev14(k))]
        __builtin_amdgcn_s_setprio(0);
        EMSPEC_STAMP(2)
        __syncthreads();
        EMSPEC_STAMP(1)

        // ---- per-bin stages on this thread's 8 consecutive bins k0 .. k0+7 (rolling 3-bin window); the results
        // wait in registers.  The Nyquist bin is not visited (it can never reach the histogram, see fused_r8).
        // Bin group g of thread (wave w, lane l): g = w[1:0] | l[4]<<2 | w[3:2]<<3 | l[5]<<5 | l[3:0]<<6.  With it the
        // 32 lanes of every bit-reversed spectrum read below hit 32 different LDS bank pairs (slot mod 32 =
        // 16(g6+g2) + 8(g7+g3) + 4(g8+g4) + 2(g9+g5) + g6: lanes vary g6..g9 and g2), and neighbouring lanes sit
        // >= 32 bins apart, so the lanes of one accumulate instruction rarely meet in a histogram cell.
        float pw[8];
        int cell[8];       // ring cell index (slot * R + row), or -1
        {
            const int ln = tt & 63, wv = tt >> 6;
            const int g = (wv & 3) | (((ln >> 4) & 1) << 2) | ((wv >> 2) << 3) | ((ln >> 5) << 5) | ((ln & 15) << 6);
            const int k0 = g << 3;
            const float2* zb = sm + zpos14(k0);                    // Z[k0+e]        at zb[zoff(e)]
            const float2* mb = sm + zpos14(N - k0 - 8);            // Z[N-k0-8+e']   at mb[zoff(e')]
            YT m_ = split_yt(sm[zpos14((k0 - 1) & (N - 1))], sm[zpos14((N - k0 + 1) & (N - 1))]);
            YT c_ = split_yt(zb[0], sm[zpos14((N - k0) & (N - 1))]);
            const int jrel = (int)(j - c0);
            __builtin_amdgcn_s_setprio(3);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e == 3) __builtin_amdgcn_s_setprio(2);
                if (e == 6) __builtin_amdgcn_s_setprio(1);
                const int k = k0 + e;
                const YT p_ = split_yt(e < 7 ? zb[zoff(e + 1)] : sm[zpos14(k0 + 8)], mb[zoff(7 - e)]);
                const float Ar = twice_minus(c_.yr, m_.yr + p_.yr), Ai = twice_minus(c_.yi, m_.yi + p_.yi);   // = (c + c) - s (emspec_device.h)
                const float Br = twice_minus(c_.tr, m_.tr + p_.tr), Bi = twice_minus(c_.ti, m_.ti + p_.ti);
                const float Dr = m_.yr - p_.yr, Di = m_.yi - p_.yi;
                const float den = __builtin_fmaf(Ar, Ar, Ai * Ai);
                const float P = den * 0.015625f;
                bool ok = (P >= pl.pfloor_abs) && (P <= kPowerMax);
                float kh = (float)k;
                int d = 0;
                if (FAST || pl.reassign) {
                    const float numT = __builtin_fmaf(Br, Ar, Bi * Ai);
                    const float numF = __builtin_fmaf(Dr, Ar, Di * Ai);
                    const float inv = FAST ? recip_normal(den) : 1.0f / den;
                    const float cf = __builtin_floorf(__builtin_fmaf(numT * inv, pl.tscale, 0.5f));
                    ok = ok && (__builtin_fabsf(cf) <= Df);
                    d = (int)cf;
                    kh = (float)k + numF * inv;
                }
                const int rr = FAST ? lk.row_signed_log(kh) : lk.row_signed(kh);   // -1 / R when k-hat is off the frequency axis
                ok = ok && ((unsigned)rr < (unsigned)R);
                ok = ok && ((unsigned)(jrel + d) < span);          // the column belongs to this segment
                int sl = sj + d + D;                               // garbage when !ok: never used then
                sl -= sl >= slots ? slots : 0;
                pw[e] = P;
                cell[e] = ok ? (int)__umul24((unsigned)sl, (unsigned)R) + rr : -1;   // (24-bit multiply: full rate; sl < 64, R <= 1024)
                m_ = c_;
                c_ = p_;
            }
            // a thread's consecutive bins often share a cell (a row spans up to ~50 bins at this size): sum such
            // runs in registers, so that one accumulate per distinct cell reaches the LDS
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                const bool same = cell[e] >= 0 && cell[e] == cell[e + 1];
                pw[e + 1] = same ? pw[e + 1] + pw[e] : pw[e + 1];
                cell[e] = same ? -1 : cell[e];
            }
            __builtin_amdgcn_s_setprio(0);
        }
        EMSPEC_STAMP(3)
        __syncthreads();                                           // every read of the spectrum is done
        EMSPEC_STAMP(1)
        // ---- the ring takes the region back
#pragma unroll
        for (int m = 0; m < NQ; ++m) reinterpret_cast<float4*>(ring)[tt + T * m] = park[m];   // (quads past the ring carry zeros)
        __builtin_amdgcn_sched_barrier(0);
        prefetch(j < jhi ? j + 1 : j, tt);                         // in flight while the barrier gathers (after the last frame: the same frame again, unused)
        EMSPEC_STAMP(4)
        __syncthreads();
        EMSPEC_STAMP(1)
        // ---- stage "Scatter", and pass 1 of the next frame beside it (waves 4-7 and 12-15 first, the others afterwards)
        const bool early = (__builtin_amdgcn_readfirstlane(tt) >> 8) & 1;
        if (early) pass1(tt);
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e == 3) __builtin_amdgcn_s_setprio(2);
            if (e == 6) __builtin_amdgcn_s_setprio(1);
            lds_accumulate(ring + (cell[e] >= 0 ? cell[e] : 0), pw[e], cell[e] >= 0);
        }
        __builtin_amdgcn_s_setprio(0);
        if (!early) pass1(tt);
        EMSPEC_STAMP(5)
        __syncthreads();
        EMSPEC_STAMP(1)
        // ---- column j - D is complete: stage "dB + colour" for it, and park the ring (its slot cleared)
        // (the thread id is laundered again: otherwise its 64-bit byte offset, computed for the twiddle loads at the top
        // of the frame, is kept for the sample prefetch below and spilled - a scratch store per frame that reaches HBM)
        tt = t;
        asm volatile("" : "+v"(tt));
        const int qlo = sj * (R >> 2), qhi = qlo + (R >> 2);
        {
            const int64_t col = j - D;
            if (tt < (R >> 2)) {
                const float4 e4 = reinterpret_cast<const float4*>(ring)[qlo + tt];
                // a finished quad among the resident cells is cleared here, by the thread that read it (the parked
                // cells are cleared in their register copy below)
                if (4 * (qlo + tt) >= PARKED_CELLS) {
                    float z;                                       // (a zero made here: hipcc otherwise keeps a zero quad in scratch)
                    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
                    reinterpret_cast<float4*>(ring)[qlo + tt] = make_float4(z, z, z, z);
                }
              if (col >= c0) {                                     // col < c1 holds: j <= c1 + D - 1
                const float d0 = cell_db_fast(dm, e4.x), d1 = cell_db_fast(dm, e4.y);
                const float d2 = cell_db_fast(dm, e4.z), d3 = cell_db_fast(dm, e4.w);
                const int i0 = cell_index(dm, d0), i1 = cell_index(dm, d1), i2 = cell_index(dm, d2), i3 = cell_index(dm, d3);
                const size_t o = ((size_t)s * C + col) * R + ((size_t)tt << 2);
                if (db) *reinterpret_cast<float4*>(db + o) = make_float4(d0, d1, d2, d3);
                if (rgba) *reinterpret_cast<uint4*>(rgba + o) = make_uint4(slut[i0], slut[i1], slut[i2], slut[i3]);
                if (index) *reinterpret_cast<uint32_t*>(index + o) =
                    (uint32_t)i0 | ((uint32_t)i1 << 8) | ((uint32_t)i2 << 16) | ((uint32_t)i3 << 24);
              }
            }
        }
        // (also after the last frame, whose parked copy is not used: the loop body stays free of frame-dependent branches,
        // which hipcc otherwise answers with copies of the sixteen pass-1 results and 40 spilled registers)
        if (fastring) {
            // 1024 rows and every parked quad a ring cell (the bench shape): plain reads, then ONE quad is cleared - the
            // finished column's 256 quads sit in register sj >> 2 of the threads of quarter sj & 3 (both wave-uniform), so
            // the clearing is a scalar jump to one group of four selects instead of two compares and four selects per quad
#pragma unroll
            for (int m = 0; m < NQ; ++m) park[m] = reinterpret_cast<const float4*>(ring)[tt + T * m];
            const int su = __builtin_amdgcn_readfirstlane(sj);
            const bool mine = (tt >> 8) == (su & 3);
#pragma unroll
            for (int m = 0; m < NQ; ++m)
                if ((su >> 2) == m)
                    park[m] = make_float4(mine ? 0.f : park[m].x, mine ? 0.f : park[m].y, mine ? 0.f : park[m].z, mine ? 0.f : park[m].w);
        } else {
#pragma unroll
        for (int m = 0; m < NQ; ++m) {
            // read first, select afterwards: no exec-masked branch per quad (every q lies inside the region:
            // 8 x 1024 quads = 128 KB of the 136 KB transform buffer the ring shares)
            const int q = tt + T * m;
            const float4 v4 = reinterpret_cast<const float4*>(ring)[q];
            const bool keep = q < nq4 && !(q >= qlo && q < qhi);
            park[m] = make_float4(keep ? v4.x : 0.f, keep ? v4.y : 0.f, keep ? v4.z : 0.f, keep ? v4.w : 0.f);
        }
        }
        EMSPEC_STAMP(6)
        __syncthreads();                                           // the next frame's FFT may overwrite the region
        EMSPEC_STAMP(1)
        sj += 1;
        sj -= sj >= slots ? slots : 0;
    }
    // ---- columns jhi-D+1 .. c1-1 (only when the stream ends inside this segment's reach): no later frame
    // exists, the ring is still in LDS and every earlier column's slot is dead, so no clearing is needed
    int te = t;            // laundered once more: the loop above must not carry this part's 64-bit offsets (they were spilled)
    asm volatile("" : "+v"(te));
    for (int64_t col = (jhi - D + 1 > c0 ? jhi - D + 1 : c0); col < c1; ++col) {
        if (te < (R >> 2)) {
            const int sl = (int)((col - (jlo - D)) % slots);       // slot of column c: (c - (jlo - D)) mod slots
            const float4 e4 = reinterpret_cast<const float4*>(ring)[sl * (R >> 2) + te];
            store_cells4<true>(dm, slut, e4, ((size_t)s * C + col) * R + ((size_t)te << 2), db, rgba, index);
        }
    }
    if constexpr (STAMP) {
        if ((t & 63) == 0) {
            unsigned long long* o = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (t >> 6)) * 8;
            // slot 7: low word = accumulate rounds (r8 kernel), high word = the walk's duration in 100 MHz ticks; the
            // shader clock it held = (sum of slots 0..6) / ticks * 100 MHz (MI355X_MICROARCH.md "DVFS give-back" item 6)
            acc_[7] = (acc_[7] & 0xFFFFFFFFull) | ((__builtin_amdgcn_s_memrealtime() - real0_) << 32);
            for (int i = 0; i < 8; ++i) o[i] = acc_[i];
        }
    }
}
#undef EMSPEC_STAMP

static hipError_t launch_fused16384(dim3 grid, const PlanDev& pl, const DbMap& m, const uint32_t* lut, const float* pcm,
                                    int64_t L, int64_t C, SegPlan seg, float* db, uint32_t* rgba, uint8_t* index,
                                    hipStream_t st, unsigned long long* stamps) {
    return pick_bool(emspec_plan_is_fast(pl), [&](auto FA) {
        auto go = [&](auto kernel) {
            return launch_k(kernel, grid, dim3(1024), fused16384_lds_bytes(pl.rows), st, pl, m, lut, pcm, L, C, seg, db, rgba, index, stamps);
        };
#ifdef EMSPEC_DIAG
        if (stamps) return go(fused16384_kernel<true, FA()>);   // the stamped build of the kernel the product runs for this plan
#endif
        return go(fused16384_kernel<false, FA()>);
    });
}

}  // namespace emspec
