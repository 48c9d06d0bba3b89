// exact_fused_lr.hip.inc — EXACT mode, N = 4096, one kernel, NO PARKING: the column ring's sparse low rows live in L2.
// Included by kernels.hip after exact_fused.hip.inc (whose kernel stays as the form for axes this one does not serve).
//
// Round 4's kernel (exact_fused.hip.inc) keeps the whole u64 ring (18 slots x 1024 rows x 8 B = 144 KB at hop 256) in LDS
// and lays the binary64 planes (64 KB) over its first 64 KB; every frame its F team parks the 8,192 cells under the planes
// in registers and puts them back: 2 of the frame's 7 trips through the LDS pipe and 2 of its 5 syncs serve nothing but
// that, and the scatter has to wait for the unpark (profiles/r04_exact64_phase_cycles.txt: a 13.4 k-cycle serial chain of
// which the LDS pipe's own floor is 6.8 k).
//
// On a log-frequency axis the rows are not hit evenly: row r collects the bins around fmin (fmax/fmin)^(r/R), so the lowest
// 456 of 1024 rows (20 .. 470 Hz at the default axis) receive the energy of ~40 of the frame's 2,049 bins - 2 % of the
// scatter - while holding 44 % of the ring's bytes.  This kernel keeps only rows >= RL of the ring in LDS,
//     [slots][R - RL] u64 = 82 KB at hop 256,   beside the 64 KB planes: no overlay, nothing to park,
// and rows < RL in a per-workgroup scratch in global memory ([slots][RL] u64, 66 KB per workgroup: L2-resident) that is
// touched by device-scope atomics ONLY: `global_atomic_add_x2` for the few low bins of a frame, `global_atomic_swap_x2`
// (read + clear in one) when the finished column leaves the ring.  Atomics of one agent to one address are serialised at
// the point of coherence, so no cache-line state can go stale; what has to be ordered is completion: a wave waits for
// vmcnt(0) before the workgroup barrier that ends its half-iteration, and every pair (add -> swap of that column,
// swap -> first add to the slot's next column) has such a barrier between them.  The scratch is all-zero between launches
// (every cell that is ever added to belongs to a column of the segment, and each of those is swapped out exactly once);
// the launcher clears it once per launch all the same, so a launch that was cut short cannot leak into the next.
//
// Same two teams and roles as round 4's kernel, one frame per half-iteration:
//   role F (LDS side):  take the finished column out (LDS rows: read + clear; low rows: swaps) and scatter the team's
//        previous frame (ds_add_u64 / the rare global adds), store pass A | passes B, C, D (wave-local) | read the twelve
//        spectrum values of the thread's four bins - THREE phases, two arrival-counter syncs of the F team + the closing
//        workgroup barrier (round 4: five phases, four syncs + the barrier);
//   role V (VALU side): unchanged - conjugate split, branch-free per-bin core, run pre-summing, fetch + pass A of the
//        team's next frame, all in registers.
// Same butterflies, same per-bin core, integer accumulation: bit-identical to the bit model (oracle/emspec_exact.c) and to
// round 4's kernel; the whole exact suite runs on it.
namespace emspec {
namespace exl {
constexpr int LOG2N = 12, N = 4096, T = 512;
using ex::XTwLds4;
using ex::tw4_slot;
using ex::XBinF;
using ex::exact_core_fast;
using exf::bar_lds;
using exf::bar_only;
using exf::edge_cells;

using ex::XTwRegs4;   // the four twiddle sources of a radix-8 pass from registers

// Byte offsets into the planes that depend on the thread only, one 32-byte row per thread of a team: the bases of passes B, C
// and D and the five computed spectrum positions of phase 3 (the kernel is bound by vector issue - DESIGN.md section 4.6 - and
// computing these per frame was ~110 of a thread's ~1,650 vector instructions per frame pair: two bit reversals' worth of
// shifts per position.  Two 16-byte loads per frame instead, issued at the head of role F; the table is built at compile time.)
//   [0] pass B base  swz(hi*512 + lo)         point i at  base ^ (cswz(i << 6) << 3)   (the swizzle is GF(2)-linear, fused_r8.hip.inc)
//   [1] pass C base  swz((t>>3)*64 + (t&7))   point i at  base ^ (cswz(i << 3) << 3)
//   [2] pass D base  swz(8 t)                 point i at  base ^ (i << 3)
//   [3] fB = zpos(4bg)   [4] fL = zpos(4bg-4) + 3072   [5] fH = zpos(4bg+4)   [6] mB = zpos(N-4bg)   [7] mL = zpos(N-4bg-4)
typedef __attribute__((address_space(3))) double LdsDouble;
struct LrPos { int v[T][8]; };
constexpr int c_brev12(int k) {
    k &= N - 1;
    int r = 0;
    for (int b = 0; b < LOG2N; ++b) r |= ((k >> b) & 1) << (LOG2N - 1 - b);
    return r;
}
constexpr int c_zpos(int k) { return f8::cswz(c_brev12(k)); }
// Small sizes (template parameter S of the kernel: N = 4096 >> S): the 4096-point carrier network with its first S stages
// skipped is 2^S independent (4096 >> S)-point networks side by side (fused_small.hip.inc), so a team runs FPT = 2^S consecutive
// frames through the planes at once.  Frame slot bf of a block lives in carrier part bf; its spectrum sample Z[m] ends at
// zpos((m << S) | bitrev_S(bf)).  A team's 512 threads take FPT x (512 >> S) groups of 4 bins: wave w takes frame slot
// w mod FPT, its lanes sit (8 >> S) groups apart.  Bin e of an aligned group of four lies at (base position) XOR c_cc(S, e): the
// bits of e land, bit-reversed, on position bits (11 - S) and (10 - S), which the swizzle reads from S = 1 on, so it is an XOR
// with a compile-time constant, not an added offset (S = 0: the same thing, the bits 10 and 11 are beyond the swizzle).
constexpr int c_cc(int S, int e) { return f8::cswz(c_brev12(e << S)); }
constexpr LrPos make_lrpos(int S) {
    LrPos p{};
    const int NS = N >> S, FPT = 1 << S;
    for (int t = 0; t < T; ++t) {
        const int bf = (t >> 6) & (FPT - 1);
        const int bg = ((t & 63) << (3 - S)) | (t >> (6 + S));
        const int bpart = S == 2 ? (((bf & 1) << 1) | (bf >> 1)) : bf;   // bitrev_S(bf)
        p.v[t][0] = f8::cswz(((t >> 6) << 9) + (t & 63)) * 8;
        p.v[t][1] = f8::cswz(((t >> 3) << 6) + (t & 7)) * 8;
        p.v[t][2] = f8::cswz(t << 3) * 8;
        p.v[t][3] = c_zpos((((4 * bg) & (NS - 1)) << S) | bpart) * 8;
        p.v[t][4] = (c_zpos((((4 * bg - 4) & (NS - 1)) << S) | bpart) ^ c_cc(S, 3)) * 8;
        p.v[t][5] = c_zpos((((4 * bg + 4) & (NS - 1)) << S) | bpart) * 8;
        p.v[t][6] = c_zpos((((NS - 4 * bg) & (NS - 1)) << S) | bpart) * 8;
        p.v[t][7] = c_zpos((((NS - 4 * bg - 4) & (NS - 1)) << S) | bpart) * 8;
    }
    return p;
}
__device__ const LrPos g_lrpos = make_lrpos(0);
__device__ const LrPos g_lrpos1 = make_lrpos(1);
__device__ const LrPos g_lrpos2 = make_lrpos(2);
template <int S>
__device__ __forceinline__ const int4* lrpos_row(int tt) {
    if constexpr (S == 0) return reinterpret_cast<const int4*>(&g_lrpos.v[tt][0]);
    else if constexpr (S == 1) return reinterpret_cast<const int4*>(&g_lrpos1.v[tt][0]);
    else return reinterpret_cast<const int4*>(&g_lrpos2.v[tt][0]);
}
// (lr_slots, the ring's slots, and ring_cells / mask_words of the LDS budget - planes + ring + edges + pass twiddles + LUT +
// counters + one bit per low-row cell: emspec_kernel_plan.h)
// stages U0..2 of a radix-8 register pass (pass A of the small sizes skips the carrier's first S stages)
template <int U0, class W>
__device__ __forceinline__ void xstages8_from(double (&vr)[8], double (&vi)[8], const W& w) {
    if constexpr (U0 <= 0) ex::xstage8<0>(vr, vi, w);
    if constexpr (U0 <= 1) ex::xstage8<1>(vr, vi, w);
    ex::xstage8<2>(vr, vi, w);
}


#define EXL_STAMP(slot)                                                            \
    if constexpr (STAMP) {                                                         \
        const unsigned long long now_ = __builtin_readcyclecounter();              \
        acc_[slot] += now_ - last_;                                                \
        last_ = now_;                                                              \
    }

// RL: rows [0, RL) of every slot live in `low` (global, [blocks][slots][RL]); RH = R - RL rows in LDS.  RL % 4 == 0.
// S: the size, N = 4096 >> S (0, 1, 2): FPT = 2^S frames per team and half-iteration (see make_lrpos)
// (The timing builds this kernel had - pass A at the head of role F, and four ablations with wrong results by design - are
// retired: docs/HISTORY.md "Retired kernel forms".)
template <bool STAMP, bool FASTX, int S = 0>
__global__ __launch_bounds__(1024, 4) void exact_fused4096_lr_kernel(
    ExactPlanDev pl, ExactDbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, int slots, int RL, unsigned long long* __restrict__ lowbase, float* __restrict__ db,
    uint32_t* __restrict__ rgba, uint8_t* __restrict__ index, unsigned long long* __restrict__ stamps) {
    using ex::YTd;
    constexpr int NS = N >> S;          // FFT size
    constexpr int FPT = 1 << S;         // frames per team and half-iteration
    constexpr int RPF = 8 >> S;         // sample registers per frame (512 samples each)
    static_assert(S >= 0 && S <= 2 && (S == 0 || !STAMP), "the stamped build exists for N = 4096 only");
    unsigned long long acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last_ = 0;
    extern __shared__ double smemd[];
    const int R = pl.rows, D = pl.D, RH = R - RL;
    double* sre = smemd;
    double* sim = smemd + N;
    unsigned long long* ring = reinterpret_cast<unsigned long long*>(smemd + 2 * N);   // [slots][RH]
    double* seb = smemd + 2 * N + ring_cells(RH, slots);                // [R+1]
    double2* stwB = reinterpret_cast<double2*>(seb + edge_cells(R));    // [4][64]
    double2* stwC = stwB + 4 * 64;                                      // [4][8]
    uint32_t* slut = reinterpret_cast<uint32_t*>(stwC + 4 * 8);         // [256]
    unsigned* cnt = slut + 256;                                         // [2 teams][4] arrival counters
    unsigned* lmask = cnt + 8;                                          // [slots][mask_words(RL)]: low-row cells that took an add
    const int MW = mask_words(RL);

    const int tid = threadIdx.x, h = tid >> 9, t = tid & 511;
    int s;
    int64_t c0, c1;
    if (!seg_of_block(sp, C, s, c0, c1)) return;
    // role F addresses the planes by absolute LDS byte address (g_lrpos): they must start the workgroup's LDS
    if ((unsigned)(size_t)(__attribute__((address_space(3))) char*)smemd != 0u) {
        if (tid == 0) g_kernel_error = 1;
        return;
    }
    const int64_t j0 = c0 - D > 0 ? c0 - D : 0;
    const int64_t jstop = c1 + D < C ? c1 + D : C;
    const float* x0 = pcm + (size_t)s * L;
    unsigned long long* low = lowbase + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(slots * RL);

    // ---- workgroup set-up
    for (int q = tid; q < ring_cells(RH, slots); q += 1024) ring[q] = 0ull;
    for (int r = tid; r <= R; r += 1024) seb[r] = pl.ebin[r];
    if (tid < 256) slut[tid] = lut[tid];
    // (pl.tw is the NS-point table: carrier index >> S - the double argument is identical, fused_small.hip.inc)
    if (tid < 4 * 64) stwB[tid] = pl.tw[f8::tw_index8<3>(tw4_slot(tid >> 6), tid & 63) >> S];
    else if (tid < 4 * 64 + 4 * 8) stwC[tid - 4 * 64] = pl.tw[f8::tw_index8<6>(tw4_slot((tid - 4 * 64) >> 3), (tid - 4 * 64) & 7) >> S];
    else if (tid < 4 * 64 + 4 * 8 + 8) cnt[tid - (4 * 64 + 4 * 8)] = 0u;
    for (int q = tid; q < slots * MW; q += 1024) lmask[q] = 0u;
    const double rs = 2.0 / (double)NS;
    const double ramp0 = (double)(t - NS / 2) * rs;   // ramp of this thread's point 0 of a frame; register ii of the frame lies 512 ii samples = ii 1024 / NS further (exact)
    constexpr double rstep = 1024.0 / (double)NS;
    // the four twiddle sources of pass A (stages 0..2; slots 0, 1, 4, 6 - the other three are a quarter turn on) depend on the
    // thread only: registers for the whole walk.  (Round 4's kernel loads them per frame, one exposed L2 round trip per
    // stage in the V role - hidden there behind the F team's chain, on the critical path here.)
    // (the generic per-bin core - custom axes, reassignment off, no power floor - needs the sixteen registers itself: that form
    // loads them per frame, as round 4 did; with them resident it ran at 128 VGPRs and three spilled dwords reloaded per bin)
    double2 twA[4];
    auto load_twA = [&](int tq) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) twA[r4] = pl.tw[f8::tw_index8<0>(tw4_slot(r4), tq) >> S];   // (S > 0: only the sources of stages S..2 are used)
    };
    load_twA(t);

    // What a team hands from one role to the next, in registers.  After role F: the twelve spectrum values of the thread's
    // bins, carry[4i .. 4i+3] = Z[4bg-1+i] (re, im), Z[N-4bg+1-i] (re, im).  After role V: pass A of the next frame (re 0..7,
    // im 8..15), the four fixed-point energies (16..19, bit patterns) and their cell codes (20, 21: two ints each):
    // code >= 0: cell of the LDS ring (slot * RH + row - RL); code <= -2: -2 - code = slot * 1024 + row of a low row (the
    // scratch cell is slot * RL + row).  A result with nothing to add carries an LDS cell of the lane's own and a zero.
    double carry[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) carry[i] = 0.0;
    carry[20] = carry[21] = __hiloint2double(0, 0);
    if (h == 0) {   // pass A of team 0's first block, frames j0 .. (team 1's first role V, at k = 0, runs pass A of block 1 itself)
        double vr[8], vi[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t jq = j0 + (i / RPF) < jstop ? j0 + (i / RPF) : jstop - 1;
            const double xv = (double)x0[jq * pl.hop + t + T * (i % RPF)];
            vr[i] = xv;
            vi[i] = xv * ((double)(t + T * (i % RPF) - NS / 2) * rs);
        }
        xstages8_from<S>(vr, vi, XTwRegs4{twA});
#pragma unroll
        for (int i = 0; i < 8; ++i) { carry[i] = vr[i]; carry[8 + i] = vi[i]; }
    }
    __syncthreads();
    ex::RowLookup64 lk;
    lk.init(seb, R, pl.log_rows);
    unsigned long long real0_ = 0;
    if constexpr (STAMP) { last_ = __builtin_readcyclecounter(); real0_ = __builtin_amdgcn_s_memrealtime(); }
    unsigned visits = 0;   // role-F visits of this team so far (x 8 waves = the arrival counters' target)
    // F-team sync after a phase: this wave's LDS operations of the phase are issued - the LDS pipe serves one wave's operations
    // in order, so its arrival is counted behind them - then wait for the eight waves of the team.  Every wave arrives before
    // it polls, so the wait always ends; the spin is bounded all the same and a timeout raises g_kernel_error.
    auto team_arrive = [&](int ph, int lane) {
        asm volatile("" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(cnt + 4 * h + ph, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm volatile("" ::: "memory");
    };
    auto team_wait = [&](int ph) {
        unsigned spins = 0;
        while ((int)(__hip_atomic_load(cnt + 4 * h + ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - 8u * visits) < 0) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1u << 20)) { g_kernel_error = 1; break; }
        }
        asm volatile("" ::: "memory");
    };

    // half-iterations k = 0 .. klast: the last column c1-1 leaves the ring at the first k with j0 + (k-3) FPT - D + FPT - 1 >= c1 - 1
    // (FPT = 1: k = c1 - 1 + 3 + D - j0)
    const int klast = (int)((c1 + D - j0 + FPT - 1) / FPT) + 2;
    int sk = 0;   // ring slot of column j0 + k
#pragma unroll 1
    for (int k = 0; k <= klast; ++k) {
        int tt = t;
        asm volatile("" : "+v"(tt));   // addresses are recomputed per half-iteration, not kept (and spilled) across the loop
        if (((k + h) & 1) == 0) {
            // ================= role F: the LDS side, block k = frames jf .. jf + FPT - 1 (past the last frame: a repeat, results dropped)
            const int64_t jf = j0 + (int64_t)k * FPT;
            visits += 1;
            __builtin_amdgcn_s_setprio(1);
            const int4* const ptab = lrpos_row<S>(tt);
            const int4 pa = ptab[0], pb = ptab[1];   // needed from phase 2 on
            // plane accesses by ABSOLUTE LDS byte address: the planes start the workgroup's LDS (checked at the head of the kernel),
            // and an address formed from the extern array's symbol costs one more vector add per access - its value is not
            // known before the link, so the compiler cannot fold it
            auto re_at = [&](int boff) -> LdsDouble& { return *reinterpret_cast<LdsDouble*>((unsigned)boff); };
            auto im_at = [&](int boff) -> LdsDouble& { return *reinterpret_cast<LdsDouble*>((unsigned)boff + (unsigned)(N * 8)); };
            // -- phase 1: the finished column j0+k-3-D leaves the ring (four cells per thread of the team's first four waves;
            // its dB + colour arithmetic fills their wait at the sync below), the results of frame j0+k-2 go in, pass A is stored
            const int64_t cfin = jf - 3 * FPT - D;   // the first of the FPT columns that leave now
            // (separate registers for the two sources: the swaps' results are not needed before the second sync, and a shared
            // set would make the join of the two branches wait for them here, at the head of the F chain)
            unsigned long long g0 = 0ull, g1 = 0ull, g2 = 0ull, g3 = 0ull;
            unsigned long long f0 = 0ull, f1 = 0ull, f2 = 0ull, f3 = 0ull;
            int sf = sk - 3 * FPT - D;
            sf += sf < 0 ? slots : 0;
            if constexpr (S > 0) sf += sf < 0 ? slots : 0;   // (3 FPT + D can exceed the 2 D + 2 FPT slots once)
            // which quad of four cells this thread takes out here: S = 0: quad tt of the one column (low rows: swaps, the others
            // from LDS).  S > 0: the FPT columns' LOW quads, one per thread (FPT RL / 4 <= 512), swapped here and finished at the
            // second sync like S = 0's; their LDS quads are read, cleared and finished between this phase's arrival and wait.
            bool finlow, finlds = false;
            int64_t lcol = cfin;   // column and first row of the thread's low quad, its ring slot
            int lcell = 4 * tt, sfl = sf;
            if constexpr (S == 0) {
                const bool fin = cfin >= c0 && cfin < c1 && tt < (R >> 2);
                finlow = fin && 4 * tt < RL;
                finlds = fin && 4 * tt >= RL;
            } else {
                const int lq = RL >> 2;
                int lcc = 0;
#pragma unroll
                for (int c = 1; c < FPT; ++c) lcc += tt >= c * lq ? 1 : 0;
                lcol = cfin + lcc;
                lcell = (tt - lcc * lq) << 2;
                sfl = sf + lcc;
                sfl -= sfl >= slots ? slots : 0;
                finlow = tt < FPT * lq && lcol >= c0 && lcol < c1;
            }
            if (finlow) {   // low rows: read + clear in one returning atomic each (the longest latency: issued first) - but only
                            // the cells that took an add (a bit per cell in LDS): most of a column's low rows are empty, and a
                            // device-scope atomic is a 32-byte request to the memory side whether the cell holds anything or not
                const int ql = lcell >> 2;
                unsigned* mw = lmask + sfl * MW + (ql >> 3);                   // rows 4 ql .. 4 ql + 3: bits 4 (ql & 7) .. + 3
                const unsigned sh = 4u * (unsigned)(ql & 7);
                const unsigned bits = (*mw >> sh) & 0xFu;
                unsigned long long* lp = low + sfl * RL + lcell;
                if (bits & 1u) g0 = __hip_atomic_exchange(lp + 0, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (bits & 2u) g1 = __hip_atomic_exchange(lp + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (bits & 4u) g2 = __hip_atomic_exchange(lp + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (bits & 8u) g3 = __hip_atomic_exchange(lp + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (bits) __hip_atomic_fetch_and(mw, ~(0xFu << sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (finlds) {
                ulonglong2* cp = reinterpret_cast<ulonglong2*>(ring + sf * RH + (4 * tt - RL));
                const ulonglong2 va = cp[0], vb = cp[1];
                cp[0] = ulonglong2{0ull, 0ull};
                cp[1] = ulonglong2{0ull, 0ull};
                f0 = va.x; f1 = va.y; f2 = vb.x; f3 = vb.y;
            }
            {
                const int ca = __double2hiint(carry[20]), cb = __double2loint(carry[20]);
                const int cc = __double2hiint(carry[21]), cd = __double2loint(carry[21]);
                const int own = 2 * tt;   // a cell of this lane's own for the zero-adds (no exec-mask branch per add)
                __hip_atomic_fetch_add(ring + (ca >= 0 ? ca : own), ca >= 0 ? (unsigned long long)__double_as_longlong(carry[16]) : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(ring + (cb >= 0 ? cb : own + 1), cb >= 0 ? (unsigned long long)__double_as_longlong(carry[17]) : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(ring + (cc >= 0 ? cc : own), cc >= 0 ? (unsigned long long)__double_as_longlong(carry[18]) : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(ring + (cd >= 0 ? cd : own + 1), cd >= 0 ? (unsigned long long)__double_as_longlong(carry[19]) : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // the frame's few low bins (wave-uniform test; a lane or two per wave take the branch)
                if (__builtin_amdgcn_ballot_w64((ca | cb | cc | cd) < 0) != 0ull) {
                    auto low_add = [&](int code, double qbits) {
                        if (code < 0) {
                            const int g = -2 - code, sl = g >> 10, row = g & 1023;
                            __hip_atomic_fetch_add(low + (__mul24(sl, RL) + row), (unsigned long long)__double_as_longlong(qbits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_fetch_or(lmask + __mul24(sl, MW) + (row >> 5), 1u << (row & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    };
                    low_add(ca, carry[16]);
                    low_add(cb, carry[17]);
                    low_add(cc, carry[18]);
                    low_add(cd, carry[19]);
                }
            }
            EXL_STAMP(0)
            {
                const int a0 = f8::swz(tt), a1 = a0 ^ 8;   // swz(tt + 512 i) = (swz(tt) ^ 8 (i & 1)) + 512 i
#pragma unroll
                for (int i = 0; i < 8; ++i) { const int p = ((i & 1) ? a1 : a0) + T * i; sre[p] = carry[i]; sim[p] = carry[8 + i]; }
            }
            EXL_STAMP(1)
            team_arrive(1, tt & 63);
            auto finish = [&](int64_t col, int cell, unsigned long long q0, unsigned long long q1, unsigned long long q2, unsigned long long q3) {
                const ex::CellOut o0 = ex::exact_cell(dm, q0), o1 = ex::exact_cell(dm, q1);
                const ex::CellOut o2 = ex::exact_cell(dm, q2), o3 = ex::exact_cell(dm, q3);
                const size_t o = ((size_t)s * C + col) * R + cell;
                if (db) *reinterpret_cast<float4*>(db + o) = make_float4(o0.db, o1.db, o2.db, o3.db);
                if (rgba) *reinterpret_cast<uint4*>(rgba + o) = make_uint4(slut[o0.index], slut[o1.index], slut[o2.index], slut[o3.index]);
                if (index) *reinterpret_cast<uint32_t*>(index + o) =
                    (uint32_t)o0.index | ((uint32_t)o1.index << 8) | ((uint32_t)o2.index << 16) | ((uint32_t)o3.index << 24);
            };
            // stage "dB + colour" of the column taken out above, between this wave's arrival and its wait: the rows that came
            // from LDS here, the low rows (whose swaps are still in flight) at the second sync
            if constexpr (S == 0) {
                if (finlds) finish(cfin, 4 * tt, f0, f1, f2, f3);
            } else {
                const int hq = RH >> 2;   // LDS quads per column
                for (int q = tt; q < FPT * hq; q += T) {
                    int cc = 0;
#pragma unroll
                    for (int c = 1; c < FPT; ++c) cc += q >= c * hq ? 1 : 0;
                    const int64_t col = cfin + cc;
                    if (col >= c0 && col < c1) {
                        const int cell = RL + ((q - cc * hq) << 2);
                        int sl = sf + cc;
                        sl -= sl >= slots ? slots : 0;
                        ulonglong2* cp = reinterpret_cast<ulonglong2*>(ring + sl * RH + (cell - RL));
                        const ulonglong2 va = cp[0], vb = cp[1];
                        cp[0] = ulonglong2{0ull, 0ull};
                        cp[1] = ulonglong2{0ull, 0ull};
                        finish(col, cell, va.x, va.y, vb.x, vb.y);
                    }
                }
                // low quads beyond the one per thread that was swapped out at the head of the phase (more than 512 low rows per
                // block: N = 1024 at hop < 128): swapped and finished here, one after the other - rare shapes, and few cells are set
                const int lq = RL >> 2;
                for (int q = tt + T; q < FPT * lq; q += T) {
                    int cc = 0;
#pragma unroll
                    for (int c = 1; c < FPT; ++c) cc += q >= c * lq ? 1 : 0;
                    const int64_t col = cfin + cc;
                    if (col >= c0 && col < c1) {
                        const int ql = q - cc * lq;
                        int sl = sf + cc;
                        sl -= sl >= slots ? slots : 0;
                        unsigned* mw = lmask + sl * MW + (ql >> 3);
                        const unsigned sh = 4u * (unsigned)(ql & 7);
                        const unsigned bits = (*mw >> sh) & 0xFu;
                        unsigned long long* lp = low + sl * RL + 4 * ql;
                        unsigned long long h0 = 0ull, h1 = 0ull, h2 = 0ull, h3 = 0ull;
                        if (bits & 1u) h0 = __hip_atomic_exchange(lp + 0, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (bits & 2u) h1 = __hip_atomic_exchange(lp + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (bits & 4u) h2 = __hip_atomic_exchange(lp + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (bits & 8u) h3 = __hip_atomic_exchange(lp + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (bits) __hip_atomic_fetch_and(mw, ~(0xFu << sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        finish(col, 4 * ql, h0, h1, h2, h3);
                    }
                }
            }
            team_wait(1);
            EXL_STAMP(5)
            // -- phase 2: passes B, C, D on this wave's 512 positions
            {
                {   // pass B = stages 3..5: p = hi*512 + i*64 + lo
                    double vr[8], vi[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = pa.x ^ (f8::cswz(i << 6) << 3); vr[i] = re_at(p); vi[i] = im_at(p); }
                    ex::xstages8(vr, vi, XTwLds4<64>{stwB + (tt & 63)});
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = pa.x ^ (f8::cswz(i << 6) << 3); re_at(p) = vr[i]; im_at(p) = vi[i]; }
                    wave_lds_sync();
                }
                {   // pass C = stages 6..8: p = (t >> 3)*64 + i*8 + (t & 7)
                    double vr[8], vi[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = pa.y ^ (f8::cswz(i << 3) << 3); vr[i] = re_at(p); vi[i] = im_at(p); }
                    ex::xstages8(vr, vi, XTwLds4<8>{stwC + (tt & 7)});
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = pa.y ^ (f8::cswz(i << 3) << 3); re_at(p) = vr[i]; im_at(p) = vi[i]; }
                    wave_lds_sync();
                }
                {   // pass D = stages 9..11: p = 8 t + i, twiddles are constants
                    double vr[8], vi[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = pa.z ^ (i << 3); vr[i] = re_at(p); vi[i] = im_at(p); }
                    ex::xfft_stages<LOG2N - S, 9 - S, 3>(vr, vi, 0, pl.tw);   // the last three stages of the NS-point network
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = pa.z ^ (i << 3); re_at(p) = vr[i]; im_at(p) = vi[i]; }
                }
            }
            EXL_STAMP(2)
            team_arrive(2, tt & 63);
            // (laundered: the compiler otherwise starts the cells' arithmetic - and so the wait for the swaps - where they were issued)
            asm volatile("" : "+v"(g0), "+v"(g1), "+v"(g2), "+v"(g3));
            if (finlow) finish(lcol, lcell, g0, g1, g2, g3);
            team_wait(2);
            EXL_STAMP(5)
            // -- phase 3: the spectrum values of this thread's bins 4 bg .. 4 bg + 3 (lanes 32 bins apart): F(i) = Z[4bg-1+i],
            // M(i) = Z[N-4bg+1-i], i = 0..5, read in place (Z[k] sits at swz(bitrev12(k))); five computed positions, the
            // rest are immediate offsets (exact_fused.hip.inc)
            {
                const int fB = pa.w, fL = pb.x, fH = pb.y, mB = pb.z, mL = pb.w;   // byte offsets (g_lrpos)
                // bins 1, 2, 3 of an aligned group: the base position XOR a compile-time constant (make_lrpos; S = 0: the constants
                // are 2048, 1024, 3072 elements and lie beyond the bases' bits, so the XOR is the addition it used to be)
                // (S = 0 keeps the addition: it folds into the LDS instruction's immediate offset, an XOR is a vector instruction)
                constexpr int c1b = c_cc(S, 1) * 8, c2b = c_cc(S, 2) * 8, c3b = c_cc(S, 3) * 8;
                const int pf[6] = {fL, fB, S ? fB ^ c1b : fB + c1b, S ? fB ^ c2b : fB + c2b, S ? fB ^ c3b : fB + c3b, fH};
                const int pm[6] = {S ? mB ^ c1b : mB + c1b, mB, S ? mL ^ c3b : mL + c3b, S ? mL ^ c2b : mL + c2b, S ? mL ^ c1b : mL + c1b, mL};
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    carry[4 * i] = re_at(pf[i]); carry[4 * i + 1] = im_at(pf[i]);
                    carry[4 * i + 2] = re_at(pm[i]); carry[4 * i + 3] = im_at(pm[i]);
                }
            }
            EXL_STAMP(3)
            // this wave's global atomics and column stores are complete before the barrier that lets the other team's
            // role F touch the same slots (issued a whole role ago: nothing is waited for in practice)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bar_lds();
            EXL_STAMP(5)
        } else {
            // ================= role V: the VALU side; per-bin stage of block k - 1 (this thread: its frame jv), pass A of block k + 1
            const int bf = S ? (tt >> 6) & (FPT - 1) : 0;          // frame slot of this thread's bins within the block
            const int64_t jv = j0 + (int64_t)(k - 1) * FPT + bf;
            const bool activeV = k >= 1 && jv < jstop;
            __builtin_amdgcn_s_setprio(0);
            // the team's next block (past the end: the last frame once more; its results are dropped)
            float xs[8];
            if constexpr (S == 0) {
                const int64_t jn = jv + 2 < jstop ? jv + 2 : jstop - 1;
                const float* x = x0 + jn * pl.hop;
#pragma unroll
                for (int i = 0; i < 8; ++i) xs[i] = x[tt + T * i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int64_t jq = j0 + (int64_t)(k + 1) * FPT + (i / RPF);
                    const int64_t jn = jq < jstop ? jq : jstop - 1;
                    xs[i] = x0[jn * pl.hop + tt + T * (i % RPF)];
                }
            }
            int skv = sk - FPT + bf;   // ring slot of column jv
            skv += skv < 0 ? slots : 0;
            if constexpr (S > 0) skv -= skv >= slots ? slots : 0;
            const int jrel = (int)(jv - c0);
            const unsigned span = (unsigned)(c1 - c0);
            const int bg = ((tt & 63) << (3 - S)) | (tt >> (6 + S));
            long long rq[4];
            int rc[4];
            const double kd0 = (double)(4 * bg), Dd = (double)D;
            // conjugate split of the twelve spectrum values role F left (exact.hip.inc: split_d)
            YTd yt[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) yt[i] = ex::split_d(carry[4 * i], carry[4 * i + 1], carry[4 * i + 2], carry[4 * i + 3]);
            auto bin = [&](int e) {
                XBinF o;
                if constexpr (FASTX) {
                    o = exact_core_fast(pl, seb, kd0 + (double)e, Dd, yt[e], yt[e + 1], yt[e + 2]);
                } else {
                    const ex::XBin g = ex::exact_core(pl, lk, 4 * bg + e, yt[e], yt[e + 1], yt[e + 2]);
                    o = XBinF{g.q, g.dcol, g.row};
                }
                const bool ok = activeV & (o.row >= 0) & ((unsigned)(jrel + o.dcol) < span);
                int sl = skv + o.dcol;
                sl += sl < 0 ? slots : 0;
                sl -= sl >= slots ? slots : 0;
                const int hi = __mul24(sl, RH) + (o.row - RL);        // the LDS ring's cell (rows >= RL)
                const int lo = -2 - ((sl << 10) + o.row);             // a low row: (slot, row) as a code <= -2
                const int cell = o.row >= RL ? hi : lo;
                rc[e] = ok ? cell : -1;
                rq[e] = ok ? o.q : 0ll;
            };
            EXL_STAMP(6)
            bin(0);
            bin(1);
            bin(2);
            bin(3);
            // a lane's consecutive bins often share a cell: sum such runs first (integer adds: any order gives the same sum)
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const bool same = rc[e] != -1 && rc[e] == rc[e + 1];
                rq[e + 1] += same ? rq[e] : 0ll;
                rq[e] = same ? 0ll : rq[e];
                rc[e] = same ? -1 : rc[e];
            }
            // nothing to add: a zero into an LDS cell of this lane's own (2 tt + e mod 2: distinct per lane, no conflict)
#pragma unroll
            for (int e = 0; e < 4; ++e) rc[e] = rc[e] == -1 ? 2 * tt + (e & 1) : rc[e];
            double vr[8], vi[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double xv = (double)xs[i];
                vr[i] = xv;
                vi[i] = xv * (ramp0 + rstep * (double)(i % RPF));   // = (n - NS/2) 2/NS exactly, n = t + 512 (i mod RPF)
            }
            if constexpr (!FASTX) load_twA(tt);
            xstages8_from<S>(vr, vi, XTwRegs4{twA});
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) { carry[i] = vr[i]; carry[8 + i] = vi[i]; }
            carry[22] = carry[23] = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) carry[16 + e] = __longlong_as_double(rq[e]);
            carry[20] = __hiloint2double(rc[0], rc[1]);
            carry[21] = __hiloint2double(rc[2], rc[3]);
            __builtin_amdgcn_sched_barrier(0);
            EXL_STAMP(6)
            bar_only();
            EXL_STAMP(7)
        }
        sk += FPT;
        sk -= sk >= slots ? slots : 0;
    }
    if constexpr (STAMP) {
        if ((tid & 63) == 0) {
            unsigned long long* o = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (tid >> 6)) * 8;
            acc_[7] = (acc_[7] & 0xFFFFFFFFull) | ((__builtin_amdgcn_s_memrealtime() - real0_) << 32);
            for (int i = 0; i < 8; ++i) o[i] = acc_[i];
        }
    }
}
#undef EXL_STAMP

}  // namespace exl

// (The shapes this kernel serves - N = 4096 / 2048 / 1024, rows a multiple of 4 - the rows that stay in LDS and RL, the low rows
// per slot that live in the global scratch, and whether an AXIS is served: exact_lr_low_rows and exact_route, emspec_kernel_plan.h)

// segments: the rounds-by-efficiency choice with this kernel's floor and pipeline fill (emspec_seg_plan.h)
static int64_t exact_lr_seglen(int n, const ExactPlanDev& pl, int S, int64_t C) {
    return exact_lr_seglen(device_cus(), n, S, C, pl.D, diag_seglen());
}

size_t exact_fused_lr_scratch_bytes(int n, const ExactPlanDev& pl, int rl, int S, int64_t C) {
    if (rl <= 0 || S <= 0 || C <= 0 || exact_lr_skip(n) < 0) return 0;
    const int slots = exl::lr_slots(exact_lr_skip(n), pl.D);
    const int64_t seg = exact_lr_seglen(n, pl, S, C);
    return (size_t)scratch_groups((C + seg - 1) / seg, S) * (size_t)slots * (size_t)rl * 8;
}

hipError_t launch_exact_fused_lr(int n, const ExactPlanDev& pl, const ExactDbMap& m, const uint8_t* lut, const float* pcm,
                                 int64_t L, int S, int64_t C, int rl, unsigned long long* low, size_t low_bytes, float* db,
                                 uint8_t* rgba, uint8_t* index, hipStream_t st, unsigned long long* stamps,
                                 int64_t* stamp_groups) {
    const int skip = exact_lr_skip(n);
    if (skip < 0) return hipErrorNotSupported;
    if (S <= 0 || C <= 0) return hipSuccess;
    if (S > 65535) return hipErrorInvalidValue;
#ifndef EMSPEC_DIAG
    if (stamps || stamp_groups) return hipErrorNotSupported;
#endif
    if (skip > 0 && (stamps || stamp_groups)) return hipErrorNotSupported;   // the stamped build exists for N = 4096 only
    const int slots = exl::lr_slots(skip, pl.D);
    const int rh = pl.rows - rl;
    if (!exact_lr_split_ok(pl.rows, rl, slots)) return hipErrorInvalidValue;
    const int64_t seg = exact_lr_seglen(n, pl, S, C);
    const int64_t nseg = (C + seg - 1) / seg;
    if (!exact_fused_grid_ok(nseg, seg)) return hipErrorInvalidValue;
    if (stamp_groups) *stamp_groups = nseg * S;
#ifdef EMSPEC_DIAG
    if ((stamps || stamp_groups) && !stamps) return hipSuccess;
#endif
    const SegPlan sp{(int)seg, 1 << 30, (int)seg, 0};
    const size_t lds = exact_lr_lds_bytes(pl.rows, rh, slots);
    const uint32_t* l32 = reinterpret_cast<const uint32_t*>(lut);
    uint32_t* r32 = reinterpret_cast<uint32_t*>(rgba);
    // streams per launch: as many as the low-row scratch has slices for ([group][slots][rl]; emspec_seg_plan.h)
    const size_t per_group = (size_t)slots * (size_t)rl * 8;
    if (rl > 0 && (!low || !scratch_holds_a_stream(low_bytes, per_group, nseg))) return hipErrorInvalidValue;
    const int64_t s_per = streams_per_launch(S, nseg, low_bytes, per_group);
    if (stamps && s_per < S) return hipErrorNotSupported;   // the stamped build runs one launch
    const size_t col_cells = (size_t)C * pl.rows;
    auto run = [&](auto kernel) -> hipError_t {   // (`stamps` is null unless the kernel is the stamped build)
        for (int64_t s0 = 0; s0 < S; s0 += s_per) {
            const int sc = (int)std::min<int64_t>(s_per, S - s0);
            hipError_t e;
            if (rl > 0 && (e = hipMemsetAsync(low, 0, per_group * (size_t)nseg * (size_t)sc, st)) != hipSuccess) return e;
            e = launch_k(kernel, dim3((unsigned)nseg, (unsigned)sc), dim3(1024), lds, st, pl, m, l32, pcm + (size_t)s0 * L, L, C, sp, slots,
                         rl, low, db ? db + (size_t)s0 * col_cells : nullptr, r32 ? r32 + (size_t)s0 * col_cells : nullptr,
                         index ? index + (size_t)s0 * col_cells : nullptr, stamps);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    // SKIP = 1 / 2 (N = 2048 / 1024): two / four frames per team and half-iteration
    return pick_int<0, 1, 2>(skip, [&](auto SKIP) { return pick_bool(ex::exact_fast(pl), [&](auto FASTX) {
#ifdef EMSPEC_DIAG
        if constexpr (SKIP() == 0) {
            if (stamps) return run(exl::exact_fused4096_lr_kernel<true, FASTX()>);
        }
#endif
        return run(exl::exact_fused4096_lr_kernel<false, FASTX(), SKIP()>);
    }); });
}

}  // namespace emspec
