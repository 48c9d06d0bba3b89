// exact_fused.hip.inc — EXACT mode (EMSPEC_MODE_EXACT), N = 4096: the whole path in ONE kernel.  Included by kernels.hip
// after exact.hip.inc (same arithmetic: ex::xfft_stages / xstages8 / exact_core / exact_cell, bit model oracle/emspec_exact.c).
//
// Rounds 2-3 ran this mode as two kernels with 12 B of (q, key) records per bin in HBM between them (56 KB per column, 9x
// the algorithmic 6,144 B): the u64 column ring of the scatter (18 slots x 1024 rows x 8 B = 144 KB at hop 256) and the
// binary64 FFT planes (64 KB per frame) do not fit a CU's 160 KB of LDS together.  Here one 1024-thread workgroup walks
// a segment of one stream in time order with the ring RESIDENT in LDS and ONE set of planes laid over the ring's first
// 64 KB; while a frame's FFT owns those 64 KB the ring cells under them wait in the registers of the threads that
// overwrite them (16 doubles per thread of the FFT team).
//
// Two 512-thread teams alternate two roles every half-iteration k (one frame per half-iteration):
//   role F (k + h even), the LDS side:   scatter the team's previous frame (ds_add_u64; a zero into a cell of the lane's own
//        where there is nothing to add: no exec-mask branches) and take the finished column out of the ring
//        | park the 16 cells under this thread's pass-A points, write pass A | passes B, C, D (wave-local)
//        | read the twelve spectrum values of the thread's four bins | put the parked cells back
//   role V (k + h odd), the VALU side:   conjugate split + per-bin stage of the frame the team transformed at k - 1
//        (registers and the edge table only: no ring, no planes), fetch + pass A of the team's next frame (registers)
// so in every half-iteration exactly one team touches the ring and the planes and the other one only computes.  The four
// '|' are ARRIVAL COUNTERS of the F team (one ds_add per wave and phase, then a poll): the V team never stops at them and
// meets the F team at ONE workgroup barrier per half-iteration (with workgroup barriers for all five the V team's chunks have
// to match the F team's phases: 25.4 vs 23.4 ms; that form was the timing build EMSPEC_EXACT_SYNC=0 until it was retired,
// docs/HISTORY.md "Retired kernel forms").  The finished column's binary64 dB + colour runs on the first four F
// waves between their arrival and their wait at the second sync - they finish every phase ahead of the other four (the LDS
// queue serves them first) and would only wait.  A thread parks exactly the cells its own pass-A stores overwrite and
// restores them itself, so parking needs no sync of its own (one wave's LDS operations execute in order).
// Ring: at half-iteration k the F team scatters frame j0+k-2 (columns j0+k-2-D .. j0+k-2+D) and takes column j0+k-3-D out:
// 2D+2 slots.  Per frame the teams hand over through registers only: role F leaves the twelve spectrum values of the
// thread's bins (24 doubles), role V leaves pass A of the next frame (16) and the four (energy, cell) results (6); the two
// sets share one 24-double array so that the loop carries 48 VGPRs, not 92.
// What bounds it (profiles/r04_exact64*, docs/HISTORY.md 10): the F team's serial chain through the single plane set - with the
// V team's bins removed the kernel is as fast; LDS store bandwidth (ds_write_b64: 85 B/clk) puts that chain near 6.8 k cycles
// per frame, it runs at ~13 k.
namespace emspec {
namespace exf {
constexpr int LOG2N = 12, N = 4096, T = 512;

__device__ __forceinline__ void bar_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void bar_only() { asm volatile("s_barrier" ::: "memory"); }
using ex::XTwLds4;
using ex::tw4_slot;

// (region_cells, edge_cells - the sizes of the region the ring and the planes share and of the edge table: emspec_kernel_plan.h)

using ex::recip_normal64;
using ex::kFastMinFloor64;
using ex::kFastMaxPower64;
using ex::XBinF;
using ex::exact_core_fast;

#define EXF_STAMP(slot)                                                            \
    if constexpr (STAMP) {                                                         \
        const unsigned long long now_ = __builtin_readcyclecounter();              \
        acc_[slot] += now_ - last_;                                                \
        last_ = now_;                                                              \
    }

// The F team orders its own phases with arrival counters in LDS that only its eight waves touch (one ds_add per wave and
// phase, then a poll with s_sleep) - the V team computes straight through its half-iteration and meets the F team once, at
// its end.  Stamped build, slots: 0-4 the F phases | 5 the F team's sync waits | 6 role V's work | 7 its barrier wait (low
// word; the three stamps inside role V mark where the retired barrier form stopped and add next to nothing), 100 MHz
// ticks (high word) - tools/phase_cycles_exact.py.
template <bool STAMP, bool FASTX>
__global__ __launch_bounds__(1024, 4) void exact_fused4096_kernel(
    ExactPlanDev pl, ExactDbMap dm, const uint32_t* __restrict__ lut, const float* __restrict__ pcm, int64_t L, int64_t C,
    SegPlan sp, int slots, float* __restrict__ db, uint32_t* __restrict__ rgba, uint8_t* __restrict__ index,
    unsigned long long* __restrict__ stamps) {
    using ex::YTd;
    unsigned long long acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last_ = 0;
    extern __shared__ double smemd[];
    const int R = pl.rows, D = pl.D;
    unsigned long long* ring = reinterpret_cast<unsigned long long*>(smemd);   // [slots][R]; the first 64 KB double as the planes
    double* sre = smemd;
    double* sim = smemd + N;
    double* seb = smemd + region_cells(R, slots);                  // [R+1]
    double2* stwB = reinterpret_cast<double2*>(seb + edge_cells(R));   // [4][64]
    double2* stwC = stwB + 4 * 64;                                      // [4][8]
    uint32_t* slut = reinterpret_cast<uint32_t*>(stwC + 4 * 8);         // [256]
    unsigned* cnt = slut + 256;                                         // [2 teams][4 phases] arrival counters

    const int tid = threadIdx.x, h = tid >> 9, t = tid & 511;
    int s;
    int64_t c0, c1;
    if (!seg_of_block(sp, C, s, c0, c1)) return;
    const int64_t j0 = c0 - D > 0 ? c0 - D : 0;
    const int64_t jstop = c1 + D < C ? c1 + D : C;
    const float* x0 = pcm + (size_t)s * L;

    // ---- workgroup set-up
    for (int q = tid; q < slots * R; q += 1024) ring[q] = 0ull;
    for (int r = tid; r <= R; r += 1024) seb[r] = pl.ebin[r];
    if (tid < 256) slut[tid] = lut[tid];
    if (tid < 4 * 64) stwB[tid] = pl.tw[f8::tw_index8<3>(tw4_slot(tid >> 6), tid & 63)];
    else if (tid < 4 * 64 + 4 * 8) stwC[tid - 4 * 64] = pl.tw[f8::tw_index8<6>(tw4_slot((tid - 4 * 64) >> 3), (tid - 4 * 64) & 7)];
    else if (tid < 4 * 64 + 4 * 8 + 8) cnt[tid - (4 * 64 + 4 * 8)] = 0u;
    const double rs = 2.0 / (double)N;

    // What a team hands from one role to the next, in registers (see the header).  After role F: the twelve spectrum values
    // of the thread's bins, carry[4i .. 4i+3] = Z[4bg-1+i] (re, im), Z[N-4bg+1-i] (re, im).  After role V: pass A of the next frame (re 0..7,
    // im 8..15), the four fixed-point energies (16..19, bit patterns) and their ring cells (20, 21: two ints each; -1 =
    // nothing to add).
    double carry[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) carry[i] = 0.0;
    carry[20] = carry[21] = __hiloint2double(0, 0);   // (cell 0, energy 0): nothing to add
    if (h == 0) {   // pass A of team 0's first frame, j0 (team 1's first role V, at k = 0, runs pass A of frame j0 + 1 itself)
        const float* x = x0 + j0 * pl.hop;
        double vr[8], vi[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double xv = (double)x[t + T * i];
            vr[i] = xv;
            vi[i] = xv * ((double)(t + T * i - N / 2) * rs);
        }
        ex::xfft_stages<LOG2N, 0, 3>(vr, vi, t, pl.tw);
#pragma unroll
        for (int i = 0; i < 8; ++i) { carry[i] = vr[i]; carry[8 + i] = vi[i]; }
    }
    __syncthreads();
    ex::RowLookup64 lk;
    lk.init(seb, R, pl.log_rows);
    unsigned long long real0_ = 0;
    if constexpr (STAMP) { last_ = __builtin_readcyclecounter(); real0_ = __builtin_amdgcn_s_memrealtime(); }
    unsigned visits = 0;   // role-F visits of this team so far (x 8 waves = the arrival counters' target)
    // F-team sync after phase ph (0..3): this wave's LDS operations of the phase are issued - the LDS pipe serves one wave's
    // operations in order, so its arrival is counted behind them - then wait for the eight waves of the team.  Every wave
    // arrives before it polls, so the wait always ends; the spin is bounded all the same and a timeout raises g_kernel_error
    // (kernels.hip), which emspec_device_status reports.
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
    auto team_sync = [&](int ph, int lane) { team_arrive(ph, lane); team_wait(ph); };

    // half-iterations k = 0 .. klast: the last column c1-1 leaves the ring at k = c1 - 1 + 3 + D - j0
    const int klast = (int)(c1 + 2 + D - j0);
    int sk = 0;   // ring slot of column j0 + k
#pragma unroll 1
    for (int k = 0; k <= klast; ++k) {
        int tt = t;
        asm volatile("" : "+v"(tt));   // addresses are recomputed per half-iteration, not kept (and spilled) across the loop
        if (((k + h) & 1) == 0) {
            // ================= role F: the LDS side, frame jf = j0 + k
            // (Past the last frame, jf >= jstop, the team transforms whatever role V left - a repeat of the last frame - and the
            // results are dropped: everything below runs unconditionally, so that `carry` has ONE definition per role.  With
            // `if (frame exists)` around each phase the compiler kept the incoming 24 doubles alive through the whole role for
            // the path that skips - beside the parked cells and the pass working set: 112 spilled registers.)
            const int64_t jf = j0 + k;
            visits += 1;
            __builtin_amdgcn_s_setprio(1);   // the F team is the critical path (measured: raising the second half of a team, or
                                             // lowering a V wave as it advances, changes nothing or loses 2-3 %)
            // -- phase 1 (ring whole): scatter the results of frame j0+k-2, take the finished column j0+k-3-D out
            {   // (a result with nothing to add carries a cell of its own lane and a zero: no exec-mask branch per add)
                const int ca = __double2hiint(carry[20]), cb = __double2loint(carry[20]);
                const int cc = __double2hiint(carry[21]), cd = __double2loint(carry[21]);
                __hip_atomic_fetch_add(ring + ca, (unsigned long long)__double_as_longlong(carry[16]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(ring + cb, (unsigned long long)__double_as_longlong(carry[17]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(ring + cc, (unsigned long long)__double_as_longlong(carry[18]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(ring + cd, (unsigned long long)__double_as_longlong(carry[19]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            // (the finished column: four cells per thread of the team's FIRST four waves - they finish every phase ahead of the
            // second four, which issue arbitration serves last, and would only wait for them: the column's dB + colour
            // arithmetic fills that wait, below)
            const int64_t cfin = jf - 3 - D;
            const bool fin = cfin >= c0 && cfin < c1 && tt < (R >> 2);
            unsigned long long f0 = 0ull, f1 = 0ull, f2 = 0ull, f3 = 0ull;
            if (fin) {
                int sf = sk - 3 - D;
                sf += sf < 0 ? slots : 0;
                ulonglong2* cp = reinterpret_cast<ulonglong2*>(ring + sf * R + 4 * tt);
                const ulonglong2 va = cp[0], vb = cp[1];
                cp[0] = ulonglong2{0ull, 0ull};
                cp[1] = ulonglong2{0ull, 0ull};
                f0 = va.x; f1 = va.y; f2 = vb.x; f3 = vb.y;
            }
            EXF_STAMP(0)
            team_sync(0, tt & 63);
            EXF_STAMP(5)
            // -- phase 2: park the ring cells under this thread's pass-A points, then store pass A over them
            double pr[8], pi[8];
            const int a0 = f8::swz(tt), a1 = a0 ^ 8;   // swz(tt + 512 i) = (swz(tt) ^ 8 (i & 1)) + 512 i
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = ((i & 1) ? a1 : a0) + T * i; pr[i] = sre[p]; pi[i] = sim[p]; }
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = ((i & 1) ? a1 : a0) + T * i; sre[p] = carry[i]; sim[p] = carry[8 + i]; }
            EXF_STAMP(1)
            team_arrive(1, tt & 63);
            if (fin) {   // stage "dB + colour" of the column taken out above, between this wave's arrival and its wait
                const ex::CellOut o0 = ex::exact_cell(dm, f0), o1 = ex::exact_cell(dm, f1);
                const ex::CellOut o2 = ex::exact_cell(dm, f2), o3 = ex::exact_cell(dm, f3);
                const size_t o = ((size_t)s * C + cfin) * R + 4 * tt;
                if (db) *reinterpret_cast<float4*>(db + o) = make_float4(o0.db, o1.db, o2.db, o3.db);
                if (rgba) *reinterpret_cast<uint4*>(rgba + o) = make_uint4(slut[o0.index], slut[o1.index], slut[o2.index], slut[o3.index]);
                if (index) *reinterpret_cast<uint32_t*>(index + o) =
                    (uint32_t)o0.index | ((uint32_t)o1.index << 8) | ((uint32_t)o2.index << 16) | ((uint32_t)o3.index << 24);
            }
            team_wait(1);
            EXF_STAMP(5)
            // -- phase 3: passes B, C, D on this wave's 512 positions
            {
                {   // pass B = stages 3..5: p = hi*512 + i*64 + lo
                    double vr[8], vi[8];
                    const int base = ((tt >> 6) << 9) + (tt & 63);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 6)); vr[i] = sre[p]; vi[i] = sim[p]; }
                    ex::xstages8(vr, vi, XTwLds4<64>{stwB + (tt & 63)});
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 6)); sre[p] = vr[i]; sim[p] = vi[i]; }
                    wave_lds_sync();
                }
                {   // pass C = stages 6..8: p = (t >> 3)*64 + i*8 + (t & 7)
                    double vr[8], vi[8];
                    const int base = ((tt >> 3) << 6) + (tt & 7);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 3)); vr[i] = sre[p]; vi[i] = sim[p]; }
                    ex::xstages8(vr, vi, XTwLds4<8>{stwC + (tt & 7)});
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 3)); sre[p] = vr[i]; sim[p] = vi[i]; }
                    wave_lds_sync();
                }
                {   // pass D = stages 9..11: p = 8 t + i, twiddles are constants
                    double vr[8], vi[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = f8::swz((tt << 3) + i); vr[i] = sre[p]; vi[i] = sim[p]; }
                    ex::xfft_stages<LOG2N, 9, 3>(vr, vi, 0, pl.tw);
#pragma unroll
                    for (int i = 0; i < 8; ++i) { const int p = f8::swz((tt << 3) + i); sre[p] = vr[i]; sim[p] = vi[i]; }
                }
            }
            EXF_STAMP(2)
            team_sync(2, tt & 63);
            EXF_STAMP(5)
            // -- phase 4: the spectrum values of this thread's bins 4 bg .. 4 bg + 3 (lanes 32 bins apart, fused_r8.hip.inc):
            // F(i) = Z[4bg-1+i], M(i) = Z[N-4bg+1-i], i = 0..5, read in place (Z[k] sits at swz(bitrev12(k))).  The four bins
            // of an aligned group lie at base + {0, 2048, 1024, 3072} (bit-reversed low bits; the swizzle reads bits 5..9
            // only), so five positions are computed and the rest are immediate offsets: F(1..4) = group bg, F(0) = element 3 of
            // group bg-1, F(5) = element 0 of group bg+1, M(1), M(0) = elements 0, 1 of group 1024-bg, M(5..2) = elements 0..3
            // of group 1023-bg.
            {
                const int bg = ((tt & 63) << 3) | (tt >> 6);
                const int fB = f8::zpos(4 * bg), fL = f8::zpos((4 * bg - 4) & (N - 1)) + 3072, fH = f8::zpos(4 * bg + 4);
                const int mB = f8::zpos((N - 4 * bg) & (N - 1)), mL = f8::zpos(N - 4 * bg - 4);
                const int pf[6] = {fL, fB, fB + 2048, fB + 1024, fB + 3072, fH};
                const int pm[6] = {mB + 2048, mB, mL + 3072, mL + 1024, mL + 2048, mL};
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    carry[4 * i] = sre[pf[i]]; carry[4 * i + 1] = sim[pf[i]];
                    carry[4 * i + 2] = sre[pm[i]]; carry[4 * i + 3] = sim[pm[i]];
                }
            }
            EXF_STAMP(3)
            team_sync(3, tt & 63);
            EXF_STAMP(5)
            // -- phase 5: the parked ring cells go back
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = ((i & 1) ? a1 : a0) + T * i; sre[p] = pr[i]; sim[p] = pi[i]; }
            EXF_STAMP(4)
            bar_lds();
            EXF_STAMP(5)
        } else {
            // ================= role V: the VALU side; per-bin stage of frame jv = j0 + k - 1, pass A of frame jv + 2
            const int64_t jv = j0 + k - 1;
            const bool activeV = k >= 1 && jv < jstop;
            __builtin_amdgcn_s_setprio(0);
            // the team's next frame (past the end: the last frame once more; its results are dropped)
            const int64_t jn = jv + 2 < jstop ? jv + 2 : jstop - 1;
            float xs[8];
            {
                const float* x = x0 + jn * pl.hop;
#pragma unroll
                for (int i = 0; i < 8; ++i) xs[i] = x[tt + T * i];
            }
            int skv = sk - 1;   // ring slot of column jv
            skv += skv < 0 ? slots : 0;
            const int jrel = (int)(jv - c0);
            const unsigned span = (unsigned)(c1 - c0);
            const int bg = ((tt & 63) << 3) | (tt >> 6);
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
                const int cell = __mul24(sl, R) + o.row;
                rc[e] = ok ? cell : -1;
                rq[e] = ok ? o.q : 0ll;
            };
            EXF_STAMP(6)
            EXF_STAMP(7)
            bin(0);
            __builtin_amdgcn_sched_barrier(0);
            EXF_STAMP(6)
            EXF_STAMP(7)
            bin(1);
            bin(2);
            bin(3);
            // a lane's consecutive bins often share a cell: sum such runs first (integer adds: any order gives the same sum)
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const bool same = rc[e] >= 0 && rc[e] == rc[e + 1];
                rq[e + 1] += same ? rq[e] : 0ll;
                rq[e] = same ? 0ll : rq[e];
                rc[e] = same ? -1 : rc[e];
            }
            // nothing to add: a zero into a cell of this lane's own (2 tt + e mod 2 in slot 0: distinct per lane, no conflict)
#pragma unroll
            for (int e = 0; e < 4; ++e) rc[e] = rc[e] < 0 ? 2 * tt + (e & 1) : rc[e];
            double vr[8], vi[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double xv = (double)xs[i];
                vr[i] = xv;
                vi[i] = xv * ((double)(tt + T * i - N / 2) * rs);
            }
            ex::xfft_stages<LOG2N, 0, 3>(vr, vi, tt, pl.tw);
            __builtin_amdgcn_sched_barrier(0);
            EXF_STAMP(6)
            EXF_STAMP(7)
#pragma unroll
            for (int i = 0; i < 8; ++i) { carry[i] = vr[i]; carry[8 + i] = vi[i]; }
            carry[22] = carry[23] = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) carry[16 + e] = __longlong_as_double(rq[e]);
            carry[20] = __hiloint2double(rc[0], rc[1]);
            carry[21] = __hiloint2double(rc[2], rc[3]);
            __builtin_amdgcn_sched_barrier(0);
            EXF_STAMP(6)
            bar_only();
            EXF_STAMP(7)
        }
        sk += 1;
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
#undef EXF_STAMP
// (ring slots and dynamic LDS: exact_fused_slots, exact_fused_lds_bytes, emspec_kernel_plan.h)
}  // namespace exf

#ifdef EMSPEC_DIAG
// Diagnostic: the short binary64 reciprocal beside the IEEE division (tests/test_gpu_exact.py)
__global__ void recip64_probe_kernel(const double* __restrict__ d, int64_t count, double* __restrict__ out_short,
                                     double* __restrict__ out_ieee) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        out_short[i] = exf::recip_normal64(d[i]);
        out_ieee[i] = 1.0 / d[i];
    }
}
hipError_t launch_recip64_probe(const double* d, int64_t count, double* out_short, double* out_ieee, hipStream_t st) {
    hipLaunchKernelGGL(recip64_probe_kernel, dim3(1024), dim3(256), 0, st, d, count, out_short, out_ieee);
    return hipGetLastError();
}
// A/B aids: EMSPEC_EXACT_RECORDS=1 forces the two-kernel records path of rounds 2-3 (read once), EMSPEC_EXACT_PARKED=1 round 4's
// parking kernel where the no-parking one would serve (read at every call)
static ExactSwitches diag_exact_switches() {
    static int rec = -1;
    if (rec < 0) { const char* e = getenv("EMSPEC_EXACT_RECORDS"); rec = (e && e[0] == '1') ? 1 : 0; }
    const char* pk = getenv("EMSPEC_EXACT_PARKED");
    return ExactSwitches{pk && pk[0] == '1', rec != 0};
}
#else
static constexpr ExactSwitches diag_exact_switches() { return ExactSwitches{}; }
#endif

// the kernel family that serves the plan with this build's switches (emspec_kernel_plan.h: exact_route)
Route exact_route(int n, const ExactPlanDev& pl, int row0, const Axis& axis) { return exact_route(n, pl.rows, pl.D, row0, axis, diag_exact_switches()); }
static bool exact_fused_supported(int n, const ExactPlanDev& pl) { return !diag_exact_switches().records && exact_parked_fits(n, pl.rows, pl.D); }

hipError_t launch_exact_fused(int n, const ExactPlanDev& pl, const ExactDbMap& m, const uint8_t* lut, const float* pcm,
                              int64_t L, int S, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st,
                              unsigned long long* stamps, int64_t* stamp_groups) {
    if (!exact_fused_supported(n, pl)) return hipErrorNotSupported;
    if (S <= 0 || C <= 0) return hipSuccess;
    if (S > 65535) return hipErrorInvalidValue;
#ifndef EMSPEC_DIAG
    if (stamps || stamp_groups) return hipErrorNotSupported;
#endif
    // segments: the rounds-by-efficiency choice with this kernel's floor (emspec_seg_plan.h)
    const int64_t seg = exact_fused_seglen(device_cus(), S, C, pl.D, diag_seglen());
    const int64_t nseg = (C + seg - 1) / seg;
    if (!exact_fused_grid_ok(nseg, seg)) return hipErrorInvalidValue;
    const SegPlan sp{(int)seg, 1 << 30, (int)seg, 0};
    const int slots = exact_fused_slots(pl.D);
    const size_t lds = exact_fused_lds_bytes(pl.rows, slots);
    const dim3 grid((unsigned)nseg, (unsigned)S), block(1024);
    if (stamp_groups) *stamp_groups = nseg * S;
    const uint32_t* l32 = reinterpret_cast<const uint32_t*>(lut);
    uint32_t* r32 = reinterpret_cast<uint32_t*>(rgba);
    // the branch-free per-bin core needs reassignment ON, log-spaced rows and a gate that keeps 64 P inside recip_normal64's range
    const bool fast = ex::exact_fast(pl);
    auto go = [&](auto STAMP, auto FASTX) {
        return launch_k(exf::exact_fused4096_kernel<STAMP(), FASTX()>, grid, block, lds, st, pl, m, l32, pcm, L, C, sp, slots,
                        db, r32, index, STAMP() ? stamps : nullptr);
    };
#ifdef EMSPEC_DIAG
    if (stamps || stamp_groups) {
        if (!stamps) return hipSuccess;
        return pick_bool(fast, [&](auto FASTX) { return go(std::true_type{}, FASTX); });
    }
#endif
    return pick_bool(fast, [&](auto FASTX) { return go(std::false_type{}, FASTX); });
}

}  // namespace emspec
