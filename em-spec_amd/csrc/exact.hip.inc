// exact.hip.inc — EXACT mode (EMSPEC_MODE_EXACT): the whole path in IEEE binary64 with a 64-bit fixed-point
// histogram.  Included by kernels.hip.
//
// Why it exists (BASELINE.json north_star): results must match "the reference JS/WebAudio CPU path ... exactly on
// reassigned integer (time,freq) bin indices" — JavaScript arithmetic is binary64 — and byte output should be
// bit-reproducible.  The float32 kernels are exact against their own float32 bit model only: against a binary64
// evaluation a few 1e-4 of the bins sit close enough to a cell edge to land in the neighbouring cell, and float
// accumulation in arrival order makes the last bit of a cell's sum depend on the schedule.  Here
//   * every operation of "Frame gather" .. "Index quantise" (SURVEY.md §8a) is binary64, one rounding each, in the order
//     oracle/emspec_exact.c states (the same canonical radix-2 DIF network and spectral Hann identities as the float32
//     path, DESIGN.md §3.7); the row edges are the binary64 table;
//   * "Scatter" adds each bin's energy as a 64-bit integer (units of 2^-52 full-scale-sine powers): integer adds commute,
//     so the finished cells do not depend on the order of arrival;
//   * "dB + colour" evaluates 10 log10 by a specified binary64 polynomial (no library call), so dB, palette index and
//     RGBA are the same bytes on the GPU and in the oracle.
// MI355X runs v_fma_f64 / v_add_f64 / v_mul_f64 at half the float32 rate, so a flag-and-repair scheme (float32 first,
// binary64 only for bins near an edge) does not pay: re-evaluating ONE bin directly costs 6 N multiply-adds, a whole
// binary64 frame 2.5 N log2 N — the whole frame is cheaper as soon as two bins of it are in doubt (measured: ~30).
//
//   exact_frames_kernel<LOG2N>   one workgroup (N/8 threads) per frame, N <= 8192: radix-8 register passes over an
//                                in-place LDS buffer (re / im planes of doubles), bins read in place (bit-reversed),
//                                4 consecutive bins per thread; sinks: parity dump, (q, key) records, u64 ring atomics.
//   exact_frames16384_kernel     N = 16384: 256 KB of spectrum do not fit in LDS, so the first DIF stage is done in
//                                registers and the even-bin and odd-bin halves (8192 points each) are transformed one
//                                after the other in the same 136 KB buffer; the even half's split spectra wait in registers.
//   exact_tile_scatter_kernel    records -> u64 LDS histogram of a 16-column tile -> dB / index / RGBA.
//   exact_walk_scatter_kernel    the same through a walking u64 ring (every record read once) when the ring fits in LDS.
//   exact_finalize_kernel        u64 cells -> dB / index / RGBA (streaming ring).
// Since round 4 the batch path at N = 4096 runs none of the record kernels: exact_fused.hip.inc does the whole path in one
// kernel (ring resident in LDS, planes laid over its first 64 KB); the kernels here serve the other sizes, the parity dump
// and the streaming calls.
namespace emspec {
namespace ex {

struct YTd { double yr, yi, tr, ti; };
__device__ __forceinline__ YTd split_d(double zx, double zy, double wx, double wy) {
    YTd o;
    o.yr = zx + wx; o.yi = zy - wy; o.tr = zy + wy; o.ti = wx - zx;
    return o;
}
__device__ __forceinline__ YTd conj_d(const YTd& a) { return YTd{a.yr, -a.yi, a.tr, -a.ti}; }

// radix-2 DIF stages S0 .. S0+R-1 of the 2^LOG2N network on 2^R register values (same index maps as fft_stages)
// LEAN: a scheduling barrier after every stage keeps the max-ILP scheduler from fetching all of a pass's twiddles (4
// registers each) up front - the N = 16384 kernel, at 1024 threads and 128 registers, otherwise spills inside its passes
template <int LOG2N, int S0, int R, bool LEAN = false>
__device__ __forceinline__ void xfft_stages(double (&vr)[1 << R], double (&vi)[1 << R], int lo, const double2* __restrict__ tw) {
    constexpr int N = 1 << LOG2N;
    constexpr int B0 = LOG2N - S0 - R;
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int mloc = 1 << (R - 1 - u);
        const int s = S0 + u;
#pragma unroll
        for (int i = 0; i < (1 << R); ++i) {
            if (i & mloc) continue;
            const double ar = vr[i], ai = vi[i], br = vr[i + mloc], bi = vi[i + mloc];
            vr[i] = ar + br;
            vi[i] = ai + bi;
            const double dr = ar - br, di = ai - bi;
            bool done = false;
            if constexpr (B0 == 0) {   // last pass: lo == 0, q is a compile-time constant
                const int q = (i & (mloc - 1)) << s;
                if (q == 0) { vr[i + mloc] = dr; vi[i + mloc] = di; done = true; }
                else if (q == N / 4) { vr[i + mloc] = di; vi[i + mloc] = -dr; done = true; }
            }
            if (!done) {
                // the upper half of a stage's butterflies lies a quarter turn beyond the lower half, and the table is
                // quarter-turn symmetric (tw[q + N/4] = (tw[q].y, -tw[q].x) exactly, ex_twiddle): one load serves both
                const int mm = i & (mloc - 1);
                const bool rot = mloc >= 2 && mm >= mloc / 2;
                const int q = ((((rot ? mm - mloc / 2 : mm)) << B0) + lo) << s;
                const double2 w0 = tw[q];   // tw[0] = (1,-0), tw[N/4] = (0,-1): the products below are then exact
                const double2 w = rot ? make_double2(w0.y, -w0.x) : w0;
                const double t = di * w.y;
                const double uu = di * w.x;
                vr[i + mloc] = __builtin_fma(dr, w.x, -t);
                vi[i + mloc] = __builtin_fma(dr, w.y, uu);
            }
        }
        if constexpr (LEAN) __builtin_amdgcn_sched_barrier(0);
    }
}

// Where point p of the in-place transform lives in the binary64 planes.  PadIx: one slot of pad per 16 (emspec_device.h: padi),
// the layout of every size but 16384.  Swz13Ix (round 5), for the 8192-point halves of N = 16384: no padding, the low five bits
// of p XORed with a GF(2)-linear function of bits 5..10,
//     s = ((p >> 5 & 7) << 2) ^ (p >> 8 & 7) ^ (p >> 6 & 3),
// found by exhaustive search so that the 32 lanes of every 8-byte access group of the kernel hit 32 different bank pairs: the
// lanes vary p[4:0] (pass-1 store, pass at stage 4), {p[3:0], p7} (stage 7), {p0, p[7:4]} (stage 10), p[7:3] (stage 13) and
// p[10:6] (the bit-reversed spectrum reads) - each set maps onto the five bank bits injectively.  With padi, 32 consecutive
// points wrap onto their own first bank pair and the strided passes collide in pairs: 27 % of the kernel's LDS cycles were
// bank conflicts (profiles/r05_exact_n16384.json, first take).
struct PadIx { static constexpr bool linear_low5 = false; __device__ static __forceinline__ int at(int p) { return padi(p); } };
struct Swz13Ix {
    static constexpr bool linear_low5 = true;   // at(P + x) = at(P) ^ x for x < 32 when P has those bits clear
    __device__ static __forceinline__ int at(int p) { return p ^ ((((p >> 5) & 7) << 2) ^ ((p >> 8) & 7) ^ ((p >> 6) & 3)); }
};

// passes after the first one, over the padded in-place planes (local index p < 2^(LOG2N-SKIP) for the N = 16384 halves:
// SKIP stages were done before and the planes hold one half; the index maps do not change)
template <int LOG2N, int S0, bool LEAN = false, class IX = PadIx>
__device__ __forceinline__ void xfft_rest(double* sre, double* sim, int t, const double2* __restrict__ tw) {
    constexpr int REM = LOG2N - S0;
    if constexpr (REM > 3) {
        constexpr int B0 = LOG2N - S0 - 3;
        const int lo = t & ((1 << B0) - 1), hi = t >> B0;
        const int base = (hi << (B0 + 3)) + lo;
        double vr[8], vi[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int p = IX::at(base + (i << B0)); vr[i] = sre[p]; vi[i] = sim[p]; }
        if constexpr (LEAN) __builtin_amdgcn_sched_barrier(0);
        xfft_stages<LOG2N, S0, 3, LEAN>(vr, vi, lo, tw);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int p = IX::at(base + (i << B0)); sre[p] = vr[i]; sim[p] = vi[i]; }
        // a pass with B0 <= 6 touches only the 512 positions [512 w, 512 w + 512) of its wave w, and so does every later
        // pass: those are ordered by the in-order LDS pipe alone, no workgroup barrier (as in the float32 kernels)
        if constexpr (B0 <= 6) wave_lds_sync(); else __syncthreads();
        xfft_rest<LOG2N, S0 + 3, LEAN, IX>(sre, sim, t, tw);
    } else {
        constexpr int R = REM, G = 8 >> R;
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            double vr[1 << R], vi[1 << R];
#pragma unroll
            for (int i = 0; i < (1 << R); ++i) { const int p = IX::at(8 * t + (gi << R) + i); vr[i] = sre[p]; vi[i] = sim[p]; }
            xfft_stages<LOG2N, S0, R, LEAN>(vr, vi, 0, tw);
#pragma unroll
            for (int i = 0; i < (1 << R); ++i) { const int p = IX::at(8 * t + (gi << R) + i); sre[p] = vr[i]; sim[p] = vi[i]; }
        }
        __syncthreads();
    }
}

// row = largest r with eb[r] <= kh, or -1 unless eb[0] <= kh < eb[R] (binary64 compares against the binary64 table).
// For the log axis a float32 log2 hint starts the search; the two loops make the result exact whatever the hint.
struct RowLookup64 {
    const double* eb; int R; int log_rows; float l2e0, rscale; double e0, eR;
    __device__ __forceinline__ void init(const double* table, int rows, int lr) {
        eb = table; R = rows; log_rows = lr; e0 = table[0]; eR = table[rows];
        l2e0 = __log2f((float)table[0]);
        rscale = (float)rows / (__log2f((float)table[rows]) - l2e0);
    }
    __device__ __forceinline__ int operator()(double kh) const {
        if (!(kh >= e0) || !(kh < eR)) return -1;
        if (log_rows) {
            // the float32 log2 hint is within one row of the answer (its error is ~1e-6 rows): read the four edges
            // around it at once and pick the row without a branch; the final check makes the result exact whatever the
            // hint (a miss - never observed - takes the walk)
            int r = (int)((__log2f((float)kh) - l2e0) * rscale);
            r = max(1, min(r, R - 2));
            const double a = eb[r - 1], b = eb[r], c = eb[r + 1], d = eb[r + 2];
            int rr = r + (kh >= c ? 1 : 0) - (kh < b ? 1 : 0);
            if (kh >= a && kh < d) return rr;
            r = max(0, min(rr, R - 1));
            while (r > 0 && kh < eb[r]) --r;
            while (r < R - 1 && kh >= eb[r + 1]) ++r;
            return r;
        }
        int lo = 0, hi = R;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (eb[mid] <= kh) lo = mid; else hi = mid;
        }
        return lo;
    }
};

struct XBin { double power; long long q; int dcol; int row; };

// stages "Power + gate", "Reassign", "Index quantise" in binary64 (oracle/emspec_exact.c:ex_frame)
__device__ __forceinline__ XBin exact_core(const ExactPlanDev& pl, const RowLookup64& lk, int k, const YTd& m, const YTd& c,
                                           const YTd& p) {
    const double Ar = (c.yr + c.yr) - (m.yr + p.yr), Ai = (c.yi + c.yi) - (m.yi + p.yi);
    const double Br = (c.tr + c.tr) - (m.tr + p.tr), Bi = (c.ti + c.ti) - (m.ti + p.ti);
    const double Dr = m.yr - p.yr, Di = m.yi - p.yi;
    const double den = __builtin_fma(Ar, Ar, Ai * Ai);
    XBin o;
    o.power = den * 0.015625;
    o.dcol = 0;
    o.row = -1;
    if (o.power >= pl.pfloor && o.power <= pl.pmax) {
        if (pl.reassign) {
            const double numT = __builtin_fma(Br, Ar, Bi * Ai);
            const double numF = __builtin_fma(Dr, Ar, Di * Ai);
            const double inv = 1.0 / den;   // IEEE division
            const double ts = numT * inv;
            const double ks = numF * inv;
            const double cf = __builtin_floor(__builtin_fma(ts, pl.tscale, 0.5));
            if (__builtin_fabs(cf) <= (double)pl.D) {
                o.dcol = (int)cf;
                o.row = lk((double)k + ks);
            }
        } else {
            o.row = lk((double)k);
        }
    }
    o.q = o.row >= 0 ? (long long)__builtin_rint(o.power * pl.qscale) : 0ll;   // round to nearest even; < 2^61 by the gate
    return o;
}

// 1/d, correctly rounded, for 2^-700 < d < 2^1000: hipcc's IEEE binary64 division 1.0 / d (v_div_scale x2, v_rcp_f64, 6 fma,
// one multiply by 1.0, v_div_fmas, v_div_fixup) without the instructions that only serve arguments whose reciprocal needs
// scaling or is a special case - the same v_rcp_f64 seed, the same two Newton steps, the same residual correction, in the
// same order (LLVM's f64 division expansion with numerator 1: its scaled numerator is 1.0, its scaled denominator d, the
// product 1.0 * r is r, div_fmas is a plain fma, div_fixup returns its first operand).  The gate of the per-bin stage keeps
// every USED d = 64 P inside [64 pfloor, 64 pmax]; the launcher selects this core only when that lies inside the range
// (tests/test_gpu_exact.py::test_short_reciprocal64_equals_ieee_division compares the two on the GPU).
__device__ __forceinline__ double recip_normal64(double d) {
    const double r0 = __builtin_amdgcn_rcp(d);
    const double e0 = __builtin_fma(-d, r0, 1.0);
    const double r1 = __builtin_fma(r0, e0, r0);
    const double e1 = __builtin_fma(-d, r1, 1.0);
    const double r2 = __builtin_fma(r1, e1, r1);
    const double e2 = __builtin_fma(-d, r2, 1.0);
    return __builtin_fma(e2, r2, r2);
}
constexpr double kFastMinFloor64 = 1e-200, kFastMaxPower64 = 1e290;

// Stages "Power + gate", "Reassign", "Index quantise" + the fixed-point conversion for a plan the launcher knows to be
// "fast" (reassignment ON, log-spaced rows, power floor >= kFastMinFloor64): exact_core without a branch - everything
// is computed, the gates select at the end - so a thread's four bins are one basic block and their chains overlap.  Same
// operations in the same order on every value that is used, hence the same bits (the whole exact suite runs on it).  The
// branchy form cost ~390 instructions per bin here, two thirds of them scalar exec-mask bookkeeping and selects.
// DUMP: the result also carries the power and follows exact_core's conventions for bins that are not accumulated (q = 0;
// the column offset of a bin that passed the power and reach gates but left the frequency axis is kept) - the parity dump
// shows those; the fused kernel and the records only ever look at accumulated bins.
struct XBinF { long long q; int dcol; int row; double power; };
template <bool DUMP = false>
__device__ __forceinline__ XBinF exact_core_fast(const ExactPlanDev& pl, const double* seb, double kd, double Dd,
                                                 const YTd& m, const YTd& c, const YTd& p) {
    // (c + c) - s in one instruction: c + c is exact, so fma(2, c, -s) rounds the same real number once
    const double Ar = __builtin_fma(2.0, c.yr, -(m.yr + p.yr)), Ai = __builtin_fma(2.0, c.yi, -(m.yi + p.yi));
    const double Br = __builtin_fma(2.0, c.tr, -(m.tr + p.tr)), Bi = __builtin_fma(2.0, c.ti, -(m.ti + p.ti));
    const double Dr = m.yr - p.yr, Di = m.yi - p.yi;
    const double den = __builtin_fma(Ar, Ar, Ai * Ai);
    const double P = den * 0.015625;   // (only the dump shows it: the gates and the fixed point below work on den = 64 P,
                                       //  powers of two away, so P >= pfloor <=> den >= 64 pfloor and P qscale == den qscale / 64)
    const double numT = __builtin_fma(Br, Ar, Bi * Ai);
    const double numF = __builtin_fma(Dr, Ar, Di * Ai);
    const double inv = recip_normal64(den);
    const double cf = __builtin_floor(__builtin_fma(numT * inv, pl.tscale, 0.5));
    const double kh = kd + numF * inv;
    const bool gates = (den >= pl.pfloor64) & (den <= pl.pmax64) & (__builtin_fabs(cf) <= Dd);
    // row: the float32 log2 hint r is the answer unless k-hat lies within the hint's error (~1e-4 rows) of an edge.  The two
    // edges of row r decide that exactly - eb[r] <= kh < eb[r+1] is the definition of "row r", and it implies that k-hat is
    // on the axis - and anything else (one bin in ~10^4, and every bin whose k-hat is off the axis' ends, where the hint was
    // clamped) is looked at again: on the axis it takes a bisection of the table, so the result never depends on the hint.
    int r = (int)((__log2f((float)kh) - pl.l2e0) * pl.rscale);
    r = max(0, min(r, pl.rows - 1));
    const double eb = seb[r], ec = seb[r + 1];
    int rr = r;
    const bool inrow = (kh >= eb) & (kh < ec);
    bool ok = gates & inrow;
    const bool miss = gates & !inrow;
    if (__builtin_amdgcn_ballot_w64(miss) != 0ull) {   // wave-uniform, rarely taken
        if (miss && (kh >= pl.e0) && (kh < pl.eR)) {
            int lo = 0, hi = pl.rows;
#pragma unroll 1
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (seb[mid] <= kh) lo = mid; else hi = mid;
            }
            rr = lo;
            ok = true;
        }
    }
    // q = (int64) rint(P qscale): the product is exact (qscale is a power of two) and < 2^61 by the gate
    const double x = __builtin_rint(den * pl.qscale64);
    const unsigned hi = (unsigned)(x * 0x1p-32);                                   // floor(x / 2^32): x >= 0
    const unsigned lo = (unsigned)__builtin_fma((double)hi, -0x1p32, x);          // exact
    XBinF o;
    o.q = (long long)(((unsigned long long)hi << 32) | lo);
    o.dcol = ok ? (int)cf : 0;
    o.row = ok ? rr : -1;
    o.power = P;
    if constexpr (DUMP) {
        o.q = ok ? o.q : 0ll;
        o.dcol = gates ? (int)cf : 0;
    }
    return o;
}

// the plans the branch-free core serves (the launchers check)
static bool exact_fast_plan(const ExactPlanDev& pl) {
    return pl.reassign && pl.log_rows && pl.pfloor >= kFastMinFloor64 && pl.pmax <= kFastMaxPower64 && pl.rows >= 4;
}
// every EXACT launcher's FASTX: the plan qualifies (read per call; the diagnostic build can force the generic core)
static bool exact_fast(const ExactPlanDev& pl) {
#ifdef EMSPEC_DIAG
    if (const char* ev = getenv("EMSPEC_EXACT_NOFAST")) if (ev[0] == '1') return false;   // A/B aid
#endif
    return exact_fast_plan(pl);
}

// stage "dB + colour" with a specified binary32 evaluation of 10 log10 (oracle/emspec_exact.c:eo_exact_db32 / eo_exact_sum32: the
// same IEEE operations in the same order).  Round 5: binary32 - a binary64 vector instruction occupies the SIMD four times as
// long, and this stage was 12 % of the fused kernel - and, in its last form, no division and no 64-bit integer conversion:
// log2 of the folded mantissa is f P(f), f = m - 1, P of degree 8 (a correctly rounded binary32 division is ten vector
// instructions, (float)(long long) twelve; the fused kernel is bound by vector issue, DESIGN.md section 4.6).
__device__ __forceinline__ float exact_sum32(unsigned long long sum) {
    return __builtin_fmaf((float)(unsigned)(sum >> 32), 4294967296.0f, (float)(unsigned)(sum & 0xffffffffull));
}
__device__ __forceinline__ float exact_db32(float x) {
    unsigned u = __float_as_uint(x);
    int e = (int)((u >> 23) & 0xffu) - 127;
    u = (u & 0x007fffffu) | 0x3f800000u;
    float m = __uint_as_float(u);
    if (m > 1.41421354f) { m = m * 0.5f; e += 1; }
    const float f = m - 1.0f;
    float p = 0.123109683f;
    p = __builtin_fmaf(p, f, -0.205861881f);
    p = __builtin_fmaf(p, f, 0.216078222f);
    p = __builtin_fmaf(p, f, -0.239169881f);
    p = __builtin_fmaf(p, f, 0.287903249f);
    p = __builtin_fmaf(p, f, -0.360693276f);
    p = __builtin_fmaf(p, f, 0.480910748f);
    p = __builtin_fmaf(p, f, -0.721347451f);
    p = __builtin_fmaf(p, f, 1.44269502f);
    const float l2 = f * p;
    return ((float)e + l2) * 3.01029992f;
}
struct CellOut { float db; int index; };
__device__ __forceinline__ CellOut exact_cell(const ExactDbMap& m, unsigned long long sum) {
    const float d = exact_db32(__builtin_fmaf(exact_sum32(sum), m.sc, 1e-20f));
    float v = (d - m.lo) * m.inv_range;
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    if (d < m.gate) v = 0.0f;
    return CellOut{d, (int)(v * 255.0f + 0.5f)};
}

// (rec_stride, records per frame: emspec_kernel_plan.h)

// SINK: 0 = whatever the ExactSinks say at run time; 1 = parity dump only; 2 = records only (compile-time, so that the four
// bins of a thread stay in one basic block - the run-time form tests three sink pointers per bin)
template <int SINK = 0>
struct BinSinkT;
struct BinSink {
    const ExactSinks& sk; const ExactPlanDev& pl; int s; size_t fidx; int64_t jcol; int K, Kp;
    int slot_j = 0;   // ring sinks: slot of column jcol (a bin lands at most D < slots columns away: an add and a wrap per bin)
    __device__ __forceinline__ void operator()(int k, const XBin& o, bool records = true) const {
        const int64_t col = jcol + o.dcol;
        if (sk.power) {
            const size_t at = fidx * K + k;
            sk.power[at] = o.power;
            sk.col[at] = (int32_t)col;
            sk.row[at] = o.row;
            if (sk.q) sk.q[at] = o.q;
        }
        if (records && sk.rec_q) {
            const size_t at = fidx * Kp + k;
            sk.rec_q[at] = o.q;
            sk.rec_key[at] = o.row >= 0 ? ((unsigned)(o.dcol + 32768) << 16) | (unsigned)o.row : 0xFFFFFFFFu;
        }
        if (sk.hist && o.row >= 0 && col >= 0 && col < sk.total_cols) {
            const int64_t slot = sk.ring ? (int64_t)live_slot(slot_j, o.dcol, (int)sk.hist_slots) : col;
            atomicAdd(sk.hist + ((size_t)s * sk.hist_slots + slot) * pl.rows + o.row, (unsigned long long)o.q);
        }
    }
    // four consecutive bins k0 .. k0+3 (k0 a multiple of 4) at once: the records leave as 16-byte stores
    __device__ __forceinline__ void four(int k0, const XBin (&o)[4]) const {
        if (sk.power || sk.hist) {
#pragma unroll
            for (int e = 0; e < 4; ++e) (*this)(k0 + e, o[e], false);
        }
        if (sk.rec_q) {
            const size_t at = fidx * Kp + k0;
            unsigned key[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) key[e] = o[e].row >= 0 ? ((unsigned)(o[e].dcol + 32768) << 16) | (unsigned)o[e].row : 0xFFFFFFFFu;
            *reinterpret_cast<longlong2*>(sk.rec_q + at) = longlong2{o[0].q, o[1].q};
            *reinterpret_cast<longlong2*>(sk.rec_q + at + 2) = longlong2{o[2].q, o[3].q};
            *reinterpret_cast<uint4*>(sk.rec_key + at) = make_uint4(key[0], key[1], key[2], key[3]);
        }
    }
    __device__ __forceinline__ void pads() const {
        if (sk.rec_q)
            for (int k = K; k < Kp; ++k) { sk.rec_q[fidx * Kp + k] = 0; sk.rec_key[fidx * Kp + k] = 0xFFFFFFFFu; }
    }
};

template <int SINK>
struct BinSinkT {
    const ExactSinks& sk; size_t fidx; int64_t jcol; int K, Kp;
    __device__ __forceinline__ void operator()(int k, const XBin& o) const {
        if constexpr (SINK == 1) {
            const size_t at = fidx * K + k;
            sk.power[at] = o.power;
            sk.col[at] = (int32_t)(jcol + o.dcol);
            sk.row[at] = o.row;
            if (sk.q) sk.q[at] = o.q;
        } else {
            const size_t at = fidx * Kp + k;
            sk.rec_q[at] = o.q;
            sk.rec_key[at] = o.row >= 0 ? ((unsigned)(o.dcol + 32768) << 16) | (unsigned)o.row : 0xFFFFFFFFu;
        }
    }
    __device__ __forceinline__ void pads() const {
        if constexpr (SINK == 2)
            for (int k = K; k < Kp; ++k) { sk.rec_q[fidx * Kp + k] = 0; sk.rec_key[fidx * Kp + k] = 0xFFFFFFFFu; }
    }
};

// workgroups are re-dealt so that each XCD (own L2) takes a contiguous run of frames: neighbouring frames share
// (N - hop)/N of their samples (kernels.hip:frames_kernel)
__device__ __forceinline__ void frame_of_block(int64_t& f, int& s) {
    const int64_t total = (int64_t)gridDim.x * gridDim.y, lin = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int64_t full = total & ~(int64_t)7;
    const int64_t work = lin < full ? (lin & 7) * (full >> 3) + (lin >> 3) : lin;
    if (total <= 0xFFFFFFFFll) {   // 32-bit division (a 64-bit one is ~140 scalar instructions, and this runs once per frame)
        const unsigned w32 = (unsigned)work, q32 = w32 / gridDim.x;
        s = (int)q32;
        f = (int64_t)(w32 - q32 * gridDim.x);
    } else {
        f = work % gridDim.x;
        s = (int)(work / gridDim.x);
    }
}

struct LiveConvExact {
    ExactDbMap m;
    __device__ __forceinline__ void operator()(unsigned long long e, float& db, int& idx) const {
        const CellOut o = exact_cell(m, e);
        db = o.db;
        idx = o.index;
    }
};
__device__ __forceinline__ int ring_slot_of(const ExactSinks& sk, int64_t jcol) {
    return (sk.hist && sk.ring) ? (int)(jcol % sk.hist_slots) : 0;
}

// LIVE: the launch is a live multi-stream one (sk.live; a separate instantiation, so the batch form pays nothing for it)
template <int LOG2N, bool FASTX = false, bool LIVE = false>   // FASTX: the branch-free per-bin core (exact_fast_plan)
__global__ __launch_bounds__((1 << LOG2N) / 8) void exact_frames_kernel(ExactPlanDev pl, const float* __restrict__ pcm,
                                                                          int64_t L, int64_t frame0, int64_t nframes,
                                                                          ExactSinks sk) {
    constexpr int N = 1 << LOG2N, T = N / 8, K = N / 2 + 1, PN = PaddedSize<N>::value, Kp = rec_stride(N);
    extern __shared__ double smemd[];
    double* sre = smemd;
    double* sim = sre + PN;
    double* seb = sim + PN;   // [rows+1]
    const int t = threadIdx.x;
    int64_t f;
    int s;
    LiveBlock lb;                                        // live multi-stream launch (live.hip.inc)
    constexpr bool live = LIVE;
    if (live) {
        if (!lb.init(sk.live, pl.hop, T)) return;
        s = lb.s; f = lb.f;
    } else {
        frame_of_block(f, s);
    }
    const int64_t j = live ? f : frame0 + f;
    const int64_t jcol = live ? lb.column() : j + sk.col_offset;
    // (edges_lds == 0: the table does not fit beside the transform - 4096 rows at N >= 8192 - and is read from global memory)
    if (sk.edges_lds)
        for (int r = t; r <= pl.rows; r += T) seb[r] = pl.ebin[r];

    // stage "Frame gather" + packing z = x + j ramp x (exact in binary64)
    const float* x = pcm + (size_t)s * L + j * pl.hop;
    double vr[8], vi[8];
    const double rs = 2.0 / (double)N;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = t + T * i;
        const double xv = (double)(live ? lb.sample(n) : x[n]);
        vr[i] = xv;
        vi[i] = xv * ((double)(n - N / 2) * rs);
    }
    xfft_stages<LOG2N, 0, 3>(vr, vi, t, pl.tw);
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int p = padi(t + T * i); sre[p] = vr[i]; sim[p] = vi[i]; }
    __syncthreads();
    xfft_rest<LOG2N, 3>(sre, sim, t, pl.tw);

    // per-bin stages: bins 4t .. 4t+3 from Z[4t-1 .. 4t+4] and the mirrored Z[N-4t+1 .. N-4t-4], read in place:
    // Z[k] sits at position bitrev(k); lanes are 4 bins apart, i.e. 2^(LOG2N-8) .. positions apart in the low bits
    RowLookup64 lk;
    lk.init(sk.edges_lds ? seb : pl.ebin, pl.rows, pl.log_rows);
    const BinSink sink{sk, pl, s, (size_t)s * nframes + f, jcol, K, Kp, ring_slot_of(sk, jcol)};
    // Bin group g of thread t: lane bits 0..4 -> group bits 1..5, lane bit 5 -> group bit 0 (for workgroups of at least one
    // wave).  The 32 lanes of a half-wave (one LDS cycle of a ds_read_b64) then differ in bin bits 3..7 = position bits 8..4,
    // i.e. they read padded slots base + 17 m, m = 0..31: 32 different bank pairs.  With g = t the half-wave covered bin
    // bits 2..6 and the even slots only: a 2-way conflict on every spectrum read (42 % conflict cycles, r03 profile).
    const int g = T >= 64 ? ((t & ~63) | ((t & 31) << 1) | ((t >> 5) & 1)) : t;
    YTd yt[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int kf = (4 * g - 1 + i) & (N - 1), km = (N - 4 * g + 1 - i) & (N - 1);
        const int pf = padi((int)(__brev((unsigned)kf) >> (32 - LOG2N))), pm = padi((int)(__brev((unsigned)km) >> (32 - LOG2N)));
        yt[i] = split_d(sre[pf], sim[pf], sre[pm], sim[pm]);
    }
    // (collecting the four results and storing the records as 16-byte vectors - BinSink::four, which the N = 16384 kernel
    // uses, -12 % there - was measured 21 % SLOWER here: four bins' results held at once at 128 VGPRs)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (FASTX) {
            const XBinF b = exact_core_fast<true>(pl, lk.eb, (double)(4 * g + e), (double)pl.D, yt[e], yt[e + 1], yt[e + 2]);
            sink(4 * g + e, XBin{b.power, b.q, b.dcol, b.row});
        } else {
            sink(4 * g + e, exact_core(pl, lk, 4 * g + e, yt[e], yt[e + 1], yt[e + 2]));
        }
    }
    if (g == T - 1) {   // the Nyquist bin: Y[N/2+1] = conj Y[N/2-1], T[N/2+1] = conj T[N/2-1] exactly
        sink(N / 2, exact_core(pl, lk, N / 2, yt[4], yt[5], conj_d(yt[4])));
        sink.pads();
    }
    if (live && live_last_arrival(sk.live, s, lb.bframes, sre))
        live_finalize<unsigned long long>(sk.live, lb.d, s, sk.hist, (int)sk.hist_slots, pl.rows, pl.D + sk.live.lat_extra, T, LiveConvExact{sk.fin_map});
}


// N = 4096, the headline shape of the mode: a PERSISTENT workgroup (512 threads, two per CU) walks a contiguous run of
// (stream, frame) work items, so that what the per-frame kernel above fetches for every frame is set up once:
//   - the in-place buffer uses the float32 kernel's GF(2) swizzle (fused_r8.hip.inc: f8::swz; the planes hold 8-byte
//     elements like its float2 buffer) instead of 1-in-16 padding: pass A / B / C / D accesses and the bit-reversed bin
//     reads of 4 consecutive bins per lane are all bank-conflict-free;
//   - the twiddles of passes B and C (they depend on 6 and 3 bits of the thread id) are staged in LDS once per workgroup
//     instead of 14 L2 loads per thread and frame; pass A's seven come from L2 with the samples, pass D's are constants;
//   - the next frame's samples are fetched before the per-bin stage of the current one.
// Same butterflies in the same order: bit-identical to exact_frames_kernel<12> and the bit model.
template <int U, class W>
__device__ __forceinline__ void xstage8(double (&vr)[8], double (&vi)[8], const W& w) {   // stage U (0..2) of a radix-8 pass
    constexpr int mloc = 4 >> U;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i & mloc) continue;
        const double ar = vr[i], ai = vi[i], br = vr[i + mloc], bi = vi[i + mloc];
        vr[i] = ar + br;
        vi[i] = ai + bi;
        const double dr = ar - br, di = ai - bi;
        const double2 tw = w(8 - 2 * mloc + (i & (mloc - 1)));
        const double t = di * tw.y;
        const double uu = di * tw.x;
        vr[i + mloc] = __builtin_fma(dr, tw.x, -t);
        vi[i + mloc] = __builtin_fma(dr, tw.y, uu);
    }
}
template <class W>
__device__ __forceinline__ void xstages8(double (&vr)[8], double (&vi)[8], const W& w) {
    xstage8<0>(vr, vi, w);
    xstage8<1>(vr, vi, w);
    xstage8<2>(vr, vi, w);
}
template <int STRIDE>
struct XTwLds {   // slots 2, 3 and 5 are slots 0, 1 and 4 a quarter turn on (f8::sym8_src / sym8_rot): four reads for seven slots
    const double2* base;
    __device__ __forceinline__ double2 operator()(int e) const {
        const double2 x = base[f8::sym8_src(e) * STRIDE];
        return f8::sym8_rot(e) ? make_double2(x.y, -x.x) : x;
    }
};

// the four twiddle SOURCES of a radix-8 pass (rows 0..3 = slots 0, 1, 4, 6; slots 2, 3, 5 are 0, 1, 4 a quarter turn on)
template <int STRIDE>
struct XTwLds4 {
    const double2* base;
    __device__ __forceinline__ double2 operator()(int e) const {
        const int src = f8::sym8_src(e);
        const int row = src < 2 ? src : (src == 4 ? 2 : 3);
        const double2 x = base[row * STRIDE];
        return f8::sym8_rot(e) ? make_double2(x.y, -x.x) : x;
    }
};
// ... and from registers (the rows in VGPRs)
struct XTwRegs4 {
    const double2* w;
    __device__ __forceinline__ double2 operator()(int e) const {
        const int src = f8::sym8_src(e);
        const double2 x = w[src < 2 ? src : (src == 4 ? 2 : 3)];
        return f8::sym8_rot(e) ? make_double2(x.y, -x.x) : x;
    }
};
__device__ __forceinline__ constexpr int tw4_slot(int row) { return row < 2 ? row : (row == 2 ? 4 : 6); }
// table index of source row `row` (slot tw4_slot(row)) of the radix-8 pass that starts at stage S0 of a 2^LOG2N network, low index lo
template <int LOG2N, int S0>
__device__ __forceinline__ int tw4_index(int row, int lo) {
    constexpr int B0 = LOG2N - S0 - 3;
    const int e = tw4_slot(row), u = e < 4 ? 0 : (e < 6 ? 1 : 2);
    const int mloc = 4 >> u, mm = e - (8 - 2 * mloc);
    return ((mm << B0) + lo) << (S0 + u);
}
// one radix-8 pass (stages S0 .. S0+2) over the padded planes with its twiddles from an LDS table [4][2^B0]
template <int LOG2N, int S0, class IX = PadIx>
__device__ __forceinline__ void xfft_pass8_lds(double* sre, double* sim, int t, const double2* stw) {
    constexpr int B0 = LOG2N - S0 - 3;
    const int lo = t & ((1 << B0) - 1), hi = t >> B0;
    const int base = (hi << (B0 + 3)) + lo;
    double vr[8], vi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int p = IX::at(base + (i << B0)); vr[i] = sre[p]; vi[i] = sim[p]; }
    xstages8(vr, vi, XTwLds4<(1 << B0)>{stw + lo});
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int p = IX::at(base + (i << B0)); sre[p] = vr[i]; sim[p] = vi[i]; }
}

// The LAST radix-8 pass of a network whose final stage is left over (LOG2N - S0 == 4: stages S0 .. S0+2 here, then the
// twiddle-free stage S0+3 on adjacent positions p, p ^ 1): after the pass thread (hi, lo) holds positions 16 hi + 2 i + lo, so
// the last stage's partners sit in the NEIGHBOURING LANE, same register.  They are exchanged by DPP (quad_perm [1,0,3,2]) and
// the stage is finished in registers: even lanes a + b, odd lanes a - b = a + (-b) (the same IEEE results, signed zeros
// included) - written as partner + (own with its sign flipped in odd lanes), one add for both.  Saves the network's last trip
// through LDS (round 5: 16 KB read + 16 KB written per wave and half-transform at N = 16384) and its barrier.
__device__ __forceinline__ double dpp_swap_pair(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int plo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true);
    const int phi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true);
    return __hiloint2double(phi, plo);
}
template <int LOG2N, int S0, class IX = PadIx>
__device__ __forceinline__ void xfft_pass8_last_lds(double* sre, double* sim, int t, const double2* stw) {
    static_assert(LOG2N - S0 == 4, "the pass before the final stage");
    constexpr int B0 = 1;
    const int lo = t & 1, hi = t >> 1;
    // the eight positions are at(base + 2 i) = at(base) ^ 2 i for an index map that is GF(2)-linear and leaves the low five
    // bits of a position alone (Swz13Ix): ONE register instead of eight addresses held from the loads to the stores (the
    // N = 16384 kernel sits at its 128-register limit; with eight it spilled six registers' worth of the waiting spectra)
    static_assert(IX::linear_low5, "positions by XOR need a linear index map");
    int p0 = IX::at((hi << 4) + lo);
    double vr[8], vi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int p = p0 ^ (i << B0); vr[i] = sre[p]; vi[i] = sim[p]; }
    xstages8(vr, vi, XTwLds4<(1 << B0)>{stw + lo});
    asm volatile("" : "+v"(p0));   // the store addresses are formed again from p0, not kept
    const int flip = lo << 31;   // odd lanes: -own
    // (point by point, each stored as soon as it is finished, two points per scheduling region: with all sixteen exchanges
    // hoisted to the front by the max-ILP scheduler the N = 16384 kernel spilled six registers)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double pr = dpp_swap_pair(vr[i]), pi = dpp_swap_pair(vi[i]);
        const double yr = __hiloint2double(__double2hiint(vr[i]) ^ flip, __double2loint(vr[i]));
        const double yi = __hiloint2double(__double2hiint(vi[i]) ^ flip, __double2loint(vi[i]));
        const int p = p0 ^ (i << B0);
        sre[p] = pr + yr;
        sim[p] = pi + yi;
        if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
}

template <int SINK>
__global__ __launch_bounds__(512, 4) void exact_frames4096_kernel(ExactPlanDev pl, const float* __restrict__ pcm, int64_t L,
                                                               int64_t frame0, int64_t nframes, int S, ExactSinks sk) {
    constexpr int LOG2N = 12, N = 4096, T = 512, K = N / 2 + 1, Kp = rec_stride(N);
    extern __shared__ double smemd[];
    double* sre = smemd;
    double* sim = sre + N;
    double2* stwB = reinterpret_cast<double2*>(sim + N);   // [7][64]
    double2* stwC = stwB + 7 * 64;                         // [7][8]
    double* seb = reinterpret_cast<double*>(stwC + 7 * 8); // [rows+1]
    const int t = threadIdx.x;
    for (int r = t; r <= pl.rows; r += T) seb[r] = pl.ebin[r];
    if (t < 7 * 64) stwB[t] = pl.tw[f8::tw_index8<3>(t >> 6, t & 63)];
    else if (t < 7 * 64 + 7 * 8) stwC[t - 7 * 64] = pl.tw[f8::tw_index8<6>((t - 7 * 64) >> 3, (t - 7 * 64) & 7)];
    __syncthreads();
    RowLookup64 lk;
    lk.init(seb, pl.rows, pl.log_rows);
    // this workgroup's contiguous run of the (stream, frame) sequence
    const int64_t total = (int64_t)S * nframes;
    const int64_t w0 = total * blockIdx.x / gridDim.x, w1 = total * (blockIdx.x + 1) / gridDim.x;
    const double rs = 2.0 / (double)N;
    float xs[8];
    auto fetch = [&](int64_t s_, int64_t f_, unsigned tl) {
        const float* x = pcm + (size_t)s_ * L + (frame0 + f_) * pl.hop;
#pragma unroll
        for (int i = 0; i < 8; ++i) xs[i] = x[tl + (unsigned)(T * i)];
    };
    // (stream, frame) of the current work item, advanced by counting: a 64-bit division per frame is ~140 scalar
    // instructions on this hardware, and the first version had three of them in the frame loop
    int64_t s_ = w0 / nframes, f_ = w0 - s_ * nframes;
    if (w0 < w1) fetch(s_, f_, (unsigned)t);
    // the twelve spectrum positions of this thread's bins depend on the thread id only: computed once (12 VGPRs)
    int pf[6], pm[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        pf[i] = f8::zpos((4 * t - 1 + i) & (N - 1));
        pm[i] = f8::zpos((N - 4 * t + 1 - i) & (N - 1));
    }
#pragma unroll 1
    for (int64_t w = w0; w < w1; ++w) {
        int tt = t;
        asm volatile("" : "+v"(tt));   // the pass addresses are recomputed per frame, not kept (and spilled) across the loop
        {
            double vr[8], vi[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double xv = (double)xs[i];
                vr[i] = xv;
                vi[i] = xv * ((double)(tt + T * i - N / 2) * rs);
            }
            xfft_stages<LOG2N, 0, 3>(vr, vi, tt, pl.tw);
            // swz(tt + 512 i) = (swz(tt) ^ 8 (i & 1)) + 512 i (fused_r8.hip.inc)
            const int a0 = f8::swz(tt), a1 = a0 ^ 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = ((i & 1) ? a1 : a0) + T * i; sre[p] = vr[i]; sim[p] = vi[i]; }
        }
        __syncthreads();
        {   // pass B = stages 3..5: p = hi*512 + i*64 + lo (this wave's 512 positions from here on)
            double vr[8], vi[8];
            const int base = ((tt >> 6) << 9) + (tt & 63);
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 6)); vr[i] = sre[p]; vi[i] = sim[p]; }
            xstages8(vr, vi, XTwLds<64>{stwB + (tt & 63)});
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 6)); sre[p] = vr[i]; sim[p] = vi[i]; }
            wave_lds_sync();
        }
        {   // pass C = stages 6..8: p = (t >> 3)*64 + i*8 + (t & 7)
            double vr[8], vi[8];
            const int base = ((tt >> 3) << 6) + (tt & 7);
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 3)); vr[i] = sre[p]; vi[i] = sim[p]; }
            xstages8(vr, vi, XTwLds<8>{stwC + (tt & 7)});
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = f8::swz(base + (i << 3)); sre[p] = vr[i]; sim[p] = vi[i]; }
            wave_lds_sync();
        }
        {   // pass D = stages 9..11: p = 8 t + i, twiddles are constants
            double vr[8], vi[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = f8::swz((tt << 3) + i); vr[i] = sre[p]; vi[i] = sim[p]; }
            xfft_stages<LOG2N, 9, 3>(vr, vi, 0, pl.tw);
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int p = f8::swz((tt << 3) + i); sre[p] = vr[i]; sim[p] = vi[i]; }
        }
        __syncthreads();
        const int64_t sc = s_, fc = f_;
        if (++f_ == nframes) { f_ = 0; ++s_; }
        if (w + 1 < w1) fetch(s_, f_, (unsigned)tt);   // in flight during the per-bin stage
        {
            (void)sc;
            const BinSinkT<SINK> sink{sk, (size_t)w, frame0 + fc + sk.col_offset, K, Kp};
            YTd yt[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) yt[i] = split_d(sre[pf[i]], sim[pf[i]], sre[pm[i]], sim[pm[i]]);
            // (a branch-free form of the core - everything computed, gates selected at the end - measured the same: 7.64 vs 7.61 ms)
#pragma unroll
            for (int e = 0; e < 4; ++e) sink(4 * tt + e, exact_core(pl, lk, 4 * tt + e, yt[e], yt[e + 1], yt[e + 2]));
            if (tt == T - 1) {
                sink(N / 2, exact_core(pl, lk, N / 2, yt[4], yt[5], conj_d(yt[4])));
                sink.pads();
            }
        }
        __syncthreads();   // the next frame's pass A overwrites the planes
    }
}

// N = 16384: stage 0 of the DIF network in registers, a[n] = z[n] + z[n+N/2] (even bins), b[n] = (z[n] - z[n+N/2]) W^n
// (odd bins); each half is the remaining 13 stages on 8192 points, in the same planes one after the other.
// FASTX: the plan is one the branch-free per-bin core serves (exact_fast_plan) - the eight bins of a thread are then two
// basic blocks of four instead of ~50 (round 4; same bits: tests/test_gpu_exact.py runs both forms against the bit model)
template <bool FASTX, bool LIVE = false>
__global__ __launch_bounds__(1024) void exact_frames16384_kernel(ExactPlanDev pl, const float* __restrict__ pcm, int64_t L,
                                                                 int64_t frame0, int64_t nframes, ExactSinks sk) {
    constexpr int LOG2N = 14, N = 1 << LOG2N, NH = N / 2, T = 1024, K = N / 2 + 1, PN = NH, Kp = rec_stride(N);   // (swizzled planes: no padding)
    using IX = Swz13Ix;
    extern __shared__ double smemd[];
    double* sre = smemd;
    double* sim = sre + PN;
    // twiddle sources of the passes at stages 4, 7, 10 (they depend on 7, 4 and 1 bits of the thread id): 4 x (128 + 16 + 2)
    // double2 = 9.1 KB in LDS instead of 12 L2 loads per thread and half-transform (round 4: the kernel is lock-step, one
    // workgroup per CU, and every one of those loads was a ~500-cycle stall of all sixteen waves)
    double2* stw4 = reinterpret_cast<double2*>(sim + PN);   // [4][128]
    double2* stw7 = stw4 + 4 * 128;                          // [4][16]
    double2* stw10 = stw7 + 4 * 16;                          // [4][2]
    double* seb = reinterpret_cast<double*>(stw10 + 4 * 2);
    const int t = threadIdx.x;
    int64_t f;
    int s;
    LiveBlock lb;                                        // live multi-stream launch (live.hip.inc)
    constexpr bool live = LIVE;
    if (live) {
        if (!lb.init(sk.live, pl.hop, T)) return;
        s = lb.s; f = lb.f;
    } else {
        frame_of_block(f, s);
    }
    const int64_t j = live ? f : frame0 + f;
    const int64_t jcol = live ? lb.column() : j + sk.col_offset;
    if (sk.edges_lds)
        for (int r = t; r <= pl.rows; r += T) seb[r] = pl.ebin[r];
    if (t < 4 * 128) stw4[t] = pl.tw[tw4_index<LOG2N, 4>(t >> 7, t & 127)];
    else if (t < 4 * 128 + 4 * 16) stw7[t - 512] = pl.tw[tw4_index<LOG2N, 7>((t - 512) >> 4, (t - 512) & 15)];
    else if (t < 4 * 128 + 4 * 16 + 4 * 2) stw10[t - 576] = pl.tw[tw4_index<LOG2N, 10>((t - 576) >> 1, (t - 576) & 1)];
    const float* x = pcm + (size_t)s * L + j * pl.hop;
    const double rs = 2.0 / (double)N;
    // YT[8t-1+u], u = 0..9, are the split spectra the thread's eight bins need: odd u (even bins) come from the first half,
    // even u (odd bins) from the second.  The five of the first half wait in registers (20 doubles) while the second half is
    // transformed; the per-bin stage then runs on the second half's planes and reads its five straight from LDS.
    // (Until round 4 all ten waited in PRIVATE memory - 40 doubles stored and loaded once per frame through a laundered index,
    // because ten in registers pushed the second transform past 128 VGPRs and the compiler spilled 210 of them: a timing-only
    // build without that traffic ran 10.6 instead of 16.1 ms on 8 streams.)
    YTd ev[5];
    // (Round 5, measured and not kept: fetching the frame's samples once and holding them as sixteen floats across the first
    // half's passes - 128 VGPRs + 11 spilled dwords, 63.2 vs 62.1 ms per 64-stream step.  Both halves load them.)
    const double ramp0 = (double)(t - N / 2) * rs;   // ramp of point t; point t + 1024 i lies 0.125 i further, point + N/2 another 1.0 (exact)
    // The sixteen samples of this thread (the same for both halves) are requested a second time at the END of the first half -
    // behind its last pass, where the transform's registers are free - so that the second half finds them there instead of
    // waiting for a global round trip at its head (holding them across the first half's passes costs sixteen registers at the
    // kernel's tightest spot: measured slower, see above).
    float xs0[8], xs1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        xs0[i] = live ? lb.sample(t + T * i) : x[t + T * i];
        xs1[i] = live ? lb.sample(t + T * i + NH) : x[t + T * i + NH];
    }
    // ... and with them the second half's four stage-0 twiddles W^(t + 1024 r) (two more exposed round trips at its head)
    double2 wq[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    // (the first two twiddle sources of stages 1..3 fetched the same way: 17.71 against 17.55 ms - not kept)
    // The two halves as two copies of the code (a generic lambda called with a compile-time half): registers are then
    // allocated per half - the first one has no waiting spectra (40 registers) beside it: 119 registers and no spill instead of
    // 128 and one; 16.69 -> 16.56 ms on 16 streams.  (All four stage-1..3 twiddle sources at once in the first half: the same.)
    auto do_half = [&](auto half_c) {
        constexpr int half = decltype(half_c)::value;
        double vr[8], vi[8];
        // launder the thread id per half: the sample / twiddle addresses are then recomputed (one add each) instead of
        // being kept as 64-bit pairs across the whole transform - the compiler spilled two dozen of them
        unsigned tt = (unsigned)t;
        asm volatile("" : "+v"(tt));
#pragma unroll
        for (int ii = 0; ii < 8; ++ii) {
            const int i = (ii >> 1) | ((ii & 1) << 2);   // 0, 4, 1, 5, ...: the two points that share a twiddle load side by side
            const double x0 = (double)xs0[i], x1 = (double)xs1[i];
            const double ra = ramp0 + 0.125 * (double)i;
            const double ar = x0, ai = x0 * ra, br = x1, bi = x1 * (ra + 1.0);
            if constexpr (half == 0) {
                vr[i] = ar + br;
                vi[i] = ai + bi;
            } else {
                const double dr = ar - br, di = ai - bi;
                // W^n for n = t + 1024 i: points i and i + 4 lie a quarter turn apart, and the table is quarter-turn symmetric
                // (tw[q + N/4] = (tw[q].y, -tw[q].x) exactly): four loads serve the eight points
                const double2 w0 = wq[i & 3];
                const double2 w = (i & 4) ? make_double2(w0.y, -w0.x) : w0;
                const double tt = di * w.y;
                const double uu = di * w.x;
                vr[i] = __builtin_fma(dr, w.x, -tt);
                vi[i] = __builtin_fma(dr, w.y, uu);
            }
            if ((ii & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // two twiddle loads (four points) in flight at a time
        }
        // the four twiddle sources of stages 1..3 (slots 0, 1, 4, 6; the other three are a quarter turn on) in TWO round trips:
        // loaded stage by stage they were three exposed L2 round trips of all sixteen lock-step waves per half (all four at
        // once: 8 registers spilled; fetched with the samples: 12)
        double2 twh[4];
        twh[0] = pl.tw[tw4_index<LOG2N, 1>(0, (int)tt)];
        twh[1] = pl.tw[tw4_index<LOG2N, 1>(1, (int)tt)];
        xstage8<0>(vr, vi, XTwRegs4{twh});
        __builtin_amdgcn_sched_barrier(0);
        twh[2] = pl.tw[tw4_index<LOG2N, 1>(2, (int)tt)];
        twh[3] = pl.tw[tw4_index<LOG2N, 1>(3, (int)tt)];
        xstage8<1>(vr, vi, XTwRegs4{twh});
        xstage8<2>(vr, vi, XTwRegs4{twh});
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();   // the previous half's spectrum reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int p = IX::at((int)tt + T * i); sre[p] = vr[i]; sim[p] = vi[i]; }
        __syncthreads();
        xfft_pass8_lds<LOG2N, 4, IX>(sre, sim, (int)tt, stw4);
        __syncthreads();                                      // B0 = 7: the pass at stage 7 reads across waves
        xfft_pass8_lds<LOG2N, 7, IX>(sre, sim, (int)tt, stw7);
        wave_lds_sync();                                      // from here on a wave touches its own 512 positions only
        xfft_pass8_last_lds<LOG2N, 10, IX>(sre, sim, (int)tt, stw10);   // stages 10..12 and, through DPP, the last one
        if constexpr (half == 0) {                                      // the second half's samples: in flight across the barrier and the spectrum reads
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                xs0[i] = live ? lb.sample((int)tt + T * i) : x[tt + (unsigned)(T * i)];
                xs1[i] = live ? lb.sample((int)tt + T * i + NH) : x[tt + (unsigned)(T * i) + NH];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) wq[r] = pl.tw[tt + (unsigned)(T * r)];
        }
        __syncthreads();                                                // the closing barrier: the spectrum is read across waves
        // local position p holds Z[2 bitrev13(p) + half]
        if constexpr (half == 0) {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                // (a lane map that makes these reads conflict-free - half-waves over bin bits 5..9 - was measured 4 % SLOWER: the
                // records of neighbouring lanes then lie 256 B apart and the stores coalesce worse than the reads gain)
                const int kf = (8 * (int)tt + 2 * i) & (N - 1), km = (N - kf) & (N - 1);
                const int pf = IX::at((int)(__brev((unsigned)(kf >> 1)) >> (32 - 13))), pm = IX::at((int)(__brev((unsigned)(km >> 1)) >> (32 - 13)));
                ev[i] = split_d(sre[pf], sim[pf], sre[pm], sim[pm]);   // YT[8t-1+u], u = 2i + 1
            }
        }
    };
    do_half(std::integral_constant<int, 0>{});
    do_half(std::integral_constant<int, 1>{});
    // the second half's planes are complete (closing barrier of xfft_rest): YT[8t-1+u] for even u
    int tb = t;
    asm volatile("" : "+v"(tb));
    auto od_at = [&](int u) {
        const int kf = (8 * tb - 1 + u) & (N - 1), km = (N - kf) & (N - 1);
        const int pf = IX::at((int)(__brev((unsigned)(kf >> 1)) >> (32 - 13))), pm = IX::at((int)(__brev((unsigned)(km >> 1)) >> (32 - 13)));
        return split_d(sre[pf], sim[pf], sre[pm], sim[pm]);
    };
    RowLookup64 lk;
    lk.init(sk.edges_lds ? seb : pl.ebin, pl.rows, pl.log_rows);
    const BinSink sink{sk, pl, s, (size_t)s * nframes + f, jcol, K, Kp, ring_slot_of(sk, jcol)};
    const int g = t;
    auto core = [&](int k, const YTd& wm, const YTd& wc, const YTd& wp) {
        if constexpr (FASTX) {
            const XBinF b = exact_core_fast<true>(pl, lk.eb, (double)k, (double)pl.D, wm, wc, wp);
            return XBin{b.power, b.q, b.dcol, b.row};
        } else {
            return exact_core(pl, lk, k, wm, wc, wp);
        }
    };
#pragma unroll 1
    for (int h4 = 0; h4 < 2; ++h4) {   // two groups of four bins: u = 4 h4 .. 4 h4 + 5, three from LDS (even u), three from ev
        const YTd od0 = od_at(4 * h4), od1 = od_at(4 * h4 + 2), od2 = od_at(4 * h4 + 4);
        const int k0 = 8 * g + 4 * h4;
        XBin o[4];
        o[0] = core(k0, od0, ev[0], od1);
        o[1] = core(k0 + 1, ev[0], od1, ev[1]);
        o[2] = core(k0 + 2, od1, ev[1], od2);
        o[3] = core(k0 + 3, ev[1], od2, ev[2]);
        sink.four(k0, o);
        ev[0] = ev[2]; ev[1] = ev[3]; ev[2] = ev[4];   // the next group's three (after the second group: ev[0] = YT[8t+8])
    }
    if (g == T - 1) {   // the Nyquist bin: Y[N/2+1] = conj Y[N/2-1], T[N/2+1] = conj T[N/2-1] exactly
        const YTd wm = od_at(8);
        sink(N / 2, exact_core(pl, lk, N / 2, wm, ev[0], conj_d(wm)));
        sink.pads();
    }
    if (live && live_last_arrival(sk.live, s, lb.bframes, sre))
        live_finalize<unsigned long long>(sk.live, lb.d, s, sk.hist, (int)sk.hist_slots, pl.rows, pl.D + sk.live.lat_extra, T, LiveConvExact{sk.fin_map});
}

// records of all C frames of a stream chunk -> finished columns: workgroup (tile of `tile` columns, stream), u64 LDS
// histogram (ds_add_u64: integer LDS atomics run at the rate of plain stores), frames [c0-D, c0+tile+D) streamed through it
__global__ __launch_bounds__(1024) void exact_tile_scatter_kernel(const long long* __restrict__ rec_q,
                                                                  const uint32_t* __restrict__ rec_key, int Kp, int R, int D,
                                                                  int tile, ExactDbMap dm, const uint32_t* __restrict__ lut,
                                                                  int64_t C, float* __restrict__ db, uint32_t* __restrict__ rgba,
                                                                  uint8_t* __restrict__ index) {
    extern __shared__ double smemd[];
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(smemd);   // [tile][R]
    uint32_t* slut = reinterpret_cast<uint32_t*>(hist + (size_t)tile * R);
    const int tid = threadIdx.x, s = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * tile;
    const int64_t c1 = (c0 + tile < C) ? c0 + tile : C;
    for (int q = tid; q < tile * R; q += 1024) hist[q] = 0ull;
    if (tid < 256) slut[tid] = lut[tid];
    __syncthreads();
    const int64_t jlo = c0 - D > 0 ? c0 - D : 0, jhi = (c1 + D < C) ? c1 + D : C;
    const int span = (int)(c1 - c0);
    const int nch = Kp / 4;   // chunks of 4 records per frame
    const int64_t njobs = (jhi - jlo) * nch;
    const size_t base = (size_t)s * C * Kp;
    for (int64_t job = tid; job < njobs; job += 1024) {
        const int64_t j = jlo + job / nch;
        const int k0 = (int)(job % nch) * 4;
        const size_t at = base + (size_t)j * Kp + k0;
        const uint4 key4 = *reinterpret_cast<const uint4*>(rec_key + at);
        const longlong2 qa = *reinterpret_cast<const longlong2*>(rec_q + at);
        const longlong2 qb = *reinterpret_cast<const longlong2*>(rec_q + at + 2);
        const unsigned keys[4] = {key4.x, key4.y, key4.z, key4.w};
        const long long qs[4] = {qa.x, qa.y, qb.x, qb.y};
        const int jrel = (int)(j - c0);
        unsigned cur = 0xFFFFFFFFu;
        unsigned long long acc = 0ull;
        auto flush = [&]() {
            const int colrel = jrel + (int)(cur >> 16) - 32768;
            if (cur != 0xFFFFFFFFu && (unsigned)colrel < (unsigned)span)
                __hip_atomic_fetch_add(hist + (size_t)colrel * R + (cur & 0xFFFFu), acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (keys[u] != cur) { flush(); acc = 0ull; cur = keys[u]; }
            acc += (unsigned long long)qs[u];
        }
        flush();
    }
    __syncthreads();
    const int ncell4 = span * R / 4;
    for (int q = tid; q < ncell4; q += 1024) {
        const CellOut o0 = exact_cell(dm, hist[4 * q]), o1 = exact_cell(dm, hist[4 * q + 1]);
        const CellOut o2 = exact_cell(dm, hist[4 * q + 2]), o3 = exact_cell(dm, hist[4 * q + 3]);
        const size_t o = ((size_t)s * C + c0) * R + (size_t)q * 4;
        if (db) *reinterpret_cast<float4*>(db + o) = make_float4(o0.db, o1.db, o2.db, o3.db);
        if (rgba) *reinterpret_cast<uint4*>(rgba + o) = make_uint4(slut[o0.index], slut[o1.index], slut[o2.index], slut[o3.index]);
        if (index) *reinterpret_cast<uint32_t*>(index + o) =
            (uint32_t)o0.index | ((uint32_t)o1.index << 8) | ((uint32_t)o2.index << 16) | ((uint32_t)o3.index << 24);
    }
}


// The same job with a WALKING ring: one workgroup walks a segment of one stream, F frames per step, through a (2D+F)-slot
// u64 ring in LDS, so every record is read once (plus a 2D-frame halo per segment) instead of (16+2D)/16 times.  Used
// whenever the ring fits (N = 4096 / hop 256: 18 slots x 8 KB = 144 KB) - and, since round 5, when it fits after the ROW SPLIT
// of exact_fused_lr.hip.inc: rows >= RL of every slot in LDS ([slots][R - RL]), rows < RL - the sparse low end of a
// log-frequency axis - in a per-workgroup scratch in global memory ([slots][RL] u64) touched by device-scope atomics only
// (adds while scattering, one swap per cell = read + clear when a column leaves).  N = 16384 / hop 512 (38 slots): 516 rows
// in LDS, the 508 below 680 Hz (2.8 % of the bins) in L2; every record is read 1.1x instead of 3x.
__global__ __launch_bounds__(1024) void exact_walk_scatter_kernel(const long long* __restrict__ rec_q,
                                                                  const uint32_t* __restrict__ rec_key, int Kp, int R, int D, int F,
                                                                  int seglen, ExactDbMap dm, const uint32_t* __restrict__ lut,
                                                                  int64_t C, float* __restrict__ db, uint32_t* __restrict__ rgba,
                                                                  uint8_t* __restrict__ index, int RL,
                                                                  unsigned long long* __restrict__ lowbase, int abl) {
    // abl (diagnostic builds only, WRONG results; 0 in the product): 1 = no low-row (global) atomics, 2 = no LDS atomics either,
    // 3 = no finalize arithmetic / stores, 4 = no record loads (the first batch is reused)
    extern __shared__ double smemd[];
    const int slots = 2 * D + F, RH = R - RL;
    unsigned long long* ring = reinterpret_cast<unsigned long long*>(smemd);   // [slots][RH]
    uint32_t* slut = reinterpret_cast<uint32_t*>(ring + (size_t)slots * RH);
    uint32_t* lmask = slut + 256;                                    // [slots][MW]: one bit per low-row cell that took an add
    const int MW = (RL + 31) >> 5;
    const int tid = threadIdx.x, s = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * seglen;
    if (c0 >= C) return;
    const int64_t c1 = (c0 + seglen < C) ? c0 + seglen : C;
    unsigned long long* low = lowbase + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(slots * RL);
    for (int q = tid; q < slots * RH; q += 1024) ring[q] = 0ull;
    for (int q = tid; q < slots * MW; q += 1024) lmask[q] = 0u;
    if (tid < 256) slut[tid] = lut[tid];
    __syncthreads();
    const int nch = Kp / 4;
    const size_t base = (size_t)s * C * Kp;
    const int64_t jfirst = c0 - D, jstop = c1 + D;
    const int span = (int)(c1 - c0);
    const unsigned nch_magic = (unsigned)((0x100000000ull + (unsigned)nch - 1) / (unsigned)nch);   // job / nch for job < 2^16 by one multiply
    const int qpc = R / 4;                                           // quads of four cells per column
    const unsigned qpc_magic = (unsigned)((0x100000000ull + (unsigned)qpc - 1) / (unsigned)qpc);
    int slot0 = 0;                                                   // ring slot of column j0 (frame j0's own column), = (j0 - jfirst) mod slots
    // A step's F * nch jobs (one job = four records of one frame: 48 bytes) go to the threads 1024 apart, two jobs to a batch.
    // The batches are double-buffered: the loads of batch b + 1 are in flight while batch b is scattered, and the first batch
    // of the NEXT step is requested before the step's barriers and the finalize phase, so the record stream never stops (the
    // kernel is one lock-step workgroup per CU; with plain rounds it ran at 45 % of the HBM rate the tile kernel reaches).
    const int njobs = F * nch;
    const int nb = ((njobs + 1023) / 1024 + 1) / 2;                  // batches of two jobs per thread and step
    struct Batch { uint4 key[2]; longlong2 qa[2], qb[2]; };
    auto load = [&](Batch& bt, int64_t jb, int b) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int job = tid + 1024 * (2 * b + u);
            const int fo = (int)__umulhi((unsigned)job, nch_magic);
            const int64_t j = jb + fo;
            const bool live = job < njobs && j >= 0 && j < C;
            const size_t at = live ? base + (size_t)j * Kp + (size_t)(job - fo * nch) * 4 : base;   // (a dead job reads the stream's first chunk)
            bt.key[u] = *reinterpret_cast<const uint4*>(rec_key + at);
            bt.qa[u] = *reinterpret_cast<const longlong2*>(rec_q + at);
            bt.qb[u] = *reinterpret_cast<const longlong2*>(rec_q + at + 2);
        }
    };
    auto scatter = [&](const Batch& bt, int64_t jb, int b, int slotb) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int job = tid + 1024 * (2 * b + u);
            const int fo = (int)__umulhi((unsigned)job, nch_magic);
            const int64_t j = jb + fo;
            if (!(job < njobs && j >= 0 && j < C)) continue;
            const int jrel = (int)(j - c0);
            // ring slot of column c0 + colrel is (colrel + D) mod slots; colrel = jrel + dcol with |dcol| <= D < slots, so one
            // modulo per job (the frame's own slot) and a wrap per run replace a modulo per run (~20 instructions each)
            const int jslot = slotb + fo >= slots ? slotb + fo - slots : slotb + fo;
            const unsigned keys[4] = {bt.key[u].x, bt.key[u].y, bt.key[u].z, bt.key[u].w};
            const long long qs[4] = {bt.qa[u].x, bt.qa[u].y, bt.qb[u].x, bt.qb[u].y};
            unsigned cur = 0xFFFFFFFFu;
            unsigned long long acc = 0ull;
            auto flush = [&]() {
                const int dcol = (int)(cur >> 16) - 32768;
                const int colrel = jrel + dcol;
                if (cur != 0xFFFFFFFFu && (unsigned)colrel < (unsigned)span) {
                    int sl = jslot + dcol;
                    sl += sl < 0 ? slots : 0;
                    sl -= sl >= slots ? slots : 0;
                    const int row = (int)(cur & 0xFFFFu);
                    if (row >= RL) { if (abl != 2) __hip_atomic_fetch_add(ring + (size_t)sl * RH + (row - RL), acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
                    else if (abl != 1 && abl != 2) {
                        __hip_atomic_fetch_add(low + (size_t)sl * RL + row, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_or(lmask + sl * MW + (row >> 5), 1u << (row & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            };
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (keys[w] != cur) { flush(); acc = 0ull; cur = keys[w]; }
                acc += (unsigned long long)qs[w];
            }
            flush();
        }
    };
    Batch ba, bb;
    load(ba, jfirst, 0);
    for (int64_t j0 = jfirst; j0 < jstop; j0 += F, slot0 = slot0 + F >= slots ? slot0 + F - slots : slot0 + F) {
#pragma unroll 1
        for (int b = 0; b < nb; b += 2) {
            if (b + 1 < nb && abl != 4) load(bb, j0, b + 1);
            scatter(ba, j0, b, slot0);
            if (b + 2 < nb && abl != 4) load(ba, j0, b + 2);
            if (b + 1 < nb) scatter(abl != 4 ? bb : ba, j0, b + 1, slot0);
        }
        // this wave's low-row adds are complete before the columns leave (no load is outstanding here); then the next step's
        // first batch, in flight across the barriers and the finalize phase
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (j0 + F < jstop && abl != 4) load(ba, j0 + F, 0);
        __syncthreads();
        // columns j0-D .. j0+F-1-D are complete: finalise, store, clear
        for (int q = tid; q < F * qpc; q += 1024) {
            const int cc = (int)__umulhi((unsigned)q, qpc_magic), cell = (q - cc * qpc) << 2;
            const int64_t col = j0 - D + cc;
            if (col >= c0 && col < c1 && abl != 3) {
                int sl = slot0 - D + cc;                             // (col - jfirst) mod slots, col = j0 - D + cc
                sl += sl < 0 ? slots : 0;
                sl -= sl >= slots ? slots : 0;
                unsigned long long e0, e1, e2, e3;
                if (cell < RL) {   // low rows: read + clear in one returning device-scope atomic each (RL % 4 == 0) - only the cells
                                   // that took an add (their bit in lmask): an atomic is a 32-byte request to the memory side
                    unsigned long long* lp = low + (size_t)sl * RL + cell;
                    uint32_t* mw = lmask + sl * MW + (cell >> 5);
                    const unsigned sh = (unsigned)(cell & 31), bits = (*mw >> sh) & 0xFu;
                    e0 = e1 = e2 = e3 = 0ull;
                    if (bits & 1u) e0 = __hip_atomic_exchange(lp + 0, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bits & 2u) e1 = __hip_atomic_exchange(lp + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bits & 4u) e2 = __hip_atomic_exchange(lp + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bits & 8u) e3 = __hip_atomic_exchange(lp + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bits) __hip_atomic_fetch_and(mw, ~(0xFu << sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    unsigned long long* cp = ring + (size_t)sl * RH + (cell - RL);
                    e0 = cp[0]; e1 = cp[1]; e2 = cp[2]; e3 = cp[3];
                    cp[0] = 0ull; cp[1] = 0ull; cp[2] = 0ull; cp[3] = 0ull;
                }
                const CellOut o0 = exact_cell(dm, e0), o1 = exact_cell(dm, e1), o2 = exact_cell(dm, e2), o3 = exact_cell(dm, e3);
                const size_t o = ((size_t)s * C + col) * R + cell;
                if (db) *reinterpret_cast<float4*>(db + o) = make_float4(o0.db, o1.db, o2.db, o3.db);
                if (rgba) *reinterpret_cast<uint4*>(rgba + o) = make_uint4(slut[o0.index], slut[o1.index], slut[o2.index], slut[o3.index]);
                if (index) *reinterpret_cast<uint32_t*>(index + o) =
                    (uint32_t)o0.index | ((uint32_t)o1.index << 8) | ((uint32_t)o2.index << 16) | ((uint32_t)o3.index << 24);
            }
        }
        if (RL > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the swaps are complete before the slots take adds again
        __syncthreads();
    }
}

}  // namespace ex

// (LDS of a frame kernel - its planes, and the binary64 row edges when they fit beside them: exact_frames_lds, emspec_kernel_plan.h)
// (a live multi-stream launch, LIVE: nframes = the largest per-stream frame count + 1, the ingest workgroup)
template <int LOG2N>
static hipError_t launch_exact_frames_t(const ExactPlanDev& pl, const float* pcm, int64_t L, int S, int64_t frame0,
                                        int64_t nframes, const ExactSinks& sk, hipStream_t st) {
    constexpr int N = 1 << LOG2N;
    ExactSinks sk2 = sk;
    const ExactFramesLds lds = exact_frames_lds(exact_frames_planes(N), pl.rows);
    sk2.edges_lds = lds.edges_lds;
    if (lds.bytes > kLdsBytes) return hipErrorInvalidValue;
    return pick_bool(ex::exact_fast(pl), [&](auto FASTX) { return pick_bool(sk.live.streams != nullptr, [&](auto LIVE) {
        return launch_k(ex::exact_frames_kernel<LOG2N, FASTX(), LIVE()>, dim3((unsigned)nframes, (unsigned)S), dim3(N / 8), lds.bytes, st, pl, pcm, L, frame0, nframes, sk2);
    }); });
}

hipError_t launch_exact_frames(int n, const ExactPlanDev& pl, const float* pcm, int64_t L, int S, int64_t frame0,
                               int64_t nframes, const ExactSinks& sk, hipStream_t st) {
    if (nframes <= 0 || S <= 0) return hipSuccess;
    if (S > 65535 || nframes > 0x7fffffffLL) return hipErrorInvalidValue;
    if (n == 4096) {
        // the persistent kernel when its 80 KB fit twice per CU (rows <= 1024) and the launch is a batch
        const size_t lds = exact_frames4096_lds_bytes(pl.rows);
        const bool dump_only = sk.power && !sk.rec_q && !sk.hist, rec_only = sk.rec_q && !sk.power && !sk.hist;
        if (exact_frames4096_persistent(pl.rows, S, nframes) && (dump_only || rec_only)) {
            const int64_t g = std::min<int64_t>((int64_t)2 * device_cus(), (int64_t)S * nframes);
            return pick_int<1, 2>(dump_only ? 1 : 2, [&](auto SINK) {
                return launch_k(ex::exact_frames4096_kernel<SINK()>, dim3((unsigned)g), dim3(512), lds, st, pl, pcm, L, frame0, nframes, S, sk);
            });
        }
    }
    if (n == 16384) {
        ExactSinks sk2 = sk;
        const ExactFramesLds lds = exact_frames_lds(exact_frames_planes(n), pl.rows);
        sk2.edges_lds = lds.edges_lds;
        return pick_bool(ex::exact_fast(pl), [&](auto FASTX) { return pick_bool(sk.live.streams != nullptr, [&](auto LIVE) {
            return launch_k(ex::exact_frames16384_kernel<FASTX(), LIVE()>, dim3((unsigned)nframes, (unsigned)S), dim3(1024), lds.bytes, st, pl, pcm, L, frame0, nframes, sk2);
        }); });
    }
    if (!supported_fft(n)) return hipErrorInvalidValue;
    return pick_int<8, 9, 10, 11, 12, 13>(__builtin_ctz((unsigned)n), [&](auto LOG2N) {
        return launch_exact_frames_t<LOG2N()>(pl, pcm, L, S, frame0, nframes, sk, st);
    });
}

// (ExactScatterPlan - walking ring whole, walking ring with its low rows in a global scratch, or tiles - and its segment rule:
// emspec_seg_plan.h)
static ExactScatterPlan exact_scatter_plan(int n, const ExactPlanDev& pl, int S, int64_t C, const float* ebin_f32) {
    return exact_scatter_plan(device_cus(), ex::rec_stride(n), n, pl.rows, pl.D, S, C, ebin_f32);
}
// bytes of low-row scratch a batch of S streams needs (0: none); the launcher runs the streams in groups that fit what it gets
size_t exact_scatter_scratch_bytes(int n, const ExactPlanDev& pl, int S, int64_t C, const float* ebin_f32) {
    if (S <= 0 || C <= 0) return 0;
    const ExactScatterPlan sp = exact_scatter_plan(n, pl, S, C, ebin_f32);
    if (!sp.F || !sp.rl) return 0;
    return (size_t)scratch_groups(sp.nseg, S) * sp.scratch_per_group;
}

hipError_t launch_exact_tile_scatter(const long long* rec_q, const uint32_t* rec_key, int n, const ExactPlanDev& pl,
                                     const ExactDbMap& m, const uint8_t* lut, int S, int64_t C, float* db, uint8_t* rgba,
                                     uint8_t* index, hipStream_t st, const float* ebin_f32, unsigned long long* low,
                                     size_t low_bytes) {
    if (S <= 0 || C <= 0) return hipSuccess;
    if (S > 65535) return hipErrorInvalidValue;
    {
        ExactScatterPlan sp = exact_scatter_plan(n, pl, S, C, ebin_f32);
        if (sp.F && sp.rl && (!low || !scratch_holds_a_stream(low_bytes, sp.scratch_per_group, sp.nseg))) sp.F = 0;   // no scratch: tiles
        if (sp.F) {
            const int64_t s_per = streams_per_launch(S, sp.nseg, low_bytes, sp.scratch_per_group);
            int walk_abl = 0;
#ifdef EMSPEC_DIAG
            if (const char* ev = getenv("EMSPEC_WALK_ABL")) walk_abl = atoi(ev);   // timing-only ablations
#endif
            const size_t Kp = (size_t)ex::rec_stride(n), cells = (size_t)C * pl.rows;
            for (int64_t s0 = 0; s0 < S; s0 += s_per) {
                const int sc = (int)std::min<int64_t>(s_per, S - s0);
                const hipError_t e = launch_k(ex::exact_walk_scatter_kernel, dim3((unsigned)sp.nseg, (unsigned)sc), dim3(1024), sp.lds, st,
                                              rec_q + (size_t)s0 * C * Kp, rec_key + (size_t)s0 * C * Kp, Kp, pl.rows, pl.D, sp.F, sp.seg, m,
                                              reinterpret_cast<const uint32_t*>(lut), C, db ? db + (size_t)s0 * cells : nullptr,
                                              rgba ? reinterpret_cast<uint32_t*>(rgba) + (size_t)s0 * cells : nullptr,
                                              index ? index + (size_t)s0 * cells : nullptr, sp.rl, low, walk_abl);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        }
    }
    const TilePlan tp = tile_scatter_plan(pl.rows, C, 8, 16);
    if (!tp.ok) return hipErrorInvalidValue;
    return launch_k(ex::exact_tile_scatter_kernel, dim3((unsigned)tp.ntiles, (unsigned)S), dim3(1024), tp.lds, st, rec_q, rec_key,
                    ex::rec_stride(n), pl.rows, pl.D, tp.tile, m, reinterpret_cast<const uint32_t*>(lut), C, db,
                    reinterpret_cast<uint32_t*>(rgba), index);
}

}  // namespace emspec
