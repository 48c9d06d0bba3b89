// fused.hip.inc — launcher of the fused batch kernels (LDS column ring).  Included by kernels.hip.
//
// Kernels (each in its own .inc):
//   fused4096_pp_kernel<HOP>   N = 4096, hop 256/512/1024 — the headline path: two teams half an iteration apart (fused_pp.hip.inc;
//                              fused_r8.hip.inc holds its helpers and the lock-step form, a diagnostic A/B variant since round 3)
//   fused8192_kernel<HOP>      N = 8192, hop 512/1024                                  (fused_n8192.hip.inc)
//   fused_small_pp_kernel<S>   N = 4096/2048/1024 at any hop whose ring fits in LDS    (fused_small.hip.inc; same schedule)
//   fused16384_kernel          N = 16384 (ring parked in registers while the FFT owns LDS) (fused_n16384.hip.inc)
// Diagnostic builds (-DEMSPEC_DIAG -> libemspec_diag.so) add the stamped builds and the
// A/B variants r8 (lock step) / pp3, ppt (round 3's schedule) / r16 / r8t (diag/*.inc), selectable with EMSPEC_FUSED_VARIANT;
// none of that is in libemspec.so.
#include "fused_r8.hip.inc"
#include "fused_n8192.hip.inc"
#include "fused_small.hip.inc"
#include "fused_n16384.hip.inc"
#include "fused_pp.hip.inc"
#ifdef EMSPEC_DIAG
#include "diag/fused_r16.hip.inc"
#include "diag/fused_r8t.hip.inc"
#include "diag/fused_pp3.hip.inc"
#endif
namespace emspec {

#ifdef EMSPEC_DIAG
// 0 = the product kernel: 1024 threads, radix 8, the two teams half an iteration apart (default),
// 1 = 512-thread radix-16 variant ("r16"), 2 = 1024-thread radix-8 with decoupled teams ("r8t"),
// 3 = the lock-step form of the product kernel ("r8": the default until round 3),
// 4 = round 3's form of the product kernel (spectrum reads at the start of role 1) with per-team software barriers
//     instead of the workgroup barrier ("ppt"), 5 = that form as it was the product in rounds 3-4 ("pp3")
static int fused_variant() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("EMSPEC_FUSED_VARIANT");
        v = 0;
        if (e && e[0] == 'r' && e[1] == '1') v = 1;
        if (e && e[0] == 'r' && e[1] == '8' && e[2] == 't') v = 2;
        if (e && e[0] == 'r' && e[1] == '8' && e[2] != 't') v = 3;
        if (e && e[0] == 'p' && e[1] == 'p' && e[2] == 't') v = 4;
        if (e && e[0] == 'p' && e[1] == 'p' && e[2] == '3') v = 5;
    }
    return v;
}
static int* fused_errflag() {   // device word raised by a timed-out spin in the decoupled-team kernel
    static int* p[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!p[dev & 63]) {
        if (hipMalloc(&p[dev & 63], sizeof(int)) != hipSuccess) return nullptr;
        (void)hipMemset(p[dev & 63], 0, sizeof(int));
    }
    return p[dev & 63];
}
int fused_read_errflag() {
    int v = 0;
    int* p = fused_errflag();
    if (p) (void)hipMemcpy(&v, p, sizeof(int), hipMemcpyDeviceToHost);
    return v;
}
int fused_waves_per_group() { return fused_variant() == 1 ? 8 : 16; }
static bool diag_no_fused() {
    static int off = -1;
    if (off < 0) { const char* e = getenv("EMSPEC_NO_FUSED"); off = (e && e[0] == '1') ? 1 : 0; }   // A/B aid
    return off != 0;
}
#else
static constexpr int fused_variant() { return 0; }
static constexpr bool diag_no_fused() { return false; }
#endif

// (the specialised FAST kernels serve the plans of emspec_plan_is_fast, emspec_device.h: reassignment ON, log-spaced rows, and
// a power floor that keeps every accumulated bin's 64 P inside the range of recip_normal)

bool fused_supported(int n, int hop, int rows, int reassign) {
    if (diag_no_fused()) return false;
    // the default (r8) kernel is built for hop 256, 512 and 1024 (the diagnostic A/B variants for hop 256 only);
    // N = 8192 (fused_n8192.hip.inc) for hop 512 and 1024; N = 16384 for any hop whose ring fits the register park
    const bool rows_ok = rows % 4 == 0 && rows >= 64 && rows <= 1024;
    if (n == f14::N) return fused_variant() == 0 && fused16384_supported(hop, rows, reassign);
    if (n == f13::N) return fused_variant() == 0 && (hop == 512 || hop == 1024) && rows_ok;
    const bool r8_hop = hop == 256 || ((fused_variant() == 0 || fused_variant() >= 3) && (hop == 512 || hop == 1024));
    if (n == f8::N && r8_hop) return rows_ok;
    if (n == 4096 || n == 2048 || n == 1024) {   // fused_small.hip.inc: any hop whose ring (2D + F column slots) fits in LDS
        const int D = reassign ? (n + 2 * hop - 1) / (2 * hop) : 0;
        return (fused_variant() == 0 || fused_variant() == 3) && rows_ok && hop >= 1 && hop <= n &&
               fused_small_lds_bytes(rows, fused_small_slots(n, D)) <= (size_t)160 * 1024;
    }
    return false;
}

hipError_t launch_fused(int n, const PlanDev& pl, const DbMap& m, const uint8_t* lut, const float* pcm, int64_t L,
                        int S, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st,
                        unsigned long long* stamps, int64_t* stamp_groups) {
    const bool big_n = n == f14::N;
    const bool r8_shape = n == f8::N && (pl.hop == 256 || pl.hop == 512 || pl.hop == 1024);
    const bool small_n = (n == 4096 || n == 2048 || n == 1024) && !r8_shape;   // fused_small: ring sized from pl.D at run time
    if (!fused_supported(n, pl.hop, pl.rows, pl.reassign) || (!small_n && !big_n && pl.D > n / (2 * pl.hop))) return hipErrorNotSupported;
    if (S <= 0 || C <= 0) return hipSuccess;
    if (S > 65535) return hipErrorInvalidValue;
#ifndef EMSPEC_DIAG
    if (stamps || stamp_groups) return hipErrorNotSupported;   // stamped builds live in libemspec_diag.so only
#endif
    // Segments: as long as possible (every segment recomputes a 2D-frame halo) while the launch still
    // has at least one workgroup per CU, and - as long as segments stay >= 256 columns - about four:
    //   nseg = max(ceil(CUs/S), min(floor(4 CUs/S), ceil(C/256)), ceil(C/1024)) per stream.
    // Equal segments and a workgroup count near a multiple of the CU count keep the last round of workgroups
    // full (256 CUs: 64 streams -> 16 x 1024 columns = 1024 workgroups; 16 streams -> 64 x 256 = 1024;
    // 1 stream -> 256 x 64).  Several rounds matter when another kernel (an RCCL send/recv) holds a
    // few CUs: a workgroup fills its CU, so a one-round launch would then take two rounds
    // (tools/occupancy_probe.py: 8 chunks of 256 workgroups 13.4 -> 26.8 ms; 1024 per launch -> 16.3).
    const int64_t ncu = device_cus();
    int64_t nseg_want = (ncu + S - 1) / S;
    const int64_t nseg_min = (C + 1023) / 1024;
    // (rounded down: S x nseg <= 4 CUs, so stream counts that do not divide the CU count - 34, 36, 70 - never start a
    // nearly empty fifth round)
    const int64_t nseg_rounds = std::min<int64_t>(std::max<int64_t>(1, 4 * ncu / S), (C + 255) / 256);
    if (nseg_want < nseg_rounds) nseg_want = nseg_rounds;
    if (nseg_want < nseg_min) nseg_want = nseg_min;
    int64_t seg = (C + nseg_want - 1) / nseg_want;
    // shortest segment: as many columns as a segment has halo frames (2D; at least 16 / 32) - the choice below weighs halo
    // against idle CUs, and a batch that cannot fill the chip with longer segments is a LATENCY case: a workgroup walks its
    // segment frame after frame, so one stream of 4,081 columns took 0.18 ms as 64 segments of 64 (until late round 6 the
    // floor: 64 columns; 8D at N = 16384) and takes 0.08 ms as 256 segments of 16.  The small-N kernel has a short reach and
    // 4-8 frames per iteration: its floor was always low.
    const int64_t seg_min = small_n ? std::max<int64_t>(16, 4 * pl.D) : (big_n ? std::max<int64_t>(32, 2 * pl.D) : std::max<int64_t>(16, 2 * pl.D));
    seg = seg < seg_min ? seg_min : seg;
    bool shared = pl.shared == 1;
#ifdef EMSPEC_DIAG
    if (const char* ev = getenv("EMSPEC_SHARED")) shared = ev[0] == '1';   // lets one GPU exercise the plan
#endif
    if (!shared) {
        // The device is this launch's alone: nothing takes CUs away mid-launch, so the rule above (about four rounds of
        // workgroups) only buys halo.  Choose the number of rounds r = 1..4 by what it costs: the fill of the last round
        // (S x nseg workgroups over r x CUs) times the share of a workgroup's frames that are not halo (2D per segment
        // + ~3 frames of pipeline fill), fewer rounds winning ties.  64 streams x 16,369 columns: 256 workgroups of 4,096
        // columns instead of 1,024 of 1,024 (measured 9.21 vs 9.29 ms); 16 streams: 256 x 1,024 instead of 1,024 x 256.
        double best = -1.0;
        int64_t best_seg = seg;
        for (int r = 1; r <= 4; ++r) {
            int64_t ns = std::max<int64_t>(1, (int64_t)r * ncu / S);
            ns = std::min<int64_t>(ns, std::max<int64_t>(1, (C + seg_min - 1) / seg_min));   // (ceil: 16,369 columns still make 256 segments of 64)
            const int64_t sl = (C + ns - 1) / ns;
            ns = (C + sl - 1) / sl;
            const double groups = (double)S * (double)ns;
            const double rounds = std::ceil(groups / (double)ncu);
            const double eff = groups / (rounds * (double)ncu) * (double)sl / ((double)sl + 2.0 * pl.D + 3.0);
            if (eff > best * 1.002) { best = eff; best_seg = sl; }
        }
        seg = best_seg < seg_min ? seg_min : best_seg;
        if (pl.shared == 2 && seg > 1024) seg = 1024;   // two launches share the chip (emspec_batch's two-lane pipeline)
    }
#ifdef EMSPEC_DIAG
    if (const char* ev = getenv("EMSPEC_SEGLEN")) {   // tuning aid
        const long v = atol(ev);
        if (v >= 2) seg = v;
    }
#endif
    seg = (seg + 1) & ~(int64_t)1;
    // Shared device (the engine has a communicator with other ranks, so RCCL transfers and the gather's pack / expand
    // kernels take CUs while this launch runs): the last quarter of every stream is cut into quarter-length pieces and
    // the grid becomes (streams, segments), so all long segments are dispatched first - the launch ends on short
    // workgroups instead of on a mostly empty extra round (a workgroup fills its CU: losing 8 CUs turned 4 rounds into 5).
    SegPlan sp{(int)seg, 1 << 30, (int)seg, 0};
    int64_t nseg = (C + seg - 1) / seg;
    if (shared) {
        const int64_t tail = ((seg / 4) + 1) & ~(int64_t)1;
        if (tail >= seg_min && nseg >= 2) {
            const int64_t nlong = nseg - (nseg + 3) / 4;              // the last quarter (at least one segment) is cut finer
            const int64_t rest = C - nlong * seg;
            sp = SegPlan{(int)seg, (int)nlong, (int)tail, 1};
            nseg = nlong + (rest + tail - 1) / tail;
        }
    }
    if (nseg > 65535) return hipErrorInvalidValue;
    const dim3 grid = sp.short_last ? dim3((unsigned)S, (unsigned)nseg) : dim3((unsigned)nseg, (unsigned)S), block(1024);
    if (stamp_groups) *stamp_groups = nseg * S;
    const uint32_t* l32 = reinterpret_cast<const uint32_t*>(lut);
    uint32_t* r32 = reinterpret_cast<uint32_t*>(rgba);
    const bool fast = emspec_plan_is_fast(pl);   // the usual case, specialised (one basic block per-bin stage)
    auto go = [&](auto kernel, dim3 blk, size_t lds, auto... more) {
        return launch_k(kernel, grid, blk, lds, st, pl, m, l32, pcm, L, C, sp, db, r32, index, more...);
    };
    if (big_n) {
        if (stamp_groups && !stamps) return hipSuccess;            // sizing call of the diagnostic entry point
        return launch_fused16384(grid, pl, m, l32, pcm, L, C, sp, db, r32, index, st, stamps);
    }
    if (small_n) {
        if (stamps || stamp_groups) return hipErrorNotSupported;   // no stamped build of this kernel
        const int slots = fused_small_slots(n, pl.D);
        auto go_small = [&](auto kernel) {
            return launch_k(kernel, grid, block, fused_small_lds_bytes(pl.rows, slots), st, pl, m, l32, pcm, L, C, sp, slots, db, r32, index);
        };
        return pick_int<0, 1, 2>(n == 4096 ? 0 : (n == 2048 ? 1 : 2), [&](auto S_) { return pick_bool(fast, [&](auto FA) {
#ifdef EMSPEC_DIAG
            if (fused_variant() == 3) return go_small(fused_small_kernel<S_(), FA()>);   // the lock-step form (A/B)
#endif
            return go_small(fused_small_pp_kernel<S_(), FA()>);
        }); });
    }
    if (n == f13::N) {
        if (stamps || stamp_groups) return hipErrorNotSupported;   // no stamped build of this kernel
        return pick_int<512, 1024>(pl.hop, [&](auto H) { return pick_bool(fast, [&](auto FA) {
            return go(fused8192_kernel<H(), FA()>, block, fused8192_lds_bytes(pl.rows, pl.hop));
        }); });
    }
    // N = 4096 at hop 256 / 512 / 1024: a kernel family <HOP, STAMP, FAST>; name(H, ST, FA) gives the instantiation.  The
    // stamped (diagnostic) builds exist for hop 256 only, and stamp_groups alone is the sizing call of their entry point.
    auto family = [&](size_t lds, auto name) -> hipError_t {
#ifdef EMSPEC_DIAG
        if (stamps || stamp_groups) {
            if (pl.hop != 256) return hipErrorNotSupported;
            if (!stamps) return hipSuccess;
            return pick_bool(fast, [&](auto FA) { return go(name(std::integral_constant<int, 256>{}, std::true_type{}, FA), block, lds, stamps); });
        }
#endif
        return pick_int<256, 512, 1024>(pl.hop, [&](auto H) { return pick_bool(fast, [&](auto FA) {
            return go(name(H, std::false_type{}, FA), block, lds, nullptr);
        }); });
    };
#ifdef EMSPEC_DIAG
    if (fused_variant() == 2) {   // decoupled teams (A/B)
        int* ef = fused_errflag();
        if (!ef) return hipErrorOutOfMemory;
        if (stamps) return go(fused4096_r8t_kernel<true>, block, fused_r8t_lds_bytes(pl.rows), stamps, ef);
        if (stamp_groups) return hipSuccess;
        return go(fused4096_r8t_kernel<false>, block, fused_r8t_lds_bytes(pl.rows), nullptr, ef);
    }
    if (fused_variant() == 3)   // the lock-step kernel (A/B)
        return family(fused_r8_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto FA) { return fused4096_r8_kernel<H(), ST(), FA()>; });
    if (fused_variant() == 4 && fast)   // team barriers (A/B): built for fast plans only
        return family(fused_pp_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto) { return fused4096_pp3_kernel<H(), ST(), true, true>; });
    if (fused_variant() == 5)   // round 3's form of the product kernel (A/B)
        return family(fused_pp_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto FA) { return fused4096_pp3_kernel<H(), ST(), FA()>; });
    if (fused_variant() == 1) {   // 512 threads, radix 16 (A/B)
        if (stamps) return go(fused4096_kernel<true>, dim3(512), fused_lds_bytes(pl.rows), stamps);
        if (stamp_groups) return hipSuccess;
        return go(fused4096_kernel<false>, dim3(512), fused_lds_bytes(pl.rows), nullptr);
    }
#endif
    return family(fused_pp_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto FA) { return fused4096_pp_kernel<H(), ST(), FA()>; });
}

}  // namespace emspec
