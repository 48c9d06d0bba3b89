// fused.hip.inc — launcher of the fused batch kernels (LDS column ring).  Included by kernels.hip.
//
// Kernels (each in its own .inc):
//   fused4096_pp_kernel<HOP>   N = 4096, hop 256/512/1024 — the headline path: two teams half an iteration apart (fused_pp.hip.inc;
//                              fused_r8.hip.inc holds its helpers and the lock-step form, a diagnostic A/B variant since round 3)
//   fused8192_kernel<HOP>      N = 8192, hop 512/1024                                  (fused_n8192.hip.inc)
//   fused_small_pp_kernel<S>   N = 4096/2048/1024 at any hop whose ring fits in LDS    (fused_small.hip.inc; same schedule)
//   fused16384_kernel          N = 16384 (ring parked in registers while the FFT owns LDS) (fused_n16384.hip.inc)
// Diagnostic builds (-DEMSPEC_DIAG -> libemspec_diag.so) add the stamped builds and the
// A/B variants r8 (lock step) / pp3, ppt (round 3's schedule) / pp4 (stores at the end of each FFT pass) / r16 / r8t (diag/*.inc),
// selectable with EMSPEC_FUSED_VARIANT;
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
#include "diag/fused_pp4.hip.inc"
#endif
namespace emspec {

#ifdef EMSPEC_DIAG
// 0 = the product kernel: 1024 threads, radix 8, the two teams half an iteration apart (default),
// 1 = 512-thread radix-16 variant ("r16"), 2 = 1024-thread radix-8 with decoupled teams ("r8t"),
// 3 = the lock-step form of the product kernel ("r8": the default until round 3),
// 4 = round 3's form of the product kernel (spectrum reads at the start of role 1) with per-team software barriers
//     instead of the workgroup barrier ("ppt"), 5 = that form as it was the product in rounds 3-4 ("pp3"),
// 6 = the product kernel with every FFT pass's stores behind the whole pass, as it was until the stores went pair by pair ("pp4")
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
        if (e && e[0] == 'p' && e[1] == 'p' && e[2] == '4') v = 6;
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
static int64_t diag_seglen() { const char* e = getenv("EMSPEC_SEGLEN"); return e ? atol(e) : 0; }   // tuning aid: a segment length (>= 2)
#else
static constexpr int fused_variant() { return 0; }
static constexpr bool diag_no_fused() { return false; }
static constexpr int64_t diag_seglen() { return 0; }
#endif

// (the specialised FAST kernels serve the plans of emspec_plan_is_fast, emspec_device.h: reassignment ON, log-spaced rows, and
// a power floor that keeps every accumulated bin's 64 P inside the range of recip_normal)

// the kernel family that serves the shape with this build's switches, or the records path (emspec_kernel_plan.h: fast_route)
Route fused_route(int n, int hop, int rows, int reassign) { return fast_route(n, hop, rows, reassign, FastSwitches{diag_no_fused(), fused_variant()}); }
bool fused_supported(int n, int hop, int rows, int reassign) { return !is_records(fused_route(n, hop, rows, reassign)); }

hipError_t launch_fused(int n, const PlanDev& pl, const DbMap& m, const uint8_t* lut, const float* pcm, int64_t L,
                        int S, int64_t C, float* db, uint8_t* rgba, uint8_t* index, hipStream_t st,
                        unsigned long long* stamps, int64_t* stamp_groups) {
    const RouteKind kind = fused_route(n, pl.hop, pl.rows, pl.reassign).kind;
    if (kind == RouteKind::records_f32 || !fused_reach_ok(kind, n, pl.hop, pl.D)) return hipErrorNotSupported;
    if (S <= 0 || C <= 0) return hipSuccess;
    if (S > 65535) return hipErrorInvalidValue;
#ifndef EMSPEC_DIAG
    if (stamps || stamp_groups) return hipErrorNotSupported;   // stamped builds live in libemspec_diag.so only
#endif
    // the segment plan (the four-round rule, the exclusive-device choice, the shared-device tail cut): emspec_seg_plan.h
    int force_shared = -1;
#ifdef EMSPEC_DIAG
    if (const char* ev = getenv("EMSPEC_SHARED")) force_shared = ev[0] == '1';   // lets one GPU exercise the plan
#endif
    const FusedSegPlan fp = fused_seg_plan(device_cus(), S, C, pl.D, fused_kind(kind), pl.shared, force_shared, diag_seglen());
    if (!fp.ok) return hipErrorInvalidValue;
    const SegPlan sp = fp.sp;
    const int64_t nseg = fp.nseg;
    const dim3 grid = fp.streams_first ? dim3((unsigned)S, (unsigned)nseg) : dim3((unsigned)nseg, (unsigned)S), block(1024);
    if (stamp_groups) *stamp_groups = nseg * S;
    const uint32_t* l32 = reinterpret_cast<const uint32_t*>(lut);
    uint32_t* r32 = reinterpret_cast<uint32_t*>(rgba);
    const bool fast = emspec_plan_is_fast(pl);   // the usual case, specialised (one basic block per-bin stage)
    auto go = [&](auto kernel, dim3 blk, size_t lds, auto... more) {
        return launch_k(kernel, grid, blk, lds, st, pl, m, l32, pcm, L, C, sp, db, r32, index, more...);
    };
    switch (kind) {
    case RouteKind::fused_16384:
        if (stamp_groups && !stamps) return hipSuccess;            // sizing call of the diagnostic entry point
        return launch_fused16384(grid, pl, m, l32, pcm, L, C, sp, db, r32, index, st, stamps);
    case RouteKind::fused_small: {
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
    case RouteKind::fused_8192:
        if (stamps || stamp_groups) return hipErrorNotSupported;   // no stamped build of this kernel
        return pick_int<512, 1024>(pl.hop, [&](auto H) { return pick_bool(fast, [&](auto FA) {
            return go(fused8192_kernel<H(), FA()>, block, fused8192_lds_bytes(pl.rows, pl.hop));
        }); });
    default: break;   // fused_pp, below
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
    if (fused_variant() == 6)   // the product kernel before store-as-you-go passes (A/B)
        return family(fused_pp_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto FA) { return fused4096_pp4_kernel<H(), ST(), FA()>; });
    if (fused_variant() == 1) {   // 512 threads, radix 16 (A/B)
        if (stamps) return go(fused4096_kernel<true>, dim3(512), fused_lds_bytes(pl.rows), stamps);
        if (stamp_groups) return hipSuccess;
        return go(fused4096_kernel<false>, dim3(512), fused_lds_bytes(pl.rows), nullptr);
    }
#endif
    return family(fused_pp_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto FA) { return fused4096_pp_kernel<H(), ST(), FA()>; });
}

}  // namespace emspec
