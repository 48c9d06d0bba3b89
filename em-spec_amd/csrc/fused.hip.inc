// fused.hip.inc — launcher of the fused batch kernels (LDS column ring).  Included by kernels.hip.
//
// Kernels (each in its own .inc):
//   fused4096_pp_kernel<HOP>   N = 4096, hop 256/512/1024 — the headline path: two teams half an iteration apart (fused_pp.hip.inc;
//                              fused_r8.hip.inc holds the helpers all four kernels share, namespace f8)
//   fused8192_kernel<HOP>      N = 8192, hop 512/1024                                  (fused_n8192.hip.inc)
//   fused_small_pp_kernel<S>   N = 4096/2048/1024 at any hop whose ring fits in LDS    (fused_small.hip.inc; same schedule)
//   fused16384_kernel          N = 16384 (ring parked in registers while the FFT owns LDS) (fused_n16384.hip.inc)
// Diagnostic builds (-DEMSPEC_DIAG -> libemspec_diag.so) add the stamped builds and the one A/B form pp4 (the product kernel
// with the stores at the end of each FFT pass, diag/fused_pp4.hip.inc), selected with EMSPEC_FUSED_VARIANT=pp4;
// none of that is in libemspec.so.  (The earlier A/B forms r16, r8t, r8, pp3 and ppt: docs/HISTORY.md "Retired kernel forms".)
#include "fused_r8.hip.inc"
#include "fused_n8192.hip.inc"
#include "fused_small.hip.inc"
#include "fused_n16384.hip.inc"
#include "fused_pp.hip.inc"
#ifdef EMSPEC_DIAG
#include "diag/fused_pp4.hip.inc"
#endif
namespace emspec {

#ifdef EMSPEC_DIAG
// EMSPEC_FUSED_VARIANT=pp4: the product kernel with every FFT pass's stores behind the whole pass, as it was until the stores
// went pair by pair (A/B).  Consulted only where the fused_pp kernel is picked: the route does not depend on it.
static bool diag_pp4() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("EMSPEC_FUSED_VARIANT"); v = (e && e[0] == 'p' && e[1] == 'p' && e[2] == '4') ? 1 : 0; }
    return v != 0;
}
static bool diag_no_fused() {
    static int off = -1;
    if (off < 0) { const char* e = getenv("EMSPEC_NO_FUSED"); off = (e && e[0] == '1') ? 1 : 0; }   // A/B aid
    return off != 0;
}
static int64_t diag_seglen() { const char* e = getenv("EMSPEC_SEGLEN"); return e ? atol(e) : 0; }   // tuning aid: a segment length (>= 2)
#else
static constexpr bool diag_no_fused() { return false; }
static constexpr int64_t diag_seglen() { return 0; }
#endif

// (the specialised FAST kernels serve the plans of emspec_plan_is_fast, emspec_device.h: reassignment ON, log-spaced rows, and
// a power floor that keeps every accumulated bin's 64 P inside the range of recip_normal)

// the kernel family that serves the shape with this build's switches, or the records path (emspec_kernel_plan.h: fast_route)
Route fused_route(int n, int hop, int rows, int reassign) { return fast_route(n, hop, rows, reassign, FastSwitches{diag_no_fused()}); }
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
    // SegPlan holds ints, and the N = 4096 kernel counts its walk in int (emspec_seg_plan.h: fused_pp_walk_ok)
    if (fused_seglen_max(C, pl.D, fused_kind(kind), diag_seglen()) > 0x7fffffff) return hipErrorInvalidValue;
    if (kind == RouteKind::fused_pp && !fused_pp_walk_ok(fp.sp.seglen, pl.D, pl.hop)) return hipErrorInvalidValue;
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
    if (diag_pp4())   // the product kernel before store-as-you-go passes (A/B)
        return family(fused_pp_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto FA) { return fused4096_pp4_kernel<H(), ST(), FA()>; });
#endif
    return family(fused_pp_lds_bytes(pl.rows, pl.hop), [](auto H, auto ST, auto FA) { return fused4096_pp_kernel<H(), ST(), FA()>; });
}

}  // namespace emspec
