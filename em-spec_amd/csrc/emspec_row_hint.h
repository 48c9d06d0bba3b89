// emspec_row_hint.h — internal: the decision of the FAST kernels' hinted row lookup (emspec_device.h: HintLookup), from the hint
// to the row.  The kernels supply the hint's logarithm (v_log_f32) and the table in LDS; everything after that is here.  No HIP,
// nothing of the engine: tests/test_row_lookup_cpu.py runs exactly this code through a stand-alone program
// (tests/cdriver/row_lookup_driver.cpp) without a GPU.  The error budget that lets one compare decide: emspec_tables.h,
// hint_rows_ok.
#pragma once

#ifndef EMSPEC_HD
#ifdef __HIPCC__
#define EMSPEC_HD __host__ __device__
#else
#define EMSPEC_HD
#endif
#endif

namespace emspec {

// The constant of the hint: f = fma(log2 k, rscale, c0) is k's position on the axis in rows, plus one half, so that its integer
// part is the NEAREST edge.  One rounding (the library is built with -ffp-contract=off: the fma is explicit).
EMSPEC_HD inline float row_hint_offset(float l2e0, float rscale) { return __builtin_fmaf(-l2e0, rscale, 0.5f); }
EMSPEC_HD inline float row_hint(float log2k, float rscale, float c0) { return __builtin_fmaf(log2k, rscale, c0); }

// Row of kh on the table eb[0 .. R] (strictly increasing) from the hint f of kh: the largest r with eb[r] <= kh, -1 when kh lies
// below eb[0] and R when it lies at or above eb[R], so `(unsigned)row < R` is the range test.  f is off by less than half a row
// (hint_rows_ok), so its integer part m is one of the two edges around kh, and ONE compare against that edge decides: one table
// read per lookup.  The clamp is done on the float: -inf (kh = 0), NaN (kh < 0 or NaN) and values past the table all land on an
// edge that exists, on the device and on a host alike (a float -> int conversion out of range is not defined on a host).  A NaN kh
// fails `kh >= eb[m]` at m = 0 and comes out as -1.
EMSPEC_HD inline int row_from_hint(float f, float kh, const float* eb, int R) {
    const int m = (int)__builtin_fminf(__builtin_fmaxf(f, 0.0f), (float)R);
    return m - (kh >= eb[m] ? 0 : 1);
}

}  // namespace emspec
