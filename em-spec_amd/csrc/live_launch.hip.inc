// live_launch.hip.inc — the live multi-stream calls' kernels that are not frame kernels (flush, display post-process) and
// their launchers.  Device helpers: live.hip.inc.  Included last by kernels.hip (needs ex::exact_cell).
namespace emspec {

// Finalise columns outside the frame kernel, one workgroup per (column, stream): emspec_columns_flush (no new frame; stream s
// emits streams[s].flush of its pending columns, 0: none) and the deferred finalize of a launch that completed many columns
// per stream (streams[s].frames of them; the kernel boundary orders the frame kernel's scatter before it).
template <class CELL, class CONV>
__global__ __launch_bounds__(256) void live_finalize_kernel(LiveSinks lv, CELL* cells, int slots, int rows, int D, CONV conv) {
    const int s = (int)blockIdx.y, i = (int)blockIdx.x;
    const LiveStream d = lv.uniform ? lv.uni : lv.streams[s];
    if (i >= (d.flush ? d.flush : d.frames)) return;
    live_finalize_column<CELL>(lv, d, s, i, cells, slots, rows, D, 256, conv);
}

hipError_t launch_live_flush(bool exact, const LiveSinks& lv, void* cells, int slots, int rows, int D, const DbMap& m,
                             const ExactDbMap& xm, int S, int ncol, hipStream_t st) {
    if (S <= 0 || ncol <= 0) return hipSuccess;
    const dim3 grid((unsigned)ncol, (unsigned)S);
    if (exact)
        hipLaunchKernelGGL((live_finalize_kernel<unsigned long long, ex::LiveConvExact>), grid, dim3(256), 0, st, lv,
                           reinterpret_cast<unsigned long long*>(cells), slots, rows, D, ex::LiveConvExact{xm});
    else
        hipLaunchKernelGGL((live_finalize_kernel<float, LiveConvF32>), grid, dim3(256), 0, st, lv,
                           reinterpret_cast<float*>(cells), slots, rows, D, LiveConvF32{m});
    return hipGetLastError();
}

// Finalise every band's rows of a column in one launch (a live multi-band session, DESIGN.md §3.13; emspec_live_plan.h): grid
// (columns, S) as above, and workgroup (i, s) runs one live_finalize_column per band - that band's ring, slots, rows, first row and
// conversion, all in the kernel arguments - so a column of K bands costs one launch, not K.  It serves the session's flush and
// its deferred finalize; as for live_finalize_kernel, the kernel boundary behind the bands' frame launches on the one stream
// orders their scatter before these loads.  Bands own disjoint rows of the output column and rings of their own: nothing is
// shared between the K passes of a workgroup.
template <class CELL, class CONV>
struct LiveBandFin {
    CELL* cells;             // [S][slots][rows]
    int slots, rows, row0;   // the band fills rows [row0, row0 + rows) of the output column
    CONV conv;
};
template <class CELL, class CONV>
struct LiveBandsFin {
    int bands;
    LiveBandFin<CELL, CONV> b[kMaxBands];
};
template <class CELL, class CONV>
__global__ __launch_bounds__(256) void live_finalize_bands_kernel(LiveSinks lv, LiveBandsFin<CELL, CONV> f, int D) {
    const int s = (int)blockIdx.y, i = (int)blockIdx.x;
    const LiveStream d = lv.uniform ? lv.uni : lv.streams[s];
    if (i >= (d.flush ? d.flush : d.frames)) return;
#pragma unroll
    for (int k = 0; k < kMaxBands; ++k) {
        if (k >= f.bands) break;
        lv.row0 = f.b[k].row0;
        live_finalize_column<CELL>(lv, d, s, i, f.b[k].cells, f.b[k].slots, f.b[k].rows, D, 256, f.b[k].conv);
    }
}

hipError_t launch_live_finalize_bands(bool exact, const LiveSinks& lv, const LiveBandRings& r, int D, int S, int ncol, hipStream_t st) {
    if (S <= 0 || ncol <= 0 || r.bands <= 0) return hipSuccess;
    if (r.bands > kMaxBands) return hipErrorInvalidValue;
    const dim3 grid((unsigned)ncol, (unsigned)S);
    if (exact) {
        LiveBandsFin<unsigned long long, ex::LiveConvExact> f{};
        f.bands = r.bands;
        for (int k = 0; k < r.bands; ++k)
            f.b[k] = {reinterpret_cast<unsigned long long*>(r.cells[k]), r.slots[k], r.rows[k], r.row0[k], ex::LiveConvExact{r.xm[k]}};
        hipLaunchKernelGGL((live_finalize_bands_kernel<unsigned long long, ex::LiveConvExact>), grid, dim3(256), 0, st, lv, f, D);
    } else {
        LiveBandsFin<float, LiveConvF32> f{};
        f.bands = r.bands;
        for (int k = 0; k < r.bands; ++k)
            f.b[k] = {reinterpret_cast<float*>(r.cells[k]), r.slots[k], r.rows[k], r.row0[k], LiveConvF32{r.m[k]}};
        hipLaunchKernelGGL((live_finalize_bands_kernel<float, LiveConvF32>), grid, dim3(256), 0, st, lv, f, D);
    }
    return hipGetLastError();
}

// Display post-process of a live launch (DESIGN.md §3.6; post.hip.inc's laws, state per stream): the frame kernels wrote the
// RAW dB columns to raw[S][raw_cols][rows] (device memory, same slots as the outputs, its own stride); this turns each stream's columns, in
// time order, into the caller's out_db / out_rgba.  The empty columns of the per-frame form pass through unprocessed, as in
// emspec_column.
__global__ __launch_bounds__(256) void live_post_kernel(LiveSinks lv, const float* __restrict__ raw, int raw_cols, int rows, int D,
                                                        float sm, float agc, float db_top, DbMap dm, float* __restrict__ pstate) {
    __shared__ float red[4];
    const int s = (int)blockIdx.x;
    const LiveStream d = lv.uniform ? lv.uni : lv.streams[s];
    const int ncol = d.flush ? d.flush : d.frames;
    float* state = pstate + (size_t)s * (size_t)(rows + 4);
    int oc = d.out_at;
    for (int i = 0; i < ncol; ++i) {
        const long long c = d.j0 - D + i;
        if (c < 0 && !lv.empty_col) continue;
        const size_t at = ((size_t)s * (size_t)lv.out_cols + (size_t)oc) * (size_t)rows;
        const size_t rat = ((size_t)s * (size_t)raw_cols + (size_t)oc) * (size_t)rows;   // (the raw block has its own stride)
        ++oc;
        float* odb = lv.out_db ? lv.out_db + at : nullptr;
        uint32_t* orgba = lv.out_rgba ? lv.out_rgba + at : nullptr;
        if (c < 0) {
            for (int r = (int)threadIdx.x; r < rows; r += 256) {
                const float x = raw[rat + r];
                if (odb) odb[r] = x;
                if (orgba) orgba[r] = lv.lut[cell_index(dm, x)];
            }
            continue;
        }
        post_column_body(raw + rat, odb, orgba, rows, sm, agc, db_top, dm, lv.lut, state, state + 4, red);
    }
}

hipError_t launch_live_post(const LiveSinks& lv, const float* raw, int raw_cols, int rows, int D, float sm, float agc, float db_top,
                            const DbMap& dm, float* pstate, int S, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    hipLaunchKernelGGL(live_post_kernel, dim3((unsigned)S), dim3(256), 0, st, lv, raw, raw_cols, rows, D, sm, agc, db_top, dm, pstate);
    return hipGetLastError();
}

}  // namespace emspec
