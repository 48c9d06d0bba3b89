// pipe_plan_driver.cpp — prints the plan of the host-buffer pipeline (em-spec_amd/csrc/emspec_pipe_plan.h) for a list of cases,
// as a JSON list with one object per case: the arithmetic that decides which bytes of the caller's arrays each unit writes, without a GPU.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I em-spec_amd/csrc tests/cdriver/pipe_plan_driver.cpp -o pipe_plan_driver
// tests/test_pipe_plan_cpu.py compares the output with tests/golden/pipe_plans.json.  With -DPIPE_PLAN_VERBATIM the same cases go
// through pipe_plan_verbatim.h, the arithmetic as it was before the reshaping: that build wrote the fixture.
#ifdef PIPE_PLAN_VERBATIM
#include "pipe_plan_verbatim.h"
#else
#include "emspec_pipe_plan.h"
#endif

#include <cstdio>

using namespace emspec;

namespace {

struct Case {
    int S; int64_t L; int n, hop; bool exact;
    bool whole; int min_streams;   // the unit rule: whole streams (at least min_streams per unit), else runs of columns
    int f, V, frame_bytes, k;      // time reduction; PCM views and bytes per raw frame (0: float streams); peaks per column
    bool db, rgba, idx, packed;
    int R;
};

int64_t num_columns(int64_t L, int n, int hop) { return L < n ? 0 : (L - n) / hop + 1; }
// (include/emspec.h, emspec_wire_bound: 32 + 4 C (1 + ceil(R / 32)) + C R + 32)
int64_t wire_bound(int64_t C, int R) { return 32 + C * 4 + C * (int64_t)((R + 31) / 32) * 4 + C * (int64_t)R + 32; }

// what host_batch (emspec_host.cpp: plan_pipe) works out before its first HIP call
struct Planned { size_t per_stream, bytes_out; int target; std::vector<PipeItem> items; Stage g; int64_t C; long long out_off[4]; };
Planned plan_case(const Case& c) {
    Planned p;
    const int64_t C = p.C = num_columns(c.L, c.n, c.hop), Cr = (C + c.f - 1) / c.f;
    const int fb = c.frame_bytes ? c.frame_bytes : 4, D = (c.n + 2 * c.hop - 1) / (2 * c.hop);
    const size_t in_s = (size_t)c.L * fb, wire_s = c.packed ? (size_t)wire_bound(Cr, c.R) : 0;
#ifdef PIPE_PLAN_VERBATIM
    const size_t col_cells = (size_t)C * c.R, out_cells = (size_t)Cr * c.R;
    const bool want_idx = c.idx || c.packed, stage_db = c.db || c.k;
    p.per_stream = per_stream_bytes(in_s, c.L, c.frame_bytes != 0, c.V, col_cells, out_cells, wire_s, C, c.k, c.db, stage_db, c.rgba, want_idx, c.f);
    p.bytes_out = bytes_out_estimate(c.packed, c.S, c.V, out_cells, C, c.k, c.db, c.rgba, want_idx);
#else
    // the table of what is delivered (no host arrays here: only the sizes count)
    OutRow outs[kOutRows] = {};
    outs[kDb].unit = c.db ? 4 : 0;
    outs[kRgba].unit = c.rgba ? 4 : 0;
    outs[kIdx].unit = c.idx || c.packed ? 1 : 0;
    outs[kPeaks].unit = c.k * sizeof(emspec_peak);
    p.per_stream = per_stream_bytes(outs, in_s, c.frame_bytes ? (size_t)c.L * 4 * c.V : 0, c.V, C, Cr, c.R, wire_s, c.f);
    p.bytes_out = bytes_out_estimate(outs, c.packed, (size_t)c.S * c.V, C, Cr, c.R);
#endif
    p.target = pipe_units(c.exact, c.n, (int64_t)c.S * c.V * C, (size_t)c.S * in_s, p.bytes_out);
    if (c.whole) p.target = std::min(p.target, std::max(c.S / c.min_streams, 1));
    p.items = pipe_items(c.S, c.L, C, c.n, c.hop, D, p.per_stream, !c.whole, p.target, c.f);
#ifdef PIPE_PLAN_VERBATIM
    p.g = stage_layout(p.items, c.R, stage_db, c.rgba, want_idx, wire_s, c.V, c.frame_bytes, c.f, c.k);
#else
    p.g = stage_layout(p.items, c.R, outs, wire_s, c.V, c.frame_bytes, c.f);
#endif
    // where the delivered copy of each row (dB, RGBA, index, peaks) lies in set 1 of the staging buffer, -1 without that array
    static char stage[1];
    const Set q = p.g.at(stage, 1);
    const char* at[4] = {(const char*)q.odb, (const char*)q.orgba, (const char*)q.oidx, (const char*)q.peaks};
    for (int w = 0; w < 4; ++w) {
#ifdef PIPE_PLAN_VERBATIM
        p.out_off[w] = at[w] ? (long long)(at[w] - stage) - (long long)p.g.bytes() : -1;
#else
        p.out_off[w] = at[w] ? (long long)p.g.out_off(w) : -1;
        if (at[w] && at[w] - stage != (long long)(p.g.bytes() + p.g.out_off(w))) p.out_off[w] = -2;   // Stage::at disagrees with out_off
#endif
    }
    return p;
}

void print_case(const Case& c) {
    const Planned p = plan_case(c);
    static bool first = true;
    printf("%s{\"case\": {\"S\": %d, \"L\": %lld, \"n\": %d, \"hop\": %d, \"exact\": %d, \"whole\": %d, \"min_streams\": %d, \"f\": %d, \"V\": %d, "
           "\"frame_bytes\": %d, \"k\": %d, \"db\": %d, \"rgba\": %d, \"idx\": %d, \"packed\": %d, \"R\": %d}, ",
           first ? "[\n" : ",\n", c.S, (long long)c.L, c.n, c.hop, c.exact, c.whole, c.min_streams, c.f, c.V, c.frame_bytes, c.k, c.db, c.rgba, c.idx, c.packed, c.R);
    printf("\"per_stream\": %zu, \"bytes_out\": %zu, \"target\": %d, \"units\": %zu, \"items\": [", p.per_stream, p.bytes_out, p.target, p.items.size());
    for (size_t i = 0; i < p.items.size(); ++i) {
        const PipeItem& it = p.items[i];
        printf("%s[%d, %d, %lld, %lld, %lld, %lld, %lld, %lld]", i ? ", " : "", it.s0, it.sc, (long long)it.c0, (long long)it.cn,
               (long long)it.first_sample, (long long)it.samples, (long long)it.skip, (long long)it.cols);
    }
    const Stage& g = p.g;
    printf("], \"stage\": {\"in\": %zu, \"db\": %zu, \"rgba\": %zu, \"idx\": %zu, \"wire\": %zu, \"raw\": %zu, \"rdb\": %zu, \"rrgba\": %zu, \"ridx\": %zu, "
           "\"reduced\": %d, \"peaks\": %zu, \"chunk\": %d, \"bytes\": %zu}, \"out_off\": [%lld, %lld, %lld, %lld], \"spans\": [",
           g.in, g.db, g.rgba, g.idx, g.wire, g.raw, g.rdb, g.rrgba, g.ridx, g.reduced, g.peaks, g.chunk, g.bytes(),
           p.out_off[0], p.out_off[1], p.out_off[2], p.out_off[3]);
    for (size_t i = 0; i < p.items.size(); ++i) {
        printf("%s[", i ? ", " : "");
        for (int k = 0; k < spans_of(p.items[i], p.C, c.V); ++k) {
            const Span sp = span_of(p.items[i], p.C, c.R, c.V, k, c.f);
            printf("%s[%zu, %zu, %zu]", k ? ", " : "", sp.from, sp.to, sp.cells);
        }
        printf("]");
    }
    printf("]}");
    first = false;
}

}  // namespace

int main() {
    const int shapes[4][2] = {{1024, 256}, {4096, 256}, {4096, 1000}, {16384, 512}};
    const int streams[6] = {1, 3, 8, 16, 23, 64};
    Case b{1, (int64_t)1 << 22, 4096, 256, false, false, 1, 1, 1, 0, 0, false, false, true, false, 1024};   // the bench shape, index out
    auto with = [&](auto&& edit) { Case c = b; edit(c); print_case(c); };
    // streams x lengths (one column, 2^18, 2^22, and 2^25: the length at which a stream is cut into runs of columns)
    for (int S : streams)
        for (int64_t L : {(int64_t)4096, (int64_t)1 << 18, (int64_t)1 << 22, (int64_t)1 << 25})
            with([&](Case& c) { c.S = S; c.L = L; });
    // sizes and hops, both modes
    for (auto& sh : shapes)
        for (int S : {1, 8})
            for (int64_t L : {(int64_t)sh[0], (int64_t)1 << 22, (int64_t)1 << 25})
                for (bool exact : {false, true})
                    with([&](Case& c) { c.S = S; c.L = L; c.n = sh[0]; c.hop = sh[1]; c.exact = exact; });
    // the unit rule: whole streams, and at least four of them per unit
    for (int S : streams)
        for (int ms : {1, 4})
            with([&](Case& c) { c.S = S; c.whole = true; c.min_streams = ms; c.db = true; });
    // time reduction: f beyond C, C no multiple of f, fewer than two groups per stream (not cut), runs and whole streams
    for (int f : {1, 2, 7, 65536})
        for (int S : {1, 3, 16})
            for (int64_t L : {(int64_t)1 << 18, (int64_t)1 << 22, (int64_t)1 << 25})
                for (bool whole : {false, true})
                    with([&](Case& c) { c.S = S; c.L = L; c.f = f; c.whole = whole; c.rgba = true; });
    // views of PCM sources: stereo s16 (4 bytes per frame), three channels of s24 as two views (9), mono s16 (V = 1)
    for (int f : {1, 7})
        for (int S : {1, 8})
            for (int64_t L : {(int64_t)1 << 18, (int64_t)1 << 25})
                for (int R : {1024, 500}) {
                    with([&](Case& c) { c.S = S; c.L = L; c.f = f; c.R = R; c.V = 2; c.frame_bytes = 4; c.db = true; });
                    with([&](Case& c) { c.S = S; c.L = L; c.f = f; c.R = R; c.V = 2; c.frame_bytes = 9; c.whole = true; });
                    with([&](Case& c) { c.S = S; c.L = L; c.f = f; c.R = R; c.V = 1; c.frame_bytes = 2; c.rgba = true; });
                }
    // peaks (f = 1): the dB is staged, only the lists are delivered
    for (int k : {0, 5})
        for (int S : {1, 3, 16})
            for (int64_t L : {(int64_t)1 << 22, (int64_t)1 << 25})
                for (bool whole : {false, true})
                    with([&](Case& c) { c.S = S; c.L = L; c.k = k; c.whole = whole; c.idx = k == 0; c.db = k == 0; });
    with([&](Case& c) { c.L = (int64_t)1 << 25; c.k = 5; c.idx = false; c.V = 2; c.frame_bytes = 4; c.R = 500; });
    // every subset of the outputs
    for (int m = 0; m < 8; ++m)
        for (int f : {1, 2, 7})
            for (int S : {1, 3})
                with([&](Case& c) { c.S = S; c.L = S == 1 ? (int64_t)1 << 25 : (int64_t)1 << 22; c.f = f; c.db = m & 1; c.rgba = m & 2; c.idx = m & 4; c.R = S == 1 ? 1024 : 500; });
    // packed: one wire image per stream, whole streams
    for (int f : {1, 2})
        for (int S : {1, 8, 64}) {
            with([&](Case& c) { c.S = S; c.f = f; c.whole = true; c.idx = false; c.packed = true; });
            with([&](Case& c) { c.S = S; c.f = f; c.whole = true; c.idx = false; c.packed = true; c.V = 2; c.frame_bytes = 6; c.R = 500; c.exact = true; });
        }
    // the 1 GiB staging cap: a stream that exceeds it on its own (one stream per unit), and one that lets three in where the
    // unit count asks for four
    with([&](Case& c) { c.S = 8; c.L = (int64_t)1 << 25; c.whole = true; c.db = c.rgba = true; });
    with([&](Case& c) { c.S = 64; c.L = (int64_t)1 << 23; c.whole = true; c.db = c.rgba = true; });
    with([&](Case& c) { c.S = 64; c.L = (int64_t)1 << 23; c.whole = true; c.min_streams = 4; c.db = c.rgba = true; c.f = 2; });
    printf("\n]\n");
    return 0;
}
