// wave_plan_driver.cpp — checks the envelope's part of the host pipeline's plan (em-spec_amd/csrc/emspec_pipe_plan.h: the kWave
// row, wave_run_of, wave_span_of) without a GPU: for a grid of streams, views, lengths, factors and forced unit counts, the
// pieces of all units cover the caller's [S * V][Cr] pairs exactly once, every piece comes from inside the unit's pair array
// in its staging set, the kernel's windows lie inside the unit's staged samples and are the stream's own windows, and a job
// without an envelope has the layout it had.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I em-spec_amd/csrc tests/cdriver/wave_plan_driver.cpp -o wave_plan_driver
// Prints "ok <cases> <units>" and returns 0, or prints the first violation and returns 1 (tests/test_wave_cpu.py).
#include "emspec_pipe_plan.h"

#include <cstdio>

using namespace emspec;

namespace {

long long cases = 0, units_seen = 0, run_units = 0;

#define CHECK(cond, what)                                                                                                     \
    do {                                                                                                                      \
        if (!(cond)) {                                                                                                        \
            printf("FAIL %s: S=%d V=%d L=%lld n=%d hop=%d f=%d target=%d whole=%d unit=%d\n", what, S, V, (long long)L, n, hop, f, target, \
                   (int)whole, u);                                                                                            \
            return false;                                                                                                     \
        }                                                                                                                     \
    } while (0)

bool check(int S, int V, int64_t L, int n, int hop, int f, int target, bool whole, bool idx) {
    int u = -1;
    const int R = 64, D = (n + 2 * hop - 1) / (2 * hop);
    const int64_t C = L < n ? 0 : (L - n) / hop + 1, Cr = (C + f - 1) / f, off = n / 2 - hop / 2;
    OutRow outs[kOutRows] = {}, plain[kOutRows] = {};
    outs[kIdx].unit = plain[kIdx].unit = idx ? 1 : 0;
    outs[kDb].unit = plain[kDb].unit = idx ? 0 : 4;
    outs[kWave].unit = sizeof(emspec_wave);
    const size_t in_s = (size_t)L * 4;
    const size_t per_stream = per_stream_bytes(outs, in_s, V > 1 ? in_s * V : 0, V, C, Cr, R, 0, f);
    const std::vector<PipeItem> items = pipe_items(S, L, C, n, hop, D, per_stream, !whole, target, f);
    const Stage g = stage_layout(items, R, outs, 0, V, V > 1 ? 4 : 0, f), g0 = stage_layout(items, R, plain, 0, V, V > 1 ? 4 : 0, f);
    // the row is the last array of a set: without it every offset and the size are what they were
    for (int a = 0; a <= 10; ++a) CHECK(g.off(a) == g0.off(a), "an offset in front of the envelope moved");
    CHECK(g0.wave == 0 && g0.bytes() == g0.off(10) && g.bytes() == g0.bytes() + g.wave, "layout without the envelope");
    CHECK(g.out_off(kWave) == g0.bytes() && g.out_off(kWave) % 8 == 0, "the pair array's offset");
    static char stage[1];
    CHECK((char*)g.at(stage, 2).wave == stage + 2 * g.bytes() + g.out_off(kWave) && g0.at(stage, 2).wave == nullptr, "Stage::at");
    std::vector<int> hit((size_t)S * V * Cr, 0);
    for (u = 0; u < (int)items.size(); ++u) {
        const PipeItem& it = items[u];
        const WaveRun wr = wave_run_of(it, n, hop, f);
        // the kernel's windows: inside the staged samples, and the stream's own (a run starts on a multiple of f)
        CHECK(it.c0 % f == 0, "a run does not start on a multiple of f");
        CHECK(wr.first >= 0 && wr.first + wr.cols * hop <= it.samples, "windows outside the staged samples");
        CHECK(it.first_sample + wr.first == it.c0 * hop + off, "the first window is not the stream's");
        CHECK(wr.cols == it.cn && wr.pairs == (it.cn + f - 1) / f, "pairs of the unit");
        CHECK((size_t)wr.pairs * it.sc * V * sizeof(emspec_wave) <= g.wave, "the unit's pairs do not fit the set's array");
        if (it.cn != C) ++run_units;
        for (int k = 0; k < spans_of(it, C, V); ++k) {
            const Span ws = wave_span_of(it, C, V, k, f);
            CHECK(ws.from + ws.cells <= (size_t)wr.pairs * it.sc * V, "a piece from outside the unit's pair array");
            CHECK(ws.to + ws.cells <= hit.size(), "a piece beyond the caller's array");
            // pair i of the piece is pair (ws.from + i) of the unit = stream ws.from / pairs of the unit, group (ws.from + i) % pairs
            for (size_t i = 0; i < ws.cells; ++i) {
                const size_t us = (ws.from + i) / (size_t)wr.pairs, ug = (ws.from + i) % (size_t)wr.pairs;
                CHECK(ws.to + i == ((size_t)it.s0 * V + us) * Cr + (size_t)(it.c0 / f) + ug, "a pair goes to another stream or group");
                ++hit[ws.to + i];
            }
            // the cells' spans and the pairs' agree: the same delivered columns
            const Span sp = span_of(it, C, R, V, k, f);
            CHECK(sp.to == ws.to * R && sp.cells == ws.cells * R, "the pairs' span is not the cells'");
        }
    }
    u = -1;
    for (int h : hit) CHECK(h == 1, "a pair of the caller's array is not written exactly once");
    ++cases;
    units_seen += (long long)items.size();
    return true;
}

}  // namespace

int main() {
    const int shapes[5][2] = {{256, 1}, {1024, 255}, {4096, 256}, {4096, 4096}, {16384, 512}};
    for (auto& sh : shapes)
        for (int S : {1, 3, 8})
            for (int V : {1, 4})
                for (int64_t extra : {(int64_t)0, (int64_t)1, (int64_t)7 * sh[1] + 5, (int64_t)70001 * sh[1] + 3})
                    for (int f : {1, 2, 7, 4096, 65536})
                        for (int target : {1, 2, 3, 16})
                            for (bool whole : {false, true}) {
                                const int n = sh[0], hop = sh[1];
                                if (extra > 4000000 && S * V > 8) continue;   // (keeps the hit map small)
                                if (!check(S, V, n + extra, n, hop, f, target, whole, (S + f) % 2 == 0)) return 1;
                            }
    if (run_units == 0) { printf("FAIL no case was cut into runs of columns\n"); return 1; }
    printf("ok %lld %lld %lld\n", cases, units_seen, run_units);
    return 0;
}
