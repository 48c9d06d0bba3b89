// band_plan_driver.cpp — prints, for a list of cases, what the multi-band batch accepts and how it lays out its workspace
// (em-spec_amd/csrc/emspec_band_plan.h), as a JSON list with one object per case: the rule a shape breaks or its shifts, row ranges
// and plane offsets, without a GPU.  With the argument "two": the two-band rules (multires_shape_error, multires_split_error) beside
// the K = 2 answers of the multi-band ones over a grid of shapes and every split row, one object per shape.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc
//       tests/cdriver/band_plan_driver.cpp -o band_plan_driver
// tests/test_band_plan_cpu.py checks the output against a numpy restatement of the rules.
#include "emspec_band_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace emspec;

namespace {

bool g_first = true;

void list(const char* key, const std::vector<long long>& v, const char* tail) {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? ", " : "", v[i]);
    printf("]%s", tail);
}

// L samples per stream, `chunk` streams per workspace, post: the display post-process is on
void run_case(std::vector<int32_t> n, int hop, std::vector<int32_t> split, int rows, long long L, int chunk, int post) {
    printf("%s{", g_first ? "[\n" : ",\n");
    g_first = false;
    const int K = (int)n.size();
    list("n", std::vector<long long>(n.begin(), n.end()), ", ");
    list("split", std::vector<long long>(split.begin(), split.end()), ", ");
    printf("\"hop\": %d, \"rows\": %d, \"L\": %lld, \"chunk\": %d, \"post\": %d, ", hop, rows, L, chunk, post);
    // (the entry points hand the arrays over as they come: K - 1 splits are read only once K is known to be in range)
    const char* why = band_shape_error(K, n.data(), hop);
    const char* stage = "shape";
    if (!why && (int)split.size() != K - 1) { why = "driver: need bands - 1 splits"; stage = "driver"; }
    if (!why) { why = band_split_error(K, split.data(), rows); stage = "split"; }
    if (why) {
        printf("\"error\": \"%s\", \"stage\": \"%s\"}", why, stage);
        return;
    }
    const BandPlan p = band_plan(K, n.data(), split.data(), hop, rows);
    const long long C = L >= n[0] ? (L - n[0]) / hop + 1 : 0;
    const BandLayout w = band_layout(p, C, rows, post != 0);
    std::vector<long long> shift, lo, hi, plane, off;
    for (int k = 0; k < K; ++k) {
        shift.push_back(p.shift[k]), lo.push_back(p.lo[k]), hi.push_back(p.hi[k]);
        plane.push_back((long long)w.plane[k]), off.push_back((long long)w.chunk_offset(k, chunk));
    }
    printf("\"error\": null, \"columns\": %lld, ", C);
    list("shift", shift, ", "), list("lo", lo, ", "), list("hi", hi, ", "), list("plane", plane, ", "), list("offset", off, ", ");
    printf("\"raw_plane\": %lld, \"raw_offset\": %lld, \"per_stream\": %lld, \"chunk_bytes\": %lld, \"pad\": %lld}", (long long)w.plane[K],
           (long long)w.chunk_offset(K, chunk), (long long)w.per_stream, (long long)w.chunk_bytes(chunk), (long long)kBandPad);
}

void text(const char* s) { s ? printf("\"%s\"", s) : printf("null"); }

// What the two-band entries hand to band_plan after their own rules.  Per shape: both shape answers; when the two-band rules take the
// shape, per (rows, split) "cells": [rows, split, two-band answer, multi-band answer] and, where the two-band rule takes the split,
// behind them shift[0], shift[1], lo[0], hi[0], lo[1], hi[1] and band_layout's per_stream without / with the raw plane at C columns.
void two_band_sweep() {
    const int sizes[] = {1024, 2048, 4096, 8192, 16384}, hops[] = {1, 64, 128, 256, 512, 1024, 4096, 4097};
    const int row_counts[] = {128, 256, 1024, 1000};
    const long long C = 373;
    printf("{\"C\": %lld, \"shapes\": [", C);
    bool first_shape = true;
    for (int n_low : sizes)
        for (int n_high : sizes)
            for (int hop : hops) {
                const int32_t n[2] = {n_low, n_high};
                const char* two = multires_shape_error(n_low, n_high, hop);
                printf("%s\n{\"n_low\": %d, \"n_high\": %d, \"hop\": %d, \"two\": ", first_shape ? "" : ",", n_low, n_high, hop);
                first_shape = false;
                text(two), printf(", \"band\": "), text(band_shape_error(2, n, hop)), printf(", \"cells\": [");
                bool first = true;
                for (int rows : row_counts) {
                    if (two) break;
                    std::vector<int32_t> splits;
                    for (int s = 0; s <= rows; s += 4) splits.push_back(s);
                    for (int s : {-4, 1, 62, 66, 367, rows - 62, rows - 1, rows + 4}) splits.push_back(s);
                    for (int32_t split : splits) {
                        const char* why = multires_split_error(split, rows);
                        printf("%s[%d, %d, ", first ? "" : ", ", rows, split);
                        first = false;
                        text(why), printf(", "), text(band_split_error(2, &split, rows));
                        if (!why) {
                            const BandPlan p = band_plan(2, n, &split, hop, rows);
                            printf(", %d, %d, %d, %d, %d, %d, %lld, %lld", p.shift[0], p.shift[1], p.lo[0], p.hi[0], p.lo[1], p.hi[1],
                                   (long long)band_layout(p, C, rows, false).per_stream, (long long)band_layout(p, C, rows, true).per_stream);
                        }
                        printf("]");
                    }
                }
                printf("]}");
            }
    printf("\n]}\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "two")) return two_band_sweep(), 0;
    const long long L = 1 << 17;
    // ---- accepted ----
    for (int post = 0; post < 2; ++post)
        for (int chunk : {1, 3, 64}) {
            run_case({16384, 4096, 1024}, 256, {368, 668}, 1024, L, chunk, post);
            run_case({16384, 8192, 4096, 2048}, 128, {260, 468, 668}, 1024, L, chunk, post);
            run_case({8192, 2048, 1024}, 512, {368, 668}, 1024, L, chunk, post);
            run_case({16384, 4096}, 256, {368}, 1024, L, chunk, post);
            run_case({8192, 2048}, 128, {368}, 1024, L, chunk, post);
        }
    run_case({16384, 4096, 1024}, 256, {612, 828}, 1024, L, 2, 1);             // the warped axis's rows
    run_case({16384, 8192, 4096, 2048}, 128, {516, 692, 828}, 1024, L, 2, 0);
    run_case({4096, 2048, 1024}, 512, {64, 128}, 256, 4096, 1, 0);             // the smallest bands, one column
    run_case({4096, 2048}, 1024, {64}, 256, 8192, 1, 0);                       // hop = n[K-1]
    run_case({16384, 4096, 1024}, 256, {64, 960}, 1024, 16383, 1, 1);          // L < n[0]: no column (the entry points refuse it)
    run_case({16384, 1024}, 1, {500}, 1024, L, 1, 0);                          // hop 1: the largest shift
    run_case({2048, 1024}, 512, {64}, 128, 1 << 22, 7, 1);
    // ---- rejected: each rule ----
    run_case({16384}, 256, {}, 1024, L, 1, 0);                                            // K = 1
    run_case({16384, 8192, 4096, 2048, 1024}, 128, {200, 400, 600, 800}, 1024, L, 1, 0);  // K = 5
    run_case({4096, 16384, 1024}, 256, {368, 668}, 1024, L, 1, 0);                        // sizes not decreasing
    run_case({16384, 4096, 4096}, 256, {368, 668}, 1024, L, 1, 0);                        // ... not strictly
    run_case({16384, 4096, 512}, 256, {368, 668}, 1024, L, 1, 0);                         // a size of 512
    run_case({32768, 4096, 1024}, 256, {368, 668}, 1024, L, 1, 0);                        // a size of 32768
    run_case({16384, 4096, 2048}, 1000, {368, 668}, 1024, L, 1, 0);                       // a shift that is no integer
    run_case({16384, 4096, 1024}, 2048, {368, 668}, 1024, L, 1, 0);                       // hop above n[K-1]
    run_case({16384, 4096, 1024}, 0, {368, 668}, 1024, L, 1, 0);                          // hop 0
    run_case({16384, 4096, 1024}, 256, {366, 668}, 1024, L, 1, 0);                        // a split not a multiple of 4
    run_case({16384, 4096, 1024}, 256, {368, 428}, 1024, L, 1, 0);                        // a band 60 rows high: the middle one
    run_case({16384, 4096, 1024}, 256, {60, 668}, 1024, L, 1, 0);                         // ... the first
    run_case({16384, 4096, 1024}, 256, {368, 964}, 1024, L, 1, 0);                        // ... the last
    run_case({16384, 4096, 1024}, 256, {668, 368}, 1024, L, 1, 0);                        // splits not increasing
    run_case({16384, 4096, 1024}, 256, {368, 368}, 1024, L, 1, 0);                        // ... not strictly
    printf("\n]\n");
    return 0;
}
