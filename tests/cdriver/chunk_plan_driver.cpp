// chunk_plan_driver.cpp — answers, one JSON object per input line, what the HIP-free headers say about the stream-chunked engine
// workspaces (em-spec_amd/csrc/emspec_kernel_plan.h, emspec_band_plan.h): the record bytes per stream, the chunk rule and its
// halvings, the second array's offset, the multi-band layout.  Without a GPU.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc
//       tests/cdriver/chunk_plan_driver.cpp -o chunk_plan_driver
// Input lines (whitespace-separated integers behind the word):
//   f32    n C                                     -> per_stream
//   exact  n C                                     -> q, key, per_stream
//   chunk  free have per_stream extra cap S budget -> chunk, bytes, halvings [[chunk, bytes] ...]   (budget < 0: none set)
//   second first_per_stream chunk                  -> offset
//   band   K n[K] split[K-1] hop rows C post chunk -> planes, offsets, per_stream, chunk_bytes
//   pads                                           -> chunk_pad, band_pad, max_bands
// tests/test_chunk_ref_cpu.py checks the output against the restatement in tests/chunk_ref.py.
#include "emspec_band_plan.h"
#include "emspec_kernel_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace emspec;

namespace {

void list(const char* key, const std::vector<long long>& v, const char* tail) {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? ", " : "", v[i]);
    printf("]%s", tail);
}

bool run_line(const std::string& line) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) return true;   // an empty line
    std::vector<long long> a;
    for (long long v; in >> v;) a.push_back(v);
    printf("{\"kind\": \"%s\", ", kind.c_str());
    list("args", a, ", ");
    if (kind == "f32" && a.size() == 2) {
        printf("\"per_stream\": %lld}\n", (long long)f32_record_bytes((int)a[0], a[1]));
    } else if (kind == "exact" && a.size() == 2) {
        const ExactRecords r = exact_record_bytes((int)a[0], a[1]);
        printf("\"q\": %lld, \"key\": %lld, \"per_stream\": %lld}\n", (long long)r.q_per_stream, (long long)r.key_per_stream, (long long)r.per_stream);
    } else if (kind == "chunk" && a.size() == 7) {
        const size_t per = (size_t)a[2], extra = (size_t)a[3];
        ChunkPlan p = first_chunk((size_t)a[0], (size_t)a[1], per, extra, (size_t)a[4], (int)a[5], a[6]);
        printf("\"chunk\": %d, \"bytes\": %lld, \"halvings\": [", p.chunk, (long long)p.bytes);
        for (bool first = true; p.chunk > 1; first = false) {
            p = next_chunk(p, per, extra);
            printf("%s[%d, %lld]", first ? "" : ", ", p.chunk, (long long)p.bytes);
        }
        printf("]}\n");
    } else if (kind == "second" && a.size() == 2) {
        printf("\"offset\": %lld}\n", (long long)second_array_offset((size_t)a[0], (int)a[1]));
    } else if (kind == "band" && !a.empty() && a[0] >= 2 && a[0] <= kMaxBands && (long long)a.size() == 2 * a[0] + 5) {
        const int K = (int)a[0];
        std::vector<int32_t> n(a.begin() + 1, a.begin() + 1 + K), split(a.begin() + 1 + K, a.begin() + 2 * K);
        const int hop = (int)a[2 * K], rows = (int)a[2 * K + 1], post = (int)a[2 * K + 3], chunk = (int)a[2 * K + 4];
        const long long C = a[2 * K + 2];
        if (band_shape_error(K, n.data(), hop) || band_split_error(K, split.data(), rows)) { printf("\"error\": 1}\n"); return true; }
        const BandLayout w = band_layout(band_plan(K, n.data(), split.data(), hop, rows), C, rows, post != 0);
        std::vector<long long> planes, off;
        for (int k = 0; k <= K; ++k) planes.push_back((long long)w.plane[k]), off.push_back((long long)w.chunk_offset(k, chunk));
        list("planes", planes, ", "), list("offsets", off, ", ");
        printf("\"per_stream\": %lld, \"chunk_bytes\": %lld}\n", (long long)w.per_stream, (long long)w.chunk_bytes(chunk));
    } else if (kind == "pads" && a.empty()) {
        printf("\"chunk_pad\": %lld, \"band_pad\": %lld, \"max_bands\": %d}\n", (long long)kChunkPad, (long long)kBandPad, kMaxBands);
    } else {
        printf("\"error\": \"unknown line\"}\n");
        return false;
    }
    return true;
}

}  // namespace

int main() {
    bool ok = true;
    for (std::string line; std::getline(std::cin, line);) ok = run_line(line) && ok;
    return ok ? 0 : 2;
}
