// audio_plan_driver.cpp — runs the arithmetic of em-spec_amd/csrc/emspec_audio_plan.h without a GPU, on one stream: in place of
// live_audio_store_kernel a model of what its threads do to the ring (which of a launch's samples are stored, from which place
// of the fresh block, in which slot, and how often a slot is written in one launch), in place of audio_view_kernel the samples a
// view reads through the two runs across the wrap, and the head / body / tail split applied to a copy between two blocks of
// exactly `count` samples.  The ring is a host block of exactly W entries, each carrying the sample that wrote it, so that a
// wrong slot is ASan's to report.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/audio_plan_driver.cpp -o audio_plan_driver
// tests/test_audio_plan_cpu.py checks the output.  Input, one line each:
//   ring W | reset | block NEWBASE COUNT | frame J N HOP | view FIRST COUNT STRIDE | check FIRST COUNT STRIDE END W |
//   split SA DA COUNT | bytes S W
// Output: a JSON list, one object per line.  `ring` is printed only for W <= 64.
#include "emspec_audio_plan.h"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace emspec;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: see the head of audio_plan_driver.cpp\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int64_t W = 0, end = 0;
    std::vector<long long> ring;   // [W]: the sample each slot holds, -1: none
    bool first = true;
    printf("[");
    while (std::getline(in, line)) {
        std::istringstream w(line);
        std::string op;
        if (!(w >> op)) continue;
        long long a = 0, b = 0, c = 0, d = 0, e = 0;
        w >> a >> b >> c >> d >> e;
        printf("%s{\"op\":\"%s\"", first ? "" : ",\n", op.c_str());
        first = false;
        if (op == "ring") {
            W = a; end = 0;
            ring.assign((size_t)W, -1);
            ring.shrink_to_fit();
        } else if (op == "reset") {
            end = 0;
            ring.assign((size_t)W, -1);
        } else if (op == "block" || op == "frame") {
            // the fresh block of the launch: entry i carries the absolute sample it is (block form: NEWBASE + i; per-frame form:
            // J HOP + i), in a vector of exactly its length
            const bool frame = op == "frame";
            const int64_t len = b, base = frame ? a * c : a;
            std::vector<long long> fresh((size_t)len);
            for (int64_t i = 0; i < len; ++i) fresh[(size_t)i] = base + i;
            const AudioRange all = frame ? audio_fresh(1, a, a * c, 0, 1, 0, (int)b, (int)c) : audio_fresh(2, 0, a, b, 0, 0, 0, 0);
            const AudioRange r = audio_keep(all, W);
            const AudioRuns run = audio_runs(r.a0, r.count, W);
            std::vector<int> writes((size_t)W, 0);
            int most = 0;
            for (int64_t i = 0; i < r.count; ++i) {   // (the kernel's two runs)
                const int64_t slot = i < run.n0 ? run.slot0 + i : i - run.n0;
                ring.at((size_t)slot) = fresh.at((size_t)(r.src + i));
                most = std::max(most, ++writes.at((size_t)slot));
            }
            end = frame ? audio_end(1, a + 1, 0, (int)b, (int)c) : audio_end(2, 0, a + b, 0, 0);
            printf(",\"all\":[%lld,%lld,%lld],\"kept\":[%lld,%lld,%lld],\"runs\":[%lld,%lld,%lld],\"most_writes\":%d", (long long)all.src,
                   (long long)all.a0, (long long)all.count, (long long)r.src, (long long)r.a0, (long long)r.count, (long long)run.slot0,
                   (long long)run.n0, (long long)run.n1, most);
        } else if (op == "view") {
            const int rc = audio_view_check(a, b, c, end, W);
            printf(",\"rc\":%d,\"samples\":[", rc);
            if (rc == kAudioViewOk) {
                const AudioRuns r = audio_runs(a, b, W);
                for (int64_t k = 0; k < r.n0; ++k) printf("%s%lld", k ? "," : "", ring.at((size_t)(r.slot0 + k)));
                for (int64_t k = 0; k < r.n1; ++k) printf(",%lld", ring.at((size_t)k));
                printf("],\"runs\":[%lld,%lld,%lld", (long long)r.slot0, (long long)r.n0, (long long)r.n1);
            }
            printf("]");
        } else if (op == "check") {
            printf(",\"rc\":%d", audio_view_check(a, b, c, d, e));
        } else if (op == "split") {
            // COUNT samples from a block SA samples behind a 16-byte boundary to one DA behind: the split, and the copy it makes
            // between two vectors of exactly COUNT entries; a 16-byte piece must start on a boundary on both sides
            const AudioSplit sp = audio_split((int)a, (int)b, c);
            std::vector<long long> src((size_t)c), dst((size_t)c, -1);
            for (int64_t i = 0; i < c; ++i) src[(size_t)i] = 1000 + i;
            bool aligned = true;
            std::vector<int> writes((size_t)c, 0);
            for (int64_t i = 0; i < sp.head; ++i) { dst.at((size_t)i) = src.at((size_t)i); ++writes.at((size_t)i); }
            for (int64_t q = 0; q < sp.body; ++q) {
                const int64_t at = sp.head + 4 * q;
                aligned = aligned && (a + at) % 4 == 0 && (b + at) % 4 == 0;
                for (int k = 0; k < 4; ++k) { dst.at((size_t)(at + k)) = src.at((size_t)(at + k)); ++writes.at((size_t)(at + k)); }
            }
            for (int64_t i = 0; i < sp.tail; ++i) {
                const int64_t at = sp.head + 4 * sp.body + i;
                dst.at((size_t)at) = src.at((size_t)at);
                ++writes.at((size_t)at);
            }
            const bool once = std::all_of(writes.begin(), writes.end(), [](int k) { return k == 1; });
            printf(",\"split\":[%lld,%lld,%lld],\"copied\":%s,\"aligned\":%s,\"once\":%s", (long long)sp.head, (long long)sp.body,
                   (long long)sp.tail, src == dst ? "true" : "false", aligned ? "true" : "false", once ? "true" : "false");
        } else if (op == "bytes") {
            printf(",\"bytes\":%llu,\"stride\":%lld", (unsigned long long)audio_ring_bytes((int)a, b), (long long)audio_stride(b));
        } else {
            return 2;
        }
        printf(",\"end\":%lld,\"first\":%lld", (long long)end, (long long)(W ? audio_first(end, W) : 0));
        if (W <= 64) {
            printf(",\"ring\":[");
            for (size_t k = 0; k < ring.size(); ++k) printf("%s%lld", k ? "," : "", ring[k]);
            printf("]");
        }
        printf("}");
    }
    printf("]\n");
    return 0;
}
