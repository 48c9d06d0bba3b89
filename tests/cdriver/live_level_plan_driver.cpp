// live_level_plan_driver.cpp — runs the live level meters' arithmetic of em-spec_amd/csrc/emspec_live_plan.h without a GPU
// (live_level_ring_bytes, live_cross_ring_bytes, live_level_bytes, live_cross_bytes, live_cross_error, live_cross_pairs, the
// capacity rule live_overlay_fits with per = 1): the calls of emspec_live.cpp with every HIP call left out, and in place of
// live_overlay_kernel a model of what its waves do to the two record rings - a 24-byte level record per stream and a 16-byte
// cross record per pair written at slot j % slots when frame j arrives, read when column j is emitted.  The rings are heap blocks
// of EXACTLY live_level_ring_bytes / live_cross_ring_bytes, so that a slot past the end is ASan's to report; every record
// carries the (epoch, frame) that wrote it.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/live_level_plan_driver.cpp -o live_level_plan_driver
// tests/test_live_level_plan_cpu.py checks the output.  Input, one line each:
//   open S n hop reassign form n_high split views
//   frame | flush | push COUNT | reset STREAM | fits S VIEWS COLS CAPACITY
// Output: a JSON list, one object per line after `open`.
#include "emspec_live_plan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

using namespace emspec;

namespace {

struct LevelRec { uint64_t frame, epoch; uint32_t live, pad; };   // 24 bytes, as emspec_level
struct CrossRec { uint64_t frame; int64_t epoch; };                // 16 bytes, as emspec_cross
static_assert(sizeof(LevelRec) == kLiveLevelRecord && sizeof(CrossRec) == kLiveCrossRecord, "the model's records have the real sizes");

struct Session {
    LiveGeometry g;
    LiveCounters c;
    std::vector<LiveStream> desc;
    std::vector<long long> epoch;   // per stream: resets so far
    int views = 1, pairs = 0, slots = 0;
    char *lring = nullptr, *xring = nullptr;
    long long writes = 0, reads = 0, stale = 0, lost = 0, own = 0;

    ~Session() { std::free(lring); std::free(xring); }
    void open(int S, int n, int hop, int reassign, int form, int n_high, int split, int v) {
        g = live_session(n_high ? live_ask_two_band(S, n, n_high, hop, split, reassign, form, 1024) : live_ask_single(S, n, hop, reassign, form, 1024)).g;
        c.open(S);
        desc.assign(S, LiveStream{});
        epoch.assign(S, 0);
        views = v;
        pairs = live_cross_error(S, v) ? 0 : live_cross_pairs(S, v);
        slots = live_wave_slots(g);
        std::free(lring); std::free(xring);
        lring = static_cast<char*>(std::calloc(1, live_level_ring_bytes(g)));
        xring = static_cast<char*>(std::calloc(1, std::max<size_t>(1, pairs ? live_cross_ring_bytes(g, v) : 0)));
    }
    // the byte a record of `size` bytes in slot j % slots of row r starts at: what the kernel's 64-bit offsets compute
    size_t at(int r, long long j, size_t size) const { return ((size_t)r * (size_t)slots + (size_t)(j % slots)) * size; }
    // one launch as the kernel's waves serve it: all writes first, then all reads (no wave waits for another)
    void launch() {
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < g.S; ++s) {
                const LiveStream& d = desc[s];
                const int ncol = d.flush ? d.flush : d.frames;
                const bool crossed = pairs && s % views == 0;
                for (int i = 0; i < ncol; ++i) {
                    if (pass == 0) {
                        if (d.flush || i >= d.frames) continue;
                        LevelRec old, rec{(uint64_t)(d.j0 + i), (uint64_t)epoch[s], 1, 0};
                        std::memcpy(&old, lring + at(s, d.j0 + i, sizeof rec), sizeof old);
                        if (old.live && old.epoch == (uint64_t)epoch[s]) ++lost;   // a record still to be emitted
                        std::memcpy(lring + at(s, d.j0 + i, sizeof rec), &rec, sizeof rec);
                        ++writes;
                        if (crossed) {
                            const CrossRec x{(uint64_t)(d.j0 + i), (int64_t)epoch[s]};
                            std::memcpy(xring + at(s / views, d.j0 + i, sizeof x), &x, sizeof x);
                        }
                        continue;
                    }
                    const long long col = d.j0 - g.D + i;
                    if (col < 0) continue;
                    LevelRec rec;
                    std::memcpy(&rec, lring + at(s, col, sizeof rec), sizeof rec);
                    const bool ring = d.flush || col < d.j0;
                    if (!ring) ++own;
                    ++reads;
                    if (rec.frame != (uint64_t)col || rec.epoch != (uint64_t)epoch[s] || !rec.live) { if (ring) ++stale; }
                    else { rec.live = 0; std::memcpy(lring + at(s, col, sizeof rec), &rec, sizeof rec); }
                    if (crossed) {
                        CrossRec x;
                        std::memcpy(&x, xring + at(s / views, col, sizeof x), sizeof x);
                        if (ring && (x.frame != (uint64_t)col || x.epoch != (int64_t)epoch[s])) ++stale;
                    }
                }
            }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: see the head of live_level_plan_driver.cpp\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    Session t;
    bool first = true;
    printf("[");
    while (std::getline(in, line)) {
        std::istringstream w(line);
        std::string op;
        if (!(w >> op)) continue;
        if (op == "open") {
            int S, n, hop, reassign, form, n_high, split, views;
            if (!(w >> S >> n >> hop >> reassign >> form >> n_high >> split >> views)) return 2;
            t.open(S, n, hop, reassign, form, n_high, split, views);
            continue;
        }
        long long a = 0, b = 0, m = 0, q = 0;
        w >> a >> b >> m >> q;
        int refused = 0;
        if (op == "frame") {
            live_frame_fill(t.g, t.c, t.desc.data());
            t.launch();
            live_frame_commit(t.g, t.c, nullptr);
        } else if (op == "flush") {
            if (!t.c.any_pending()) refused = 1;
            else {
                live_flush_fill(t.g, t.c, t.desc.data());
                t.launch();
                live_flush_commit(t.g, t.c, nullptr);
            }
        } else if (op == "push") {
            LivePush p(t.g.S);
            while (p.used < a) {
                live_push_take(t.g, t.c, p, a);
                if (!live_push_round(t.g, t.c, p, false, t.desc.data())) continue;
                if (p.mx > 0) t.launch();
                live_push_commit(t.g, t.c, p);
            }
        } else if (op == "reset") {
            if (t.pairs) refused = 1;   // (a live cross is set: the streams of a pair stay in step)
            else { t.c.reset_stream((int)a); t.epoch[(size_t)a] += 1; }
        } else if (op == "fits") {
            // the cross's capacity rule: no pairs at all for a stream count that is no multiple of views, else pairs x cols records
            refused = live_cross_error((int)a, (int)b) ? 2 : (live_overlay_fits(live_cross_pairs((int)a, (int)b), m, 1, q) ? 0 : 1);
        } else {
            return 2;
        }
        printf("%s{\"op\":\"%s\",\"slots\":%d,\"cap\":%lld,\"level_ring\":%lld,\"cross_ring\":%lld,\"level_out\":%lld,\"cross_out\":%lld,\"pairs\":%d,"
               "\"refused\":%d,\"writes\":%lld,\"reads\":%lld,\"own\":%lld,\"stale\":%lld,\"lost\":%lld,\"fed\":[",
               first ? "" : ",\n", op.c_str(), t.slots, (long long)t.g.cap, (long long)live_level_ring_bytes(t.g),
               (long long)(t.pairs ? live_cross_ring_bytes(t.g, t.views) : 0), (long long)live_level_bytes(t.g, 7),
               (long long)(t.pairs ? live_cross_bytes(t.g, t.views, 7) : 0), t.pairs, refused, t.writes, t.reads, t.own, t.stale, t.lost);
        first = false;
        for (int s = 0; s < t.g.S; ++s) printf("%s%lld", s ? "," : "", (long long)t.c.fed[s]);
        printf("],\"emitted\":[");
        for (int s = 0; s < t.g.S; ++s) printf("%s%lld", s ? "," : "", (long long)t.c.emitted[s]);
        printf("]}");
    }
    printf("]\n");
    return 0;
}
