// live_overlay_plan_driver.cpp — runs the overlay arithmetic of em-spec_amd/csrc/emspec_live_plan.h without a GPU: the calls of
// emspec_live.cpp with every HIP call left out, and in place of live_overlay_kernel a model of what its waves do to the
// envelope's pair ring - which slot each frame's pair is written to, where each emitted column's pair comes from (the ring, the
// launch's own samples, or the empty column), and which slot of the caller's arrays it goes to.  The ring is a host block of
// exactly live_wave_ring_bytes, so that a wrong slot is ASan's to report; every slot carries the (epoch, frame) that wrote it.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/live_overlay_plan_driver.cpp -o live_overlay_plan_driver
// tests/test_live_overlay_plan_cpu.py checks the output.  Input, one line each:
//   open S n hop reassign form n_high split
//   frame | flush | push COUNT DIRECT MAX_COLUMNS | reset STREAM | fits S COLS PER CAPACITY
// Output: a JSON list, one object per line after `open`.
#include "emspec_live_plan.h"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

using namespace emspec;

namespace {

struct Tag { long long epoch = -1, frame = -1; bool read = true; };   // (8-byte pairs on the device; the model keeps who wrote them)

struct Session {
    LiveGeometry g;
    LiveCounters c;
    std::vector<LiveStream> desc;
    std::vector<long long> epoch;      // per stream: resets so far
    std::vector<Tag> ring;             // [S][wslots]
    int wslots = 0;
    long long stale = 0, lost = 0;     // reads of a slot that does not hold the column; writes over a pair still to be emitted
    bool first_event = true;

    void open(int S, int n, int hop, int reassign, int form, int n_high, int split) {
        // (the overlays read the session at its first fft size only: the same for a two-band session, whatever its rows)
        g = live_session(n_high ? live_ask_two_band(S, n, n_high, hop, split, reassign, form, 1024) : live_ask_single(S, n, hop, reassign, form, 1024)).g;
        c.open(S);
        desc.assign(S, LiveStream{});
        epoch.assign(S, 0);
        wslots = live_wave_slots(g);
        ring.assign(live_wave_ring_bytes(g) / 8, Tag{});
    }
    // one launch as live_overlay_kernel serves it: wave (s, i), i < max(frames, flush).  out_cols: the launch's stride;
    // base[s]: where the launch's slot 0 of stream s lands in the caller's [S][cols] arrays (a staged push: the columns produced so far)
    void launch(bool empty_col, int64_t cols, const std::vector<int64_t>& base) {
        // every wave of the kernel may run in any order: all writes first, then all reads, must give what reads first give
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < g.S; ++s) {
                const LiveStream& d = desc[s];
                const int ncol = d.flush ? d.flush : d.frames;
                for (int i = 0; i < ncol; ++i) {
                    if (pass == 0 && !d.flush && i < d.frames) {
                        Tag& t = ring[(size_t)s * wslots + (size_t)((d.j0 + i) % wslots)];
                        // the pair it overwrites: emitted (read), or of an earlier life of the stream, or none
                        if (t.epoch == epoch[s] && !t.read) ++lost;
                        t = Tag{epoch[s], d.j0 + i, false};
                    }
                    if (pass == 0) continue;
                    const int oc = live_out_slot(d.j0, d.out_at, g.D, i, empty_col);
                    if (oc < 0) continue;
                    const long long col = d.j0 - g.D + i;
                    int src = 0;   // 0: the empty column, 1: the ring, 2: this launch's samples
                    if (col >= 0) {
                        src = (d.flush || col < d.j0) ? 1 : 2;
                        Tag& t = ring[(size_t)s * wslots + (size_t)(col % wslots)];
                        // (a column of this launch is taken from the samples, but its slot holds it too: mark it emitted)
                        if (t.epoch != epoch[s] || t.frame != col) { if (src == 1) ++stale; }
                        else t.read = true;
                    }
                    printf("%s[%d,%d,%d,%lld,%d,%lld]", first_event ? "" : ",", s, i, oc, col, src,
                           (long long)live_overlay_pair(cols, s, base[s] + oc));
                    first_event = false;
                }
            }
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: see the head of live_overlay_plan_driver.cpp\n"); return 2; }
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
            int S, n, hop, reassign, form, n_high, split;
            if (!(w >> S >> n >> hop >> reassign >> form >> n_high >> split)) return 2;
            t.open(S, n, hop, reassign, form, n_high, split);
            continue;
        }
        long long a = 0, b = 0, m = 0, q = 0;
        w >> a >> b >> m >> q;
        printf("%s{\"op\":\"%s\",\"wslots\":%d,\"D\":%d,\"mmax\":%d,\"ring_bytes\":%lld,\"off\":%d,", first ? "" : ",\n", op.c_str(), t.wslots,
               t.g.D, t.g.mmax, (long long)live_wave_ring_bytes(t.g), live_wave_offset(t.g));
        first = false;
        t.first_event = true;
        const std::vector<int64_t> zero((size_t)t.g.S, 0);
        int refused = 0;
        printf("\"events\":[");
        if (op == "frame") {
            live_frame_fill(t.g, t.c, t.desc.data());
            t.launch(true, 1, zero);
            live_frame_commit(t.g, t.c, nullptr);
        } else if (op == "flush") {
            if (!t.c.any_pending()) refused = 1;
            else {
                live_flush_fill(t.g, t.c, t.desc.data());
                t.launch(true, 1, zero);
                live_flush_commit(t.g, t.c, nullptr);
            }
        } else if (op == "push") {
            const int64_t count = a, max_columns = m;
            const bool direct = b != 0;
            if (live_push_columns(t.g, t.c, count, t.g.n, t.g.hop, t.g.reassign) > max_columns) refused = 1;
            LivePush p(t.g.S);
            while (!refused && p.used < count) {
                live_push_take(t.g, t.c, p, count);
                if (!live_push_round(t.g, t.c, p, direct, t.desc.data())) continue;
                // in place: the kernel writes [S][max_columns] at out_at = the columns produced so far; staged: [S][mmax] from 0,
                // copied to the columns produced so far
                if (p.mx > 0) t.launch(false, max_columns, direct ? zero : p.produced);
                live_push_commit(t.g, t.c, p);
            }
        } else if (op == "reset") {
            t.c.reset_stream((int)a);
            t.epoch[(size_t)a] += 1;
        } else if (op == "fits") {
            refused = live_overlay_fits((int)a, b, (int)m, q) ? 0 : 1;
        } else {
            return 2;
        }
        printf("],\"refused\":%d,\"stale\":%lld,\"lost\":%lld,\"fed\":[", refused, t.stale, t.lost);
        for (int s = 0; s < t.g.S; ++s) printf("%s%lld", s ? "," : "", (long long)t.c.fed[s]);
        printf("],\"emitted\":[");
        for (int s = 0; s < t.g.S; ++s) printf("%s%lld", s ? "," : "", (long long)t.c.emitted[s]);
        printf("]}");
    }
    printf("]\n");
    return 0;
}
