// live_plan_driver.cpp — runs em-spec_amd/csrc/emspec_live_plan.h without a GPU: the calls of emspec_live.cpp with every HIP
// call left out (no allocation on a device, no launch, no synchronisation), the staging copies done into host blocks of exactly
// the header's sizes so that a wrong offset is ASan's to report.  Prints JSON.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/live_plan_driver.cpp -o live_plan_driver
// tests/test_live_plan_cpu.py compares the output with tests/live_ref.py.
//   geometry FILE   one session per line: S n hop reassign form n_high split R cell views frame_bytes cols
//                   -> a list of objects: the geometry and every byte size
//   trace FILE      a scripted session -> a list with one object per call.  First line:
//                       open S n hop reassign form n_high split pcm_views frame_bytes
//                   then: frame | flush | push COUNT DIRECT | predict COUNT | reset STREAM
#include "emspec_live_plan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

using namespace emspec;

namespace {

template <class T> void list(const char* name, const std::vector<T>& v, const char* end = ",") {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]%s", end);
}
void num(const char* name, long long v, const char* end = ",") { printf("\"%s\":%lld%s", name, v, end); }

// ---- one launch as the kernels would see it, and one call ----
struct Launch {
    bool launched = true;
    int64_t take = 0;            // push: the round's samples per stream, where each copy went, the fullest stream before it
    std::vector<int64_t> at;
    int maxpend = 0, mx = 0;
    bool uniform = false, priming = false;
    std::vector<LiveStream> desc;
    std::vector<int64_t> nc;     // push: the round's columns per stream
};
struct Call {
    std::string op;
    int64_t arg = 0, predict = -1;
    std::string refused;         // empty: the call went through
    std::vector<Launch> launches;
    std::vector<int64_t> counts, first;   // per stream: a push's counts and first columns; a frame's / flush's column in `first`
};

// ---- the session: emspec_live.cpp's calls on the header ----
struct Session {
    LiveGeometry g;
    LiveCounters c;
    int views = 0, fb = 1;                 // views != 0: a PCM-style session (raw frames per source, a drain before a reset)
    std::vector<LiveStream> desc;          // [S]
    std::vector<float> fresh;              // [S][cap]
    std::vector<unsigned char> raw;        // [S / views][cap] frames
    std::vector<float> block;              // the caller's samples of one push

    void open(int S, int n, int hop, int reassign, int form, int n_high, int split, int pcm_views, int frame_bytes) {
        g = live_geometry(S, n, hop, reassign, form, n_high, split);
        c.open(S);
        views = pcm_views, fb = frame_bytes;
        desc.assign(g.desc_bytes() / sizeof(LiveStream), LiveStream{});
        fresh.assign(g.fresh_bytes() / 4, 0.0f);
        if (views) raw.assign(g.raw_bytes(views, fb), 0);
    }
    Launch seen(Launch l = Launch()) const {
        l.uniform = live_uniform(desc.data(), g.S);
        l.priming = live_priming(desc.data(), g.S);
        l.desc = desc;
        return l;
    }
    // live_check's rule
    std::string refusal() const {
        for (int s = 0; s < g.S; ++s)
            if (c.flushed(s, g.D)) return "stream " + std::to_string(s) + " was flushed";
        return "";
    }
    Call frame() {
        Call k;
        k.op = "frame";
        if (!(k.refused = refusal()).empty()) return k;
        live_frame_fill(g, c, desc.data());
        k.launches.push_back(seen());
        k.first.assign(g.S, -7);
        live_frame_commit(g, c, k.first.data());
        return k;
    }
    Call flush() {
        Call k;
        k.op = "flush";
        if (!c.any_pending()) { k.refused = "no pending column"; return k; }
        live_flush_fill(g, c, desc.data());
        k.launches.push_back(seen());
        k.first.assign(g.S, -7);
        live_flush_commit(g, c, k.first.data());
        return k;
    }
    int64_t predict(int64_t count) const { return live_push_columns(g, c, count, g.n, g.hop, g.reassign); }
    Call push(int64_t count, bool direct) {
        Call k;
        k.op = "push", k.arg = count;
        if (!(k.refused = refusal()).empty()) return k;
        k.predict = predict(count);
        block.assign((size_t)count, 1.0f);
        const std::vector<unsigned char> rawblock(views ? (size_t)count * fb : 0, 1);
        LivePush p(g.S);
        while (p.used < count) {
            live_push_take(g, c, p, count);
            Launch l;
            l.take = p.take, l.maxpend = p.maxpend;
            for (int i = 0; views && i < g.S / views; ++i) {
                l.at.push_back((int64_t)g.raw_at(i, p.maxpend, fb));
                std::memcpy(raw.data() + g.raw_at(i, p.maxpend, fb), rawblock.data() + (size_t)p.used * fb, (size_t)p.take * fb);
            }
            for (int s = 0; !views && s < g.S; ++s) {
                l.at.push_back((int64_t)g.fresh_at(s, c.pend[s]));
                std::memcpy(fresh.data() + g.fresh_at(s, c.pend[s]), block.data() + p.used, (size_t)p.take * 4);
            }
            l.launched = live_push_round(g, c, p, direct, desc.data());
            l.mx = p.mx;
            if (l.launched) {
                l = seen(l);
                l.nc = p.nc;
                live_push_commit(g, c, p);
            }
            k.launches.push_back(l);
        }
        k.counts = p.produced, k.first = p.first;
        return k;
    }
    Call reset(int s) {
        Call k;
        k.op = "reset", k.arg = s;
        if (views && c.pcm_staged() != 0) {   // live_pcm_drain
            live_drain_fill(g, c, desc.data());
            k.launches.push_back(seen());
            live_drain_commit(g, c);
        }
        c.reset_stream(s);
        return k;
    }
    std::vector<int64_t> pending() const {
        std::vector<int64_t> v;
        for (int s = 0; s < g.S; ++s) v.push_back(c.pending(s) ? 1 : 0);
        return v;
    }
};

void print_geometry(const Session& t, int R, int cell, int views, int fb, int cols) {
    const LiveGeometry& g = t.g;
    printf("{");
    num("S", g.S), num("n", g.n), num("hop", g.hop), num("reassign", g.reassign), num("D", g.D), num("form", g.form);
    num("mmax", g.mmax), num("slots", g.slots), num("cap", g.cap), num("ring_mask", g.ring_mask), num("n_high", g.n_high);
    num("split", g.split), num("shift", g.shift), num("D_high", g.D_high), num("slots_high", g.slots_high);
    num("ring_bytes", g.ring_bytes(R, cell)), num("ring_high_bytes", g.ring_high_bytes(R, cell));
    num("rings_bytes", g.rings_bytes(R, cell)), num("rings_high_bytes", g.rings_high_bytes(R, cell));
    num("sring_bytes", g.sring_bytes()), num("done_bytes", g.done_bytes()), num("desc_bytes", g.desc_bytes());
    num("fresh_bytes", g.fresh_bytes()), num("decoded_bytes", g.decoded_bytes()), num("raw_bytes", g.raw_bytes(views, fb));
    num("raw_stride", g.raw_stride(fb)), num("out_bytes", g.out_bytes(R, cols)), num("out1_bytes", g.out_bytes(R, 1));
    num("out_cell", LiveGeometry::out_cell(R, cols, g.S - 1, cols - 1)), num("columns_bytes", LiveGeometry::columns_bytes(R, cols));
    num("fresh_at", g.fresh_at(g.S - 1, 5)), num("raw_at", g.raw_at(g.S / views - 1, 5, fb));
    num("pstate_bytes", LiveGeometry::pstate_bytes(R), "}");
}

void print_call(const Session& t, const Call& k) {
    printf("{\"op\":\"%s\",", k.op.c_str());
    num("arg", k.arg), num("predict", k.predict);
    printf("\"refused\":\"%s\",\"launches\":[", k.refused.c_str());
    for (size_t i = 0; i < k.launches.size(); ++i) {
        const Launch& l = k.launches[i];
        printf("%s{", i ? "," : "");
        num("launched", l.launched), num("take", l.take), num("maxpend", l.maxpend), num("mx", l.mx);
        num("uniform", l.uniform), num("priming", l.priming);
        list("at", l.at), list("nc", l.nc);
        printf("\"desc\":[");
        for (size_t s = 0; s < l.desc.size(); ++s) {
            const LiveStream& d = l.desc[s];
            printf("%s[%lld,%lld,%d,%d,%d,%d]", s ? "," : "", d.j0, d.newbase, d.frames, d.newcount, d.out_at, d.flush);
        }
        printf("]}");
    }
    printf("],");
    list("counts", k.counts), list("first", k.first);
    list("fed", t.c.fed), list("emitted", t.c.emitted), list("seen", t.c.seen), list("newbase", t.c.newbase), list("pend", t.c.pend);
    list("pending", t.pending());
    num("any_pending", t.c.any_pending(), "}");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: see the head of live_plan_driver.cpp\n"); return 2; }
    const std::string cmd = argv[1];
    std::ifstream in(argv[2]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::string line;
    Session t;
    bool first = true;
    printf("[");
    while (std::getline(in, line)) {
        std::istringstream w(line);
        const char* sep = first ? "" : ",\n";
        if (cmd == "geometry") {
            int S, n, hop, reassign, form, n_high, split, R, cell, views, fb, cols;
            if (!(w >> S >> n >> hop >> reassign >> form >> n_high >> split >> R >> cell >> views >> fb >> cols)) continue;
            t.g = live_geometry(S, n, hop, reassign, form, n_high, split);   // (no buffers: sizes only)
            printf("%s", sep);
            print_geometry(t, R, cell, views, fb, cols);
        } else if (cmd == "trace") {
            std::string op;
            long long a = 0, b = 0;
            if (!(w >> op)) continue;
            if (op == "open") {
                int S, n, hop, reassign, form, n_high, split, views, fb;
                if (!(w >> S >> n >> hop >> reassign >> form >> n_high >> split >> views >> fb)) return 2;
                t.open(S, n, hop, reassign, form, n_high, split, views, fb);
                continue;
            }
            w >> a >> b;
            Call k;
            if (op == "frame") k = t.frame();
            else if (op == "flush") k = t.flush();
            else if (op == "push") k = t.push(a, b != 0);
            else if (op == "predict") { k.op = "predict", k.arg = a, k.predict = t.predict(a); }
            else if (op == "reset") k = t.reset((int)a);
            else return 2;
            printf("%s", sep);
            print_call(t, k);
        } else {
            return 2;
        }
        first = false;
    }
    printf("]\n");
    return 0;
}
