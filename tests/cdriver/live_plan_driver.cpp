// live_plan_driver.cpp — runs em-spec_amd/csrc/emspec_live_plan.h without a GPU: the geometry of a session of every kind, the rule
// that refuses a call, and scripted sessions - the calls of emspec_live.cpp with every HIP call left out (no allocation on a
// device, no launch, no synchronisation), the staging copies done into host blocks of exactly the header's sizes so that a wrong
// offset is ASan's to report, and per launch the steps of the header's launch plan.  Prints JSON.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/live_plan_driver.cpp -o live_plan_driver
// tests/test_live_plan_cpu.py and tests/test_live_band_plan_cpu.py compare the output with tests/live_ref.py and
// tests/live_band_ref.py.  A session is written SHAPE = KIND S hop reassign form R views frame_bytes K n[0..K) split[0..K-1), KIND
// 1 single-resolution, 2 two-band, 3 multi-band (views 0: a float session).
//   geometry FILE   one session per line: SHAPE cell cols -> a list of objects: the geometry and every byte size.  Kinds 1 and 2:
//                   the second band's numbers under the two-band names (n_high, split, shift, D_high, slots_high, ..., 0
//                   without one).  Kind 3: "error" (the rule broken, or "") and, when accepted, the bands' numbers as lists; for
//                   K = 2 also the two-band session of the same sizes and split ("two")
//   compat FILE     one pair per line: SHAPE | SHAPE, the open session and what a call asks for -> {"why": the refusal or ""}
//   trace FILE      a scripted session -> a list with one object per call.  First line: open SHAPE
//                   then: frame | flush | push COUNT DIRECT | predict COUNT | reset STREAM
#include "emspec_live_plan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

using namespace emspec;

namespace {

constexpr int kInlineFinalize = 2;   // emspec_live.cpp's

template <class T> void list(const char* name, const std::vector<T>& v, const char* end = ",") {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]%s", end);
}
void num(const char* name, long long v, const char* end = ",") { printf("\"%s\":%lld%s", name, v, end); }

struct Shape {
    int kind = 0, S = 0, hop = 0, reassign = 0, form = 0, R = 0, views = 0, fb = 1, K = 0;
    int32_t n[8] = {}, split[8] = {};
    bool read(std::istream& w) {
        if (!(w >> kind >> S >> hop >> reassign >> form >> R >> views >> fb >> K) || K < 0 || K > 8) return false;
        for (int k = 0; k < K; ++k)
            if (!(w >> n[k])) return false;
        for (int k = 0; k + 1 < K; ++k)
            if (!(w >> split[k])) return false;
        return kind == kLiveMultiBand || K == kind;
    }
    const char* error() const {   // the multi-band entries' checks
        if (kind != kLiveMultiBand) return nullptr;
        if (const char* why = band_shape_error(K, n, hop)) return why;
        return band_split_error(K, split, R);
    }
    // what the entry of the session's kind makes of its arguments
    LiveAsk ask() const {
        if (kind == kLiveSingle) return live_ask_single(S, n[0], hop, reassign, form, R);
        if (kind == kLiveTwoBand) return live_ask_two_band(S, n[0], n[1], hop, split[0], reassign, form, R);
        return live_ask_bands(S, band_plan(K, n, split, hop, R), hop, reassign, form);
    }
};

// ---- geometry ----
void print_common(const LiveSession& m, int R, const char* end) {
    const LiveGeometry& g = m.g;
    num("S", g.S), num("n", g.n), num("hop", g.hop), num("reassign", g.reassign), num("D", g.D), num("form", g.form);
    num("mmax", g.mmax), num("cap", g.cap), num("ring_mask", g.ring_mask), num("sring_bytes", g.sring_bytes());
    num("desc_bytes", g.desc_bytes()), num("fresh_bytes", g.fresh_bytes()), num("out1_bytes", g.out_bytes(R, 1));
    num("done_bytes", m.done_bytes(), end);
}
// kinds 1 and 2, under the two-band names
void print_flat(const LiveSession& m, int R, int cell, int views, int fb, int cols) {
    const LiveGeometry& g = m.g;
    const bool two = m.bands == 2;
    const LiveBand none, &h = two ? m.b[1] : none;
    print_common(m, R, ",");
    num("slots", m.b[0].slots), num("n_high", h.n), num("split", two ? m.b[0].hi : 0), num("shift", h.shift), num("D_high", h.D);
    num("slots_high", h.slots);
    num("ring_bytes", m.ring_bytes(0, cell)), num("ring_high_bytes", two ? m.ring_bytes(1, cell) : 0);
    num("rings_bytes", m.rings_bytes(0, cell)), num("rings_high_bytes", two ? m.rings_bytes(1, cell) : 0);
    num("decoded_bytes", g.decoded_bytes()), num("raw_bytes", g.raw_bytes(views, fb));
    num("raw_stride", g.raw_stride(fb)), num("out_bytes", g.out_bytes(R, cols));
    num("out_cell", LiveGeometry::out_cell(R, cols, g.S - 1, cols - 1)), num("columns_bytes", LiveGeometry::columns_bytes(R, cols));
    num("fresh_at", g.fresh_at(g.S - 1, 5)), num("raw_at", g.raw_at(g.S / views - 1, 5, fb));
    num("pstate_bytes", LiveGeometry::pstate_bytes(R), "");
}
// kind 3, band by band
void print_bands(const LiveSession& m, int R, int cell) {
    print_common(m, R, ",");
    num("bands", m.bands);
    std::vector<long long> bn, lo, hi, shift, D, fs, le, slots, ring, rings, prime;
    for (int k = 0; k < m.bands; ++k) {
        const LiveBand& b = m.b[k];
        bn.push_back(b.n), lo.push_back(b.lo), hi.push_back(b.hi), shift.push_back(b.shift), D.push_back(b.D);
        fs.push_back(b.frame_shift), le.push_back(b.lat_extra), slots.push_back(b.slots);
        ring.push_back((long long)m.ring_bytes(k, cell)), rings.push_back((long long)m.rings_bytes(k, cell));
        prime.push_back(m.launch_frames(k, 3, true) - m.launch_frames(k, 3, false));
    }
    list("band_n", bn), list("lo", lo), list("hi", hi), list("shift", shift), list("band_D", D), list("frame_shift", fs);
    list("lat_extra", le), list("slots", slots), list("ring_bytes", ring), list("rings_bytes", rings), list("priming_extra", prime);
    num("defers_1", m.defers(0, 1, kInlineFinalize)), num("defers_2", m.defers(0, 2, kInlineFinalize));
    num("defers_3", m.defers(0, 3, kInlineFinalize), "");
}
void print_geometry(const Shape& sh, int cell, int cols) {
    printf("{");
    if (sh.kind != kLiveMultiBand) {
        print_flat(live_session(sh.ask()), sh.R, cell, sh.views, sh.fb, cols);
        printf("}");
        return;
    }
    const char* why = sh.error();
    printf("\"error\":\"%s\"", why ? why : "");
    if (why) { printf("}"); return; }
    printf(",");
    print_bands(live_session(sh.ask()), sh.R, cell);
    if (sh.K == 2) {
        Shape two = sh;
        two.kind = kLiveTwoBand, two.views = 1;
        printf(",\"two\":{");
        print_flat(live_session(two.ask()), sh.R, cell, 1, 1, 1);
        printf("}");
    }
    printf("}");
}

// ---- one launch as the kernels would see it, and one call ----
struct Launch {
    bool launched = true, flush = false;
    int mlaunch = 0;             // live_launch's: the most frames any stream has
    int64_t take = 0;            // push: the round's samples per stream, where each copy went, the fullest stream before it
    std::vector<int64_t> at;
    int maxpend = 0, mx = 0;
    bool uniform = false, priming = false;
    std::vector<LiveStream> desc;
    std::vector<int64_t> nc;     // push: the round's columns per stream
    LiveSteps steps;             // the kernels, in order
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
    LiveSession m;
    LiveCounters c;
    int views = 0, fb = 1;                 // views != 0: a PCM-style session (raw frames per source, a drain before a reset)
    std::vector<LiveStream> desc;          // [S]
    std::vector<float> fresh;              // [S][cap]
    std::vector<unsigned char> raw;        // [S / views][cap] frames
    std::vector<float> block;              // the caller's samples of one push
    std::vector<std::vector<unsigned char>> rings;   // band k's [S] rings, one byte per cell: what emspec_reset_stream clears

    void open(const Shape& sh) {
        m = live_session(sh.ask());
        const LiveGeometry& g = m.g;
        c.open(g.S);
        views = sh.views, fb = sh.fb;
        desc.assign(g.desc_bytes() / sizeof(LiveStream), LiveStream{});
        fresh.assign(g.fresh_bytes() / 4, 0.0f);
        if (views) raw.assign(g.raw_bytes(views, fb), 0);
        rings.clear();
        for (int k = 0; k < m.bands; ++k) rings.emplace_back(m.rings_bytes(k, 1), (unsigned char)1);
    }
    // live_launch(mlaunch, flush) on the descriptors as they stand
    Launch seen(int mlaunch, bool flush, Launch l = Launch()) const {
        l.mlaunch = mlaunch, l.flush = flush;
        l.uniform = live_uniform(desc.data(), m.g.S);
        l.priming = live_priming(desc.data(), m.g.S);
        l.desc = desc;
        l.steps = live_steps(m, mlaunch, flush, l.priming, kInlineFinalize);
        return l;
    }
    // live_check's rule
    std::string refusal() const {
        for (int s = 0; s < m.g.S; ++s)
            if (c.flushed(s, m.g.D)) return "stream " + std::to_string(s) + " was flushed";
        return "";
    }
    Call frame() {
        Call k;
        k.op = "frame";
        if (!(k.refused = refusal()).empty()) return k;
        live_frame_fill(m.g, c, desc.data());
        k.launches.push_back(seen(1, false));
        k.first.assign(m.g.S, -7);
        live_frame_commit(m.g, c, k.first.data());
        return k;
    }
    Call flush() {
        Call k;
        k.op = "flush";
        if (!c.any_pending()) { k.refused = "no pending column"; return k; }
        live_flush_fill(m.g, c, desc.data());
        k.launches.push_back(seen(0, true));
        k.first.assign(m.g.S, -7);
        live_flush_commit(m.g, c, k.first.data());
        return k;
    }
    int64_t predict(int64_t count) const { return live_push_columns(m.g, c, count, m.g.n, m.g.hop, m.g.reassign); }
    Call push(int64_t count, bool direct) {
        const LiveGeometry& g = m.g;
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
                l = seen(p.mx, false, l);
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
            live_drain_fill(m.g, c, desc.data());
            k.launches.push_back(seen(0, false));
            live_drain_commit(m.g, c);
        }
        for (int b = 0; b < m.bands; ++b)   // emspec_reset_stream: every band's ring of the stream
            std::memset(rings[b].data() + (size_t)s * m.ring_bytes(b, 1), 0, m.ring_bytes(b, 1));
        c.reset_stream(s);
        return k;
    }
    std::vector<int64_t> pending() const {
        std::vector<int64_t> v;
        for (int s = 0; s < m.g.S; ++s) v.push_back(c.pending(s) ? 1 : 0);
        return v;
    }
    std::vector<int64_t> cleared() const {   // per band: streams whose ring is all zero
        std::vector<int64_t> v;
        for (int b = 0; b < m.bands; ++b) {
            const size_t per = m.ring_bytes(b, 1);
            int64_t z = 0;
            for (int s = 0; s < m.g.S; ++s) {
                bool zero = true;
                for (size_t i = 0; i < per && zero; ++i) zero = rings[b][(size_t)s * per + i] == 0;
                z += zero ? 1 : 0;
            }
            v.push_back(z);
        }
        return v;
    }
};

void print_call(const Session& t, const Call& k) {
    printf("{\"op\":\"%s\",", k.op.c_str());
    num("arg", k.arg), num("predict", k.predict);
    printf("\"refused\":\"%s\",\"launches\":[", k.refused.c_str());
    for (size_t i = 0; i < k.launches.size(); ++i) {
        const Launch& l = k.launches[i];
        printf("%s{", i ? "," : "");
        num("launched", l.launched), num("flush", l.flush), num("mlaunch", l.mlaunch), num("take", l.take), num("maxpend", l.maxpend);
        num("mx", l.mx), num("uniform", l.uniform), num("priming", l.priming);
        list("at", l.at), list("nc", l.nc);
        printf("\"desc\":[");
        for (size_t s = 0; s < l.desc.size(); ++s) {
            const LiveStream& d = l.desc[s];
            printf("%s[%lld,%lld,%d,%d,%d,%d]", s ? "," : "", d.j0, d.newbase, d.frames, d.newcount, d.out_at, d.flush);
        }
        printf("],\"steps\":[");
        for (int j = 0; j < (l.launched ? l.steps.count : 0); ++j) {
            const LiveStep& st = l.steps.step[j];
            printf("%s[%d,%d,%d,%d,%d,%d]", j ? "," : "", st.what, st.band, st.groups, st.ncol, (int)st.defer, (int)st.ingest);
        }
        printf("]}");
    }
    printf("],");
    list("counts", k.counts), list("first", k.first);
    list("fed", t.c.fed), list("emitted", t.c.emitted), list("seen", t.c.seen), list("newbase", t.c.newbase), list("pend", t.c.pend);
    list("pending", t.pending()), list("cleared", t.cleared());
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
            Shape sh;
            int cell, cols;
            if (!sh.read(w) || !(w >> cell >> cols)) continue;
            printf("%s", sep);
            print_geometry(sh, cell, cols);
        } else if (cmd == "compat") {
            Shape open, asked;
            std::string bar;
            if (!open.read(w) || !(w >> bar) || bar != "|" || !asked.read(w) || open.error() || asked.error()) return 2;
            const char* why = live_mismatch(live_session(open.ask()), asked.ask());
            printf("%s{\"why\":\"%s\"}", sep, why ? why : "");
        } else if (cmd == "trace") {
            std::string op;
            long long a = 0, b = 0;
            if (!(w >> op)) continue;
            if (op == "open") {
                Shape sh;
                if (!sh.read(w) || sh.error()) return 2;
                t.open(sh);
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
