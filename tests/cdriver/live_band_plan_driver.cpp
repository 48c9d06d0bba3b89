// live_band_plan_driver.cpp — runs em-spec_amd/csrc/emspec_live_band_plan.h without a GPU: the geometry of a live multi-band session,
// and scripted sessions as emspec_live.cpp runs them with every HIP call left out, the staging copies done into host blocks of
// exactly the header's sizes so that a wrong offset is ASan's to report.  Prints JSON.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/live_band_plan_driver.cpp -o live_band_plan_driver
// tests/test_live_band_plan_cpu.py compares the output with tests/live_band_ref.py (and, for the calls, tests/live_ref.py).
//   geometry FILE   one session per line: S hop reassign form R cell K n[0..K) split[0..K-1)
//                   -> a list of objects: "error" (the rule broken, or "") and, when accepted, every field and byte size;
//                      for K = 2 also what live_geometry(n[0], n[1], split[0]) gives ("two")
//   trace FILE      first line: open S hop reassign form R K n.. split..; then frame | flush | push COUNT DIRECT | predict COUNT |
//                   reset STREAM -> one object per call: the columns it reports, and per launch the bands' workgroups per stream
#include "emspec_live_band_plan.h"

#include <cstdio>
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
    int S = 0, hop = 0, reassign = 0, form = 0, R = 0, cell = 4, K = 0;
    int32_t n[8] = {}, split[8] = {};
    bool read(std::istringstream& w, bool with_cell) {
        if (!(w >> S >> hop >> reassign >> form >> R)) return false;
        if (with_cell && !(w >> cell)) return false;
        if (!(w >> K) || K < 0 || K > 8) return false;
        for (int k = 0; k < K; ++k)
            if (!(w >> n[k])) return false;
        for (int k = 0; k + 1 < K; ++k)
            if (!(w >> split[k])) return false;
        return true;
    }
    const char* error() const {
        if (const char* why = band_shape_error(K, n, hop)) return why;
        return band_split_error(K, split, R);
    }
};

void print_geometry(const Shape& sh) {
    const char* why = sh.error();
    printf("{\"error\":\"%s\"", why ? why : "");
    if (why) { printf("}"); return; }
    const LiveBandGeometry m = live_band_geometry(sh.S, band_plan(sh.K, sh.n, sh.split, sh.hop, sh.R), sh.hop, sh.reassign, sh.form);
    const LiveGeometry& g = m.g;
    printf(",");
    num("S", g.S), num("n", g.n), num("hop", g.hop), num("reassign", g.reassign), num("D", g.D), num("form", g.form);
    num("mmax", g.mmax), num("cap", g.cap), num("ring_mask", g.ring_mask), num("n_high", g.n_high), num("bands", m.bands);
    num("sring_bytes", g.sring_bytes()), num("desc_bytes", g.desc_bytes()), num("fresh_bytes", g.fresh_bytes());
    num("out1_bytes", g.out_bytes(sh.R, 1)), num("done_bytes", m.done_bytes());
    std::vector<long long> bn, lo, hi, shift, D, fs, le, slots, ring, rings, prime;
    for (int k = 0; k < m.bands; ++k) {
        const LiveBand& b = m.b[k];
        bn.push_back(b.n), lo.push_back(b.lo), hi.push_back(b.hi), shift.push_back(b.shift), D.push_back(b.D);
        fs.push_back(b.frame_shift), le.push_back(b.lat_extra), slots.push_back(b.slots);
        ring.push_back((long long)m.ring_bytes(k, sh.cell)), rings.push_back((long long)m.rings_bytes(k, sh.cell));
        prime.push_back(m.launch_frames(k, 3, true) - m.launch_frames(k, 3, false));
    }
    list("band_n", bn), list("lo", lo), list("hi", hi), list("shift", shift), list("band_D", D), list("frame_shift", fs);
    list("lat_extra", le), list("slots", slots), list("ring_bytes", ring), list("rings_bytes", rings), list("priming_extra", prime);
    num("defers_1", m.defers(1, kInlineFinalize)), num("defers_2", m.defers(2, kInlineFinalize));
    num("defers_3", m.defers(3, kInlineFinalize), "");
    if (sh.K == 2) {
        const LiveGeometry t = live_geometry(sh.S, sh.n[0], sh.hop, sh.reassign, sh.form, sh.n[1], sh.split[0]);
        printf(",\"two\":{");
        num("D", t.D), num("mmax", t.mmax), num("cap", t.cap), num("ring_mask", t.ring_mask), num("slots", t.slots);
        num("slots_high", t.slots_high), num("shift", t.shift), num("D_high", t.D_high), num("split", t.split);
        num("ring_bytes", t.ring_bytes(sh.R, sh.cell)), num("ring_high_bytes", t.ring_high_bytes(sh.R, sh.cell));
        num("rings_bytes", t.rings_bytes(sh.R, sh.cell)), num("rings_high_bytes", t.rings_high_bytes(sh.R, sh.cell));
        num("sring_bytes", t.sring_bytes()), num("desc_bytes", t.desc_bytes()), num("fresh_bytes", t.fresh_bytes());
        num("done_bytes", t.done_bytes(), "}");
    }
    printf("}");
}

// ---- a scripted session: emspec_live.cpp's calls on the two headers ----
struct Launch {
    bool launched = true, flush = false;
    int mx = 0;
    bool priming = false, defer = false;
    std::vector<int> groups;   // per band: workgroups per stream of its frame launch without the ingest workgroup; -1: not launched
    int kernels = 0;           // launches in all: the bands' frame launches + the bands finalize
};
struct Call {
    std::string op, refused;
    int64_t arg = 0, predict = -1;
    std::vector<Launch> launches;
    std::vector<int64_t> counts, first;
};

struct Session {
    LiveBandGeometry m;
    LiveCounters c;
    std::vector<LiveStream> desc;
    std::vector<float> fresh, block;
    std::vector<std::vector<unsigned char>> rings;   // band k's [S] rings, one byte per cell: what emspec_reset_stream clears

    void open(const Shape& sh) {
        m = live_band_geometry(sh.S, band_plan(sh.K, sh.n, sh.split, sh.hop, sh.R), sh.hop, sh.reassign, sh.form);
        c.open(sh.S);
        desc.assign(m.g.desc_bytes() / sizeof(LiveStream), LiveStream{});
        fresh.assign(m.g.fresh_bytes() / 4, 0.0f);
        rings.clear();
        for (int k = 0; k < m.bands; ++k) rings.emplace_back(m.rings_bytes(k, 1), (unsigned char)1);
    }
    // live_launch's sequence for a multi-band session
    Launch seen(int mlaunch, bool flush) const {
        Launch l;
        l.flush = flush, l.mx = mlaunch;
        l.priming = live_priming(desc.data(), m.g.S);
        l.defer = !flush && m.defers(mlaunch, kInlineFinalize);
        for (int k = 0; k < m.bands; ++k) {
            const bool run = !flush && (k == 0 || mlaunch > 0);
            l.groups.push_back(run ? m.launch_frames(k, mlaunch, l.priming) : -1);
            l.kernels += run ? 1 : 0;
        }
        if (flush || (l.defer && mlaunch > 0)) l.kernels += 1;
        return l;
    }
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
        Call k;
        k.op = "push", k.arg = count;
        if (!(k.refused = refusal()).empty()) return k;
        k.predict = predict(count);
        block.assign((size_t)count, 1.0f);
        LivePush p(m.g.S);
        while (p.used < count) {
            live_push_take(m.g, c, p, count);
            for (int s = 0; s < m.g.S; ++s)
                std::memcpy(fresh.data() + m.g.fresh_at(s, c.pend[s]), block.data() + p.used, (size_t)p.take * 4);
            Launch l;
            l.launched = live_push_round(m.g, c, p, direct, desc.data());
            if (l.launched) {
                l = seen(p.mx, false);
                live_push_commit(m.g, c, p);
            } else {
                l.mx = p.mx;
            }
            k.launches.push_back(l);
        }
        k.counts = p.produced, k.first = p.first;
        return k;
    }
    Call reset(int s) {
        Call k;
        k.op = "reset", k.arg = s;
        for (int b = 0; b < m.bands; ++b)   // emspec_reset_stream: every band's ring of the stream
            std::memset(rings[b].data() + (size_t)s * m.ring_bytes(b, 1), 0, m.ring_bytes(b, 1));
        c.reset_stream(s);
        return k;
    }
};

void print_call(const Session& t, const Call& k) {
    printf("{\"op\":\"%s\",", k.op.c_str());
    num("arg", k.arg), num("predict", k.predict);
    printf("\"refused\":\"%s\",\"launches\":[", k.refused.c_str());
    for (size_t i = 0; i < k.launches.size(); ++i) {
        const Launch& l = k.launches[i];
        printf("%s{", i ? "," : "");
        num("launched", l.launched), num("flush", l.flush), num("mx", l.mx), num("priming", l.priming), num("defer", l.defer);
        list("groups", l.groups);
        num("kernels", l.kernels, "}");
    }
    printf("],");
    list("counts", k.counts), list("first", k.first);
    std::vector<long long> cleared;   // per band: streams whose ring is all zero
    for (int b = 0; b < t.m.bands; ++b) {
        long long z = 0;
        for (int s = 0; s < t.m.g.S; ++s) {
            const size_t per = t.m.ring_bytes(b, 1);
            bool zero = true;
            for (size_t i = 0; i < per && zero; ++i) zero = t.rings[b][(size_t)s * per + i] == 0;
            z += zero ? 1 : 0;
        }
        cleared.push_back(z);
    }
    list("cleared", cleared);
    list("fed", t.c.fed), list("emitted", t.c.emitted), list("seen", t.c.seen, "}");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: see the head of live_band_plan_driver.cpp\n"); return 2; }
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
            if (!sh.read(w, true)) continue;
            printf("%s", sep);
            print_geometry(sh);
        } else if (cmd == "trace") {
            std::string op;
            long long a = 0, b = 0;
            if (!(w >> op)) continue;
            if (op == "open") {
                Shape sh;
                if (!sh.read(w, false) || sh.error()) return 2;
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
