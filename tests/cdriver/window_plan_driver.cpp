// window_plan_driver.cpp — pins the window walk's plan header (em-spec_amd/csrc/emspec_window_plan.h) and the level meters' rows of
// the host pipeline's plan (emspec_pipe_plan.h: kLevel, kCross, cross_span_of) without a GPU:
//   1. the quantiser against an integer evaluation from the bits written here, on the edges and on random bits;
//   2. the limb bounds: 2^30 saturated samples leave every limb of a level and of a cross record (both signs) inside 64 bits,
//      and the limbs still compose to the exact sum;
//   3. the combine: the record of a random signal is that of any split into pieces, combined in any grouping;
//   4. the pipeline table: with the rows cleared a set has the layout it had, with them set the new arrays lie behind the
//      stereo rows, and the pieces of all units cover the caller's [S V][Cr] level and [S][Cr] cross records exactly once;
//   5. the scan the kernels run (window_scan) for the three reducers: the lanes of every team size, combined, against the plain
//      loop of one sample at a time, on heap blocks that end with the window (and start with it where the alignment allows), so
//      that the sanitizer sees a read outside [a, b), and a filler in front that every reducer shows;
//   6. the split: the pieces tile each window, those past a short last window's end are empty, and the pieces' results merged
//      in either order are the window's;
//   7. the team rule on its edges.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I em-spec_amd/csrc tests/cdriver/window_plan_driver.cpp -o window_plan_driver
// Prints "ok <quantised> <splits> <plans> <scans> <pieces>" and returns 0, or prints the first violation and returns 1
// (tests/test_level_cpu.py).
#include "emspec_window_plan.h"
#include "emspec_pipe_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include <algorithm>

using namespace emspec;

namespace {

#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            printf("FAIL " __VA_ARGS__); \
            printf("\n");                \
            return false;                \
        }                                \
    } while (0)

// the definition from the bits, in integers: x 2^24 = M 2^(e - 126)
int64_t k_of_bits(uint32_t u, uint32_t& odd) {
    const uint32_t e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    const bool neg = u >> 31;
    int64_t k;
    if (e == 255 && m) { odd += 1; return 0; }
    if (e >= 134) { odd += 1; k = 0x7fffffff; }
    else if (e == 0) k = 0;
    else {
        const int64_t M = m | 0x800000u;
        const int sh = (int)e - 126;
        if (sh >= 0) k = M << sh;
        else if (-sh > 25) k = 0;
        else {
            const int r = -sh;
            const int64_t q = M >> r, rem = M & (((int64_t)1 << r) - 1), half = (int64_t)1 << (r - 1);
            k = q + ((rem > half || (rem == half && (q & 1))) ? 1 : 0);
        }
    }
    return neg ? -k : k;
}
uint32_t bits_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

// The definition on host arrays, one window of x[0 .. count): one sample at a time
template <class Red> typename Red::Acc plain(const uint32_t* xa, const uint32_t* xb, int64_t count) {
    typename Red::Acc r = Red::start();
    for (int64_t i = 0; i < count; ++i) Red::take(r, xa[i], Red::kStreams == 2 ? xb[i] : 0);
    return r;
}
emspec_level level_of(const uint32_t* x, int64_t count) { return plain<LevelRed>(x, x, count); }
emspec_cross cross_of(const uint32_t* xa, const uint32_t* xb, int64_t count) { return plain<CrossRed>(xa, xb, count); }

long long quantised = 0, splits = 0, plans = 0, scans = 0, pieces = 0;

bool check_quantiser() {
    auto one = [](uint32_t u) {
        uint32_t o1 = 0, o2 = 0;
        const int64_t want = k_of_bits(u, o1), got = level_quantise(u, o2);
        ++quantised;
        return want == got && o1 == o2;
    };
    // every exponent with a few mantissas, both signs
    for (uint32_t e = 0; e < 256; ++e)
        for (uint32_t m : {0u, 1u, 2u, 0x3fffffu, 0x400000u, 0x400001u, 0x7ffffeu, 0x7fffffu, 0x200000u, 0x600000u, 0x100000u, 0x300000u})
            for (uint32_t s : {0u, 0x80000000u}) CHECK(one(s | (e << 23) | m), "quantiser at e=%u m=%#x", e, m);
    std::mt19937 rng(24);
    for (int i = 0; i < 2000000; ++i) {
        const uint32_t u = rng();
        CHECK(one(u), "quantiser at bits %#x", u);
    }
    // ties around small integers: (j + 0.5) 2^-24 goes to the even neighbour
    for (int j = 0; j < 4096; ++j) {
        uint32_t odd = 0;
        const int32_t k = level_quantise(bits_of(std::ldexp((float)j + 0.5f, -24)), odd);
        CHECK(k == (j % 2 ? j + 1 : j) && odd == 0, "tie at %d.5 gave %d", j, k);
    }
    uint32_t odd = 0;
    CHECK(level_quantise(bits_of(std::ldexp(1.0f, -25)), odd) == 0 && level_quantise(bits_of(std::nextafterf(std::ldexp(1.0f, -25), 1.0f)), odd) == 1, "2^-25");
    CHECK(level_quantise(bits_of(std::nextafterf(128.0f, 0.0f)), odd) == 0x7fffff80 && odd == 0, "128 - ulp");
    CHECK(level_quantise(bits_of(-128.0f), odd) == -0x7fffffff && odd == 1, "-128");
    return true;
}

bool check_limbs() {
    // 2^30 saturated samples, by doubling a record: q = (2^31 - 1)^2
    emspec_level one = {0, 0, 0, 0};
    level_take(one, bits_of(INFINITY));
    const unsigned __int128 q = (unsigned __int128)0x7fffffffu * 0x7fffffffu;
    CHECK((((unsigned __int128)one.sq_hi << 32) + one.sq_lo) == q && one.peak == kLevelMax && one.odd == 1, "one saturated sample");
    emspec_level r = one;
    emspec_cross cp = {0, 0}, cn = {0, 0};
    cross_take(cp, bits_of(INFINITY), bits_of(1e30f));
    cross_take(cn, bits_of(-INFINITY), bits_of(200.0f));
    for (int d = 0; d < 30; ++d) {
        level_combine(r, emspec_level(r));
        cross_combine(cp, emspec_cross(cp));
        cross_combine(cn, emspec_cross(cn));
    }
    const unsigned __int128 N = (unsigned __int128)1 << 30;
    CHECK(r.odd == (uint32_t)N && r.peak == kLevelMax, "odd count of 2^30 samples");
    CHECK(r.sq_lo == (uint64_t)(q & 0xffffffffu) * (uint64_t)N && r.sq_hi == (uint64_t)(q >> 32) * (uint64_t)N, "limbs of 2^30 saturated squares");
    CHECK(r.sq_lo < ((uint64_t)1 << 62) && r.sq_hi < ((uint64_t)1 << 62), "a level limb reaches 2^62");
    CHECK((((unsigned __int128)r.sq_hi << 32) + r.sq_lo) == q * N, "the limbs do not compose to the sum");
    const __int128 sp = (__int128)cp.hi * ((__int128)1 << 32) + (__int128)cp.lo, sn = (__int128)cn.hi * ((__int128)1 << 32) + (__int128)cn.lo;
    CHECK(sp == (__int128)(q * N) && sn == -(__int128)(q * N), "cross limbs of 2^30 saturated products");
    CHECK(cp.lo < ((uint64_t)1 << 62) && cn.lo < ((uint64_t)1 << 62) && cp.hi < ((int64_t)1 << 61) && cn.hi >= -((int64_t)1 << 61), "a cross limb out of range");
    CHECK(kLevelWindowMax == (int64_t)N, "the longest window");
    return true;
}

bool check_combine() {
    std::mt19937 rng(7);
    std::vector<uint32_t> a(5000), b(5000);
    for (size_t i = 0; i < a.size(); ++i) {
        // a mix of ordinary samples, large ones, tiny ones and raw bit patterns
        const int kind = (int)(rng() % 8);
        auto draw = [&]() -> uint32_t {
            if (kind == 0) return rng();
            const float v = std::ldexp((float)((int)(rng() % 2000001) - 1000000) / 1000000.0f, kind == 1 ? 6 : kind == 2 ? -20 : 0);
            return bits_of(v);
        };
        a[i] = draw(); b[i] = draw();
    }
    const emspec_level whole = level_of(a.data(), (int64_t)a.size());
    const emspec_cross cwhole = cross_of(a.data(), b.data(), (int64_t)a.size());
    for (int t = 0; t < 300; ++t) {
        // random cut points, pieces combined left to right, right to left and pairwise
        std::vector<size_t> cut = {0, a.size()};
        for (int c = (int)(rng() % 9); c > 0; --c) cut.push_back(rng() % (a.size() + 1));
        std::sort(cut.begin(), cut.end());
        std::vector<emspec_level> pl; std::vector<emspec_cross> pc;
        for (size_t i = 0; i + 1 < cut.size(); ++i) {
            pl.push_back(level_of(a.data() + cut[i], (int64_t)(cut[i + 1] - cut[i])));
            pc.push_back(cross_of(a.data() + cut[i], b.data() + cut[i], (int64_t)(cut[i + 1] - cut[i])));
        }
        emspec_level l1 = {0, 0, 0, 0}, l2 = {0, 0, 0, 0};
        emspec_cross c1 = {0, 0}, c2 = {0, 0};
        for (size_t i = 0; i < pl.size(); ++i) { level_combine(l1, pl[i]); cross_combine(c1, pc[i]); }
        for (size_t i = pl.size(); i-- > 0;) { emspec_level x = pl[i]; level_combine(x, l2); l2 = x; emspec_cross y = pc[i]; cross_combine(y, c2); c2 = y; }
        while (pl.size() > 1) {   // pairwise, as a butterfly does
            std::vector<emspec_level> nl; std::vector<emspec_cross> nc;
            for (size_t i = 0; i < pl.size(); i += 2) {
                emspec_level x = pl[i]; emspec_cross y = pc[i];
                if (i + 1 < pl.size()) { level_combine(x, pl[i + 1]); cross_combine(y, pc[i + 1]); }
                nl.push_back(x); nc.push_back(y);
            }
            pl = nl; pc = nc;
        }
        for (const emspec_level* g : {&l1, &l2, &pl[0]}) CHECK(std::memcmp(g, &whole, sizeof whole) == 0, "a split's level record differs (trial %d)", t);
        for (const emspec_cross* g : {&c1, &c2, &pc[0]}) CHECK(std::memcmp(g, &cwhole, sizeof cwhole) == 0, "a split's cross record differs (trial %d)", t);
        ++splits;
    }
    // a stream against itself: the cross limbs are the level's
    const emspec_cross self = cross_of(a.data(), a.data(), (int64_t)a.size());
    CHECK(self.lo == whole.sq_lo && (uint64_t)self.hi == whole.sq_hi, "a == b does not reproduce the level's sums");
    return true;
}

bool check_plan(int S, int V, int64_t L, int n, int hop, int f, int target, bool whole) {
    const int R = 64, D = (n + 2 * hop - 1) / (2 * hop);
    const int64_t C = L < n ? 0 : (L - n) / hop + 1, Cr = (C + f - 1) / f;
    OutRow set[kOutRows] = {}, plain[kOutRows] = {};
    set[kIdx].unit = plain[kIdx].unit = 1;
    set[kWave].unit = plain[kWave].unit = sizeof(emspec_wave);
    set[kLevel].unit = sizeof(emspec_level);
    set[kCross].unit = V > 1 ? sizeof(emspec_cross) : 0;
    const size_t in_s = (size_t)L * 4;
    const size_t per_stream = per_stream_bytes(set, in_s, V > 1 ? in_s * V : 0, V, C, Cr, R, 0, f);
    const std::vector<PipeItem> items = pipe_items(S, L, C, n, hop, D, per_stream, !whole, target, f);
    const Stage g = stage_layout(items, R, set, 0, V, V > 1 ? 4 : 0, f), g0 = stage_layout(items, R, plain, 0, V, V > 1 ? 4 : 0, f);
    CHECK(kLevel == kSRgba + 1 && kCross == kLevel + 1 && kOutRows == kCross + 1, "the new rows are not behind the stereo rows");
    for (int a = 0; a <= 15; ++a) CHECK(g.off(a) == g0.off(a), "an offset in front of the level records moved (array %d)", a);
    CHECK(g0.level == 0 && g0.cross == 0 && g0.bytes() == g0.off(15), "cleared rows take room");
    CHECK(g.out_off(kLevel) == g0.bytes() && g.out_off(kCross) == g0.bytes() + g.level && g.bytes() == g0.bytes() + g.level + g.cross, "offsets of the new rows");
    CHECK(g.out_off(kLevel) % 8 == 0 && g.out_off(kCross) % 8 == 0 && g.bytes() % 8 == 0, "alignment of the new rows");
    static char stage[1];
    const Set q = g.at(stage, 2), q0 = g0.at(stage, 2);
    CHECK((char*)q.level == stage + 2 * g.bytes() + g.out_off(kLevel) && q0.level == nullptr && q0.cross == nullptr, "Stage::at (level)");
    CHECK(V > 1 ? (char*)q.cross == stage + 2 * g.bytes() + g.out_off(kCross) : q.cross == nullptr, "Stage::at (cross)");
    std::vector<int> lhit((size_t)S * V * Cr, 0), chit((size_t)S * Cr, 0);
    for (const PipeItem& it : items) {
        const WaveRun wr = wave_run_of(it, n, hop, f);
        CHECK((size_t)wr.pairs * it.sc * V * sizeof(emspec_level) <= g.level, "the unit's level records do not fit");
        CHECK(V == 1 || (size_t)wr.pairs * it.sc * sizeof(emspec_cross) <= g.cross, "the unit's cross records do not fit");
        for (int k = 0; k < spans_of(it, C, V); ++k) {
            const Span ws = wave_span_of(it, C, V, k, f);
            CHECK(ws.from + ws.cells <= (size_t)wr.pairs * it.sc * V && ws.to + ws.cells <= lhit.size(), "a level piece out of range");
            for (size_t i = 0; i < ws.cells; ++i) ++lhit[ws.to + i];
        }
        const Span cs = cross_span_of(it, C, f);
        CHECK(cs.from + cs.cells <= (size_t)wr.pairs * it.sc && cs.to + cs.cells <= chit.size(), "a cross piece out of range");
        CHECK(it.cn == C || it.sc == 1, "a run of columns holds more than one source");
        for (size_t i = 0; i < cs.cells; ++i) {
            const size_t us = (cs.from + i) / (size_t)wr.pairs, ug = (cs.from + i) % (size_t)wr.pairs;
            CHECK(cs.to + i == ((size_t)it.s0 + us) * Cr + (size_t)(it.c0 / f) + ug, "a cross record goes to another source or group");
            ++chit[cs.to + i];
        }
    }
    for (int h : lhit) CHECK(h == 1, "a level record of the caller's array is not written exactly once");
    for (int h : chit) CHECK(h == 1, "a cross record of the caller's array is not written exactly once");
    ++plans;
    return true;
}

// ---- 5. the scan.  A heap block of `pad` + count samples, 16-byte aligned: the window starts pad samples in (its start alignment)
// and ends with the block, so the sanitizer sees every read behind it and, without a pad, in front of it.  A read of the pad
// itself stays inside the block; the filler shows it.  Two kinds of window: every kind of sample (+0.0, -0.0, the infinities,
// NaN of both signs, denormals, |x| >= 128, ordinary values) in front of a saturated filler, which a level or a cross record
// that took one shows in its odd count or its sum; and `plain`, ordinary values below 1 only, in front of a filler of both
// infinities, which lies outside the window's range, so that the envelope shows it too.
struct Block {
    uint32_t* base = nullptr; const uint32_t* x = nullptr;
    Block(int pad, int64_t count, std::mt19937& rng, bool plain = false) {
        void* p = nullptr;
        if (posix_memalign(&p, 16, (size_t)(pad + count) * 4 + (pad + count == 0))) abort();
        base = static_cast<uint32_t*>(p);
        for (int i = 0; i < pad; ++i) base[i] = !plain ? 0x7f7fffffu : i % 2 ? 0xff800000u : 0x7f800000u;
        static const uint32_t special[] = {0u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x00000001u, 0x807fffffu,
                                           0x43000000u, 0xc3000001u, 0x7f7fffffu, 0x3f800000u, 0xbf800000u};
        for (int64_t i = 0; i < count; ++i) {
            const uint32_t v = rng();
            base[pad + i] = v % 4 == 0 && !plain ? special[(v >> 8) % (sizeof special / 4)]
                                                 : bits_of(std::ldexp((float)((int)((v >> 4) % 2000001) - 1000000) / 1000000.0f, v % 4 == 1 ? -20 : 0));
        }
        x = base + pad;
    }
    ~Block() { free(base); }
    Block(const Block&) = delete;
};

template <class Red> bool check_scan(const char* name) {
    std::mt19937 rng(11);
    std::vector<int64_t> lengths;
    for (int64_t n = 0; n <= 70; ++n) lengths.push_back(n);
    for (int64_t n : {255, 256, 257, 1027, 16384}) lengths.push_back(n);
    for (int64_t n : lengths)
        for (int pa = 0; pa < 4; ++pa)
            for (int pb = 0; pb < (Red::kStreams == 2 ? 8 : 2); ++pb) {   // (B's start alignment, and both kinds of window)
                const Block A(pa, n, rng, pb & 1), B(pb >> 1, Red::kStreams == 2 ? n : 0, rng, pb & 1);
                const typename Red::Acc want = plain<Red>(A.x, B.x, n);
                for (int T : {1, 2, 4, 8, 16, 32, 64, 256}) {
                    typename Red::Acc got = Red::start();
                    for (int l = 0; l < T; ++l) {
                        typename Red::Acc r = Red::start();
                        window_scan<Red>(A.x, B.x, 0, n, l, T, r);
                        Red::combine(got, r);
                    }
                    CHECK(std::memcmp(&got, &want, sizeof want) == 0, "%s: the scan of %lld samples by %d lanes differs (alignments %d, %d)", name, (long long)n, T, pa, pb >> 1);
                    ++scans;
                }
            }
    return true;
}

// ---- 6. the split: a launch of `cols` columns of hop samples in groups of f, from `first` on
template <class Red> bool check_pieces(const char* name, const uint32_t* xa, const uint32_t* xb, int64_t first, int64_t cols, int64_t hop, int64_t f, int64_t want_ppw) {
    const int64_t longest = window_longest(f, cols, hop), ppw = window_pieces(longest), Cr = (cols + f - 1) / f;
    CHECK(longest > kWindowSplit && ppw == want_ppw, "%s: %lld pieces per window of %lld samples", name, (long long)ppw, (long long)longest);
    for (int64_t g = 0; g < Cr; ++g) {
        const WindowSpan w = window_of(g, f, cols, hop, first);
        CHECK(w.a == first + g * f * hop && w.b == first + std::min((g + 1) * f, cols) * hop, "%s: window %lld", name, (long long)g);
        std::vector<typename Red::Acc> part;
        int64_t at = w.a;
        for (int64_t p = 0; p < ppw; ++p) {
            const WindowSpan ps = window_piece(w, p);
            CHECK(ps.a <= ps.b && ps.b - ps.a <= kWindowPiece && ps.b <= w.b, "%s: piece %lld of window %lld", name, (long long)p, (long long)g);
            if (at < w.b) CHECK(ps.a == at && (ps.b == w.b || ps.b - ps.a == kWindowPiece), "%s: the pieces of window %lld do not tile it", name, (long long)g);
            else CHECK(ps.a == ps.b, "%s: a piece past the end of window %lld is not empty", name, (long long)g);
            at = ps.b > at ? ps.b : at;
            typename Red::Acc r = Red::start();
            window_scan<Red>(xa, xb, ps.a, ps.b, 0, 1, r);
            part.push_back(r);
            ++pieces;
        }
        CHECK(at == w.b, "%s: the pieces of window %lld end at %lld, not %lld", name, (long long)g, (long long)at, (long long)w.b);
        typename Red::Acc fwd = Red::start(), bwd = Red::start();
        for (size_t i = 0; i < part.size(); ++i) { Red::combine(fwd, part[i]); Red::combine(bwd, part[part.size() - 1 - i]); }
        const typename Red::Acc want = plain<Red>(xa + w.a, xb + w.a, w.b - w.a);
        CHECK(std::memcmp(&fwd, &want, sizeof want) == 0 && std::memcmp(&bwd, &want, sizeof want) == 0, "%s: the merged pieces of window %lld differ from one pass", name, (long long)g);
    }
    return true;
}
bool check_split() {
    std::mt19937 rng(13);
    // windows of 76,800 samples, two pieces each, in front of a last one of 2,560; of 65,537 in front of 65,535 (its second piece
    // is empty); of 65,536 (one piece) in front of one sample
    const int64_t geoms[3][5] = {{3, 610, 256, 300, 2}, {1, 65537 + 65535, 1, 65537, 2}, {2, 2 * 65536 + 1, 1, 65536, 1}};
    for (auto& g : geoms) {
        const Block A(0, g[0] + g[1] * g[2], rng), B(1, g[0] + g[1] * g[2], rng);
        if (!check_pieces<EnvelopeRed>("envelope", A.x, A.x, g[0], g[1], g[2], g[3], g[4]) || !check_pieces<LevelRed>("level", A.x, A.x, g[0], g[1], g[2], g[3], g[4]) ||
            !check_pieces<CrossRed>("cross", A.x, B.x, g[0], g[1], g[2], g[3], g[4]))
            return false;
    }
    const WindowSpan last = window_of(2, 300, 610, 256, 0);
    CHECK(last.b - last.a == 2560 && window_longest(300, 610, 256) == 76800, "the short last window");
    return true;
}

// ---- 7. the team rule: the largest power of two up to 64 that leaves a lane 16 samples or more (T 32 <= longest doubles T)
bool check_team() {
    const int64_t edges[9][2] = {{1, 1}, {31, 1}, {32, 2}, {63, 2}, {64, 4}, {2047, 64}, {2048, 64}, {16384, 64}, {16385, 64}};
    for (auto& e : edges) CHECK(window_team(e[0]) == e[1], "window_team(%lld) = %d", (long long)e[0], window_team(e[0]));
    for (int64_t n = 1; n <= 20000; ++n) {
        int T = 1;
        while (T < 64 && T * 32 <= n) T *= 2;
        CHECK(window_team(n) == T, "window_team(%lld)", (long long)n);
    }
    CHECK(kWindowBlock == 256 && kWindowSplit == 16384 && kWindowPiece == 65536, "the split constants");
    return true;
}

}  // namespace

int main() {
    static_assert(sizeof(emspec_level) == 24 && alignof(emspec_level) == 8 && sizeof(emspec_cross) == 16 && alignof(emspec_cross) == 8, "record sizes");
    if (!check_quantiser() || !check_limbs() || !check_combine()) return 1;
    if (!check_scan<EnvelopeRed>("envelope") || !check_scan<LevelRed>("level") || !check_scan<CrossRed>("cross") || !check_split() || !check_team()) return 1;
    const int shapes[4][2] = {{256, 1}, {1024, 255}, {4096, 256}, {16384, 512}};
    for (auto& sh : shapes)
        for (int S : {1, 3, 8})
            for (int V : {1, 4})
                for (int64_t extra : {(int64_t)0, (int64_t)7 * sh[1] + 5, (int64_t)70001 * sh[1] + 3})
                    for (int f : {1, 3, 4096, 65536})
                        for (int target : {1, 3, 16})
                            for (bool whole : {false, true}) {
                                if (extra > 4000000 && S * V > 8) continue;   // (keeps the hit maps small)
                                if (!check_plan(S, V, sh[0] + extra, sh[0], sh[1], f, target, whole)) return 1;
                            }
    printf("ok %lld %lld %lld %lld %lld\n", quantised, splits, plans, scans, pieces);
    return 0;
}
