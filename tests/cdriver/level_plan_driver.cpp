// level_plan_driver.cpp — pins the level meters' plan header (em-spec_amd/csrc/emspec_level_plan.h) and their rows of the host
// pipeline's plan (emspec_pipe_plan.h: kLevel, kCross, cross_span_of) without a GPU:
//   1. the quantiser against an integer evaluation from the bits written here, on the edges and on random bits;
//   2. the limb bounds: 2^30 saturated samples leave every limb of a level and of a cross record (both signs) inside 64 bits,
//      and the limbs still compose to the exact sum;
//   3. the combine: the record of a random signal is that of any split into pieces, combined in any grouping;
//   4. the pipeline table: with the rows cleared a set has the layout it had, with them set the new arrays lie behind the
//      stereo rows, and the pieces of all units cover the caller's [S V][Cr] level and [S][Cr] cross records exactly once.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I em-spec_amd/csrc tests/cdriver/level_plan_driver.cpp -o level_plan_driver
// Prints "ok <quantised> <splits> <plans>" and returns 0, or prints the first violation and returns 1 (tests/test_level_cpu.py).
#include "emspec_level_plan.h"
#include "emspec_pipe_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

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

long long quantised = 0, splits = 0, plans = 0;

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

}  // namespace

int main() {
    static_assert(sizeof(emspec_level) == 24 && alignof(emspec_level) == 8 && sizeof(emspec_cross) == 16 && alignof(emspec_cross) == 8, "record sizes");
    if (!check_quantiser() || !check_limbs() || !check_combine()) return 1;
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
    printf("ok %lld %lld %lld\n", quantised, splits, plans);
    return 0;
}
