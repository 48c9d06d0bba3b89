// row_lookup_driver.cpp — runs the decision of the FAST kernels' hinted row lookup (em-spec_amd/csrc/emspec_row_hint.h:
// row_hint_offset, row_hint, row_from_hint - the functions HintLookup calls on the device) against a binary search of the same
// float32 table, without a GPU.  The table and the predicate are emspec_tables.h's.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/row_lookup_driver.cpp -o row_lookup_driver
// float32 arguments are given as the hex of their bits (f:).
//   sweep N rows f:sample_rate f:fmin f:fmax     every probe value x hint displaced by -1/4, 0, +1/4 row x logarithm moved by
//                                                -1, 0, +1 float32 ulp: counts, and the first mismatches
//   densest N rows f:sample_rate f:fmax          the largest float32 fmin hint_rows_ok admits (bisection), then the same sweep
//   rows N rows f:sample_rate f:fmin f:fmax      the table, the probe values and the undisturbed lookup's row of each, as bits
// Probe values: every edge and its float32 neighbours up to 4 ulp either way, the row midpoints, values below e0 (a neighbour, a
// half, a tiny one, 0, a negative one), values at or above eR (Nyquist N / 2, beyond it, a huge one, +inf) and a NaN.
// The table lives in a heap block of exactly rows + 1 floats: a read past either end is ASan's to report.
#include "emspec_row_hint.h"
#include "emspec_tables.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

using namespace emspec;

namespace {

float f32_arg(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }
uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float step(float x, int ulps) {
    for (int i = 0; i < std::abs(ulps); ++i) x = std::nextafter(x, ulps > 0 ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity());
    return x;
}

std::vector<float> probe_values(const std::vector<float>& eb, int n) {
    const int R = (int)eb.size() - 1;
    std::vector<float> v;
    for (int r = 0; r <= R; ++r)
        for (int d = -4; d <= 4; ++d) v.push_back(step(eb[r], d));
    for (int r = 0; r < R; ++r) v.push_back((float)(0.5 * ((double)eb[r] + (double)eb[r + 1])));
    const float inf = std::numeric_limits<float>::infinity();
    for (float x : {eb[0] * 0.999f, eb[0] * 0.5f, 1.0e-30f, 0.0f, -1.0f}) v.push_back(x);
    for (float x : {(float)n * 0.5f, (float)n * 0.5f + 0.5f, eb[R] * 1.001f, eb[R] * 2.0f, 1.0e30f, inf}) v.push_back(x);
    v.push_back(std::numeric_limits<float>::quiet_NaN());
    return v;
}

// the reference: bisection of the table, -1 below it (and for a NaN, which no row holds), R at or above its end
int bisect_row(const std::vector<float>& eb, float kh) {
    if (kh != kh) return -1;
    return (int)(std::upper_bound(eb.begin(), eb.end(), kh) - eb.begin()) - 1;
}

struct Hint {   // HintLookup::init, on the host's log2f
    float l2e0, rscale, c0;
    explicit Hint(const std::vector<float>& eb) {
        const int R = (int)eb.size() - 1;
        l2e0 = std::log2(eb[0]);
        rscale = (float)R / (std::log2(eb[R]) - l2e0);
        c0 = row_hint_offset(l2e0, rscale);
    }
};

// log2 of kh, correctly rounded to float32, moved by `ulps` neighbours (v_log_f32 is documented to 1 ulp)
float log2_moved(float kh, int ulps) { return step((float)std::log2((double)kh), ulps); }

std::vector<float> table(int n, int rows, float sr, float fmin, float fmax, std::vector<double>* e64_out = nullptr) {
    emspec_config c{};
    c.rows = rows, c.sample_rate = sr, c.fmin_hz = fmin, c.fmax_hz = fmax;
    const std::vector<double> e64 = edges_bin64(axis_of(c, {}), n);
    if (e64_out) *e64_out = e64;
    std::vector<float> e32 = edges_bin32(e64);
    e32.shrink_to_fit();
    return e32;
}

int sweep(int n, int rows, float sr, float fmin, float fmax) {
    std::vector<double> e64;
    const std::vector<float> eb = table(n, rows, sr, fmin, fmax, &e64);
    const char* err = edges_error(eb);
    const int ok = hint_rows_ok(e64.front(), e64.back(), rows) ? 1 : 0;
    const double l0 = spec_log2(e64.front()), lR = spec_log2(e64.back());
    const double value = 8.0 * ((double)rows / (lR - l0)) * std::max(1.0, std::max(std::fabs(l0), std::fabs(lR))) + 2.0 * (double)rows;
    printf("hint_ok %d\nbound_ratio %.9f\nerror32 %s\n", ok, value / 2097152.0, err ? err : "-");
    const int R = rows;
    const Hint h(eb);
    const std::vector<float> kh = probe_values(eb, n);
    long long cases = 0, mismatches = 0, range_bad = 0, in_range = 0, below = 0, above = 0;
    for (float k : kh) {
        const int want = bisect_row(eb, k);
        const bool inside = k >= eb[0] && k < eb[R];
        for (int ulps = -1; ulps <= 1; ++ulps) {
            const float f0 = row_hint(log2_moved(k, ulps), h.rscale, h.c0);
            for (int q = -1; q <= 1; ++q) {
                const int got = row_from_hint(f0 + 0.25f * (float)q, k, eb.data(), R);
                ++cases;
                in_range += inside, below += want == -1, above += want == R;
                if (((unsigned)got < (unsigned)R) != inside) ++range_bad;
                if (got != want && ++mismatches <= 8)
                    printf("mismatch kh %08x ulps %d quarter %d got %d want %d\n", bits(k), ulps, q, got, want);
            }
        }
    }
    printf("cases %lld\nmismatches %lld\nrange_bad %lld\nin_range %lld\nbelow %lld\nabove %lld\n", cases, mismatches, range_bad, in_range, below, above);
    return 0;
}

int usage() { fprintf(stderr, "usage: see the head of row_lookup_driver.cpp\n"); return 2; }

}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "sweep" && argc == 7) {
        return sweep(atoi(argv[2]), atoi(argv[3]), f32_arg(argv[4]), f32_arg(argv[5]), f32_arg(argv[6]));
    } else if (cmd == "densest" && argc == 6) {
        const int n = atoi(argv[2]), rows = atoi(argv[3]);
        const float sr = f32_arg(argv[4]), fmax = f32_arg(argv[5]);
        auto admits = [&](float fmin) {
            std::vector<double> e64;
            table(n, rows, sr, fmin, fmax, &e64);
            return hint_rows_ok(e64.front(), e64.back(), rows);
        };
        float lo = fmax * 0.01f, hi = fmax * 0.9999f;
        if (!admits(lo) || admits(hi)) { fprintf(stderr, "the bound is not between %g and %g Hz\n", lo, hi); return 3; }
        while (std::nextafter(lo, hi) < hi) {
            const float mid = (float)(0.5 * ((double)lo + (double)hi));
            (admits(mid) ? lo : hi) = mid;
        }
        printf("fmin %08x\n", bits(lo));
        return sweep(n, rows, sr, lo, fmax);
    } else if (cmd == "rows" && argc == 7) {
        const int n = atoi(argv[2]), rows = atoi(argv[3]);
        const std::vector<float> eb = table(n, rows, f32_arg(argv[4]), f32_arg(argv[5]), f32_arg(argv[6]));
        const Hint h(eb);
        const std::vector<float> kh = probe_values(eb, n);
        printf("e32");
        for (float e : eb) printf(" %08x", bits(e));
        printf("\nkh");
        for (float k : kh) printf(" %08x", bits(k));
        printf("\nrow");
        for (float k : kh) printf(" %d", row_from_hint(row_hint(log2_moved(k, 0), h.rscale, h.c0), k, eb.data(), rows));
        printf("\n");
    } else {
        return usage();
    }
    return 0;
}
