// tables_driver.cpp — prints what em-spec_amd/csrc/emspec_tables.h computes for the case on its command line: the tables, the
// specified evaluations, the palettes and the per-shape scalars, as lines of "name value value ..." with every floating-point
// value as the hex of its bit pattern.  No GPU, no library: only the header.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I em-spec_amd/csrc \
//       tests/cdriver/tables_driver.cpp -o tables_driver
// tests/test_tables_cpu.py compares the output with the bit models (oracle/) and with numpy restatements.
// float32 arguments are given as the hex of their bits (f:), so nothing depends on how a decimal string is parsed.
//   twiddles N
//   edges N rows f:sample_rate f:fmin f:fmax [file of rows + 1 raw float32 Hz edges]
//   hint N rows f:sample_rate f:fmin f:fmax     hint_rows_ok of the log axis' table, its ends, and whether the float32 edges serve
//   pow d:ratio R                       spec_pow(ratio, r / R), r = 0 .. R
//   palette | colormap f:brightness | warped rows f:fmin f:fmax f:boost f:scale
//   scalars N hop reassign rows f:sample_rate f:fmin f:fmax f:gain f:db_top f:db_range f:gate_db f:power_floor
#include "emspec_tables.h"

#include <cstdio>
#include <cstdlib>
#include <string>

using namespace emspec;

namespace {

float f32_arg(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }
double f64_arg(const char* s) { const uint64_t u = strtoull(s, nullptr, 16); double d; memcpy(&d, &u, 8); return d; }
void put(float f) { uint32_t u; memcpy(&u, &f, 4); printf(" %08x", u); }
void put(double d) { uint64_t u; memcpy(&u, &d, 8); printf(" %016llx", (unsigned long long)u); }
void put(int i) { printf(" %d", i); }
template <class T> void line(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (const T& x : v) put(x);
    printf("\n");
}
template <class T> void line(const char* name, T x) { line(name, std::vector<T>{x}); }
void bytes(const char* name, const uint8_t* p, int count) {
    printf("%s", name);
    for (int i = 0; i < count; ++i) printf(" %02x", p[i]);
    printf("\n");
}

// the custom table lives in a heap block of exactly its size: a read past its end is ASan's to report
std::vector<float> read_edges(const char* path, int count) {
    std::vector<float> hz((size_t)count);
    FILE* f = fopen(path, "rb");
    if (!f || fread(hz.data(), sizeof(float), (size_t)count, f) != (size_t)count) { fprintf(stderr, "cannot read %d edges from %s\n", count, path); exit(2); }
    fclose(f);
    return hz;
}

int usage() { fprintf(stderr, "usage: see the head of tables_driver.cpp\n"); return 2; }

}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "twiddles" && argc == 3) {
        const int n = atoi(argv[2]);
        line("tw32", twiddles32(n));
        line("tw64", twiddles64(n));
    } else if (cmd == "edges" && (argc == 7 || argc == 8)) {
        const int n = atoi(argv[2]), rows = atoi(argv[3]);
        const std::vector<float> custom = argc == 8 ? read_edges(argv[7], rows + 1) : std::vector<float>();
        emspec_config c{};
        c.rows = rows, c.sample_rate = f32_arg(argv[4]), c.fmin_hz = f32_arg(argv[5]), c.fmax_hz = f32_arg(argv[6]);
        const Axis axis = axis_of(c, custom);
        const std::vector<double> e64 = edges_bin64(axis, n);
        const std::vector<float> e32 = edges_bin32(e64);
        std::vector<double> hz;
        std::vector<int> low;
        for (int r = 0; r <= rows; ++r) hz.push_back(edge_hz(axis, r)), low.push_back(low_share_ok(axis, r) ? 1 : 0);
        line("hz", hz);
        line("e64", e64);
        line("e32", e32);
        line("low_share_ok", low);
        const char *w32 = edges_error(e32), *w64 = edges_error(e64);
        printf("error32 %s\nerror64 %s\n", w32 ? w32 : "-", w64 ? w64 : "-");
    } else if (cmd == "hint" && argc == 7) {
        const int n = atoi(argv[2]);
        emspec_config c{};
        c.rows = atoi(argv[3]), c.sample_rate = f32_arg(argv[4]), c.fmin_hz = f32_arg(argv[5]), c.fmax_hz = f32_arg(argv[6]);
        const std::vector<double> e64 = edges_bin64(axis_of(c, {}), n);
        line("ok", hint_rows_ok(e64.front(), e64.back(), c.rows) ? 1 : 0);
        line("e0", e64.front()), line("eR", e64.back());
        const char* w32 = edges_error(edges_bin32(e64));
        printf("error32 %s\n", w32 ? w32 : "-");
    } else if (cmd == "pow" && argc == 4) {
        const double ratio = f64_arg(argv[2]);
        const int R = atoi(argv[3]);
        std::vector<double> v;
        for (int r = 0; r <= R; ++r) v.push_back(spec_pow(ratio, (double)r / (double)R));
        line("pow", v);
    } else if (cmd == "palette" && argc == 2) {
        std::vector<uint8_t> lut(1024);
        default_lut(lut.data());
        bytes("lut", lut.data(), 1024);
    } else if (cmd == "colormap" && argc == 3) {
        std::vector<uint8_t> lut(1024);
        make_colormap(f32_arg(argv[2]), lut.data());
        bytes("lut", lut.data(), 1024);
    } else if (cmd == "warped" && argc == 7) {
        const int rows = atoi(argv[2]);
        std::vector<float> hz((size_t)rows + 1);
        warped_edges_hz(rows, f32_arg(argv[3]), f32_arg(argv[4]), f32_arg(argv[5]), f32_arg(argv[6]), hz.data());
        line("hz", hz);
    } else if (cmd == "scalars" && argc == 14) {
        const int n = atoi(argv[2]), hop = atoi(argv[3]), reassign = atoi(argv[4]);
        emspec_config c{};
        c.rows = atoi(argv[5]), c.sample_rate = f32_arg(argv[6]), c.fmin_hz = f32_arg(argv[7]), c.fmax_hz = f32_arg(argv[8]);
        c.gain = f32_arg(argv[9]), c.db_top = f32_arg(argv[10]), c.db_range = f32_arg(argv[11]), c.gate_db = f32_arg(argv[12]);
        c.power_floor = f32_arg(argv[13]);
        const std::vector<double> e64 = edges_bin64(axis_of(c, {}), n);
        const PlanScalars p = plan_scalars(c, c.rows, true, n, hop, reassign);
        const ExactScalars x = exact_scalars(n, p.rows, p.pfloor, e64.front(), e64.back());
        const DbScalars m = db_scalars(c, n), xm = exact_db_scalars(c, n, x.qscale);
        line("ints", std::vector<int>{p.rows, p.log_rows, p.D, p.reassign, p.hop, latency(n, hop, reassign)});
        line("tscale32", p.tscale32), line("pfloor_abs", p.pfloor_abs);
        line("tscale", p.tscale), line("pfloor", p.pfloor), line("pmax", x.pmax), line("qscale", x.qscale);
        line("pfloor64", x.pfloor64), line("pmax64", x.pmax64), line("qscale64", x.qscale64);
        line("e0", e64.front()), line("eR", e64.back()), line("l2e0", x.l2e0), line("rscale", x.rscale);
        line("db", std::vector<float>{m.scale, m.lo, m.inv_range, m.gate});
        line("exact_db", std::vector<float>{xm.scale, xm.lo, xm.inv_range, xm.gate});
    } else {
        return usage();
    }
    return 0;
}
