// wire_plan_driver.cpp — prints the host arithmetic of the gather and of its wire image (em-spec_amd/csrc/emspec_wire_plan.h) for
// a list of cases as one JSON object: sizes, the scratch split, roles, argument rules, the check of the announced pairs, the
// root's layouts, transfer pieces, the staging of emspec_batch_gather and what the three header checks answer - without a GPU.
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I em-spec_amd/csrc tests/cdriver/wire_plan_driver.cpp -o wire_plan_driver
// tests/test_wire_plan_cpu.py compares the output with tests/golden/gather_plans.json.  With -DWIRE_PLAN_VERBATIM the same cases go
// through wire_plan_verbatim.h, the arithmetic as it was inside emspec_comm.cpp / emspec_api.cpp / emspec_host.cpp / pack.hip.inc:
// that build wrote the fixture.
//   wire_plan_driver images LIST: every line of LIST is "image-file columns rows out-file"; the image is expanded on the host
//   into out-file and then damaged in every way of damage_names; prints what the header checks answer to each.
#ifdef WIRE_PLAN_VERBATIM
#include "wire_plan_verbatim.h"
namespace W = wire_verbatim;
#else
#include "emspec_wire_plan.h"
namespace W = emspec;
#endif

#include <array>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

using u64 = unsigned long long;
using i64 = long long;

// ---- one shape for both headers: what each caller in the library does with them ----
// (Library build: unpack_host() and answers() below restate the callers' own glue - the null / size checks of the extern "C"
// emspec_wire_unpack_host, emspec_wire_unpack's `wire_bytes >= padded`, drain()'s use of the predicate alone - because each
// caller keeps its own length rule and lives in a file that needs HIP.  What is pinned here is the header's functions; a slip
// in the glue of emspec_comm.cpp / emspec_api.cpp / emspec_host.cpp itself shows in the GPU tests, tests/test_gpu_wire_cases.py
// and tests/test_gpu_host.py.)
struct Roles { bool is_root, i_send, i_pack; };
struct Scratch { size_t local, bsum, total, bytes; };
struct Layout { std::vector<size_t> off, dst_off; std::vector<uint64_t> dir; size_t dir_bytes, need, recv_bytes; bool fits; };
struct Stage { i64 pcm, idx, db, all; size_t bytes; };   // (-1: no such array)
struct Answers { int match, unpack_ok, host_rc, drain_ok; i64 drain_bytes; };
using Pieces = std::vector<std::pair<size_t, size_t>>;

#ifdef WIRE_PLAN_VERBATIM
Roles roles(int me, int root, uint32_t flags) { const auto r = W::roles(me, root, flags); return {r.is_root, r.i_send, r.i_pack}; }
Scratch scratch(int64_t columns) {
    static char base[1];
    const auto w = W::wire_scratch_split(base, columns);
    return {(size_t)((char*)w.local - base), (size_t)((char*)w.bsum - base), (size_t)((char*)w.total - base), W::wire_scratch_bytes(columns)};
}
std::string arg_error(bool index, int64_t columns, int root, int world, bool is_root, bool gathered, int R, int* code) {
    static const uint8_t some[1] = {0};
    std::string msg;
    W::local_checks(index ? some : nullptr, columns, root, world, is_root, gathered ? some : nullptr, R, *code, msg);
    return msg;
}
std::string pairs_error(const uint64_t* pairs, int world, int R) { return W::pairs_error(pairs, world, R); }
Layout layout(const uint64_t* pairs, int world, int R, bool is_root, bool packed, int64_t capacity) {
    const auto l = W::layout(pairs, world, R, is_root, packed, capacity);
    for (int r = 0; r < world; ++r)   // what emspec_gather_packed_layout reported: the directory's first three of four
        for (int k = 0; k < 3; ++k)
            if (l.packed_layout[3 * r + k] != l.dir[4 * r + k]) abort();
    return {l.off, l.dst_off, l.dir, l.dir_bytes, l.need_cap, l.recv_grow, l.fits};
}
Pieces pieces(uint64_t bytes) { return W::pieces(bytes); }
Stage stage(int S, int64_t L, size_t cells, bool db, bool is_root, int world) {
    static char base[1];
    const auto s = W::staging(base, S, L, cells, db, is_root, world);
    return {s.d_pcm - base, s.d_idx - base, s.d_db ? s.d_db - base : -1, s.d_all ? s.d_all - base : -1, s.need};
}
size_t image_total(int64_t columns, int rows, uint64_t payload) { return (size_t)W::image_total_bytes(W::wire_fixed_bytes(columns, rows), payload); }
int unpack_host(const uint8_t* wire, int64_t n, int64_t columns, int rows, uint8_t* out) { return W::emspec_wire_unpack_host(wire, n, columns, rows, out); }
Answers answers(const uint8_t* wire, int64_t n, int64_t columns, int rows, uint8_t* out) {
    Answers a{0, 0, unpack_host(wire, n, columns, rows, out), 0, -1};
    if (n < 32) return a;   // (emspec_wire_unpack: "wire image shorter than its header"; drain() always has 32 bytes)
    uint32_t h[8];
    memcpy(h, wire, 32);
    a.unpack_ok = !W::unpack_refuses(h, n, columns, rows);
    int64_t bytes = -1;
    a.drain_ok = a.match = !W::drain_refuses(h, columns, rows, &bytes);
    a.drain_bytes = bytes;
    return a;
}
#else
Roles roles(int me, int root, uint32_t flags) { const auto r = W::gather_roles(me, root, flags); return {r.is_root, r.i_send, r.i_pack}; }
Scratch scratch(int64_t columns) { const auto w = W::wire_scratch_split(columns); return {w.local, w.bsum, w.total, W::wire_scratch_bytes(columns)}; }
std::string arg_error(bool index, int64_t columns, int root, int world, bool is_root, bool gathered, int R, int* code) {
    const W::PlanError e = W::gather_arg_error(index, columns, root, world, is_root, gathered, R);
    *code = e.code;
    return e.code ? e.msg : "";
}
std::string pairs_error(const uint64_t* pairs, int world, int R) {   // (the texts of emspec_gather_columns)
    const int bad = W::gather_pairs_check(pairs, world, R);
    if (bad >= 0) return "rank " + std::to_string(bad) + " failed before the exchange: no columns were transferred";
    return bad == W::kPairsImpossible ? "a rank announced an impossible wire image (column count / size)" : "";
}
Layout layout(const uint64_t* pairs, int world, int R, bool is_root, bool packed, int64_t capacity) {
    const auto l = W::gather_layout(pairs, world, R, is_root, packed, capacity);
    return {l.off, l.dst_off, W::gather_directory(l, pairs, world), l.dir_bytes, l.need, l.recv_bytes, l.fits};
}
Pieces pieces(uint64_t bytes) {
    Pieces p;
    W::for_transfer_pieces((size_t)bytes, [&](size_t o, size_t n) { p.push_back({o, n}); return true; });
    return p;
}
Stage stage(int S, int64_t L, size_t cells, bool db, bool is_root, int world) {
    const auto s = W::gather_stage((size_t)S * L * 4, cells, db, is_root, world);
    return {(i64)s.pcm, (i64)s.idx, db ? (i64)s.db : -1, is_root ? (i64)s.all : -1, s.bytes};
}
size_t image_total(int64_t columns, int rows, uint64_t payload) { return (size_t)W::wire_padded_bytes(columns, rows, payload); }
int unpack_host(const uint8_t* wire, int64_t n, int64_t columns, int rows, uint8_t* out) {   // (emspec_wire_unpack_host)
    if (!wire || !out || columns < 1 || rows < 1) return EMSPEC_ERR_INVALID_ARG;
    return W::wire_unpack_host(wire, n, columns, rows, out) ? EMSPEC_OK : EMSPEC_ERR_INVALID_ARG;
}
Answers answers(const uint8_t* wire, int64_t n, int64_t columns, int rows, uint8_t* out) {
    Answers a{0, 0, unpack_host(wire, n, columns, rows, out), 0, -1};
    if (n < 32) return a;
    const W::WireHeader h = W::wire_header(wire);
    a.match = W::wire_header_matches(h, columns, rows);
    a.unpack_ok = a.match && n >= W::wire_padded_bytes(columns, rows, h.payload);    // emspec_wire_unpack
    a.drain_ok = a.match;                                                            // drain()
    if (a.drain_ok) a.drain_bytes = W::wire_padded_bytes(columns, rows, h.payload);
    return a;
}
#endif

// ---- printing ----
bool g_first;
void open_list(const char* name, bool first_section = false) { printf("%s\"%s\": [", first_section ? "{\n" : ",\n", name); g_first = true; }
void item() { printf("%s", g_first ? "\n  " : ",\n  "); g_first = false; }
void close_list() { printf("\n]"); }
template <class T>
void print_vec(const char* name, const std::vector<T>& v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%llu", i ? ", " : "", (u64)v[i]);
    printf("]");
}

// an image size as a rank with `cols` columns of R rows announces it, with permille / 1000 of its cells non-zero
uint64_t announced(uint64_t cols, int R, int permille) {
    const uint64_t fixed = 32 + cols * 4 + cols * (uint64_t)((R + 31) / 32) * 4;
    return fixed + ((cols * R * permille / 1000 + 15) & ~(uint64_t)15);
}

void print_layout(const char* name, const std::vector<uint64_t>& pairs, int R, int root, int rank, bool packed, bool loopback, int cap_mode) {
    const int world = (int)pairs.size() / 2;
    const bool is_root = rank == root;
    // cap_mode: 0 exactly the need, 1 one byte less, 2 zero, 3 negative, 4 plenty
    const size_t need = layout(pairs.data(), world, R, is_root, packed, INT64_MAX).need;
    const int64_t cap = cap_mode == 0 ? (int64_t)need : cap_mode == 1 ? (int64_t)need - 1 : cap_mode == 2 ? 0 : cap_mode == 3 ? -4096 : (int64_t)need + 12345;
    const Layout l = layout(pairs.data(), world, R, is_root, packed, cap);
    item();
    printf("{\"case\": {\"name\": \"%s\", \"world\": %d, \"R\": %d, \"root\": %d, \"rank\": %d, \"packed\": %d, \"loopback\": %d, \"capacity\": %lld, ",
           name, world, R, root, rank, packed, loopback, (i64)cap);
    print_vec("pairs", pairs);
    printf("}, ");
    print_vec("off", l.off); printf(", ");
    print_vec("dst_off", l.dst_off); printf(", ");
    print_vec("dir", l.dir);
    printf(", \"dir_bytes\": %zu, \"need\": %zu, \"recv_bytes\": %zu, \"fits\": %d}", l.dir_bytes, l.need, l.recv_bytes, l.fits);
}

// shards of `counts` streams x cols_per x R; the root announces 0 bytes when it packs nothing
std::vector<uint64_t> shard_pairs(const std::vector<int>& counts, int cols_per, int R, int root, bool packed, bool loopback) {
    std::vector<uint64_t> p;
    for (size_t r = 0; r < counts.size(); ++r) {
        const uint64_t cols = (uint64_t)counts[r] * cols_per;
        p.push_back((int)r == root && !packed && !loopback ? 0 : announced(cols, R, 40 + 7 * (int)r));
        p.push_back(cols);
    }
    return p;
}

const char* const damage_names[] = {"intact", "magic", "rows+4", "rows-4", "columns+1", "columns-1", "payload=cells+1", "len31", "len32",
                                    "len=fixed+payload-1", "len=fixed+payload", "len=padded-1"};
// what the header checks answer to the image (n bytes; payload bytes of payload) damaged in every way; out: columns * rows bytes
void print_damaged(const uint8_t* image, size_t n, int64_t columns, int rows, uint64_t payload, uint8_t* out) {
    const size_t fixed = 32 + (size_t)columns * 4 * (1 + (size_t)((rows + 31) / 32));
    printf("{");
    for (size_t d = 0; d < sizeof(damage_names) / sizeof(*damage_names); ++d) {
        size_t len = n;
        uint32_t h[8];
        memcpy(h, image, 32);
        const uint64_t cells = (uint64_t)columns * rows;
        switch (d) {
            case 1: h[0] ^= 0x00010000u; break;
            case 2: h[1] += 4; break;
            case 3: h[1] -= 4; break;
            case 4: h[2] += 1; break;
            case 5: h[2] -= 1; break;
            case 6: h[4] = (uint32_t)(cells + 1); h[5] = (uint32_t)((cells + 1) >> 32); break;
            case 7: len = 31; break;
            case 8: len = 32; break;
            case 9: len = fixed + payload - 1; break;
            case 10: len = fixed + payload; break;
            case 11: len = n - 1; break;
        }
        // a copy of exactly `len` bytes, so that a read past what the caller handed over is seen
        uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
        memcpy(copy, image, len);
        memcpy(copy, h, len < 32 ? len : 32);
        const Answers a = answers(copy, (int64_t)len, columns, rows, out);
        free(copy);
        printf("%s\"%s\": [%d, %d, %d, %d, %lld]", d ? ", " : "", damage_names[d], a.match, a.unpack_ok, a.host_rc, a.drain_ok, a.drain_bytes);
    }
    printf("}");
}

int run_images(const char* list) {
    FILE* f = fopen(list, "r");
    if (!f) return 2;
    char path[4096], outpath[4096];
    i64 columns; int rows;
    open_list("images", true);
    while (fscanf(f, "%4095s %lld %d %4095s", path, &columns, &rows, outpath) == 4) {
        FILE* g = fopen(path, "rb");
        if (!g) return 2;
        std::vector<uint8_t> img;
        for (int ch; (ch = fgetc(g)) != EOF;) img.push_back((uint8_t)ch);
        fclose(g);
        std::vector<uint8_t> out((size_t)columns * rows, 0xCD);
        const int rc = unpack_host(img.data(), (int64_t)img.size(), columns, rows, out.data());
        g = fopen(outpath, "wb");
        if (!g || fwrite(out.data(), 1, out.size(), g) != out.size()) return 2;
        fclose(g);
        const uint64_t payload = img.size() >= 32 ? (uint64_t)img[16] | (uint64_t)img[17] << 8 | (uint64_t)img[18] << 16 | (uint64_t)img[19] << 24 : 0;
        item();
        printf("{\"columns\": %lld, \"rows\": %d, \"bytes\": %zu, \"payload\": %llu, \"rc\": %d, \"damaged\": ", columns, rows, img.size(), (u64)payload, rc);
        print_damaged(img.data(), img.size(), columns, rows, payload, out.data());
        printf("}");
    }
    fclose(f);
    close_list();
    printf("\n}\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "images") return run_images(argv[2]);
    const int64_t kMaxCols = ((int64_t)1 << 22) - 1;   // x 1024 rows: one under 2^32 cells
    const int rows_list[5] = {4, 64, 68, 1024, 4096};

    // ---- the size functions and the scratch split ----
    open_list("sizes", true);
    for (int R : rows_list)
        for (int64_t C : {(int64_t)1, (int64_t)7, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)70000, ((int64_t)1 << 20) - 1, kMaxCols}) {
            item();
            printf("{\"columns\": %lld, \"rows\": %d, \"mask_words\": %d, \"fixed\": %lld, \"bound\": %lld, \"padded\": [%zu, %zu, %zu, %zu]}", (i64)C, R,
                   W::wire_mask_words(R), (i64)W::wire_fixed_bytes(C, R), (i64)W::wire_bound_bytes(C, R), image_total(C, R, 0), image_total(C, R, 1),
                   image_total(C, R, 16), image_total(C, R, (uint64_t)C * R));
        }
    close_list();
    open_list("scratch");
    for (int64_t C : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)65536, (int64_t)65537, (int64_t)70000,
                      ((int64_t)1 << 20) + 1, kMaxCols}) {
        const Scratch s = scratch(C);
        item();
        printf("{\"columns\": %lld, \"local\": %zu, \"bsum\": %zu, \"total\": %zu, \"bytes\": %zu}", (i64)C, s.local, s.bsum, s.total, s.bytes);
    }
    close_list();

    // ---- roles ----
    open_list("roles");
    for (int root : {0, 2})
        for (int rank : {0, 1, 2})
            for (uint32_t flags : {0u, (uint32_t)EMSPEC_GATHER_LOOPBACK, (uint32_t)EMSPEC_GATHER_PACKED, (uint32_t)(EMSPEC_GATHER_LOOPBACK | EMSPEC_GATHER_PACKED), 0x80u}) {
                const Roles r = roles(rank, root, flags);
                item();
                printf("{\"rank\": %d, \"root\": %d, \"flags\": %u, \"is_root\": %d, \"i_send\": %d, \"i_pack\": %d}", rank, root, flags, r.is_root, r.i_send, r.i_pack);
            }
    close_list();

    // ---- the argument rules, each alone and each with every later one broken too (the earlier one wins) ----
    open_list("args");
    {
        struct A { bool index; int64_t columns; int root, world; bool is_root, gathered; int R; };
        const A ok{true, 100, 0, 4, true, true, 1024};
        auto show = [&](A a) {
            int code = 0;
            const std::string msg = arg_error(a.index, a.columns, a.root, a.world, a.is_root, a.gathered, a.R, &code);
            item();
            printf("{\"index\": %d, \"columns\": %lld, \"root\": %d, \"world\": %d, \"is_root\": %d, \"gathered\": %d, \"R\": %d, \"code\": %d, \"msg\": \"%s\"}",
                   a.index, (i64)a.columns, a.root, a.world, a.is_root, a.gathered, a.R, code, msg.c_str());
        };
        const int64_t big = (int64_t)1 << 22;   // x 1024 rows = 2^32 cells
        show(ok);
        for (int m = 1; m < 32; ++m) {   // bit 0: no index, 1: no columns, 2: root out of range, 3: root without buffer, 4: too many cells
            A a = ok;
            if (m & 1) a.index = false;
            if (m & 2) a.columns = 0;
            else if (m & 16) a.columns = big;
            if (m & 4) a.root = 4;
            if (m & 8) a.gathered = false;
            if ((m & 18) == 18) continue;   // (no columns and too many cells exclude each other)
            show(a);
        }
        A a = ok; a.root = -1; show(a);
        a = ok; a.is_root = false; a.gathered = false; show(a);          // only the root needs the buffer
        a = ok; a.columns = big - 1; show(a);                            // one column under the limit
        a = ok; a.columns = -3; show(a);
        a = ok; a.R = 4096; a.columns = (int64_t)1 << 20; show(a);       // 2^32 cells at 4096 rows
        a = ok; a.R = 4096; a.columns = ((int64_t)1 << 20) - 1; show(a);
        a = ok; a.world = 1; a.root = 1; show(a);
    }
    close_list();

    // ---- the check of the announced pairs ----
    open_list("pairs");
    {
        const int R = 1024;
        auto show = [&](const char* name, std::vector<uint64_t> p, int rows = 1024) {
            item();
            printf("{\"name\": \"%s\", \"R\": %d, ", name, rows);
            print_vec("pairs", p);
            printf(", \"error\": \"%s\"}", pairs_error(p.data(), (int)p.size() / 2, rows).c_str());
        };
        const std::vector<uint64_t> good = shard_pairs({3, 1, 2, 4}, 48, R, 0, false, false);
        const uint64_t failed = ~0ull;
        show("good", good);
        show("one rank", {announced(5, R, 60), 5});
        auto v = good; v[0] = failed; v[1] = 0; show("first failed", v);
        v = good; v[6] = failed; v[7] = 0; show("last failed", v);
        v = good; v[2] = failed; v[3] = 0; v[6] = failed; v[7] = 0; show("two failed", v);
        v = good; v[3] = 0; v[6] = failed; v[7] = 0; show("failed behind an impossible pair", v);
        v = good; v[3] = 0; show("cols = 0", v);
        v = good; v[5] = (uint64_t)1 << 22; show("cols * R = 2^32", v);
        v = good; v[5] = ((uint64_t)1 << 22) - 1; show("cols * R = 2^32 - R", v);
        v = good; v[5] = (uint64_t)1 << 40; show("cols * R = 2^50", v);
        v = good; v[4] = (uint64_t)W::wire_bound_bytes((int64_t)v[5], R); show("bytes = bound", v);
        v = good; v[4] = (uint64_t)W::wire_bound_bytes((int64_t)v[5], R) + 1; show("bytes = bound + 1", v);
        v = good; v[0] = 0; show("root announces 0", v);
        show("68 rows, bytes = bound", {(uint64_t)W::wire_bound_bytes(7, 68), 7, (uint64_t)W::wire_bound_bytes(9, 68), 9}, 68);
        show("68 rows, bytes = bound + 1", {(uint64_t)W::wire_bound_bytes(7, 68), 7, (uint64_t)W::wire_bound_bytes(9, 68) + 1, 9}, 68);
    }
    close_list();

    // ---- the root's layouts ----
    open_list("layouts");
    {
        const std::vector<int> mock = {3, 1, 2, 4, 2, 1, 3, 2};   // tests/test_gather.py: streams per rank, x 48 columns x 1024 rows
        for (int world : {1, 2, 3, 4, 8})
            for (int packed = 0; packed < 2; ++packed)
                for (int loopback = 0; loopback < 2; ++loopback) {
                    const std::vector<int> counts(mock.begin(), mock.begin() + world);
                    for (int cap_mode = 0; cap_mode < 5; ++cap_mode)
                        print_layout("mock shards", shard_pairs(counts, 48, 1024, 0, packed, loopback), 1024, 0, 0, packed, loopback, cap_mode);
                    print_layout("mock shards, not the root", shard_pairs(counts, 48, 1024, 0, packed, loopback), 1024, 0, world - 1 ? world - 1 : 5, packed, loopback, 2);
                }
        for (int root : {1, 2, 3})
            for (int packed = 0; packed < 2; ++packed)
                for (int cap_mode : {0, 1}) {
                    print_layout("root != 0", shard_pairs({2, 5, 1, 3}, 31, 68, root, packed, false), 68, root, root, packed, false, cap_mode);
                    print_layout("root != 0, 4096 rows", shard_pairs({1, 1, 7, 2}, 3, 4096, root, packed, true), 4096, root, root, packed, true, cap_mode);
                }
        // image sizes around the alignment and the transfer piece; columns such that each passes the pair check
        const uint64_t k277 = announced((uint64_t)kMaxCols, 1024, 517), bound_max = (uint64_t)W::wire_bound_bytes(kMaxCols, 1024);
        const uint64_t sizes[] = {0, 1, 255, 256, 257, (uint64_t)1 << 30, ((uint64_t)1 << 30) + 1, k277, bound_max};
        for (int packed = 0; packed < 2; ++packed) {
            std::vector<uint64_t> p;
            for (uint64_t s : sizes) { p.push_back(s); p.push_back(s > 4096 ? (uint64_t)kMaxCols : 8); }
            for (int cap_mode : {0, 1, 3}) print_layout("image sizes", p, 1024, 0, 0, packed, true, cap_mode);
            for (uint64_t s : sizes)
                print_layout("one image", {s, s > 4096 ? (uint64_t)kMaxCols : 8}, 1024, 0, 0, packed, true, 0);
        }
    }
    close_list();

    // ---- the pieces an image travels in ----
    open_list("pieces");
    {
        const uint64_t G = (uint64_t)1 << 30;
        for (uint64_t s : {(uint64_t)0, (uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)257, G - 1, G, G + 1, 2 * G, 2 * G + 1, announced((uint64_t)kMaxCols, 1024, 517),
                           (uint64_t)W::wire_bound_bytes(kMaxCols, 1024)}) {
            item();
            printf("{\"bytes\": %llu, \"pieces\": [", (u64)s);
            const Pieces p = pieces(s);
            for (size_t i = 0; i < p.size(); ++i) printf("%s[%zu, %zu]", i ? ", " : "", p[i].first, p[i].second);
            printf("]}");
        }
    }
    close_list();

    // ---- the staging block of emspec_batch_gather ----
    open_list("stage");
    for (int world : {1, 3, 8})
        for (int is_root = 0; is_root < 2; ++is_root)
            for (int db = 0; db < 2; ++db)
                for (auto& sh : std::vector<std::array<i64, 4>>{{1, 4096, 1, 1024}, {3, 16128, 48, 1024}, {2, 9001, 20, 68}, {5, 4096 + 256 * 299, 300, 500}, {256, 4198144, 16384, 1024}}) {
                    const int S = (int)sh[0]; const int64_t L = sh[1]; const size_t cells = (size_t)S * (size_t)sh[2] * (size_t)sh[3];
                    const Stage s = stage(S, L, cells, db, is_root, world);
                    item();
                    printf("{\"S\": %d, \"L\": %lld, \"cells\": %zu, \"db\": %d, \"is_root\": %d, \"world\": %d, \"pcm\": %lld, \"idx\": %lld, \"db_off\": %lld, \"all\": %lld, \"bytes\": %zu}",
                           S, (i64)L, cells, db, is_root, world, s.pcm, s.idx, s.db, s.all, s.bytes);
                }
    close_list();

    // ---- the header checks on images without a single non-zero cell but a payload field of every kind ----
    open_list("headers");
    for (auto& c : std::vector<std::array<i64, 3>>{{1, 64, 0}, {1, 64, 1}, {7, 68, 16}, {7, 68, 17}, {40, 1024, 40 * 1024}, {3, 4096, 31}, {300, 256, 5376}, {5, 4, 20}}) {
        const int64_t columns = c[0]; const int rows = (int)c[1]; const uint64_t payload = (uint64_t)c[2];
        const size_t n = image_total(columns, rows, payload);
        std::vector<uint8_t> img(n, 0), out((size_t)columns * rows);
        uint32_t h[8] = {0x32574D45u, (uint32_t)rows, (uint32_t)columns, 0, (uint32_t)payload, 0, 0, 0};
        memcpy(img.data(), h, 32);
        item();
        printf("{\"columns\": %lld, \"rows\": %d, \"payload\": %llu, \"bytes\": %zu, \"damaged\": ", (i64)columns, rows, (u64)payload, n);
        print_damaged(img.data(), n, columns, rows, payload, out.data());
        printf("}");
    }
    close_list();
    printf("\n}\n");
    return 0;
}
