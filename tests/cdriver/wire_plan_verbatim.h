// wire_plan_verbatim.h — the host arithmetic of the gather and of its wire image AS IT WAS in emspec_comm.cpp, emspec_api.cpp,
// emspec_host.cpp and pack.hip.inc before it moved into em-spec_amd/csrc/emspec_wire_plan.h: the statements are the old ones,
// cut out of their functions and given the surrounding variables as arguments (c->h_sizes is `h_sizes`, e->cfg.rows is `R`).
// It is the generator of tests/golden/gather_plans.json (wire_plan_driver.cpp with -DWIRE_PLAN_VERBATIM) and is not part of the
// library: do not bring it up to date.
#pragma once
#include "../../include/emspec.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace wire_verbatim {

// ---- pack.hip.inc, host side ----
constexpr uint32_t kWireMagic = 0x32574D45u;   // "EMW2" little-endian
constexpr int kWireHeader = 32;
inline int wire_mask_words(int rows) { return (rows + 31) >> 5; }
inline int64_t wire_fixed_bytes(int64_t columns, int rows) {      // header + offsets + masks
    return kWireHeader + columns * 4 + columns * (int64_t)wire_mask_words(rows) * 4;
}
inline int64_t wire_bound_bytes(int64_t columns, int rows) { return wire_fixed_bytes(columns, rows) + columns * (int64_t)rows + 32; }
inline size_t wire_scratch_bytes(int64_t columns) {   // counts/local offsets + block sums + total (pack side only)
    return (((size_t)columns * 4 + 255) & ~(size_t)255) + (((size_t)((columns + 1023) / 1024) * 4 + 255) & ~(size_t)255) + 256;
}
struct WireScratch { uint32_t* local; uint32_t* bsum; uint64_t* total; };
inline WireScratch wire_scratch_split(void* scratch, int64_t columns) {
    char* p = static_cast<char*>(scratch);
    WireScratch w;
    w.local = reinterpret_cast<uint32_t*>(p); p += ((size_t)columns * 4 + 255) & ~(size_t)255;
    w.bsum = reinterpret_cast<uint32_t*>(p); p += ((size_t)((columns + 1023) / 1024) * 4 + 255) & ~(size_t)255;
    w.total = reinterpret_cast<uint64_t*>(p);
    return w;
}
// wire_scan_b_kernel: what the device publishes as an image's size
inline uint64_t image_total_bytes(int64_t fixed_bytes, uint64_t payload) { return (uint64_t)fixed_bytes + ((payload + 15) & ~(uint64_t)15); }

// ---- the three header checks.  h: the image's first 8 dwords ----
// emspec_wire_unpack (emspec_comm.cpp): true = "wire image does not match this engine's rows / the column count"
inline bool unpack_refuses(const uint32_t* h, int64_t wire_bytes, int64_t columns, int R) {
    const uint64_t hcols = (uint64_t)h[2] | ((uint64_t)h[3] << 32), hpay = (uint64_t)h[4] | ((uint64_t)h[5] << 32);
    const int64_t need = wire_fixed_bytes(columns, R) + (int64_t)((hpay + 15) & ~(uint64_t)15);
    if (h[0] != 0x32574D45u /* "EMW2" */ || (int32_t)h[1] != R || hcols != (uint64_t)columns || hpay > (uint64_t)columns * R ||
        wire_bytes < need)
        return true;
    return false;
}
// drain() (emspec_host.cpp): true = "the packed image of a stream carries a bad header"; *bytes: what is copied out otherwise
inline bool drain_refuses(const uint32_t* h, int64_t Cr, int R, int64_t* bytes_out) {
    const uint64_t hcols = (uint64_t)h[2] | ((uint64_t)h[3] << 32), hpay = (uint64_t)h[4] | ((uint64_t)h[5] << 32);
    if (h[0] != 0x32574D45u || (int32_t)h[1] != R || hcols != (uint64_t)Cr || hpay > (uint64_t)Cr * R) {
        return true;
    }
    const int64_t bytes = wire_fixed_bytes(Cr, R) + (int64_t)((hpay + 15) & ~(uint64_t)15);
    *bytes_out = bytes;
    return false;
}
// emspec_wire_unpack_host (emspec_api.cpp), whole
inline int emspec_wire_unpack_host(const uint8_t* wire, int64_t wire_bytes, int64_t columns, int32_t rows, uint8_t* index_out) {
    if (!wire || !index_out || columns < 1 || rows < 1 || wire_bytes < 32) return EMSPEC_ERR_INVALID_ARG;
    uint32_t h[8];
    memcpy(h, wire, 32);
    const uint64_t hcols = (uint64_t)h[2] | ((uint64_t)h[3] << 32), hpay = (uint64_t)h[4] | ((uint64_t)h[5] << 32);
    const int mw = (rows + 31) >> 5;
    const int64_t fixed = 32 + columns * 4 + columns * (int64_t)mw * 4;
    if (h[0] != 0x32574D45u || (int32_t)h[1] != rows || hcols != (uint64_t)columns || hpay > (uint64_t)columns * (uint64_t)rows ||
        wire_bytes < fixed + (int64_t)hpay)
        return EMSPEC_ERR_INVALID_ARG;
    const uint8_t* offp = wire + 32;
    const uint8_t* maskp = offp + columns * 4;
    const uint8_t* pay = wire + fixed;
    for (int64_t c = 0; c < columns; ++c) {
        uint32_t off;
        memcpy(&off, offp + c * 4, 4);
        uint8_t* dst = index_out + c * (int64_t)rows;
        memset(dst, 0, (size_t)rows);
        uint64_t at = off;
        for (int w = 0; w < mw; ++w) {
            uint32_t m;
            memcpy(&m, maskp + (c * mw + w) * 4, 4);
            while (m) {
                const int bit = __builtin_ctz(m);
                m &= m - 1;
                const int r = w * 32 + bit;
                if (r >= rows || at >= hpay) return EMSPEC_ERR_INVALID_ARG;   // a damaged image must not write or read out of range
                dst[r] = pay[at++];
            }
        }
    }
    return EMSPEC_OK;
}

// ---- emspec_gather_columns (emspec_comm.cpp), in the order of its body ----
struct Roles { bool is_root, loopback, packed, i_send, i_pack; };
inline Roles roles(int me, int root, uint32_t flags) {
    const bool is_root = me == root;
    const bool loopback = (flags & EMSPEC_GATHER_LOOPBACK) != 0;   // the root's own columns take the wire too (tests)
    const bool packed = (flags & EMSPEC_GATHER_PACKED) != 0;       // the root keeps the images packed (no expand)
    const bool i_send = !is_root || loopback;
    const bool i_pack = i_send || packed;                          // packed: the root's own columns become an image too
    return Roles{is_root, loopback, packed, i_send, i_pack};
}
// the rank-local argument rules; local_rc / local_msg as the body leaves them
inline void local_checks(const uint8_t* index_dev, int64_t columns, int32_t root, int world, bool is_root, const uint8_t* gathered_dev, int R,
                         int& local_rc, std::string& local_msg) {
    local_rc = EMSPEC_OK;
    auto local_fail = [&](int code, const std::string& msg) { if (local_rc == EMSPEC_OK) { local_rc = code; local_msg = msg; } };
    if (!index_dev || columns < 1) local_fail(EMSPEC_ERR_INVALID_ARG, "null argument / no columns");
    else if (root < 0 || root >= world) local_fail(EMSPEC_ERR_INVALID_ARG, "root out of range");
    else if (is_root && !gathered_dev) local_fail(EMSPEC_ERR_INVALID_ARG, "the root needs the gathered buffer");
    else if ((uint64_t)columns * (uint64_t)R >= (1ull << 32)) local_fail(EMSPEC_ERR_INVALID_ARG, "at most 2^32 cells per call");
}
constexpr uint64_t kRankFailed = ~0ull;   // in the (bytes, columns) pair of the size exchange: "this rank cannot take part"
// after the exchange: the message of the EMSPEC_ERR_COMM the body returns, or "" when it goes on
inline std::string pairs_error(const uint64_t* h_sizes, int world, int R) {
    for (int r = 0; r < world; ++r)
        if (h_sizes[2 * r] == kRankFailed)
            return "rank " + std::to_string(r) + " failed before the exchange: no columns were transferred";
    for (int r = 0; r < world; ++r) {
        const uint64_t bytes_r = h_sizes[2 * r], cols_r = h_sizes[2 * r + 1];
        if (cols_r < 1 || cols_r * (uint64_t)R >= (1ull << 32) || bytes_r > (uint64_t)wire_bound_bytes((int64_t)cols_r, R))
            return "a rank announced an impossible wire image (column count / size)";
    }
    return "";
}
struct Layout { std::vector<size_t> off, dst_off; size_t dir_bytes, need_cap, recv_grow; bool fits; std::vector<uint64_t> dir, packed_layout; };
inline Layout layout(const uint64_t* h_sizes, int world, int R, bool is_root, bool packed, int64_t gathered_capacity) {
    std::vector<size_t> off((size_t)world + 1, 0), dst_off((size_t)world + 1, 0);
    const size_t dir_bytes = packed ? ((sizeof(uint64_t) * 4 * (size_t)world + 255) & ~(size_t)255) : 0;
    if (is_root) {
        for (int r = 0; r < world; ++r) {
            off[r + 1] = off[r] + (((size_t)h_sizes[2 * r] + 255) & ~(size_t)255);
            dst_off[r + 1] = dst_off[r] + (size_t)h_sizes[2 * r + 1] * R;
        }
    }
    const size_t recv_grow = off[world] + 256;   // (both grow() calls of d_recv ask for this)
    const size_t need_cap = packed ? dir_bytes + off[world] : dst_off[world];
    const bool fits = !is_root || need_cap <= (size_t)(gathered_capacity > 0 ? gathered_capacity : 0);
    // the directory of the packed form (written by the root when it fits)
    std::vector<uint64_t> packed_layout, dirv((size_t)world * 4, 0);
    packed_layout.assign((size_t)world * 3, 0);
    uint64_t* dir = dirv.data();
    for (int r = 0; r < world; ++r) {
        dir[4 * r] = packed_layout[3 * r] = (uint64_t)(dir_bytes + off[r]);
        dir[4 * r + 1] = packed_layout[3 * r + 1] = h_sizes[2 * r];
        dir[4 * r + 2] = packed_layout[3 * r + 2] = h_sizes[2 * r + 1];
        dir[4 * r + 3] = 0;
    }
    return Layout{off, dst_off, dir_bytes, need_cap, recv_grow, fits, dirv, packed_layout};
}
// the pieces of one image's ncclSend / ncclRecv: (offset, count)
inline std::vector<std::pair<size_t, size_t>> pieces(uint64_t image_bytes) {
    std::vector<std::pair<size_t, size_t>> out;
    constexpr size_t kMaxTransfer = (size_t)1 << 30;
    for (size_t o = 0, nbytes = (size_t)image_bytes; o < nbytes; o += kMaxTransfer)
        out.push_back({o, std::min(kMaxTransfer, nbytes - o)});
    return out;
}

// ---- emspec_batch_gather: the staging block, from a base pointer ----
struct Staging { size_t need; char *d_pcm, *d_idx, *d_db, *d_all; };
inline Staging staging(char* d_stage, int S, int64_t L, size_t cells, bool db_local, bool is_root, int world) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t need = al((size_t)S * L * 4) + al(cells) + (db_local ? al(cells * 4) : 0) + (is_root ? al(cells * world) : 0) + 256;
    char* base = d_stage;
    float* d_pcm = (float*)base; base += al((size_t)S * L * 4);
    uint8_t* d_idx = (uint8_t*)base; base += al(cells);
    float* d_db = nullptr;
    if (db_local) { d_db = (float*)base; base += al(cells * 4); }
    uint8_t* d_all = is_root ? (uint8_t*)base : nullptr;
    return Staging{need, (char*)d_pcm, (char*)d_idx, (char*)d_db, (char*)d_all};
}
}  // namespace wire_verbatim
