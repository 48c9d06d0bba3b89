// emspec_wire_plan.h — internal: the host arithmetic of the gather's wire image (pack.hip.inc: its sizes, its header, the host
// expand) and the plan of the multi-GPU gather (emspec_comm.cpp: roles, argument rules, the check of the announced sizes, the
// root's layout of uneven shards, the transfer pieces, the staging of emspec_batch_gather).  No HIP, nothing of the engine:
// tests/test_wire_plan_cpu.py.
#pragma once
#include "../../include/emspec.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace emspec {

// ---- the wire image: header 32 B | offsets columns x u32 | masks columns x MW x u32 | payload, zero-padded to 16 B ----
constexpr uint32_t kWireMagic = 0x32574D45u;   // "EMW2" little-endian
constexpr int kWireHeader = 32;
constexpr int wire_mask_words(int rows) { return (rows + 31) >> 5; }   // (constexpr: the pack kernels call it too)

inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }   // the one 256-byte round-up of the host layer
inline int64_t wire_fixed_bytes(int64_t columns, int rows) {      // header + offsets + masks
    return kWireHeader + columns * 4 + columns * (int64_t)wire_mask_words(rows) * 4;
}
// (+ 32: the payload's zero padding to 16 B, and the <= 12 B of slack that bring an image's END to a 16-byte boundary when
// images are laid one after the other - the fixed part is a multiple of 4 only: emspec_batch_packed)
inline int64_t wire_bound_bytes(int64_t columns, int rows) { return wire_fixed_bytes(columns, rows) + columns * (int64_t)rows + 32; }
inline int64_t wire_padded_bytes(int64_t columns, int rows, uint64_t payload) {   // an image as the pack kernels leave it
    return wire_fixed_bytes(columns, rows) + (int64_t)((payload + 15) & ~(uint64_t)15);
}
// The pack workspace, as byte offsets: counts / local offsets, block sums (one per 1024 columns), the image's size (u64; the
// gather keeps the column count in the u64 behind it)
struct WireScratch { size_t local, bsum, total, bytes; };
inline WireScratch wire_scratch_split(int64_t columns) {
    const size_t bsum = al((size_t)columns * 4), total = bsum + al((size_t)((columns + 1023) / 1024) * 4);
    return WireScratch{0, bsum, total, total + 256};
}
inline size_t wire_scratch_bytes(int64_t columns) { return wire_scratch_split(columns).bytes; }

struct WireHeader { uint32_t magic; int32_t rows; uint64_t columns, payload; };
inline WireHeader wire_header(const void* dwords8) {   // (any alignment)
    uint32_t h[8];
    std::memcpy(h, dwords8, sizeof(h));
    return WireHeader{h[0], (int32_t)h[1], (uint64_t)h[2] | ((uint64_t)h[3] << 32), (uint64_t)h[4] | ((uint64_t)h[5] << 32)};
}
// "this header belongs to an image of (columns, rows)"; how long the image must be is each caller's own rule
inline bool wire_header_matches(const WireHeader& h, int64_t columns, int rows) {
    return h.magic == kWireMagic && h.rows == rows && h.columns == (uint64_t)columns && h.payload <= (uint64_t)columns * (uint64_t)rows;
}
// Image of (columns, rows) in wire[0 .. wire_bytes) -> index_out[columns][rows], on the host (emspec_wire_unpack_host: an image
// need not carry its pad).  False: not such an image, or a mask or an offset points out of range (a damaged image must not
// write or read out of range).
inline bool wire_unpack_host(const uint8_t* wire, int64_t wire_bytes, int64_t columns, int rows, uint8_t* index_out) {
    if (wire_bytes < kWireHeader) return false;
    const uint64_t payload = wire_header(wire).payload;
    if (!wire_header_matches(wire_header(wire), columns, rows) || wire_bytes < wire_fixed_bytes(columns, rows) + (int64_t)payload) return false;
    const int mw = wire_mask_words(rows);
    const uint8_t* offp = wire + kWireHeader;
    const uint8_t* maskp = offp + columns * 4;
    const uint8_t* pay = wire + wire_fixed_bytes(columns, rows);
    for (int64_t c = 0; c < columns; ++c) {
        uint32_t off;
        std::memcpy(&off, offp + c * 4, 4);
        uint8_t* dst = index_out + c * (int64_t)rows;
        std::memset(dst, 0, (size_t)rows);
        uint64_t at = off;
        for (int w = 0; w < mw; ++w) {
            uint32_t m;
            std::memcpy(&m, maskp + (c * mw + w) * 4, 4);
            while (m) {
                const int bit = __builtin_ctz(m);
                m &= m - 1;
                const int r = w * 32 + bit;
                if (r >= rows || at >= payload) return false;
                dst[r] = pay[at++];
            }
        }
    }
    return true;
}

// ---- the gather (emspec_gather_columns) ----
struct GatherRoles {
    bool is_root;
    bool loopback;   // the root's own columns take the wire too (tests)
    bool packed;     // the root keeps the images packed (no expand)
    bool i_send, i_pack;   // (packed: the root's own columns become an image too)
};
inline GatherRoles gather_roles(int rank, int root, uint32_t flags) {
    GatherRoles g{rank == root, (flags & EMSPEC_GATHER_LOOPBACK) != 0, (flags & EMSPEC_GATHER_PACKED) != 0, false, false};
    g.i_send = !g.is_root || g.loopback;
    g.i_pack = g.i_send || g.packed;
    return g;
}
// What a rank can get wrong on its own: the first rule it breaks (code EMSPEC_OK: none)
struct PlanError { int code; const char* msg; };
inline PlanError gather_arg_error(bool have_index, int64_t columns, int root, int world, bool is_root, bool have_gathered, int rows) {
    if (!have_index || columns < 1) return {EMSPEC_ERR_INVALID_ARG, "null argument / no columns"};
    if (root < 0 || root >= world) return {EMSPEC_ERR_INVALID_ARG, "root out of range"};
    if (is_root && !have_gathered) return {EMSPEC_ERR_INVALID_ARG, "the root needs the gathered buffer"};
    if ((uint64_t)columns * (uint64_t)rows >= (1ull << 32)) return {EMSPEC_ERR_INVALID_ARG, "at most 2^32 cells per call"};
    return {EMSPEC_OK, nullptr};
}
// The size exchange carries one (image bytes, columns) pair per rank; kRankFailed in place of the bytes: "this rank cannot take
// part".  The check of the gathered pairs[world][2]: the first rank that failed, else whether any pair is impossible.
constexpr uint64_t kRankFailed = ~0ull;
enum { kPairsOk = -1, kPairsImpossible = -2 };
inline int gather_pairs_check(const uint64_t* pairs, int world, int rows) {
    for (int r = 0; r < world; ++r)
        if (pairs[2 * r] == kRankFailed) return r;
    for (int r = 0; r < world; ++r) {
        const uint64_t bytes = pairs[2 * r], cols = pairs[2 * r + 1];
        if (cols < 1 || cols * (uint64_t)rows >= (1ull << 32) || bytes > (uint64_t)wire_bound_bytes((int64_t)cols, rows)) return kPairsImpossible;
    }
    return kPairsOk;
}
// Where the root puts what the ranks announced.  The images land 256-byte aligned in rank order, rank r's at off[r] of the
// receive area (recv_bytes of it); expanded, rank r's columns go to dst_off[r] of the gathered buffer (blocks in rank order, each
// as long as that rank's shard); packed, the gathered buffer is a directory of dir_bytes and the receive area behind it.
// A rank that is not the root lays nothing out (all 0, fits).
struct GatherLayout {
    std::vector<size_t> off, dst_off;   // [world + 1]
    size_t dir_bytes, need, recv_bytes;
    bool fits;                          // the gathered buffer holds `need` bytes (a negative capacity counts as 0)
};
inline GatherLayout gather_layout(const uint64_t* pairs, int world, int rows, bool is_root, bool packed, int64_t capacity) {
    GatherLayout g{std::vector<size_t>((size_t)world + 1, 0), std::vector<size_t>((size_t)world + 1, 0), 0, 0, 0, true};
    g.dir_bytes = packed ? al(sizeof(uint64_t) * 4 * (size_t)world) : 0;
    for (int r = 0; is_root && r < world; ++r) {
        g.off[r + 1] = g.off[r] + al((size_t)pairs[2 * r]);
        g.dst_off[r + 1] = g.dst_off[r] + (size_t)pairs[2 * r + 1] * rows;
    }
    g.need = packed ? g.dir_bytes + g.off[world] : g.dst_off[world];
    g.recv_bytes = g.off[world] + 256;
    g.fits = !is_root || g.need <= (size_t)(capacity > 0 ? capacity : 0);
    return g;
}
// The directory of the packed form, per rank (offset from the start of the gathered buffer, image bytes, columns, 0): what the
// root writes to the buffer's head and what emspec_gather_packed_layout reports
inline std::vector<uint64_t> gather_directory(const GatherLayout& g, const uint64_t* pairs, int world) {
    std::vector<uint64_t> dir((size_t)world * 4, 0);
    for (int r = 0; r < world; ++r) {
        dir[4 * r] = (uint64_t)(g.dir_bytes + g.off[r]);
        dir[4 * r + 1] = pairs[2 * r];
        dir[4 * r + 2] = pairs[2 * r + 1];
    }
    return dir;
}
// An image may be up to 4.8 GB (2^32 - 1 cells); one ncclSend / ncclRecv of more than 2^31 bytes arrived damaged (the gather of
// 2^22 - 1 columns x 1,024 rows, a 2.77 GB image: tests/test_gpu_sizes.py), so an image travels in pieces of at most 1 GiB - the
// same pieces on both sides, matched in order within the group.  An image under 1 GiB is one transfer.
// fn(offset, bytes) for piece after piece while it returns true; false if it stopped.
constexpr size_t kMaxTransfer = (size_t)1 << 30;
template <class F>
bool for_transfer_pieces(size_t nbytes, F&& fn) {
    for (size_t o = 0; o < nbytes; o += kMaxTransfer)
        if (!fn(o, std::min(kMaxTransfer, nbytes - o))) return false;
    return true;
}

// The staging block of emspec_batch_gather, 256-byte aligned arrays one after the other: the samples, the rank's index columns,
// its dB when asked for, and on the root the gathered columns of `world` such shards (0 where absent: db, all)
struct GatherStage { size_t pcm, idx, db, all, bytes; };
inline GatherStage gather_stage(size_t pcm_bytes, size_t cells, bool with_db, bool is_root, int world) {
    GatherStage s{0, al(pcm_bytes), 0, 0, 0};
    size_t at = s.idx + al(cells);
    if (with_db) { s.db = at; at += al(cells * 4); }
    if (is_root) { s.all = at; at += al(cells * world); }
    s.bytes = at + 256;
    return s;
}
}  // namespace emspec
