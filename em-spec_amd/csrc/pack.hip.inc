// pack.hip.inc — wire format of finished palette-index columns for the multi-GPU gather.  Included by kernels.hip.
//
// xGMI is point-to-point: every rank reaches the gather root over ONE link, so the bytes a column costs on the
// wire bound the 8-GPU rate (SURVEY.md §8(e), DESIGN.md §6).  A finished column is R palette indices (uint8) of
// which most are 0: gated cells, cells below the dB floor and low rows no DFT bin can reach.  The lossless wire
// image of `columns` columns is
//     header   32 B : magic "EMW2", rows, columns (u64), payload bytes (u64), 8 B reserved
//     offsets  columns x u32: where each column's non-zero indices start in the payload (exclusive prefix sum)
//     masks    columns x MW x 4 B, MW = ceil(R/32): bit r%32 of word r/32 set  <=>  index[r] != 0
//     payload  the non-zero indices, column after column, rows ascending; padded to 16 B
// The offsets cost 4 B per column and let the receiver expand every column independently in ONE kernel (no
// popcount / prefix-sum passes on the root, which expands world-1 images per gather and is the critical path).
// On the bench input 5-7 % of the cells are non-zero: ~186 B per column instead of 1024.
// The reference has no counterpart (no GPU path, no collectives: SURVEY.md §2); format is [BUILD-DEFINED].
// (kWireMagic, kWireHeader, wire_mask_words and every size of an image or of the pack workspace: emspec_wire_plan.h)
namespace emspec {

// nz4: 4-bit mask of the non-zero bytes of a dword
__device__ __forceinline__ unsigned nz4(uint32_t w) {
    return ((w & 0xFFu) ? 1u : 0u) | ((w & 0xFF00u) ? 2u : 0u) | ((w & 0xFF0000u) ? 4u : 0u) | ((w & 0xFF000000u) ? 8u : 0u);
}
__device__ __forceinline__ unsigned nz16(uint4 v) {
    return nz4(v.x) | (nz4(v.y) << 4) | (nz4(v.z) << 8) | (nz4(v.w) << 12);
}
// exclusive prefix sum over the 64 lanes of a wave (v < 2^20), and the wave total
__device__ __forceinline__ unsigned wave_excl_scan(unsigned v, unsigned& total) {
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d, 64);
        if ((int)(threadIdx.x & 63) >= d) x += y;
    }
    total = __shfl(x, 63, 64);
    return x - v;
}

// ---- generic path (any rows % 4 == 0): one wave per column, 4 rows (one dword) per lane and iteration ----
__global__ __launch_bounds__(256) void wire_count_kernel(const uint8_t* __restrict__ index, int64_t columns, int R,
                                                         uint32_t* __restrict__ masks, uint32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= columns) return;
    const int MW = wire_mask_words(R), nd = R >> 2;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(index + (size_t)col * R);
    uint32_t* mrow = masks + (size_t)col * MW;
    unsigned cnt = 0;
    for (int d0 = 0; d0 < nd; d0 += 64) {
        const int d = d0 + lane;
        const unsigned nib = d < nd ? nz4(src[d]) : 0u;
        cnt += __popc(nib);
        // eight lanes (8 dwords = 32 rows) make one mask word
        unsigned m = nib << (4 * (lane & 7));
        m |= __shfl_xor(m, 1, 64);
        m |= __shfl_xor(m, 2, 64);
        m |= __shfl_xor(m, 4, 64);
        if ((lane & 7) == 0 && (d >> 3) < MW) mrow[d >> 3] = m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if (lane == 0) counts[col] = cnt;
}
// PACK: index -> payload (offset = local + block prefix, also published in the image);  !PACK: image -> index
template <bool PACK>
__global__ __launch_bounds__(256) void wire_move_kernel(uint8_t* __restrict__ index, int64_t columns, int R,
                                                        const uint32_t* __restrict__ masks, const uint32_t* __restrict__ local,
                                                        const uint32_t* __restrict__ bscan, uint32_t* __restrict__ offsets,
                                                        uint8_t* __restrict__ payload) {
    const int lane = threadIdx.x & 63;
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= columns) return;
    const int MW = wire_mask_words(R), nd = R >> 2;
    uint32_t* cells = reinterpret_cast<uint32_t*>(index + (size_t)col * R);
    const uint32_t* mrow = masks + (size_t)col * MW;
    uint32_t off;
    if (PACK) { off = local[col] + bscan[col >> 10]; if (lane == 0) offsets[col] = off; }
    else off = offsets[col];
    uint8_t* pay = payload + (size_t)off;
    unsigned run = 0;   // non-zero cells of this column before the current iteration
    for (int d0 = 0; d0 < nd; d0 += 64) {
        const int d = d0 + lane;
        unsigned nib = 0;
        uint32_t w = 0;
        if (d < nd) {
            if (PACK) { w = cells[d]; nib = nz4(w); }
            else nib = (mrow[d >> 3] >> (4 * (d & 7))) & 15u;
        }
        unsigned tot;
        unsigned at = run + wave_excl_scan(__popc(nib), tot);
        run += tot;
        if (PACK) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (nib & (1u << b)) pay[at++] = (uint8_t)(w >> (8 * b));
        } else if (d < nd) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (nib & (1u << b)) w |= (uint32_t)pay[at++] << (8 * b);
            cells[d] = w;
        }
    }
}

// ---- fast path, rows % 32 == 0 and rows <= 1024: 16 rows (one 16-byte access) per lane, so a column is one coalesced
// access, one wave scan and one 16-byte store per lane; a wave takes NC columns at a time so that their (dependent)
// loads are in flight together.  (The payload of an image starts 16-byte aligned only if its offsets/masks part
// happens to be: nothing below assumes more than byte alignment of a run, dword alignment of the payload base.)
constexpr int kWireNC = 4;
__global__ __launch_bounds__(256) void wire_count16_kernel(const uint8_t* __restrict__ index, int64_t columns, int R,
                                                           uint32_t* __restrict__ masks, uint32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t col0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kWireNC;
    const int MW = R >> 5, nq = R >> 4;
    uint4 v[kWireNC];
#pragma unroll
    for (int c = 0; c < kWireNC; ++c)
        v[c] = (col0 + c < columns && lane < nq) ? reinterpret_cast<const uint4*>(index + (size_t)(col0 + c) * R)[lane] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int c = 0; c < kWireNC; ++c) {
        if (col0 + c >= columns) break;
        const unsigned m16 = nz16(v[c]);
        unsigned cnt = __popc(m16);
        const unsigned hi = __shfl_xor(m16, 1, 64);
        if (!(lane & 1) && (lane >> 1) < MW) masks[(size_t)(col0 + c) * MW + (lane >> 1)] = m16 | (hi << 16);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if (lane == 0) counts[col0 + c] = cnt;
    }
}
// PACK = true: index -> payload.  The offsets come from the scan; each lane stores its (few) non-zero bytes.
__global__ __launch_bounds__(256) void wire_pack16_kernel(const uint8_t* __restrict__ index, int64_t columns, int R,
                                                          const uint32_t* __restrict__ local, const uint32_t* __restrict__ bscan,
                                                          uint32_t* __restrict__ offsets, uint8_t* __restrict__ payload) {
    const int lane = threadIdx.x & 63;
    const int64_t col0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kWireNC;
    const int nq = R >> 4;
    uint4 v[kWireNC];
    unsigned off[kWireNC];
#pragma unroll
    for (int c = 0; c < kWireNC; ++c) {      // every load of the NC columns is issued before any is used
        const int64_t col = col0 + c;
        v[c] = make_uint4(0u, 0u, 0u, 0u);
        off[c] = 0;
        if (col < columns) {
            off[c] = local[col] + bscan[col >> 10];
            if (lane < nq) v[c] = reinterpret_cast<const uint4*>(index + (size_t)col * R)[lane];
        }
    }
#pragma unroll
    for (int c = 0; c < kWireNC; ++c) {
        unsigned m = nz16(v[c]), tot;
        unsigned a = off[c] + wave_excl_scan(__popc(m), tot);
        if (col0 + c >= columns) continue;
        if (lane == 0) offsets[col0 + c] = off[c];
        const uint32_t w[4] = {v[c].x, v[c].y, v[c].z, v[c].w};
        while (m) {                                         // typically 0-2 non-zero cells of the lane's 16
            const int b = __ffs(m) - 1, q = b >> 2;
            m &= m - 1;
            const uint32_t word = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
            payload[a++] = (uint8_t)(word >> (8 * (b & 3)));
        }
    }
}
// Image -> index.  A column's non-zero bytes are one contiguous run of the payload: the wave copies the run into LDS with
// coalesced dword loads.  A lane's 16 cells take the lane's own <= 16 consecutive bytes of that run, so the lane reads
// the five aligned dwords that cover them (neighbouring lanes read neighbouring dwords: no bank conflicts to speak
// of), shifts them into place (v_alignbyte) and then DEPOSITS them cell by cell in registers: output dword j takes the
// four payload bytes from position popc(mask below 4j) on, spread by its 4 mask bits with one v_perm_b32 whose selector
// comes from a 16-entry table.  (The first version read every cell's byte from LDS on its own: 16 predicated byte reads
// per lane and column with random bank conflicts, 240 us per 524k columns.)
__device__ __forceinline__ uint32_t wire_deposit_selector(unsigned nib) {   // v_perm selector: byte i <- source byte #(set bits below i), or 0x00
    uint32_t sel = 0;
    unsigned n = 0;
    for (int i = 0; i < 4; ++i) {
        sel |= ((nib >> i) & 1u ? n : 0x0Cu) << (8 * i);
        n += (nib >> i) & 1u;
    }
    return sel;
}
__global__ __launch_bounds__(256) void wire_expand16_kernel(uint8_t* __restrict__ index, int64_t columns, int R,
                                                            const uint32_t* __restrict__ masks, const uint32_t* __restrict__ offsets,
                                                            const uint8_t* __restrict__ payload) {
    constexpr int kStage = 64;                               // dwords staged per column: runs of up to 253 bytes (the usual case); measured: NC = 4 beats NC = 8
    constexpr int kPad = 8;                                  // a lane's five-dword window may reach past the run
    __shared__ uint32_t stage[4][kWireNC][kStage + kPad];
    __shared__ uint32_t seltab[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x < 16) seltab[threadIdx.x] = wire_deposit_selector(threadIdx.x);
    const int64_t col0 = ((int64_t)blockIdx.x * 4 + wv) * kWireNC;
    const int MW = R >> 5, nq = R >> 4;
    unsigned m16[kWireNC], off[kWireNC];
#pragma unroll
    for (int c = 0; c < kWireNC; ++c) {
        const int64_t col = col0 + c;
        m16[c] = 0; off[c] = 0;
        if (col < columns) {
            off[c] = offsets[col];
            if (lane < nq) m16[c] = (masks[(size_t)col * MW + (lane >> 1)] >> (16 * (lane & 1))) & 0xFFFFu;
        }
    }
    unsigned rel[kWireNC], tot[kWireNC];
#pragma unroll
    for (int c = 0; c < kWireNC; ++c) rel[c] = wave_excl_scan(__popc(m16[c]), tot[c]);
    // stage the runs: aligned dwords from (off & ~3); the run starts (off & 3) bytes into the stage.  One dword per lane
    // covers 256 bytes; a longer run (a dense column) is read from memory directly below.
#pragma unroll
    for (int c = 0; c < kWireNC; ++c) {
        const unsigned nb = tot[c] + (off[c] & 3u);          // bytes to cover, from the aligned start
        if ((unsigned)lane * 4 < nb)                          // the image is padded to 16 B: no overrun
            stage[wv][c][lane] = reinterpret_cast<const uint32_t*>(payload + (size_t)(off[c] & ~3u))[lane];
    }
    __syncthreads();                                          // the selector table; the stages are wave-local
#pragma unroll
    for (int c = 0; c < kWireNC; ++c) {
        if (col0 + c >= columns) continue;
        const unsigned m = m16[c];
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        const bool staged = tot[c] + (off[c] & 3u) <= kStage * 4;   // wave-uniform
        if (staged) {
            const unsigned s0 = (off[c] & 3u) + rel[c];             // the lane's first byte, in bytes from the stage's start
            const uint32_t* sp = stage[wv][c] + (s0 >> 2);
            const uint32_t d0 = sp[0], d1 = sp[1], d2 = sp[2], d3 = sp[3], d4 = sp[4];   // bytes past the lane's share are never selected
            const unsigned sh = s0 & 3u;
            // A0..A3: the lane's 16 payload bytes, byte-aligned
            const uint32_t A0 = __builtin_amdgcn_alignbyte(d1, d0, sh), A1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
            const uint32_t A2 = __builtin_amdgcn_alignbyte(d3, d2, sh), A3 = __builtin_amdgcn_alignbyte(d4, d3, sh);
            // output dword j <- 4 bytes from position p_j = popc(m & (2^(4j) - 1)) on; p_j <= 4j, so the window is in A[0..j]
            const unsigned p1 = __popc(m & 0xFu), p2 = __popc(m & 0xFFu), p3 = __popc(m & 0xFFFu);
            const uint32_t W0 = A0;
            const uint32_t W1 = __builtin_amdgcn_alignbyte(p1 >= 4 ? A2 : A1, p1 >= 4 ? A1 : A0, p1 & 3u);
            const uint32_t lo2 = p2 >= 8 ? A2 : (p2 >= 4 ? A1 : A0), hi2 = p2 >= 8 ? A3 : (p2 >= 4 ? A2 : A1);
            const uint32_t W2 = __builtin_amdgcn_alignbyte(hi2, lo2, p2 & 3u);
            const uint32_t lo3 = p3 >= 12 ? A3 : (p3 >= 8 ? A2 : (p3 >= 4 ? A1 : A0));
            const uint32_t hi3 = p3 >= 12 ? 0u : (p3 >= 8 ? A3 : (p3 >= 4 ? A2 : A1));
            const uint32_t W3 = __builtin_amdgcn_alignbyte(hi3, lo3, p3 & 3u);
            w[0] = __builtin_amdgcn_perm(0u, W0, seltab[m & 15u]);
            w[1] = __builtin_amdgcn_perm(0u, W1, seltab[(m >> 4) & 15u]);
            w[2] = __builtin_amdgcn_perm(0u, W2, seltab[(m >> 8) & 15u]);
            w[3] = __builtin_amdgcn_perm(0u, W3, seltab[(m >> 12) & 15u]);
        } else {
            // a dense column (more than 253 non-zero cells): its bytes come straight from the image
            const uint8_t* sb = payload + (size_t)off[c] + rel[c];
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const unsigned pos = __popc(m & ((1u << b) - 1u));
                const uint32_t byte = ((m >> b) & 1u) ? (uint32_t)sb[pos] : 0u;
                w[b >> 2] |= byte << (8 * (b & 3));
            }
        }
        if (lane < nq) reinterpret_cast<uint4*>(index + (size_t)(col0 + c) * R)[lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// exclusive scan of counts[n] (uint32, total < 2^32 checked by the host: columns * rows < 2^32), two levels:
//   A: every 1024-block scans itself -> local offsets + block total;  B: one workgroup scans the block totals,
//   publishes the grand total and writes the image header;  the move kernel adds bscan[col >> 10].
__global__ __launch_bounds__(1024) void wire_scan_a_kernel(const uint32_t* counts, int64_t n, uint32_t* local /* may alias counts */,
                                                           uint32_t* __restrict__ bsum) {
    __shared__ unsigned wsum[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * 1024 + t;
    const unsigned v = i < n ? counts[i] : 0u;
    unsigned tot;
    const unsigned ex = wave_excl_scan(v, tot);
    if (lane == 63) wsum[w] = tot;
    __syncthreads();
    unsigned base = 0;
    for (int q = 0; q < w; ++q) base += wsum[q];
    if (i < n) local[i] = base + ex;
    if (t == 1023) bsum[blockIdx.x] = base + tot;
}
__global__ __launch_bounds__(1024) void wire_scan_b_kernel(uint32_t* __restrict__ bsum, int64_t nb, int64_t fixed_bytes,
                                                           uint64_t* __restrict__ total_bytes, uint8_t* __restrict__ header,
                                                           int rows, int64_t columns) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned carry_s;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
        const int64_t i = b0 + t;
        const unsigned v = i < nb ? bsum[i] : 0u;
        unsigned tot;
        const unsigned ex = wave_excl_scan(v, tot);
        if (lane == 63) wsum[w] = tot;
        __syncthreads();
        unsigned base = carry_s;
        for (int q = 0; q < w; ++q) base += wsum[q];
        if (i < nb) bsum[i] = base + ex;
        __syncthreads();
        if (t == 1023) carry_s = base + tot;
        __syncthreads();
    }
    if (t == 0) {
        const uint64_t payload = carry_s;
        *total_bytes = (uint64_t)fixed_bytes + ((payload + 15) & ~(uint64_t)15);
        uint32_t* h32 = reinterpret_cast<uint32_t*>(header);
        h32[0] = kWireMagic; h32[1] = (uint32_t)rows;
        h32[2] = (uint32_t)((uint64_t)columns & 0xFFFFFFFFu); h32[3] = (uint32_t)((uint64_t)columns >> 32);
        h32[4] = (uint32_t)(payload & 0xFFFFFFFFu); h32[5] = (uint32_t)(payload >> 32);
        h32[6] = 0; h32[7] = 0;
        // the payload is ZERO-padded to 16 bytes (the format, oracle/wire_ref.py): the move kernels that follow write the payload's
        // own bytes only, so the pad is cleared here - an image is then the same bytes whatever the buffer held before (round 5:
        // the host-buffer entry emspec_batch_packed hands images to the host, whose bytes must be reproducible)
        uint8_t* pay = header + fixed_bytes;
        for (uint64_t i = payload; i < ((payload + 15) & ~(uint64_t)15); ++i) pay[i] = 0;
    }
}

// ---- host side ----
template <class T>
static T* wire_scratch_at(void* scratch, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(scratch) + offset); }
uint64_t* wire_total_ptr(void* scratch, int64_t columns) { return wire_scratch_at<uint64_t>(scratch, wire_scratch_split(columns).total); }
static bool wire_fast(int rows) { return rows % 32 == 0 && rows <= 1024; }

// index[columns][rows] -> wire image at `wire` (capacity wire_bound_bytes); the image's size lands in
// *wire_total_ptr(scratch) on the device.  Everything is enqueued on st; nothing synchronises.
hipError_t launch_wire_pack(const uint8_t* index, int64_t columns, int rows, uint8_t* wire, void* scratch, hipStream_t st) {
    if (columns <= 0 || rows % 4 || (uint64_t)columns * (uint64_t)rows >= (1ull << 32)) return hipErrorInvalidValue;
    const WireScratch o = wire_scratch_split(columns);
    uint32_t* local = wire_scratch_at<uint32_t>(scratch, o.local);
    uint32_t* bsum = wire_scratch_at<uint32_t>(scratch, o.bsum);
    uint64_t* total = wire_scratch_at<uint64_t>(scratch, o.total);
    uint32_t* offsets = reinterpret_cast<uint32_t*>(wire + kWireHeader);
    uint32_t* masks = offsets + columns;
    const int64_t fixed = wire_fixed_bytes(columns, rows);
    const int64_t nb = (columns + 1023) / 1024;
    const unsigned g1 = (unsigned)((columns + 3) / 4), g4 = (unsigned)((columns + 4 * kWireNC - 1) / (4 * kWireNC));
    uint8_t* idx = const_cast<uint8_t*>(index);
    if (wire_fast(rows)) hipLaunchKernelGGL(wire_count16_kernel, dim3(g4), dim3(256), 0, st, index, columns, rows, masks, local);
    else hipLaunchKernelGGL(wire_count_kernel, dim3(g1), dim3(256), 0, st, index, columns, rows, masks, local);
    hipLaunchKernelGGL(wire_scan_a_kernel, dim3((unsigned)nb), dim3(1024), 0, st, local, columns, local, bsum);
    hipLaunchKernelGGL(wire_scan_b_kernel, dim3(1), dim3(1024), 0, st, bsum, nb, fixed, total, wire, rows, columns);
    if (wire_fast(rows)) hipLaunchKernelGGL(wire_pack16_kernel, dim3(g4), dim3(256), 0, st, index, columns, rows, local, bsum, offsets, wire + fixed);
    else hipLaunchKernelGGL(wire_move_kernel<true>, dim3(g1), dim3(256), 0, st, idx, columns, rows, masks, local, bsum, offsets, wire + fixed);
    return hipGetLastError();
}
// wire image (header validated by the caller: rows / columns match) -> index[columns][rows]: one kernel, no workspace
hipError_t launch_wire_unpack(const uint8_t* wire, int64_t columns, int rows, uint8_t* index, hipStream_t st) {
    if (columns <= 0 || rows % 4 || (uint64_t)columns * (uint64_t)rows >= (1ull << 32)) return hipErrorInvalidValue;
    uint32_t* offsets = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(wire) + kWireHeader);
    const uint32_t* masks = offsets + columns;
    uint8_t* payload = const_cast<uint8_t*>(wire) + wire_fixed_bytes(columns, rows);
    const unsigned g1 = (unsigned)((columns + 3) / 4), g4 = (unsigned)((columns + 4 * kWireNC - 1) / (4 * kWireNC));
    if (wire_fast(rows)) hipLaunchKernelGGL(wire_expand16_kernel, dim3(g4), dim3(256), 0, st, index, columns, rows, masks, offsets, payload);
    else hipLaunchKernelGGL(wire_move_kernel<false>, dim3(g1), dim3(256), 0, st, index, columns, rows, masks, nullptr, nullptr, offsets, payload);
    return hipGetLastError();
}

}  // namespace emspec
