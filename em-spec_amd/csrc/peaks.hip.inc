// peaks.hip.inc — the spectral peaks of finished columns (DESIGN.md §3.11, §4.12; include/emspec.h: emspec_peaks_device):
// per column of R dB cells the k loudest local maxima, each as (position in row units, dB), loudest first.
//   candidate r:  x[r] >= min_db && x[r] > x[r-1] && x[r] >= x[r+1]      (-inf beyond either end; plain float comparisons)
//   db  = x[r]                                                           (the cell's own bits)
//   pos = r + 0.5 at r = 0 and r = R-1;  else  (r + 0.5) + clamp((0.5 (a - c)) / ((a - b) + (c - b)), +-0.5), NaN -> 0
//   order: dB descending, ties by ascending row;  unused slots (-1, -inf)
// One HBM-bound pass: every dB cell is read once with 16-byte loads, each column's k x 8 bytes are written once.
// Included by kernels.hip after reduce.hip.inc.
namespace emspec {

constexpr int kPeakWaves = 4;   // waves (= columns in flight) per workgroup

// Order-preserving integer image of a float that is not NaN: a < b  <=>  image(a) < image(b), and -0.0 ties with +0.0.
__device__ __forceinline__ uint32_t peak_order(float x) {
    const uint32_t u = x == 0.0f ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// One wave per column, columns grid-strided (kPeakWaves per workgroup and step; the trip count is uniform in a workgroup, so
// its barriers are).  The wave copies its column into its own R floats of LDS - lane l moves quads l, l + 64, ... : 1 KB per
// load instruction, four loads in flight - and every neighbour, across lanes too, is then an LDS read.  A lane owns up to 16
// quads = 64 cells: bit 4 j + i of `cand` marks cell i of quad l + 64 j as a candidate that has not been selected yet.
// Selection: k rounds of a wave-wide maximum over each lane's best key = (order image of the dB) << 32 | ~row, so the largest
// key is the loudest candidate and among equals the lowest row; the winning lane clears the bit and rescans only its remaining
// candidates.  Lane t keeps round t's key; at the end lanes 0 .. k-1 interpolate their peak from LDS and store the column's
// k x 8 bytes in one instruction.  All global offsets are 64-bit.
__global__ __launch_bounds__(64 * kPeakWaves) void peaks_kernel(const float* __restrict__ db, int64_t columns, int R, int k,
                                                                float min_db, float2* __restrict__ peaks) {
    extern __shared__ float peaks_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* x = peaks_lds + (size_t)wave * R;
    const int Q = R >> 2;
    const float ninf = -__builtin_inff();
    for (int64_t base = (int64_t)blockIdx.x * kPeakWaves; base < columns; base += (int64_t)gridDim.x * kPeakWaves) {
        const int64_t col = base + wave;
        const bool live = col < columns;
        if (live) {
            const float4* src = reinterpret_cast<const float4*>(db + (size_t)col * (size_t)R);
            for (int q0 = 0; q0 < Q; q0 += 256) {
                // (a quad past the column's end: the last quad again, loaded and not stored)
                const int qa = q0 + lane, qb = qa + 64, qc = qa + 128, qd = qa + 192;
                const float4 va = src[qa < Q ? qa : Q - 1], vb = src[qb < Q ? qb : Q - 1];
                const float4 vc = src[qc < Q ? qc : Q - 1], vd = src[qd < Q ? qd : Q - 1];
                if (qa < Q) reinterpret_cast<float4*>(x)[qa] = va;
                if (qb < Q) reinterpret_cast<float4*>(x)[qb] = vb;
                if (qc < Q) reinterpret_cast<float4*>(x)[qc] = vc;
                if (qd < Q) reinterpret_cast<float4*>(x)[qd] = vd;
            }
        }
        __syncthreads();
        if (live) {
            unsigned long long cand = 0, best = 0;
            auto key_of = [&](int r) { return ((unsigned long long)peak_order(x[r]) << 32) | (uint32_t)~(uint32_t)r; };
            for (int j = 0; 64 * j + lane < Q; ++j) {
                const int q = 64 * j + lane;
                const float4 c = reinterpret_cast<const float4*>(x)[q];
                const float l = q > 0 ? x[4 * q - 1] : ninf, rn = q + 1 < Q ? x[4 * q + 4] : ninf;
                auto test = [&](int i, float left, float b, float right) {
                    if (b >= min_db && b > left && b >= right) {
                        cand |= 1ull << (4 * j + i);
                        const unsigned long long key = ((unsigned long long)peak_order(b) << 32) | (uint32_t)~(uint32_t)(4 * q + i);
                        best = key > best ? key : best;
                    }
                };
                test(0, l, c.x, c.y);
                test(1, c.x, c.y, c.z);
                test(2, c.y, c.z, c.w);
                test(3, c.z, c.w, rn);
            }
            unsigned long long mine = 0;   // lane t: the key of the t-th peak (0: none)
            for (int t = 0; t < k; ++t) {
                const unsigned long long top = wave_max_u64(best);
                if (top == 0) break;   // (uniform in the wave)
                if (lane == t) mine = top;
                if (best == top) {     // the one lane that owns the winner (keys carry the row: no two are equal)
                    const int r = (int)~(uint32_t)top;
                    cand &= ~(1ull << (4 * (r >> 8) + (r & 3)));
                    best = 0;
                    for (unsigned long long m = cand; m; m &= m - 1) {
                        const int bit = __builtin_ctzll(m);
                        const unsigned long long key = key_of(4 * (64 * (bit >> 2) + lane) + (bit & 3));
                        best = key > best ? key : best;
                    }
                }
            }
            if (lane < k) {
                float2 out = make_float2(-1.0f, ninf);
                if (mine) {
                    const int r = (int)~(uint32_t)mine;
                    const float b = x[r];
                    float d = 0.0f;
                    if (r > 0 && r < R - 1) {
                        const float a = x[r - 1], c = x[r + 1];
                        const float t = a - c;
                        const float u = (a - b) + (c - b);
                        d = (0.5f * t) / u;
                        if (d > 0.5f) d = 0.5f;
                        if (d < -0.5f) d = -0.5f;
                        if (d != d) d = 0.0f;
                    }
                    out = make_float2(((float)r + 0.5f) + d, b);
                }
                peaks[(size_t)col * (size_t)k + lane] = out;
            }
        }
        __syncthreads();   // the next column overwrites the wave's LDS
    }
}

// db [columns][R] float32, 16-byte aligned, R % 4 == 0, 4 <= R <= 4096; peaks [columns][k] of (pos, db), 8-byte aligned;
// 1 <= k <= 32; min_db not NaN.  The grid strides over the columns: no limit on columns * R.
hipError_t launch_peaks(const float* db, int64_t columns, int R, int k, float min_db, void* peaks, hipStream_t st) {
    if (columns <= 0) return hipSuccess;
    if (!db || !peaks || R % 4 || R < 4 || R > 4096 || k < 1 || k > 32 || min_db != min_db) return hipErrorInvalidValue;
    const int64_t groups = (columns + kPeakWaves - 1) / kPeakWaves;
    // (two 64 KB workgroups are resident per CU at R = 4096, sixteen at R <= 512: a few workgroups per CU, then stride)
    const unsigned blocks = (unsigned)(groups < 4096 ? groups : 4096);
    hipLaunchKernelGGL(peaks_kernel, dim3(blocks), dim3(64 * kPeakWaves), (size_t)kPeakWaves * R * sizeof(float), st, db, columns,
                       R, k, min_db, reinterpret_cast<float2*>(peaks));
    return hipGetLastError();
}

}  // namespace emspec
