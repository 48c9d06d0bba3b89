// live_overlay.hip.inc — the overlays of the live calls (include/emspec.h: emspec_set_live_peaks, emspec_set_live_wave,
// emspec_set_live_level, emspec_set_live_cross; DESIGN.md §3.11, §3.12, §3.17, §4.15): beside the columns a streaming launch
// delivers, their spectral peaks, the waveform envelope of the samples under them and those samples' level and cross records.
// One kernel behind the last band's frame / flush launch (behind the post kernel when the
// display post-process is on), enqueued only while a setting is on.  It reads the launch's own LiveSinks descriptors, so it
// knows j0, frames, flush, out_at, empty_col and uniform without another host round trip, and it writes exactly the column
// slots the launch writes (emspec_live_plan.h: live_out_slot).  Included by kernels.hip behind live_launch.hip.inc (needs
// peaks.hip.inc and window.hip.inc).
namespace emspec {

// ---- the peaks of one column, by one wave: peaks_kernel's body (peaks.hip.inc) as two functions.  A COPY: with the body
// factored out of peaks_kernel itself the compiler scheduled that kernel differently (one more scalar register, another loop
// test), and the batch entries' kernel stays as it is.  Any change to the selection goes into both; tests/test_gpu_live_overlay.py
// holds the two against emspec_peaks_host and against each other (the batch's lists of the same columns).

// The wave copies its column into its own R floats of LDS - lane l moves quads l, l + 64, ... : 1 KB per load instruction, four
// loads in flight - so that every neighbour, across lanes too, is an LDS read afterwards.
__device__ __forceinline__ void peaks_load_column(const float4* __restrict__ src, float* x, int Q, int lane) {
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

// The column x[R] in the wave's LDS (complete: a barrier lies behind peaks_load_column) -> its k peaks into out[k].  A lane owns
// up to 16 quads = 64 cells: bit 4 j + i of `cand` marks cell i of quad l + 64 j as a candidate that has not been selected yet.
// Selection: k rounds of a wave-wide maximum over each lane's best key = (order image of the dB) << 32 | ~row, so the largest
// key is the loudest candidate and among equals the lowest row; the winning lane clears the bit and rescans only its remaining
// candidates.  Lane t keeps round t's key; at the end lanes 0 .. k-1 interpolate their peak from LDS and store the column's
// k x 8 bytes in one instruction.
__device__ __forceinline__ void peaks_select_column(const float* x, int R, int Q, int k, float min_db, int lane, float2* __restrict__ out) {
    const float ninf = -__builtin_inff();
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
        float2 o = make_float2(-1.0f, ninf);
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
            o = make_float2(((float)r + 0.5f) + d, b);
        }
        out[lane] = o;
    }
}

// The envelope pair of frame j of stream s: key-min / key-max (emspec_window_plan.h: wave_take, wave_bits) over the hop samples
// [j hop + off, j hop + off + hop) of the stream, read by the rule of LiveBlock::sample - absolute sample a is fresh[a - newbase] when a >= newbase, else
// sring[a & mask] - by the 64 lanes of one wave; every lane returns the pair.  The caller guarantees that frame j is one of the
// launch's frames (its samples are then in the staging block or, after the launch's ingest, still in the ring).
__device__ __forceinline__ uint2 live_wave_pair(const LiveSinks& lv, const LiveStream& d, int s, long long j, int hop, int off, int lane) {
    const uint32_t* fresh = reinterpret_cast<const uint32_t*>(lv.fresh) + (size_t)s * (size_t)lv.fresh_stride;
    // (the per-frame form has no sample ring, and every sample of its frame is in the staging block)
    const uint32_t* ring = lv.sring ? reinterpret_cast<const uint32_t*>(lv.sring) + (size_t)s * (size_t)(lv.ring_mask + 1) : nullptr;
    const long long a0 = j * (long long)hop + off;
    uint32_t lo = kWaveLoNone, hi = kWaveHiNone;
    for (int t = lane; t < hop; t += 64) {
        const long long a = a0 + t, rel = a - d.newbase;
        wave_take(rel >= 0 ? fresh[rel] : ring[a & lv.ring_mask], lo, hi);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t ol = (uint32_t)__shfl_xor((int)lo, m, 64), oh = (uint32_t)__shfl_xor((int)hi, m, 64);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    return make_uint2(wave_bits(lo), wave_bits(hi));
}

// The sample reducers of frame j of stream s while a level meter is set: ONE walk over the same hop samples for the envelope's
// keys, the level record and - on a wave that serves channel a of a pair (`crossed`) - the cross record with stream sb's sample
// at the same index, read by the same rule through stream sb's own descriptor.  take / combine are the plan header's
// (emspec_window_plan.h), the butterfly is window.hip.inc's window_mix: no arithmetic is restated.  Every lane returns the
// finished records; `keys` leaves as the samples' bits.
struct LiveMeters { WaveKeys keys; emspec_level level; emspec_cross cross; };
__device__ __forceinline__ LiveMeters live_meters_take(const LiveSinks& lv, const LiveStream& d, const LiveStream& db, int s, int sb, bool crossed, long long j,
                                                       int hop, int off, int lane) {
    const size_t rlen = (size_t)lv.ring_mask + 1;
    const uint32_t* fresh = reinterpret_cast<const uint32_t*>(lv.fresh);
    const uint32_t* sring = reinterpret_cast<const uint32_t*>(lv.sring);   // (null in the per-frame form: every sample is in the staging block)
    const uint32_t *fa = fresh + (size_t)s * (size_t)lv.fresh_stride, *fb = fresh + (size_t)sb * (size_t)lv.fresh_stride;
    const uint32_t *ra = sring ? sring + (size_t)s * rlen : nullptr, *rb = sring ? sring + (size_t)sb * rlen : nullptr;
    const long long a0 = j * (long long)hop + off;
    LiveMeters m{EnvelopeRed::start(), LevelRed::start(), CrossRed::start()};
    for (int t = lane; t < hop; t += 64) {
        const long long a = a0 + t, rel = a - d.newbase;
        const uint32_t ua = rel >= 0 ? fa[rel] : ra[a & lv.ring_mask];
        EnvelopeRed::take(m.keys, ua, 0);
        LevelRed::take(m.level, ua, 0);
        if (crossed) {   // (uniform in the wave)
            const long long relb = a - db.newbase;
            CrossRed::take(m.cross, ua, relb >= 0 ? fb[relb] : rb[a & lv.ring_mask]);
        }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
        window_mix(m.keys, x);
        window_mix(m.level, x);
        if (crossed) window_mix(m.cross, x);
    }
    m.keys = EnvelopeRed::finish(m.keys);
    return m;
}

// Grid (ceil(U / kPeakWaves), S), U = the most frames (flush form: columns) any stream has in the launch: wave (s, i) serves the
// launch's i-th frame of stream s and its i-th column.
//   peaks     the column's delivered dB (ov.db, a device block laid out like the launch's output) goes into the wave's R floats of
//             LDS with 16-byte loads; from there the wave writes the caller's out_db (the frame / post kernels wrote the device
//             block instead) and selects the k peaks exactly as peaks_kernel does (the two functions above).
//   envelope  the pair of frame j0 + i goes to slot (j0 + i) % wslots of the stream's pair ring; the pair of column
//             c = j0 - D + i comes from that ring when frame c arrived in an earlier launch (c < j0) and from the samples when
//             frame c is one of this launch's: no wave waits for another (emspec_live_plan.h: live_wave_slots).
//   meters    (METERS: a level or cross setting is on) the level record of frame j0 + i, and on the waves with s % views == a the
//             cross record of the pair s / views, go to the same slot of their own rings, and a column's records come from the
//             same three sources as its pair: the ring, this wave's own walk when D == 0, else a second walk.  One walk feeds
//             the envelope, the level and the cross (live_meters_take); one lane stores a record.
// METERS is a template parameter, not a run-time branch: the instance without it is the kernel as it was before the meters,
// instruction for instruction (profiles/live_level_rate.txt), so peaks and envelope alone cost what they did.
// All global offsets are 64-bit; plain vector stores only.
template <bool METERS>
__global__ __launch_bounds__(64 * kPeakWaves) void live_overlay_kernel(LiveSinks lv, LiveOverlay ov) {
    extern __shared__ float overlay_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = (int)blockIdx.y, i = (int)blockIdx.x * kPeakWaves + wave;
    const LiveStream d = lv.uniform ? lv.uni : lv.streams[s];
    const int ncol = d.flush ? d.flush : d.frames;
    if ((int)blockIdx.x * kPeakWaves >= ncol) return;   // (uniform in the workgroup; a launch has at least as many columns as frames)
    const int oc = i < ncol ? live_out_slot(d.j0, d.out_at, ov.D, i, lv.empty_col != 0) : -1;
    const size_t pair = ((size_t)s * (size_t)lv.out_cols + (size_t)(oc < 0 ? 0 : oc));
    if (ov.k) {
        const int R = ov.rows, Q = R >> 2;
        float* x = overlay_lds + (size_t)wave * R;
        if (oc >= 0) peaks_load_column(reinterpret_cast<const float4*>(ov.db + pair * (size_t)R), x, Q, lane);
        __syncthreads();
        if (oc >= 0) {
            if (lv.out_db) {
                float* odb = lv.out_db + pair * (size_t)R;
                if ((reinterpret_cast<uintptr_t>(odb) & 15) == 0) {
                    for (int q = lane; q < Q; q += 64) reinterpret_cast<float4*>(odb)[q] = reinterpret_cast<const float4*>(x)[q];
                } else {
                    for (int r = lane; r < R; r += 64) odb[r] = x[r];
                }
            }
            peaks_select_column(x, R, Q, ov.k, ov.min_db, lane, ov.peaks + pair * (size_t)ov.k);
        }
    }
    if constexpr (METERS) {
        const bool crossed = ov.cross && s % ov.views == ov.a;
        const int sb = crossed ? s - ov.a + ov.b : s, p = s / ov.views;
        const LiveStream db = lv.uniform ? lv.uni : lv.streams[sb];
        uint2* wring = ov.wave ? ov.wring + (size_t)s * (size_t)ov.wslots : nullptr;
        emspec_level* lring = ov.level ? ov.lring + (size_t)s * (size_t)ov.wslots : nullptr;
        emspec_cross* xring = crossed ? ov.xring + (size_t)p * (size_t)ov.wslots : nullptr;
        const bool feeds = !d.flush && i < d.frames;
        // the empty column's records: the pair (+inf, -inf), sums of no sample
        LiveMeters mine{WaveKeys{0x7f800000u, 0xff800000u}, LevelRed::start(), CrossRed::start()};
        if (feeds) {
            mine = live_meters_take(lv, d, db, s, sb, crossed, d.j0 + i, ov.hop, ov.off, lane);
            const int slot = (int)((d.j0 + i) % ov.wslots);
            if (lane == 0) {
                if (wring) wring[slot] = make_uint2(mine.keys.lo, mine.keys.hi);
                if (lring) lring[slot] = mine.level;
                if (xring) xring[slot] = mine.cross;
            }
        }
        if (oc >= 0) {
            const long long c = d.j0 - ov.D + i;
            LiveMeters m{WaveKeys{0x7f800000u, 0xff800000u}, LevelRed::start(), CrossRed::start()};
            if (c >= 0) {
                if (d.flush || c < d.j0) {
                    const int slot = (int)(c % ov.wslots);
                    if (wring) { const uint2 w = wring[slot]; m.keys = WaveKeys{w.x, w.y}; }
                    if (lring) m.level = lring[slot];
                    if (xring) m.cross = xring[slot];
                } else if (ov.D == 0) {
                    m = mine;
                } else {
                    m = live_meters_take(lv, d, db, s, sb, crossed, c, ov.hop, ov.off, lane);
                }
            }
            if (lane == 0) {
                if (ov.wave) ov.wave[pair] = make_uint2(m.keys.lo, m.keys.hi);
                if (ov.level) ov.level[pair] = m.level;
                if (crossed) ov.cross[(size_t)p * (size_t)lv.out_cols + (size_t)oc] = m.cross;
            }
        }
    } else if (ov.wave) {
        uint2* ring = ov.wring + (size_t)s * (size_t)ov.wslots;
        const bool feeds = !d.flush && i < d.frames;
        uint2 mine = make_uint2(0x7f800000u, 0xff800000u);   // (+inf, -inf): the empty column's pair
        if (feeds) {
            mine = live_wave_pair(lv, d, s, d.j0 + i, ov.hop, ov.off, lane);
            if (lane == 0) ring[(int)((d.j0 + i) % ov.wslots)] = mine;
        }
        if (oc >= 0) {
            const long long c = d.j0 - ov.D + i;
            uint2 p = make_uint2(0x7f800000u, 0xff800000u);
            if (c >= 0) {
                if (d.flush || c < d.j0) p = ring[(int)(c % ov.wslots)];
                else if (ov.D == 0) p = mine;
                else p = live_wave_pair(lv, d, s, c, ov.hop, ov.off, lane);
            }
            if (lane == 0) ov.wave[pair] = p;
        }
    }
}

// lv: the launch's sinks with out_db / out_cols the CALLER's dB destination and its stride (null: dB not wanted);
// units: the most frames (flush form: columns) of any stream.  ov.k != 0 needs rows % 4 == 0, 4 <= rows <= 4096.
hipError_t launch_live_overlay(const LiveSinks& lv, const LiveOverlay& ov, int S, int units, hipStream_t st) {
    const bool meters = ov.level || ov.cross;
    if (S <= 0 || units <= 0 || (!ov.k && !ov.wave && !meters)) return hipSuccess;
    if (S > 65535) return hipErrorInvalidValue;
    if (ov.k && (!ov.db || !ov.peaks || ov.rows % 4 || ov.rows < 4 || ov.rows > 4096 || ov.k < 1 || ov.k > 32 || ov.min_db != ov.min_db))
        return hipErrorInvalidValue;
    if (ov.wave && (!ov.wring || ov.wslots < 1 || ov.hop < 1)) return hipErrorInvalidValue;
    if (meters && (ov.wslots < 1 || ov.hop < 1 || (ov.level && !ov.lring))) return hipErrorInvalidValue;
    // a pair's two streams are streams of this launch: p views + a and p views + b below S
    if (ov.cross && (!ov.xring || ov.views < 1 || S % ov.views || ov.a < 0 || ov.a >= ov.views || ov.b < 0 || ov.b >= ov.views)) return hipErrorInvalidValue;
    if (meters && ((reinterpret_cast<uintptr_t>(ov.level) | reinterpret_cast<uintptr_t>(ov.cross)) & 7)) return hipErrorInvalidValue;
    const size_t lds = ov.k ? (size_t)kPeakWaves * ov.rows * sizeof(float) : 0;
    const dim3 grid((unsigned)((units + kPeakWaves - 1) / kPeakWaves), (unsigned)S), block(64 * kPeakWaves);
    if (meters) hipLaunchKernelGGL(live_overlay_kernel<true>, grid, block, lds, st, lv, ov);
    else hipLaunchKernelGGL(live_overlay_kernel<false>, grid, block, lds, st, lv, ov);
    return hipGetLastError();
}

}  // namespace emspec
