// live_audio.hip.inc — the live audio history (include/emspec.h: emspec_set_live_audio, emspec_audio_view, emspec_audio_batch;
// DESIGN.md §3.15, §4.17): a ring of the samples the streaming calls move to the device, W per stream, and views that read a
// range back bit for bit - the input of a re-analysis at another fft size, hop or reassign setting.  Two kernels: the store goes
// behind a live launch's kernels, behind the history store (live_history.hip.inc), and reads the same LiveSinks descriptors;
// the view copies ring -> [streams][stride].  The arithmetic of slots, held ranges, runs and the head / body / tail split:
// emspec_audio_plan.h.  Included by kernels.hip behind live_history.hip.inc.
namespace emspec {

// `count` 4-byte words src -> dst (both 4-byte aligned, not overlapping), by the T threads of the workgroups that share the run,
// this thread being number t of them: where source and destination agree modulo 16 bytes, a scalar head up to the boundary, a
// body of 16-byte loads and stores (lane-linear: consecutive lanes take consecutive 16-byte pieces), a scalar tail; else word
// by word.  Words, not floats: a NaN's payload and a zero's sign are bits like any other.  64-bit offsets throughout.
__device__ __forceinline__ void audio_copy_run(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, long long count, long long t,
                                               long long T) {
    if (count <= 0) return;
    const AudioSplit sp = audio_split(audio_align(reinterpret_cast<uintptr_t>(src)), audio_align(reinterpret_cast<uintptr_t>(dst)), count);
    if (sp.body == 0) {
        for (long long i = t; i < count; i += T) dst[i] = src[i];
        return;
    }
    if (t < sp.head) dst[t] = src[t];
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src + sp.head);
    uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst + sp.head);
    for (long long q = t; q < sp.body; q += T) d4[q] = s4[q];
    const long long done = sp.head + 4 * sp.body;
    if (t < sp.tail) dst[done + t] = src[done + t];
}

// Grid (pieces, S): the `pieces` workgroups of stream s share the stream's fresh samples of this launch (audio_fresh: the
// block form's newcount samples from absolute sample newbase on, the per-frame form's not yet stored part of the frame), of
// which the last W go to slots (a mod W) of the stream's ring - at most two runs across the wrap (audio_runs).
__global__ __launch_bounds__(256) void live_audio_store_kernel(LiveSinks lv, LiveAudio a) {
    const int s = (int)blockIdx.y;
    const LiveStream d = lv.uniform ? lv.uni : lv.streams[s];
    const AudioRange r = audio_keep(audio_fresh(a.form, d.j0, d.newbase, d.newcount, d.frames, d.flush, a.n, a.hop), a.W);
    if (r.count <= 0) return;
    const AudioRuns run = audio_runs(r.a0, r.count, a.W);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(lv.fresh) + (size_t)s * (size_t)lv.fresh_stride + (size_t)r.src;
    uint32_t* ring = a.ring + (size_t)s * (size_t)a.stride;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, T = (long long)gridDim.x * 256;
    audio_copy_run(src, ring + run.slot0, run.n0, t, T);
    audio_copy_run(src + run.n0, ring, run.n1, t, T);
}

// lv: the launch's sinks (fresh / fresh_stride / the descriptors); most: the most samples any stream brings (<= the staging
// block's capacity).  A long block of few streams is cut over several workgroups per stream: 4,096 samples per workgroup.
hipError_t launch_live_audio_store(const LiveSinks& lv, const LiveAudio& a, int S, int64_t most, hipStream_t st) {
    if (S <= 0 || most <= 0) return hipSuccess;
    if (S > 65535 || !lv.fresh || !lv.streams || !a.ring || a.W < 1 || a.stride < a.W || a.form < 1 || a.form > 2 || a.hop < 1 || a.n < a.hop)
        return hipErrorInvalidValue;
    const int64_t pieces = std::min<int64_t>((std::min<int64_t>(most, a.W) + 4095) / 4096, 1024);
    hipLaunchKernelGGL(live_audio_store_kernel, dim3((unsigned)pieces, (unsigned)S), dim3(256), 0, st, lv, a);
    return hipGetLastError();
}

// Grid (pieces, streams): samples [first, first + count) of stream stream0 + blockIdx.y -> out[blockIdx.y][0 .. count).  The
// range is the same one or two slot runs in every stream (v.slot0 / v.n0 / v.n1, from audio_runs on the host); what differs per
// stream is the destination's alignment when the stride is not a multiple of four samples.
__global__ __launch_bounds__(256) void audio_view_kernel(AudioView v) {
    const int sv = (int)blockIdx.y;
    const uint32_t* ring = v.ring + (size_t)(v.stream0 + sv) * (size_t)v.stride;
    uint32_t* dst = v.out + (size_t)sv * (size_t)v.out_stride;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, T = (long long)gridDim.x * 256;
    audio_copy_run(ring + v.slot0, dst, v.n0, t, T);
    audio_copy_run(ring, dst + v.n0, v.n1, t, T);
}

// v: the view (emspec_launch.h); streams: how many from v.stream0 on.  The caller has validated the range against every addressed
// stream (emspec_audio_plan.h: audio_view_check).  4,096 samples per workgroup, at most 2,048 workgroups per stream.
hipError_t launch_audio_view(const AudioView& v, int streams, hipStream_t st) {
    if (streams <= 0) return hipSuccess;
    if (streams > 65535 || !v.ring || !v.out || reinterpret_cast<uintptr_t>(v.out) % 4 || v.W < 1 || v.stride < v.W || v.slot0 < 0 ||
        v.slot0 >= v.W || v.n0 < 1 || v.n1 < 0 || v.slot0 + v.n0 > v.W || v.n0 + v.n1 > v.W || v.out_stride < v.n0 + v.n1 || v.stream0 < 0)
        return hipErrorInvalidValue;
    const int64_t pieces = std::min<int64_t>((v.n0 + v.n1 + 4095) / 4096, 2048);
    hipLaunchKernelGGL(audio_view_kernel, dim3((unsigned)pieces, (unsigned)streams), dim3(256), 0, st, v);
    return hipGetLastError();
}

}  // namespace emspec
