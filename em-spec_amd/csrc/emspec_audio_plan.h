// emspec_audio_plan.h — internal: the arithmetic of the live audio history (include/emspec.h: emspec_set_live_audio,
// emspec_audio_view, emspec_audio_batch): a ring of the last W samples per stream of a streaming
// session, fed by every launch that moves samples to the device, and views that read a range back bit for bit.  Where a sample
// lives, what the ring holds, which of a launch's samples are stored, the per-frame form's "not yet stored" rule, the two runs a
// range occupies across the wrap, whether a view fits, the ring's size, and how a run splits into a scalar head, a 16-byte body
// and a scalar tail.  Integer arithmetic only.  No HIP, nothing of the engine: tests/test_audio_plan_cpu.py runs it through a
// stand-alone program (tests/cdriver/audio_plan_driver.cpp) without a GPU.  Host and kernels (live_audio.hip.inc) share it.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef EMSPEC_HD
#ifdef __HIPCC__
#define EMSPEC_HD __host__ __device__
#else
#define EMSPEC_HD
#endif
#endif

namespace emspec {

constexpr int64_t kAudioMaxSamples = (int64_t)1 << 28;   // W per stream, at most

// Sample a of a stream - the a-th sample its session has received since the stream was (re)started - lives in slot a mod W.
EMSPEC_HD inline int64_t audio_slot(int64_t a, int64_t W) { return a % W; }
// After `end` samples were stored the ring holds [audio_first(end, W), end).
EMSPEC_HD inline int64_t audio_first(int64_t end, int64_t W) { return end > W ? end - W : 0; }
// The ring of a stream starts on a 16-byte boundary whatever W is: its stride is W rounded up to four samples, so that slot
// and address agree modulo 16 bytes in every stream.
EMSPEC_HD inline int64_t audio_stride(int64_t W) { return (W + 3) & ~(int64_t)3; }
inline size_t audio_ring_bytes(int S, int64_t W) { return (size_t)S * (size_t)audio_stride(W) * 4; }

// What a launch brings for one stream: `count` samples, the first of them absolute sample a0, `src` samples into the
// stream's block of fresh samples.  count == 0: nothing.
struct AudioRange { int64_t src, a0, count; };
// Block form (form 2): fresh[i] is absolute sample newbase + i, i < newcount - all of them new.
// Per-frame form (form 1): the stream's block is frame j0 = samples [j0 hop, j0 hop + n); the ring has everything below
// (j0 - 1) hop + n, so frame 0 is stored whole and every later frame's last `hop` samples are (the library does not check that
// consecutive frames overlap consistently).  A stream without a frame in the launch, and a flush, bring nothing.
EMSPEC_HD inline AudioRange audio_fresh(int form, int64_t j0, int64_t newbase, int64_t newcount, int frames, int flush, int n, int hop) {
    if (flush || form == 0) return AudioRange{0, 0, 0};
    if (form == 2) return AudioRange{0, newbase, newcount > 0 ? newcount : 0};
    if (frames < 1) return AudioRange{0, 0, 0};
    if (j0 == 0) return AudioRange{0, 0, n};
    return AudioRange{n - hop, j0 * hop + n - hop, hop};
}
// ... of which the last W are stored: W consecutive samples have W distinct slots, so no slot is written twice in one launch.
EMSPEC_HD inline AudioRange audio_keep(AudioRange r, int64_t W) {
    if (r.count <= W) return r;
    const int64_t skip = r.count - W;
    return AudioRange{r.src + skip, r.a0 + skip, W};
}
// the samples stored after a session's counters say so: block form `newbase` (the samples moved to the device so far),
// per-frame form (fed - 1) hop + n once a frame was fed
EMSPEC_HD inline int64_t audio_end(int form, int64_t fed, int64_t newbase, int n, int hop) {
    if (form == 2) return newbase;
    return form == 1 && fed > 0 ? (fed - 1) * hop + n : 0;
}

// The slots samples [a0, a0 + count) occupy, in sample order: [slot0, slot0 + n0), then, across the wrap, [0, n1)
// (count <= W; n0 >= 1 when count >= 1, n0 + n1 = count)
struct AudioRuns { int64_t slot0, n0, n1; };
EMSPEC_HD inline AudioRuns audio_runs(int64_t a0, int64_t count, int64_t W) {
    const int64_t slot0 = audio_slot(a0, W);
    const int64_t n0 = count < W - slot0 ? count : W - slot0;
    return AudioRuns{slot0, n0, count - n0};
}

// A view of samples [first, first + count) of one stream whose ring holds [audio_first(end, W), end), into rows `stride`
// samples apart.  (No sum or product overflows: count is compared with end - first, both in 0 .. 2^63 - 1.)
enum AudioViewError { kAudioViewOk = 0, kAudioViewArg = 1, kAudioViewRange = 2 };
inline int audio_view_check(int64_t first, int64_t count, int64_t stride, int64_t end, int64_t W) {
    if (count < 1 || stride < count || W < 1 || end < 0) return kAudioViewArg;
    if (first < audio_first(end, W) || first >= end) return kAudioViewRange;
    return count <= end - first ? kAudioViewOk : kAudioViewRange;
}

// A run of `count` samples copied from a source whose first sample sits sa samples behind a 16-byte boundary to a destination
// da samples behind one (sa, da in 0 .. 3): when they agree, `head` single samples bring both to a boundary, `body` groups of
// four move as 16 bytes, `tail` single samples remain; when they differ no 16-byte access serves both sides and the whole run
// goes sample by sample (head = count).
struct AudioSplit { int64_t head, body, tail; };
EMSPEC_HD inline AudioSplit audio_split(int sa, int da, int64_t count) {
    if (sa != da) return AudioSplit{count, 0, 0};
    int64_t head = (4 - sa) & 3;
    if (head > count) head = count;
    const int64_t body = (count - head) >> 2;
    return AudioSplit{head, body, count - head - 4 * body};
}
// samples behind a 16-byte boundary of an address that is 4-byte aligned
EMSPEC_HD inline int audio_align(uintptr_t p) { return (int)((p >> 2) & 3); }

}  // namespace emspec
