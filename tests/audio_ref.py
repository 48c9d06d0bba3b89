"""numpy restatement of the live audio history (include/emspec.h: emspec_set_live_audio; DESIGN.md §3.15, §4.17;
em-spec_amd/csrc/emspec_audio_plan.h): a ring of W samples per stream, sample a in slot a mod W, fed by every launch of a
streaming session with the samples that launch moves to the device.  `Session` replays a script of calls - pushes of blocks,
frames, flushes, resets - with the session's own staging rule (emspec_live_plan.h: a block that completes no frame only joins
the staging block until a frame is due or the block is full) and says what each stream's ring holds after every call.

Samples are kept as their 32 bits (uint32): a NaN's payload and a zero's sign are bits like any other."""
import numpy as np

MAX_SAMPLES = 1 << 28


def slot(a, W):
    return a % W


def first_held(end, W):
    return max(0, end - W)


def stride(W):
    return (W + 3) // 4 * 4


def ring_bytes(S, W):
    return S * stride(W) * 4


def runs(a0, count, W):
    """The slots samples [a0, a0 + count) occupy, in order: [slot0, slot0 + n0), then [0, n1)."""
    slot0 = a0 % W
    n0 = min(count, W - slot0)
    return slot0, n0, count - n0


def view_fits(first, count, stride_, end, W):
    return count >= 1 and stride_ >= count and first_held(end, W) <= first < end and first + count <= end


def split(sa, da, count):
    """head / 16-byte body / tail of a run between blocks sa and da samples behind a 16-byte boundary."""
    if sa != da:
        return count, 0, 0
    head = min((4 - sa) % 4, count)
    body = (count - head) // 4
    return head, body, count - head - 4 * body


def bits(x):
    """float32 (or uint32) array -> its words."""
    x = np.ascontiguousarray(x)
    return x if x.dtype == np.uint32 else x.astype(np.float32, copy=False).view(np.uint32)


class Ring:
    """One stream's ring: W slots of 32 bits, and the sample each slot holds (-1: none)."""

    def __init__(self, W):
        assert 1 <= W <= MAX_SAMPLES
        self.W = W
        self.end = 0
        self.words = np.zeros(W, np.uint32)
        self.holds = np.full(W, -1, np.int64)

    def launch(self, words, a0):
        """A launch brings samples [a0, a0 + len(words)): its last W are stored, each in a slot of its own."""
        words = bits(words)
        n = len(words)
        if n == 0:
            return
        keep = min(n, self.W)
        a = np.arange(a0 + n - keep, a0 + n, dtype=np.int64)
        at = a % self.W
        assert len(set(at.tolist())) == keep   # (no slot twice in one launch)
        self.words[at] = words[n - keep:]
        self.holds[at] = a
        self.end = a0 + n

    def held(self):
        return self.end, first_held(self.end, self.W)

    def view(self, first, count):
        assert view_fits(first, count, count, self.end, self.W), (first, count, self.held())
        at = (first + np.arange(count, dtype=np.int64)) % self.W
        assert np.array_equal(self.holds[at], first + np.arange(count, dtype=np.int64))
        return self.words[at].copy()


def frames_after(total, n, hop):
    return (total - n) // hop + 1 if total >= n else 0


class Session:
    """A streaming session of S streams with an audio history of W samples: form "block" (emspec_push_samples*) or "frame"
    (emspec_column / emspec_columns*).  pcm: a PCM session, whose emspec_reset_stream first moves what is staged to the device."""

    def __init__(self, S, n, hop, W, form="block", pcm=False):
        self.S, self.n, self.hop, self.W, self.form, self.pcm = S, n, hop, W, form, pcm
        self.mmax = 1 if form == "frame" else max(1, min(max(8, min(64, 2048 // max(1, S))), (1 << 17) // hop))
        self.cap = n if form == "frame" else self.mmax * hop
        self.fed = [0] * S
        self.seen = [0] * S
        self.newbase = [0] * S
        self.staged = [np.zeros(0, np.uint32) for _ in range(S)]
        self.rings = [Ring(W) for _ in range(S)]
        self.launches = 0

    def _launch(self):
        for s in range(self.S):
            self.rings[s].launch(self.staged[s], self.newbase[s])
            self.rings[s].end = self.seen[s]   # (also when the launch brought nothing for the stream)
            self.newbase[s] = self.seen[s]
            self.staged[s] = np.zeros(0, np.uint32)
        self.launches += 1

    def push(self, block):
        """emspec_push_samples*: block [S][count]."""
        assert self.form == "block"
        block = bits(block).reshape(self.S, -1)
        count, used = block.shape[1], 0
        while used < count:
            maxpend = max(len(x) for x in self.staged)
            take = min(count - used, self.cap - maxpend)
            for s in range(self.S):
                self.staged[s] = np.concatenate([self.staged[s], block[s, used:used + take]])
                self.seen[s] += take
            used += take
            M = [frames_after(self.seen[s], self.n, self.hop) - self.fed[s] for s in range(self.S)]
            if max(M) == 0 and maxpend + take < self.cap:
                continue
            self._launch()
            for s in range(self.S):
                self.fed[s] += M[s]

    def frames(self, frames):
        """emspec_column / emspec_columns*: frames [S][n]; frame j is samples [j hop, j hop + n)."""
        assert self.form == "frame"
        frames = bits(frames).reshape(self.S, self.n)
        for s in range(self.S):
            j = self.fed[s]
            if j == 0:
                self.rings[s].launch(frames[s], 0)
            else:
                self.rings[s].launch(frames[s, self.n - self.hop:], j * self.hop + self.n - self.hop)
            self.fed[s] += 1
        self.launches += 1

    def flush(self):
        """emspec_column_flush / emspec_columns_flush: stores nothing."""

    def reset_stream(self, s):
        if self.pcm and len(self.staged[0]):
            self._launch()
        self.fed[s] = self.seen[s] = self.newbase[s] = 0
        self.staged[s] = np.zeros(0, np.uint32)
        self.rings[s] = Ring(self.W)

    def held(self, s):
        return self.rings[s].held()

    def view(self, first, count, stream0=0, streams=None):
        streams = self.S - stream0 if streams is None else streams
        return np.stack([self.rings[s].view(first, count) for s in range(stream0, stream0 + streams)])
