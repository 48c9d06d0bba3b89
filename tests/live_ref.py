"""The streaming session's host arithmetic restated in pure Python (the comments of LiveState in
em-spec_amd/csrc/emspec_engine.h): the geometry of a session, the sizes of its buffers, and - stream by stream - which samples a
call stages, which frames it launches and which columns it reports.  Written from those rules, one stream object at a time;
tests/test_live_plan_cpu.py compares it field for field with what em-spec_amd/csrc/emspec_live_plan.h computes.

The rules.  A stream has received `seen` samples; frame j is samples [j hop, j hop + n), so floor((seen - n) / hop) + 1 frames are
whole.  Frame j adds energy to columns j - D .. j + D, so column c is final once frame c + D is fed: a stream that has fed f frames
has emitted max(f - D, 0) columns - unless it was flushed, which emits the columns still pending one by one and puts the stream at
its end.  New samples wait in a page-locked staging block of `cap` samples per stream until a launch moves them to the stream's
ring on the device; a launch takes at most mmax frames per stream.

The kernels of a launch (Session._steps), written from live_launch of em-spec_amd/csrc/emspec_live.cpp as it stood before the
launch plan became data: the long band first, then - only when some stream has a frame, or on a flush - the short band.  A band's
flush is one finalize kernel over 1 column.  Otherwise its frame kernel runs with the launch's most frames per stream as
workgroups (the short band: 2 shift more while some stream is at its first frame), finalising in place unless the launch
completes more than 2 columns per stream or the band's fft size is below 2048; then a finalize kernel over that many columns
follows directly - none when no stream has a frame."""
from dataclasses import dataclass

INLINE = 2                                  # columns per stream a frame kernel finalises in place, at most
FRAMES, FINALIZE, FINALIZE_BANDS = 0, 1, 2  # a step: [what, band, workgroups per stream, columns, defers, carries the ingest]


def latency(n, hop, reassign):
    return -(-n // (2 * hop)) if reassign else 0


def whole_frames(samples, n, hop):
    return (samples - n) // hop + 1 if samples >= n else 0


def geometry(S, n, hop, reassign, form, n_high=0, split=0):
    """form 1: one frame per stream and call; form 2: blocks of samples.  n_high: the multi-resolution session's short band."""
    D = latency(n, hop, reassign)
    if form == 1:
        mmax, cap = 1, n                         # the staging block is the frame itself
    else:
        # about 2,048 workgroups per launch, 8 to 64 frames per stream - and a staging block of at most 2^17 samples per stream
        mmax = max(1, min(max(8, min(64, 2048 // S)), 2 ** 17 // hop))
        cap = mmax * hop
    ring = 1
    while ring < n + cap:                        # what a launch's ingest overwrites is older than anything its frames read
        ring *= 2
    g = dict(S=S, n=n, hop=hop, reassign=reassign, D=D, form=form, mmax=mmax, slots=2 * D + mmax, cap=cap, ring_mask=ring - 1,
             n_high=n_high, split=split if n_high else 0, shift=0, D_high=0, slots_high=0)
    if n_high:
        # the short band's frame j + 2 shift ends on the long band's frame j; its ring is indexed by the emitted column
        g["shift"] = (n - n_high) // (2 * hop)
        g["D_high"] = latency(n_high, hop, reassign)
        g["slots_high"] = mmax + g["shift"] + D + g["D_high"]
    return g


def sizes(g, R, cell, views, frame_bytes, cols):
    """Bytes (out_cell, fresh_at: cells / samples).  cell: 4 (FAST, float32) or 8 (EXACT, u64) per ring cell."""
    S, cap = g["S"], g["cap"]
    low_rows, high_rows = (g["split"], R - g["split"]) if g["n_high"] else (R, 0)
    sources = S // views
    return dict(ring_bytes=g["slots"] * low_rows * cell, ring_high_bytes=g["slots_high"] * high_rows * cell,
                rings_bytes=S * g["slots"] * low_rows * cell, rings_high_bytes=S * g["slots_high"] * high_rows * cell,
                sring_bytes=S * (g["ring_mask"] + 1) * 4, done_bytes=4 * S * (2 if g["n_high"] else 1), desc_bytes=32 * S,
                fresh_bytes=4 * S * cap, decoded_bytes=4 * S * cap, raw_bytes=sources * cap * frame_bytes, raw_stride=cap * frame_bytes,
                out_bytes=4 * S * cols * R, out1_bytes=4 * S * R, out_cell=((S - 1) * cols + cols - 1) * R, columns_bytes=4 * cols * R,
                fresh_at=(S - 1) * cap + 5, raw_at=((sources - 1) * cap + 5) * frame_bytes, pstate_bytes=4 * (R + 4))


@dataclass
class Stream:
    fed: int = 0        # frames launched
    emitted: int = 0    # columns reported
    seen: int = 0       # samples received
    in_ring: int = 0    # samples a launch has moved to the device ring
    staged: int = 0     # samples waiting in the staging block

    def due(self, D):
        """Columns final by the frames alone."""
        return max(self.fed - D, 0)


class Session:
    def __init__(self, S, n, hop, reassign, form, n_high=0, split=0, views=0, frame_bytes=1):
        self.g = geometry(S, n, hop, reassign, form, n_high, split)
        self.st = [Stream() for _ in range(S)]
        self.views, self.frame_bytes = views, frame_bytes
        self.zero = [set() for _ in range(2 if n_high else 1)]   # per band: streams whose ring a reset has cleared

    def _steps(self, mlaunch, flush, priming):
        g, steps = self.g, []
        bands = [(g["n"], 0)] + ([(g["n_high"], 2 * g["shift"])] if g["n_high"] else [])
        for k, (n, ahead) in enumerate(bands):
            if k and not (flush or mlaunch > 0):
                continue
            if flush:
                steps.append([FINALIZE, k, 0, 1, 0, 0])
                continue
            defer = mlaunch > INLINE or n < 2048
            steps.append([FRAMES, k, mlaunch + (ahead if priming and k else 0), 0, int(defer), int(k == 0)])
            if defer and mlaunch > 0:
                steps.append([FINALIZE, k, 0, mlaunch, 0, 0])
        return steps

    # ---- what the driver prints after every call ----
    def _launch(self, desc, launched=1, take=0, maxpend=0, mx=0, at=(), nc=()):
        if not launched:
            return dict(launched=0, flush=0, mlaunch=0, take=take, maxpend=maxpend, mx=mx, uniform=0, priming=0, at=list(at), nc=list(nc),
                        desc=[], steps=[])
        flush = int(any(d[5] for d in desc))
        mlaunch = max(d[2] for d in desc)
        priming = int(any(d[0] == 0 and d[2] > 0 for d in desc))
        return dict(launched=1, flush=flush, mlaunch=mlaunch, take=take, maxpend=maxpend, mx=mx,
                    uniform=int(all(d == desc[0] for d in desc)), priming=priming, at=list(at), nc=list(nc), desc=[list(d) for d in desc],
                    steps=self._steps(mlaunch, bool(flush), bool(priming)))

    def _call(self, op, arg=0, predict=-1, refused="", launches=(), counts=(), first=()):
        st = self.st
        return dict(op=op, arg=arg, predict=predict, refused=refused, launches=list(launches), counts=list(counts), first=list(first),
                    fed=[x.fed for x in st], emitted=[x.emitted for x in st], seen=[x.seen for x in st],
                    newbase=[x.in_ring for x in st], pend=[x.staged for x in st], pending=[int(x.fed > x.emitted) for x in st],
                    any_pending=int(any(x.fed > x.emitted for x in st)), cleared=[len(z) for z in self.zero])

    def _refusal(self):
        D = self.g["D"]
        for s, x in enumerate(self.st):
            if x.emitted > x.due(D):     # only a flush reports a column before its last frame
                return "stream %d was flushed" % s
        return ""

    # ---- the calls ----
    def frame(self):
        why = self._refusal()
        if why:
            return self._call("frame", refused=why)
        D, hop = self.g["D"], self.g["hop"]
        # every stream: its next frame, whose samples start at frame index * hop; nothing staged, output slot 0
        desc = [(x.fed, x.fed * hop, 1, 0, 0, 0) for x in self.st]
        cols = []
        for x in self.st:
            x.fed += 1
            if x.fed > D:
                x.emitted = x.fed - D
                cols.append(x.emitted - 1)
            else:
                cols.append(-1)
        return self._call("frame", launches=[self._launch(desc)], first=cols)

    def flush(self):
        if not any(x.fed > x.emitted for x in self.st):
            return self._call("flush", refused="no pending column")
        D = self.g["D"]
        desc, cols = [], []
        for x in self.st:
            if x.fed > x.emitted:        # finalise column `emitted`: the kernel is told the frame that would have completed it
                desc.append((x.emitted + D, 0, 0, 0, 0, 1))
                cols.append(x.emitted)
                x.emitted += 1
            else:                        # "column -1": the empty column
                desc.append((D - 1, 0, 0, 0, 0, 1))
                cols.append(-1)
        return self._call("flush", launches=[self._launch(desc)], first=cols)

    def predict(self, count):
        g = self.g
        most = 0
        for x in self.st if g["form"] == 2 else [Stream()]:      # no session of the block form: as for a fresh stream
            after = max(whole_frames(x.seen + count, g["n"], g["hop"]) - g["D"], 0)
            most = max(most, after - x.due(g["D"]))
        return most

    def push(self, count, direct):
        why = self._refusal()
        if why:
            return self._call("push", arg=count, refused=why)
        g, st = self.g, self.st
        S, n, hop, D, cap = g["S"], g["n"], g["hop"], g["D"], g["cap"]
        predict = self.predict(count)
        produced, first, launches = [0] * S, [-1] * S, []
        left = count
        while left > 0:
            fullest = max(x.staged for x in st)
            take = min(left, cap - fullest)              # every stream takes the same share of the block
            if self.views:                               # raw frames per source, all streams equally full
                at = [(i * cap + fullest) * self.frame_bytes for i in range(S // self.views)]
            else:
                at = [s * cap + x.staged for s, x in enumerate(st)]
            for x in st:
                x.staged += take
                x.seen += take
            left -= take
            frames = [whole_frames(x.seen, n, hop) - x.fed for x in st]
            mx = max(frames)
            if mx == 0 and fullest + take < cap:         # nothing to transform and room left: no launch
                launches.append(self._launch([], launched=0, take=take, maxpend=fullest, mx=0, at=at))
                continue
            desc, nc = [], []
            for s, x in enumerate(st):
                desc.append((x.fed, x.in_ring, frames[s], x.staged, produced[s] if direct else 0, 0))
                before = x.due(D)
                x.fed += frames[s]
                x.in_ring, x.staged = x.seen, 0
                new = x.due(D) - before
                nc.append(new)
                if new > 0:
                    if first[s] < 0:
                        first[s] = before
                    produced[s] += new
                    x.emitted = x.due(D)
            launches.append(self._launch(desc, take=take, maxpend=fullest, mx=mx, at=at, nc=nc))
        return self._call("push", arg=count, predict=predict, launches=launches, counts=produced, first=first)

    def reset(self, s):
        launches = []
        if self.views and self.st[0].staged:             # a PCM session first moves what is staged into the rings: no frame
            desc = [(x.fed, x.in_ring, 0, x.staged, 0, 0) for x in self.st]
            for x in self.st:
                x.in_ring, x.staged = x.seen, 0
            launches.append(self._launch(desc))
        self.st[s] = Stream()
        for z in self.zero:                              # every band's ring of the stream
            z.add(s)
        return self._call("reset", arg=s, launches=launches)


def open_line(kind, S, hop, reassign, form, R, n, split, views=0, fb=1):
    """The driver's first line.  kind: 1 single-resolution, 2 two-band, 3 multi-band."""
    return "open " + " ".join(map(str, [kind, S, hop, reassign, form, R, views, fb, len(n)] + list(n) + list(split)))


def parse_open(line):
    w = list(map(int, line.split()[1:]))
    K = w[8]
    return dict(kind=w[0], S=w[1], hop=w[2], reassign=w[3], form=w[4], R=w[5], views=w[6], fb=w[7], n=w[9:9 + K], split=w[9 + K:8 + 2 * K])


def run(script, session=None):
    """script: the driver's lines.  -> the list of objects the driver prints.  session: what an `open` line makes (default: the
    single-resolution or two-band session here)."""
    out, t = [], None
    for line in script:
        w = line.split()
        if w[0] == "open":
            o = parse_open(line)
            if session:
                t = session(o)
            else:
                assert o["kind"] == len(o["n"]) <= 2
                t = Session(o["S"], o["n"][0], o["hop"], o["reassign"], o["form"], *(o["n"][1:] + o["split"]), views=o["views"],
                            frame_bytes=o["fb"])
        elif w[0] == "frame":
            out.append(t.frame())
        elif w[0] == "flush":
            out.append(t.flush())
        elif w[0] == "push":
            out.append(t.push(int(w[1]), int(w[2]) != 0))
        elif w[0] == "predict":
            out.append(t._call("predict", arg=int(w[1]), predict=t.predict(int(w[1]))))
        elif w[0] == "reset":
            out.append(t.reset(int(w[1])))
        else:
            raise ValueError(line)
    return out
