"""GPU: the stream contract of every device entry under forced delays (include/emspec.h, "Streams and ordering"; DESIGN.md §4,
"Stream ordering under forced delays"; the helper and the case table: tests/stream_order.py).

A. All of an entry's work is on its stream, and the entry does not synchronise: the stream is held back by a measured delay in
   front of the copy that brings the real input and of the fill that poisons the outputs.  Work on any other stream runs on the
   decoy the input still holds; a fill or start-value pass on another stream is lost under the poison.
B. Later streaming calls are ordered behind a view: with the view held back, a push that overwrites every slot it reads, a
   reset_stream and a push, or the release of the ring must leave the view's bytes those of the ring before the follow-up.
C. The EXACT low-row scratch orders two streams by itself; a regrow waits for the launch that still uses the old buffer.
D. Calls the caller orders with an event share the engine's workspaces and tables across two streams.

Every comparison is the entry's own suite's: bytes in EXACT mode and for the integer entries, the bounds of
tests/test_gpu_route.py for the FAST routes.  Every delay is max(50 ms, 20 x the measured unobstructed duration of the step it
holds back), printed as a MEASURED line."""
import time

import numpy as np
import pytest
import torch

import audio_ref as A
import emspec
import history_ref as H
import oracle as O
import post_ref as P
import stereo_ref as T
import stream_order as SO
from stream_order import Guarded, delay, delay_ms_for, side_stream
from test_gpu_route import PLANS

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
VN, VHOP, VROWS, VW = 1024, 256, 64, 16           # the live sessions: FFT 1024 / hop 256 (D = 2), 64 rows, a ring of 16 columns
AW = VN + 16 * VHOP                               # ... or of n + 16 hop samples
LUT = H.colour_map()


@pytest.fixture(scope="module")
def engines(engine):
    """Engines by (mode, rows, axis), made on demand, closed with the module.  (`engine`: the session's engine has settled the
    torch / HIP load order.)"""
    made = {}

    def get(mode, rows, axis):
        if (mode, rows, axis) not in made:
            e = emspec.Engine(mode=emspec.MODE_EXACT if mode == "exact" else emspec.MODE_FAST, rows=rows)
            if axis:
                e.set_row_edges_hz(SO.edges_of(rows, axis))
            made[mode, rows, axis] = e
        return made[mode, rows, axis]
    yield get
    for e in made.values():
        e.close()


def _outputs(spec):
    return {k: Guarded(dtype, shape) for k, (dtype, shape) in spec.items()}


def _tensors(outs):
    return {k: g.tensor for k, g in outs.items()}


def _timed(call):
    """A warm call, then the unobstructed host-side duration of a second one plus a synchronise."""
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _done(e):
    torch.cuda.synchronize()
    e.device_status()


# ---- A. all of an entry's work is on its stream, and the entry does not synchronise -------------------------------------------
@pytest.mark.timeout(60)
@pytest.mark.parametrize("case", SO.INPUT_CASES, ids=repr)
def test_an_entrys_work_is_on_its_stream_and_it_does_not_synchronise(engines, case):
    e = engines(*case.engine)
    real, decoy = case.inputs("real"), case.inputs("decoy")
    want = case.reference(real)
    x = torch.from_numpy(np.array(decoy)).cuda()
    pinned = torch.from_numpy(np.array(real)).pin_memory()
    outs = _outputs(case.outputs)
    tens = _tensors(outs)
    cur = torch.cuda.current_stream()
    if case.null:
        assert cur.cuda_stream == 0
        st, given = cur, SO.NULL_STREAM
    else:
        st = given = side_stream(e)
    case.setup(e)
    try:
        ms = delay_ms_for(_timed(lambda: case.call(e, x, tens, cur)), case.id)
        delay(st, ms)
        with torch.cuda.stream(st):
            x.copy_(pinned, non_blocking=True)
        for g in outs.values():
            g.poison(st)
        gate = torch.cuda.Event()
        gate.record(st)
        assert not gate.query(), "the delay ran out before the entry was called"
        case.call(e, x, tens, given)
        held = not gate.query()
        if case.null:
            torch.cuda.synchronize()
        else:
            st.synchronize()
    finally:
        case.teardown(e)
    assert held or case.blocks, "the entry returned only after the work in front of it on its stream had run: it synchronises"
    got = {k: g.read() for k, g in outs.items()}
    assert case.mismatch(got, want) == {}
    _done(e)


# ---- live sessions with a ring: the views' input ------------------------------------------------------------------------------
class Live:
    """A session of S streams on an EXACT engine, fed in blocks.  Every delivered column is held against the live reference -
    the bit model's batch columns of the stream since its (re)start - and handed to the ring models (history_ref, audio_ref),
    whose held ranges the engine must report after every call."""

    def __init__(self, e, S, session, history=0, audio=0, samples=VN + 200 * VHOP):
        self.e, self.S, self.session = e, S, session
        self.pcm = H.signal(S, samples)
        self.fed, self.origin, self.refs = 0, [0] * S, {}
        e.set_colormap(LUT)
        if history:
            e.set_live_history(history)
        if audio:
            e.set_live_audio(audio)
        self.hist = H.History(S, history, e.rows) if history else None
        self.audio = A.Session(S, VN, VHOP, audio) if audio else None

    def live_ref(self, s):
        key = (s, self.origin[s])
        if key not in self.refs:
            cfg = O.make_cfg(VN, VHOP, True, rows=self.e.rows)
            self.refs[key] = O.batch_exact(cfg, self.pcm[s:s + 1, self.origin[s]:], want=("db",))[0][0]
        return self.refs[key]

    def push(self, count):
        a, e = self.fed, self.e
        assert a + count <= self.pcm.shape[1]
        if self.session == "multi":
            db, _, counts, firsts = e.push_samples_multi(self.pcm, VN, VHOP, True, count=count, offset=a)
            per = [db[s, :counts[s]].copy() for s in range(self.S)]
        else:
            db, first = e.push_samples(self.pcm[0, a:a + count], VN, VHOP, True)
            per, firsts = [np.array(db, F).reshape(-1, e.rows)], [first]
        self.fed += count
        for s in range(self.S):
            k = len(per[s])
            ref = self.live_ref(s)[int(firsts[s]):int(firsts[s]) + k] if k else per[s]
            assert ref.shape == per[s].shape and np.array_equal(ref.view(U), per[s].view(U)), \
                f"stream {s}: the delivered columns differ from the live reference"
        if self.hist:
            self.hist.launch(per)
        if self.audio:
            self.audio.push(self.pcm[:, a:a + count])
        self.held()
        return sum(len(p) for p in per)

    def held(self):
        for s in range(self.S):
            if self.hist:
                assert self.e.live_history(s, self.session) == self.hist.held(s)
            if self.audio:
                assert self.e.live_audio(s, self.session) == self.audio.held(s)

    def reset_stream(self, s):
        self.e.reset_stream(s)
        self.origin[s] = self.fed
        if self.hist:
            self.hist.reset_stream(s)
        if self.audio:
            self.audio.reset_stream(s)

    def release(self):
        """set_live_history(0) / set_live_audio(0): always allowed, frees the ring; the session goes on without it."""
        if self.hist:
            self.e.set_live_history(0)
            assert self.e.live_history(0, self.session) is None
        if self.audio:
            self.e.set_live_audio(0)
            assert self.e.live_audio(0, self.session) is None
        self.hist = self.audio = None


def _live(method, session="multi", S=None):
    """An EXACT engine and its session for a view of `method`, filled past one wrap -> (engine, Live, seconds): the unobstructed
    duration of a push of a ring's worth, the follow-up that the views hold back."""
    audio = method.startswith("audio")
    S = (1 if session == "one" else 4 if "stereo" in method else 3) if S is None else S
    e = emspec.Engine(mode=emspec.MODE_EXACT, rows=VROWS)
    lv = Live(e, S, session, history=0 if audio else VW, audio=AW if audio else 0)
    lv.push(VN + 5 * VHOP)
    fill = AW if audio else VW * VHOP
    t0 = time.perf_counter()
    lv.push(fill)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    lv.push(3 * VHOP)
    if audio:
        end, first = lv.audio.held(0)
        assert end > AW + VN and first == end - AW, "the audio ring has not wrapped"
    else:
        end, first = lv.hist.held(0)
        assert end > VW and first == end - VW, "the history ring has not wrapped"
    return e, lv, seconds


def _view(method, lv, n2=VN, hop2=VHOP):
    """The view of everything the ring holds -> (output spec, launch(tensors, stream), check(got)); the expectation is computed
    here, from the models, before any follow-up."""
    e, S, sess = lv.e, lv.S, lv.session
    if method == "history_view_device":
        end, first = lv.hist.held(0)
        f, groups = 2, VW // 2
        want = lv.hist.view(first, f, groups, map=H.VIEW_MAP, lut=LUT)
        spec = {"db": (F, (S, groups, VROWS)), "index": (np.uint8, (S, groups, VROWS)), "rgba": (np.uint8, (S, groups, VROWS, 4))}

        def launch(t, st):
            e.history_view_device(first, f, groups, map=H.VIEW_MAP, db=t["db"], index=t["index"], rgba=t["rgba"], session=sess, stream=st)

        def check(got):   # (tests/test_gpu_live_history.py: dB bytes, the index but for the cells index_borderline excuses, rgba = LUT[index])
            assert np.array_equal(got["db"].view(U), want["db"].view(U)), "the view's dB differs from the ring before the follow-up"
            border = P.index_borderline(want["shifted"], *H.VIEW_MAP[:3])
            diff = got["index"].astype(int) - want["index"].astype(int)
            assert np.all(diff[~border] == 0) and np.all(np.abs(diff) <= 1) and np.count_nonzero(diff) <= max(1, diff.size // 1000)
            assert np.array_equal(got["rgba"], LUT[got["index"]])
    elif method == "history_view_stereo_device":
        end, first = lv.hist.held(0)
        f, groups, pairs = 2, VW // 2, S // 2
        want = T.compose(lv.hist.view(first, f, groups)["db"], 2, 0, 1, T.VIEW_MAP)
        spec = {k: (F if k == "level" else np.uint8, (pairs, groups, VROWS)) for k in ("level", "index", "pan")}

        def launch(t, st):
            e.history_view_stereo_device(first, f, groups, 2, 0, 1, map=T.VIEW_MAP, want=(), session=sess, stream=st, **t)

        def check(got):
            assert SO.bytes_mismatch(got, {k: want[k] for k in spec}) == {}
    elif method == "audio_view_device":
        end, first = lv.audio.held(0)
        want = lv.audio.view(first, end - first)
        spec = {"pcm": (F, (S, end - first))}

        def launch(t, st):
            e.audio_view_device(first, end - first, t["pcm"], session=sess, stream=st)

        def check(got):
            assert np.array_equal(got["pcm"].view(U), want), "the view's samples differ from the ring before the follow-up"
    else:
        assert method == "audio_batch_device"
        end, first = lv.audio.held(0)
        held = np.ascontiguousarray(lv.audio.view(first, end - first)).view(F)
        cols = emspec.num_columns(end - first, n2, hop2)
        db, _, idx, _ = O.batch_exact(O.make_cfg(n2, hop2, True, rows=VROWS), held, want=("db", "index"))
        spec = {"db": (F, (S, cols, VROWS)), "index": (np.uint8, (S, cols, VROWS))}

        def launch(t, st):
            e.audio_batch_device(first, end - first, n2, hop2, True, db=t["db"], index=t["index"], session=sess, stream=st)

        def check(got):
            assert SO.bytes_mismatch(got, {"db": db, "index": idx}) == {}
    return spec, launch, check


@pytest.mark.timeout(60)
@pytest.mark.parametrize("case", SO.VIEW_CASES, ids=repr)
def test_a_views_work_is_on_its_stream_and_it_does_not_synchronise(case):
    """The views' input is the ring, filled by synchronising live calls: no decoy.  The late poison, the guards and the
    no-synchronise assertion apply."""
    e, lv, _ = _live(case.method)
    with e:
        st = side_stream(e, LUT)
        spec, launch, check = _view(case.method, lv)
        outs = _outputs(spec)
        tens = _tensors(outs)
        ms = delay_ms_for(_timed(lambda: launch(tens, torch.cuda.current_stream())), case.id)
        delay(st, ms)
        for g in outs.values():
            g.poison(st)
        gate = torch.cuda.Event()
        gate.record(st)
        assert not gate.query(), "the delay ran out before the entry was called"
        launch(tens, st)
        assert not gate.query(), "the view returned only after the work in front of it on its stream had run: it synchronises"
        st.synchronize()
        check({k: g.read() for k, g in outs.items()})
        assert lv.push(4 * VHOP) > 0                      # the session goes on, its columns those of the live reference
        _done(e)


# ---- B. later streaming calls are ordered behind the view ---------------------------------------------------------------------
FOLLOW_UPS = ("push", "reset_stream", "release")
VIEWS_B = ([(m, "multi", f) for m in ("history_view_device", "history_view_stereo_device", "audio_view_device", "audio_batch_device")
            for f in FOLLOW_UPS]
           + [("history_view_device", "one", "push"), ("audio_batch_device", "one", "push"), ("audio_view_device", "one", "release")])


@pytest.mark.timeout(60)
@pytest.mark.parametrize("method,session,follow", VIEWS_B, ids=lambda v: str(v))
def test_later_streaming_calls_are_ordered_behind_the_view(method, session, follow):
    S = 4 if "stereo" in method else 1 if session == "one" else 3
    e, lv, seconds = _live(method, session, S)
    with e:
        st = side_stream(e, LUT)
        ring = AW if lv.audio else VW * VHOP              # a push of this many samples overwrites every slot the view reads
        spec, launch, check = _view(method, lv)
        outs = _outputs(spec)
        for g in outs.values():
            g.poison(torch.cuda.current_stream())
        torch.cuda.synchronize()
        ms = delay_ms_for(seconds, f"{method} {session} {follow}: a push of a ring's worth")
        gate = torch.cuda.Event()
        delay(st, ms)
        gate.record(st)
        launch(_tensors(outs), st)
        assert not gate.query(), "the delay ran out before the follow-up"
        if follow == "push":
            lv.push(ring)
        elif follow == "reset_stream":
            lv.reset_stream(1)
            lv.push(ring + VN)
        else:
            lv.release()
        st.synchronize()
        check({k: g.read() for k, g in outs.items()})
        # the view has not disturbed the session: its next columns are the live reference's
        assert lv.push(6 * VHOP) > 0
        _done(e)


# ---- C. the self-ordered EXACT scratch ----------------------------------------------------------------------------------------
XN, XHOP, XROWS = 4096, 256, 1024


def _exact_outputs(S):
    return _outputs({"db": (F, (S, SO.FRAMES, XROWS)), "index": (np.uint8, (S, SO.FRAMES, XROWS))})


def _exact_equal(outs, which, S):
    db, idx = SO.model_columns(which, "exact", XN, XHOP, XROWS, 1, 0, S=S)
    assert SO.bytes_mismatch({k: g.read() for k, g in outs.items()}, {"db": db, "index": idx}) == {}, which


def _scratch_engine():
    """The shape's route keeps rl > 0 low rows in the global scratch: read from the plan fixture the CPU suite pins
    emspec_kernel_plan.h to, not assumed."""
    case = dict(n=XN, hop=XHOP, rows=XROWS, reassign=1, row0=0, axis_rows=XROWS, axis=0, parked=0, records=0)
    plan = [w for w in PLANS if w["kind"] == "exact" and w["case"] == case]
    assert plan and plan[0]["route"] == "exact_lr" and plan[0]["rl"] > 0, plan
    return emspec.Engine(mode=emspec.MODE_EXACT, rows=XROWS)


def _pair(e):
    a = side_stream(e)
    return a, side_stream(e, beside=a)


@pytest.mark.timeout(60)
def test_the_exact_scratch_orders_two_streams_by_itself():
    L = XN + (SO.FRAMES - 1) * XHOP
    with _scratch_engine() as e:
        sa, sb = _pair(e)
        x1, x2 = (torch.from_numpy(np.array(SO.pcm(w, 2, L))).cuda() for w in ("real", "decoy"))
        o1, o2 = _exact_outputs(2), _exact_outputs(2)
        run = lambda x, o, st: e.batch_device(x, XN, XHOP, True, db=o["db"].tensor, index=o["index"].tensor, stream=st)
        cur = torch.cuda.current_stream()
        run(x1, o1, cur)
        seconds = _timed(lambda: run(x2, o2, cur))
        ms = delay_ms_for(seconds, "exact scratch: call 2")
        hold = 5 * seconds
        print(f"MEASURED exact scratch: the host holds {hold * 1e3:.3f} ms")
        assert hold * 1e3 <= ms / 4
        for o in (o1, o2):
            for g in o.values():
                g.poison(cur)
        torch.cuda.synchronize()
        gate, eva, evb = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        delay(sa, ms)
        gate.record(sa)
        run(x1, o1, sa)
        eva.record(sa)
        run(x2, o2, sb)
        evb.record(sb)
        time.sleep(hold)
        b_done, a_done = evb.query(), eva.query()
        torch.cuda.synchronize()
        assert not a_done, "the delay was too short: the call on stream A had finished when the host looked"
        assert not b_done, "the call on stream B ran on the low-row scratch while the call on stream A was pending: the wait is missing"
        _exact_equal(o1, "real", 2)
        _exact_equal(o2, "decoy", 2)
        _done(e)


@pytest.mark.timeout(60)
def test_a_regrow_of_the_exact_scratch_waits_for_the_pending_call():
    """More streams on B need a larger scratch: the call may free the old one only after A's launch has finished with it, so it
    blocks the host until then (the `blocks` row batch_device-exact-scratch-regrow)."""
    L = XN + (SO.FRAMES - 1) * XHOP
    with _scratch_engine() as e:
        sa, sb = _pair(e)
        x1 = torch.from_numpy(np.array(SO.pcm("real", 2, L))).cuda()
        x2 = torch.from_numpy(np.array(SO.pcm("decoy", 4, L))).cuda()
        o1, o2 = _exact_outputs(2), _exact_outputs(4)
        run = lambda x, o, st: e.batch_device(x, XN, XHOP, True, db=o["db"].tensor, index=o["index"].tensor, stream=st)
        cur = torch.cuda.current_stream()
        ms = delay_ms_for(_timed(lambda: run(x1, o1, cur)), "exact scratch regrow: call 1")
        for o in (o1, o2):
            for g in o.values():
                g.poison(cur)
        torch.cuda.synchronize()
        gate, eva = torch.cuda.Event(), torch.cuda.Event()
        delay(sa, ms)
        gate.record(sa)
        run(x1, o1, sa)
        eva.record(sa)
        assert not gate.query(), "the delay ran out before the second call"
        run(x2, o2, sb)
        a_done = eva.query()
        torch.cuda.synchronize()
        assert a_done, "the call that regrows the scratch returned while the launch on the old buffer was pending"
        _exact_equal(o1, "real", 2)
        _exact_equal(o2, "decoy", 4)
        _done(e)


# ---- D. caller-ordered calls on two streams -----------------------------------------------------------------------------------
@pytest.mark.timeout(60)
def test_calls_the_caller_orders_with_an_event_share_the_workspaces():
    """Call 2 has a shape the engine has not seen - another n, more streams: its tables are uploaded and the record workspace
    regrown while call 1 is pending on the other stream."""
    (n1, hop1, S1), (n2, hop2, S2) = (4096, 227, 2), (2048, 127, 6)
    for n, hop in ((n1, hop1), (n2, hop2)):
        assert [w["route"] for w in PLANS if w["kind"] == "fast"
                and w["case"] == dict(n=n, hop=hop, rows=1024, reassign=1, no_fused=0, variant=0)][0] == "records_f32"
    L1, L2 = n1 + 24 * hop1, n2 + 24 * hop2
    with emspec.Engine() as e:
        sa, sb = _pair(e)
        x1 = torch.from_numpy(np.array(SO.pcm("real", S1, L1))).cuda()
        x2 = torch.from_numpy(np.array(SO.pcm("decoy", S2, L2))).cuda()
        spec = lambda S: {"db": (F, (S, SO.FRAMES, 1024)), "index": (np.uint8, (S, SO.FRAMES, 1024))}
        o1, o2 = _outputs(spec(S1)), _outputs(spec(S2))
        run = lambda x, n, hop, o, st: e.batch_device(x, n, hop, True, db=o["db"].tensor, index=o["index"].tensor, stream=st)
        cur = torch.cuda.current_stream()
        ms = delay_ms_for(_timed(lambda: run(x1, n1, hop1, o1, cur)), "caller-ordered records: call 1")
        for o in (o1, o2):
            for g in o.values():
                g.poison(cur)
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        delay(sa, ms)
        run(x1, n1, hop1, o1, sa)
        ev.record(sa)
        sb.wait_event(ev)
        run(x2, n2, hop2, o2, sb)
        torch.cuda.synchronize()
        for o, which, n, hop, S, L in ((o1, "real", n1, hop1, S1, L1), (o2, "decoy", n2, hop2, S2, L2)):
            db, _, idx = O.batch_f32(O.make_cfg(n, hop, True), SO.pcm(which, S, L), want=("db", "index"))
            assert SO.fast_mismatch({k: g.read() for k, g in o.items()}, {"db": db, "index": idx}) == {}, (n, hop)
        _done(e)


@pytest.mark.timeout(60)
def test_two_reanalyses_the_caller_orders_share_the_sample_workspace():
    e, lv, _ = _live("audio_batch_device")
    with e:
        sa = side_stream(e, LUT)
        sb = side_stream(e, LUT, beside=sa)
        plans = [_view("audio_batch_device", lv), _view("audio_batch_device", lv, 256, 128)]
        outs = [_outputs(p[0]) for p in plans]
        cur = torch.cuda.current_stream()
        ms = delay_ms_for(_timed(lambda: plans[0][1](_tensors(outs[0]), cur)), "caller-ordered re-analyses: call 1")
        for o in outs:
            for g in o.values():
                g.poison(cur)
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        delay(sa, ms)
        plans[0][1](_tensors(outs[0]), sa)
        ev.record(sa)
        sb.wait_event(ev)
        plans[1][1](_tensors(outs[1]), sb)
        torch.cuda.synchronize()
        for p, o in zip(plans, outs):
            p[2]({k: g.read() for k, g in o.items()})
        assert lv.push(4 * VHOP) > 0
        _done(e)
