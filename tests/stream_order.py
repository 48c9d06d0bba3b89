"""Stream ordering under forced delays ("Stream ordering under forced delays"): what tests/test_gpu_stream_order.py
and tests/test_stream_order_cases_cpu.py share.

    delay(stream, ms)      a spin of about ms milliseconds on a torch stream (torch.cuda._sleep, calibrated once per process)
    side_stream(engine)    a torch stream shown to run beside the engine's own stream (two HIP streams that share a hardware queue
                           serialise, which would hide a missing wait)
    CASES                  one row per device entry and kernel path: the entry, its smallest shape, the reference that checks it

An ordering mistake must give wrong bytes, not pass by luck: the stream an entry is given is held back by a delay in front of the
copy that brings its real input and of the fill that poisons its outputs.  Work the entry puts on any other stream then runs on
the decoy input (another seed of the same generator), and a fill or start-value pass on another stream is lost under the poison.

Nothing here needs a device at import: the CPU guard reads CASES and the references."""
import functools
import types

import numpy as np

import emspec
import level_ref as LR
import multiband_ref as B
import multires_ref as M
import oracle as O
import overview_ref as V
import pcm_ref as PR
import peaks_ref as PK
import post_ref as P
import stereo_ref as T
import wave_ref as W
import window_cases as WC
import wire_ref as WR
from emspec import synth
from test_gpu_route import EXACT as EXACT_ROUTES, FAST as FAST_ROUTES, WARPED

F, U8 = np.float32, np.uint8
GUARD, POISON = 16, 0xA5
MIN_DELAY_MS, MAX_DELAY_MS, JITTER = 50.0, 500.0, 20     # delay = max(50 ms, 20 x the unobstructed duration), at most 500 ms
TOL_DB = 8.7e-4                                          # the project's FAST-mode bound against the float32 bit model
STREAMS, FRAMES = 2, 25                                  # S = 2 streams of n + 24 hop samples: 25 columns
DECOY_SEED = 7                                           # synth.streams(first=7): other seeds of the same generator
NULL_STREAM = types.SimpleNamespace(cuda_stream=0)       # what the wrappers read of a torch stream: the HIP default stream


# ---- the delay --------------------------------------------------------------------------------------------------------------
_CAL = {}


def cycles_per_ms():
    """torch.cuda._sleep counts device clock ticks: one _sleep(c0) timed with two events, once per process."""
    if "rate" not in _CAL:
        import torch
        c0 = 1_000_000
        torch.cuda._sleep(c0)                             # (the first launch loads the kernel)
        torch.cuda.synchronize()
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(c0)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0 or c0 >= 1 << 32:                # (long enough that the launch itself does not count)
                break
            c0 *= 8
        assert ms > 0.0, ms
        _CAL["rate"] = c0 / ms
        print(f"MEASURED delay calibration: _sleep({c0}) took {ms:.3f} ms: {_CAL['rate']:.0f} ticks per ms")
    return _CAL["rate"]


def delay(stream, ms):
    """Enqueues a spin of about `ms` milliseconds on `stream`; never more than 500 ms in one call."""
    import torch
    assert ms > 0
    ticks = int(min(float(ms), MAX_DELAY_MS) * cycles_per_ms())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(ticks)


def delay_ms_for(seconds, what):
    """The delay that holds back a step whose unobstructed host-side duration was `seconds`: max(50 ms, 20 x that).  The factor
    covers host jitter on a shared machine; where the cap of 500 ms would bind, the shape is too large for this suite."""
    ms = max(MIN_DELAY_MS, JITTER * seconds * 1e3)
    print(f"MEASURED {what}: unobstructed {seconds * 1e3:.3f} ms, delay {ms:.1f} ms")
    assert ms <= MAX_DELAY_MS, f"{what}: 20 x {seconds * 1e3:.1f} ms is past the 500 ms cap: shrink the shape, not the factor"
    return ms


# ---- the independence control -----------------------------------------------------------------------------------------------
def _held_apart(held, probe):
    """delay + a gate event on `held`, then probe() - work on another stream that probe synchronises.  True when the gate is
    still open at probe's return: the other stream ran while `held` was held back."""
    import torch
    gate = torch.cuda.Event()
    delay(held, MIN_DELAY_MS)
    gate.record(held)
    probe()
    apart = not gate.query()
    torch.cuda.synchronize()                              # (between candidates)
    return apart


def _touch(stream):
    import torch
    with torch.cuda.stream(stream):
        torch.zeros(64, device="cuda").add_(1.0)
    stream.synchronize()


def side_stream(engine, lut=None, beside=None):
    """A torch stream that runs independently of the engine's own stream: with a delay and a gate pending on the candidate, a
    host call that runs and synchronises on the engine's stream only (set_colormap with the current map, `lut`; default: the
    default map) returns with the gate still open.  beside: a stream the candidate must also run beside while THAT one is held.
    At most 8 fresh streams are tried; none passing is a failure, never a skip."""
    import pytest
    import torch
    key = "_stream_order_side" if beside is None else "_stream_order_pair"
    if getattr(engine, key, None) is not None:
        return getattr(engine, key)
    lut = O.default_lut() if lut is None else lut
    for _ in range(8):
        st = torch.cuda.Stream()
        if st.cuda_stream == 0 or (beside is not None and st.cuda_stream == beside.cuda_stream):
            continue
        if not _held_apart(st, lambda: engine.set_colormap(lut)):
            continue
        if beside is not None and not _held_apart(beside, lambda: _touch(st)):
            continue
        setattr(engine, key, st)
        return st
    pytest.fail("none of 8 fresh torch streams runs beside the engine's own stream"
                + (" and the first side stream" if beside is not None else "")
                + ": every candidate shared a hardware queue with it, and an ordering test on such a stream proves nothing")


# ---- poisoned outputs between guards ----------------------------------------------------------------------------------------
class Guarded:
    """A device output of numpy `dtype` and `shape`, 16 guard bytes on either side; poison() fills all of it with 0xA5 on a
    stream, read() checks the guards and returns the numpy array."""

    def __init__(self, dtype, shape):
        import torch
        self.dtype, self.shape = np.dtype(dtype), tuple(int(v) for v in shape)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.buf = torch.empty(self.nbytes + 2 * GUARD, dtype=torch.uint8, device="cuda")
        body = self.buf[GUARD:GUARD + self.nbytes]
        kinds = {np.dtype(F): torch.float32, np.dtype(U8): torch.uint8, np.dtype(np.int32): torch.int32}
        self.tensor = (body if self.dtype == U8 else body.view(kinds[self.dtype])).view(self.shape)
        assert self.tensor.data_ptr() % 16 == 0

    def poison(self, stream):
        import torch
        with torch.cuda.stream(stream):
            self.buf.fill_(POISON)

    def read(self):
        got = self.buf.cpu().numpy()
        assert np.all(got[:GUARD] == POISON) and np.all(got[-GUARD:] == POISON), "an output was written outside its array"
        return got[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape).copy()


# ---- the comparisons of the entries' own suites -----------------------------------------------------------------------------
def _bytes(a):
    return np.ascontiguousarray(a).view(U8).reshape(-1)


def bytes_mismatch(got, want):
    """Every output byte for byte -> {name: what differs} (empty: equal)."""
    bad = {}
    for k, w in want.items():
        g = got[k]
        if g.shape != w.shape or g.dtype != w.dtype:
            bad[k] = f"shape / type {g.shape} {g.dtype} != {w.shape} {w.dtype}"
        elif not np.array_equal(_bytes(g), _bytes(w)):
            bad[k] = f"{int(np.count_nonzero(_bytes(g) != _bytes(w)))} of {_bytes(w).size} bytes differ"
    return bad


def fast_mismatch(got, want):
    """tests/test_gpu_route.py's FAST bounds: |dB error| < 8.7e-4, palette index within one step, at most max(8, cells / 1000)
    cells off by one."""
    bad = {}
    with np.errstate(invalid="ignore"):
        worst = float(np.max(np.abs(got["db"].astype(np.float64) - want["db"])))
    if not worst < TOL_DB:
        bad["db"] = f"worst |dB error| {worst:.3e}"
    d = np.abs(got["index"].astype(int) - want["index"].astype(int))
    if d.max() > 1 or int(np.count_nonzero(d)) > max(8, d.size // 1000):
        bad["index"] = f"index off by up to {int(d.max())} in {int(np.count_nonzero(d))} of {d.size} cells"
    return bad


def post_mismatch(sm, agc):
    """tests/test_gpu_post.py: the dB within post_ref.bound(sm, agc, max |reference|) of the binary64 reference."""
    def check(got, want):
        lim = P.bound(sm, agc, np.max(np.abs(want["db"])))
        with np.errstate(invalid="ignore"):
            err = float(np.max(np.abs(got["db"].astype(np.float64) - want["db"])))
        return {} if err <= lim else {"db": f"max error {err:.3e} dB past the bound {lim:.3e} dB"}
    return check


def prefix_mismatch(got, want):
    """A wire image: the image's bytes at the head of the destination (what lies behind it is not specified)."""
    g, w = got["wire"].reshape(-1), want["wire"].reshape(-1)
    if g.size < w.size or not np.array_equal(g[:w.size], w):
        return {"wire": "the image's bytes differ"}
    return {}


def parity_mismatch(got, want):
    """tests/test_gpu_parity.py: col and row exact; the power, computed in the same order of operations, bit for bit."""
    return bytes_mismatch(got, want)


# ---- the case table ---------------------------------------------------------------------------------------------------------
class Case:
    """One row.  kind "input": the entry reads a device input the test uploads late (inputs, outputs, call, reference,
    mismatch); kind "view": the entry reads a live ring (tests/test_gpu_stream_order.py builds the session).
    engine: (mode, rows, axis) of the engine it runs on; setup / teardown: engine settings around the calls.
    blocks: the entry may legitimately block the host on a warmed engine, for `reason`."""

    def __init__(self, id, entry, method, kind="input", engine=("exact", 1024, 0), shape="", ref="", inputs=None, outputs=None,
                 call=None, reference=None, mismatch=bytes_mismatch, setup=None, teardown=None, blocks=False, reason="",
                 null=False):
        assert not blocks or reason
        self.id, self.entry, self.method, self.kind, self.engine, self.shape, self.ref = id, entry, method, kind, engine, shape, ref
        self.inputs, self.outputs, self.call, self.reference, self.mismatch = inputs, outputs, call, reference, mismatch
        self.setup, self.teardown = setup or (lambda e: None), teardown or (lambda e: None)
        self.blocks, self.reason, self.null = blocks, reason, null

    def __repr__(self):
        return self.id


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pcm(which, S, L):
    return _frozen(synth.streams(S, L, first=0 if which == "real" else DECOY_SEED))


def edges_of(rows, axis):
    return emspec.warped_edges_hz(rows, *WARPED) if axis else None


@functools.lru_cache(maxsize=None)
def model_columns(which, mode, n, hop, rows, reassign, axis, S=STREAMS, L=None):
    """The bit model's (db, index) of pcm(which, S, L): binary64 for "exact", float32 for "fast"."""
    x = pcm(which, S, n + (FRAMES - 1) * hop if L is None else L)
    O.set_custom_edges_hz(edges_of(rows, axis))
    try:
        cfg = O.make_cfg(n, hop, bool(reassign), rows=rows)
        if mode == "exact":
            db, _, idx, _ = O.batch_exact(cfg, x, want=("db", "index"))
        else:
            db, _, idx = O.batch_f32(cfg, x, want=("db", "index"))
    finally:
        O.set_custom_edges_hz(None)
    return _frozen(db), _frozen(idx)


def _which(x, S, L):
    """The reference functions take the input array; the cached models take its name."""
    for w in ("real", "decoy"):
        if np.array_equal(_bytes(x), _bytes(pcm(w, S, L))):
            return w
    raise AssertionError("an input that is neither the real one nor the decoy")


def _batch(id, mode, n, hop, rows, reassign=1, axis=0, reduce=1, display=None, null=False, route=""):
    L = n + (FRAMES - 1) * hop
    Cr = V.reduced_columns(FRAMES, reduce)
    outputs = {"db": (F, (STREAMS, Cr, rows))}
    if display is None:
        outputs["index"] = (U8, (STREAMS, Cr, rows))

    def reference(x):
        db, idx = model_columns(_which(x, STREAMS, L), mode, n, hop, rows, reassign, axis)
        if display is not None:
            return {"db": P.reference(db, display[0], display[1], 0.0)[0]}
        if reduce > 1:
            r = V.reduce({"db": db, "index": idx}, reduce, None)
            return {"db": r["db"], "index": r["index"]}
        return {"db": db, "index": idx}

    def call(e, x, out, st):
        e.batch_device(x, n, hop, bool(reassign), db=out["db"], index=out.get("index"), stream=st)

    def setup(e):
        e.set_time_reduce(reduce)
        if display is not None:
            e.set_display(*display)

    def teardown(e):
        e.set_time_reduce(1)
        e.set_display(0.0, 0.0)

    mismatch = post_mismatch(*display) if display is not None else bytes_mismatch if mode == "exact" else fast_mismatch
    return Case(id, "emspec_batch_device", "batch_device", engine=(mode, rows, axis), shape=f"{route} {n}/{hop} rows {rows}".strip(),
                ref="oracle bit model" + (", overview_ref" if reduce > 1 else ", post_ref" if display else ""),
                inputs=lambda which: pcm(which, STREAMS, L), outputs=outputs, call=call, reference=reference, mismatch=mismatch,
                setup=setup, teardown=teardown, null=null)


def _multires():
    n_low, n_high, hop, split = 16384, 4096, 256, 512
    L = n_low + (FRAMES - 1) * hop
    return Case("batch_multires_device", "emspec_batch_multires_device", "batch_multires_device", shape="16384/4096/256 split 512",
                ref="multires_ref", inputs=lambda which: pcm(which, STREAMS, L),
                outputs={"db": (F, (STREAMS, FRAMES, 1024)), "index": (U8, (STREAMS, FRAMES, 1024))},
                call=lambda e, x, out, st: e.batch_multires_device(x, n_low, n_high, hop, split, True, db=out["db"],
                                                                   index=out["index"], stream=st),
                reference=lambda x: {k: v for k, v in M.compose(x, n_low, n_high, hop, split, exact=True,
                                                                want=("db", "index")).items() if v is not None})


def _multiband():
    n, hop, splits = (8192, 2048, 1024), 512, (368, 668)
    L = n[0] + (FRAMES - 1) * hop
    return Case("batch_multiband_device", "emspec_batch_multiband_device", "batch_multiband_device", shape="8192/2048/1024 hop 512",
                ref="multiband_ref", inputs=lambda which: pcm(which, STREAMS, L),
                outputs={"db": (F, (STREAMS, FRAMES, 1024)), "index": (U8, (STREAMS, FRAMES, 1024))},
                call=lambda e, x, out, st: e.batch_multiband_device(x, n, splits, hop, True, db=out["db"], index=out["index"],
                                                                    stream=st),
                reference=lambda x: {k: v for k, v in B.compose(x, n, splits, hop, exact=True, want=("db", "index")).items()
                                     if v is not None})


PEAKS_K, PEAKS_MIN_DB = 8, -60.0
N0, HOP0 = 4096, 256
L0 = N0 + (FRAMES - 1) * HOP0


def _db0(which, S=STREAMS):
    return model_columns(which, "exact", N0, HOP0, 1024, 1, 0, S=S)[0]


def _batch_peaks():
    return Case("batch_peaks_device", "emspec_batch_peaks_device", "batch_peaks_device", shape="4096/256, 8 peaks", ref="peaks_ref",
                inputs=lambda which: pcm(which, STREAMS, L0), outputs={"peaks": (F, (STREAMS, FRAMES, PEAKS_K, 2))},
                call=lambda e, x, out, st: e.batch_peaks_device(x, N0, HOP0, True, PEAKS_K, PEAKS_MIN_DB, out=out["peaks"], stream=st),
                reference=lambda x: {"peaks": PK.peaks(_db0(_which(x, STREAMS, L0)), PEAKS_K, PEAKS_MIN_DB)})


def _peaks():
    return Case("peaks_device", "emspec_peaks_device", "peaks_device", shape="50 columns of 1024 rows, 8 peaks", ref="peaks_ref",
                inputs=_db0, outputs={"peaks": (F, (STREAMS, FRAMES, PEAKS_K, 2))},
                call=lambda e, x, out, st: e.peaks_device(x, PEAKS_K, PEAKS_MIN_DB, out=out["peaks"], stream=st),
                reference=lambda x: {"peaks": PK.peaks(x, PEAKS_K, PEAKS_MIN_DB)})


def _pcm_decode():
    frames = L0

    def raw(which):
        x = pcm(which, 4, frames)
        return _frozen(np.stack([np.round(np.stack([x[2 * i], x[2 * i + 1]], -1).reshape(-1) * 32767).astype("<i2")
                                 for i in range(2)]))

    def call(e, x, out, st):
        fmt = emspec.PcmFormat.make("s16", 2, views=["left", "right", "mid", "side"])
        e.pcm_decode_device(x, fmt, 2, frames, out=out["pcm"], stream=st)

    return Case("pcm_decode_device", "emspec_pcm_decode_device", "pcm_decode_device", shape="s16 stereo x 2 sources to L R M S",
                ref="pcm_ref", inputs=raw, outputs={"pcm": (F, (8, frames))}, call=call,
                reference=lambda x: {"pcm": PR.decode(np.ascontiguousarray(x).view(U8), PR.S16, 2, T.LRMS)})


TEAM_CASE = (1024, 255, 1024 + 255 * 9 + 100, 4)          # a team of 32 lanes (window_cases._team)
assert TEAM_CASE in WC.DEVICE_CASES and WC._team(*TEAM_CASE) == 32 and WC._team(*WC.SPLIT_CASES[0]) == "split"


def _records(rec):
    return np.ascontiguousarray(rec).view(U8).reshape(rec.shape + (rec.dtype.itemsize,))


def _window(kind, case, path):
    n, hop, L, f = case
    Cr = V.reduced_columns(W.num_columns(L, n, hop), f)
    S = W.S_CASES
    if kind == "wave":
        sig, outputs = W.case_signal, {"wave": (F, (S, Cr, 2))}
        call = lambda e, x, out, st: e.wave_device(x, n, hop, f, out=out["wave"], stream=st)
        reference = lambda x: {"wave": W.envelope(x, n, hop, f)}
    elif kind == "level":
        sig, outputs = LR.case_signal, {"level": (U8, (S, Cr, 24))}
        call = lambda e, x, out, st: e.level_device(x, n, hop, f, out=out["level"], stream=st)
        reference = lambda x: {"level": _records(LR.levels(x, n, hop, f))}
    else:
        sig, outputs = LR.case_signal, {"cross": (U8, (1, Cr, 16))}
        call = lambda e, x, out, st: e.cross_device(x, 3, 0, 2, n, hop, f, out=out["cross"], stream=st)
        reference = lambda x: {"cross": _records(LR.crosses(x, 3, 0, 2, n, hop, f))}
    return Case(f"{kind}_device-{path}", f"emspec_{kind}_device", f"{kind}_device", shape="n%d hop%d L%d f%d" % case,
                ref="wave_ref" if kind == "wave" else "level_ref",
                inputs=lambda which: _frozen(sig(case, seed=0 if which == "real" else DECOY_SEED)), outputs=outputs, call=call,
                reference=reference)


def _stereo():
    shape = (2, FRAMES, 1024)
    outputs = {"level": (F, shape), "index": (U8, shape), "pan": (U8, shape)}
    image = lambda db: {k: v for k, v in T.compose(db, 2, 0, 1, T.VIEW_MAP).items() if k in outputs}
    one = Case("stereo_device", "emspec_stereo_device", "stereo_device", shape="2 pairs x 25 columns x 1024 rows", ref="stereo_ref",
               inputs=lambda which: _db0(which, 4), outputs=outputs,
               call=lambda e, x, out, st: e.stereo_device(x, 2, 0, 1, map=T.VIEW_MAP, want=(), stream=st, **out),
               reference=image)
    two = Case("batch_stereo_device", "emspec_batch_stereo_device", "batch_stereo_device", shape="2 pairs, 4096/256", ref="stereo_ref",
               inputs=lambda which: pcm(which, 4, L0), outputs=outputs,
               call=lambda e, x, out, st: e.batch_stereo_device(x, N0, HOP0, True, 2, 0, 1, map=T.VIEW_MAP, want=(), stream=st, **out),
               reference=lambda x: image(_db0(_which(x, 4, L0), 4)))
    return [one, two]


def _wire():
    cols, rows = STREAMS * FRAMES, 1024
    index = lambda which: _frozen(model_columns(which, "exact", N0, HOP0, rows, 1, 0)[1].reshape(cols, rows))
    bound = WR.bound(cols, rows)

    def image(which):
        w = np.zeros(bound, U8)
        img = WR.pack(index(which))
        w[:img.size] = img
        return _frozen(w)

    pack = Case("wire_pack", "emspec_wire_pack", "wire_pack", shape="50 columns of 1024 rows, no size asked for", ref="wire_ref",
                inputs=index, outputs={"wire": (U8, (bound,))},
                call=lambda e, x, out, st: e.wire_pack(x, out["wire"], stream=st, want_size=False),
                reference=lambda x: {"wire": WR.pack(x)}, mismatch=prefix_mismatch)
    unpack = Case("wire_unpack", "emspec_wire_unpack", "wire_unpack", shape="50 columns of 1024 rows", ref="wire_ref",
                  inputs=image, outputs={"index": (U8, (cols, rows))},
                  call=lambda e, x, out, st: e.wire_unpack(x, bound, out["index"], stream=st),
                  reference=lambda x: {"index": WR.unpack(x, cols, rows)}, blocks=True,
                  reason="the image's header is validated on the host before the expand is launched: one copy of 32 bytes on "
                         "hip_stream and its synchronisation")
    return [pack, unpack]


def _parity():
    K = N0 // 2 + 1
    shape = (STREAMS, FRAMES, K)

    def reference(x):
        per = [O.frames_f32(O.make_cfg(N0, HOP0, True), x[s], 0, FRAMES) for s in range(STREAMS)]
        return {"power": np.stack([p[0] for p in per]), "col": np.stack([p[1] for p in per]), "row": np.stack([p[2] for p in per])}

    return Case("parity_dump_device", "emspec_parity_dump_device", "parity_dump_device", engine=("fast", 1024, 0), shape="4096/256",
                ref="oracle bit model", inputs=lambda which: pcm(which, STREAMS, L0),
                outputs={"power": (F, shape), "col": (np.int32, shape), "row": (np.int32, shape)},
                call=lambda e, x, out, st: e.parity_dump_device(x, N0, HOP0, True, 0, FRAMES, out["power"], out["col"], out["row"],
                                                                stream=st),
                reference=reference, mismatch=parity_mismatch)


def _views():
    return [Case(m, "emspec_" + m, m, kind="view", engine=("exact", 64, 0), shape="a live ring of 16 columns / n + 16 hop samples",
                 ref=ref)
            for m, ref in (("history_view_device", "history_ref"), ("history_view_stereo_device", "stereo_ref"),
                           ("audio_view_device", "audio_ref"), ("audio_batch_device", "audio_ref, oracle bit model"))]


CASES = ([_batch(f"batch_device-fast-{route}-{n}-{hop}-{rows}-{ra}", "fast", n, hop, rows, reassign=ra, route=route)
          for n, hop, rows, ra, route in FAST_ROUTES]
         + [_batch(f"batch_device-exact-{route}-{n}-{hop}-{rows}-axis{axis}", "exact", n, hop, rows, axis=axis, route=route)
            for n, hop, rows, axis, route in EXACT_ROUTES]
         + [_batch("batch_device-time-reduce-3", "exact", N0, HOP0, 1024, reduce=3),
            _batch("batch_device-display-on", "exact", 1024, 256, 1024, display=(0.6, 0.8)),
            _batch("batch_device-null-stream", "exact", N0, HOP0, 1024, null=True),
            _multires(), _multiband(), _batch_peaks(), _peaks(), _pcm_decode()]
         + [_window(kind, case, path) for kind in ("wave", "level", "cross")
            for case, path in ((TEAM_CASE, "team"), (WC.SPLIT_CASES[0], "split"))]
         + _stereo() + _wire() + [_parity()] + _views())

# the scenarios with two caller streams (tests/test_gpu_stream_order.py, C and D): rows of the table like the others
CASES += [Case(id, "emspec_" + m, m, kind="order", engine=engine, shape=shape, ref=ref, blocks=bool(reason), reason=reason)
          for id, m, engine, shape, ref, reason in (
              ("batch_device-exact-scratch-two-streams", "batch_device", ("exact", 1024, 0), "exact_lr 4096/256, rl > 0",
               "oracle bit model", ""),
              ("batch_device-exact-scratch-regrow", "batch_device", ("exact", 1024, 0), "exact_lr 4096/256, 2 then 4 streams",
               "oracle bit model", "the low-row scratch is regrown: the old buffer may be freed only after the launch that is "
                                   "pending on it, on another stream, has finished"),
              ("batch_device-caller-ordered-records", "batch_device", ("fast", 1024, 0), "records_f32 4096/227 then 2048/127",
               "oracle bit model", ""),
              ("audio_batch_device-caller-ordered", "audio_batch_device", ("exact", 64, 0), "1024/256 then 256/128 of one ring",
               "audio_ref, oracle bit model", ""))]

INPUT_CASES = [c for c in CASES if c.kind == "input"]
VIEW_CASES = [c for c in CASES if c.kind == "view"]

# entries and methods with a stream argument that this table leaves to another suite, each with its reason
EXCLUDED_ENTRIES = {"emspec_gather_columns": "tests/test_gather.py owns it: a collective that synchronises its stream once by contract"}
EXCLUDED_METHODS = {"gather_columns": EXCLUDED_ENTRIES["emspec_gather_columns"]}
# methods whose `stream` is a live stream's number, not a HIP stream
NOT_A_HIP_STREAM = {"reset_stream", "live_history", "live_audio"}
