"""GPU: one engine kept for a long script of calls gives, at every step, the bytes a fresh engine gives for that call.

Every engine workspace is grown on demand, never shrunk, and shared between entries: d_mres by the two-band and the multi-band
batch, d_full by the time reduction and the peaks entry, d_hist by FAST and EXACT records of any size, d_xlow by two kernels with
different layouts (the records scatter clears only the bytes it needs of a possibly larger buffer), d_stage by the host pipeline,
the parity dumps and the packed entry, d_raw / d_post / d_peak by every post-processed entry; emspec_set_row_edges_hz drops the
plan and band-plan caches.  The other GPU tests use a fresh engine or one shape per engine; a renderer keeps one engine for hours.

The script is ordered so that each buffer first grows and is then used smaller than it is.  EXACT: bytes equal those of the same
call on a fresh engine with the same settings (computed once per distinct call).  FAST (a shorter script): each call within the
oracle bounds of tests/test_gpu_route.py, as in tests/test_gpu_chunks.py, whose helpers and shapes this file uses."""
import json
import os

import numpy as np
import pytest
import torch

import chunk_ref as K
import emspec
import test_gpu_chunks as G
from emspec import synth

pytestmark = pytest.mark.gpu

PLANS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kernel_plans.json")))
WARPED = (20.0, 24000.0, 0.5, 1.0)        # tests/test_gpu_route.py's axis 2: past the no-parking kernel's 6 % of low bins
ALL3 = ("db", "rgba", "index")

# ---- the calls: name -> (case of tests/test_gpu_chunks.py without its settings, streams, columns)
RECORDS = G.case("single", (16384, 512), True, records=True, want=ALL3)
CALLS = {
    "records-16384/512-S3": (RECORDS, 3, 25),
    "records-16384/512-S1": (RECORDS, 1, 25),
    "lr-1024/64": (G.case("single", (1024, 64), True, want=ALL3), 3, 40),
    "lr-4096/256": (G.case("single", (4096, 256), True, want=("db", "index")), 3, 48),
    "index-4096/256": (G.case("single", (4096, 256), True, want=("index",)), 3, 130),
    "multi-3x512": (G.case("multi", G.LADDERS["3x512"], True, want=ALL3), 3, 40),
    "multi-4x128": (G.case("multi", G.LADDERS["4x128"], True, want=("db", "index")), 3, 30),
    "two-8192": (G.case("two", G.TWO["8192"], True, want=ALL3), 2, 25),
    "peaks-4096/256": (G.case("single", (4096, 256), True, peaks=True), 3, 48),
}


def _recorded(kind, **case):
    hit = [w for w in PLANS if w["kind"] == kind and all(w["case"][k] == v for k, v in case.items())]
    assert len(hit) >= 1, (kind, case)
    return hit[0]["route"]


def _samples(c, columns):
    n0, hop = G._n0_hop(c)
    return n0 + hop * (columns - 1) + 3


class Session:
    """An engine with the settings a step asked for, and the same settings for the fresh engines it is compared with."""

    def __init__(self, exact, monkeypatch):
        self.exact, self.mp = exact, monkeypatch
        self.display, self.f, self.edges, self.budget = None, 1, None, None
        self.engine = self._new()
        self.fresh = {}

    def _new(self):
        return emspec.Engine(mode=emspec.MODE_EXACT if self.exact else emspec.MODE_FAST, diag=True)

    def close(self):
        self.engine.close()

    def _apply(self, e):
        if self.edges is not None:
            e.set_row_edges_hz(self.edges)
        if self.display:
            e.set_display(*self.display)
        e.set_time_reduce(self.f)

    def set(self, what, value):
        if what == "display":
            self.display = value
            self.engine.set_display(*(value or (0.0, 0.0)))
        elif what == "f":
            self.f = value
            self.engine.set_time_reduce(value)
        elif what == "edges":
            self.edges = value
            self.engine.set_row_edges_hz(value)
        else:
            assert what == "budget"
            self.budget = value

    def case(self, name):
        c, streams, columns = CALLS[name]
        c = dict(c, exact=self.exact)
        if self.display:
            c["display"] = True
        if self.f > 1:
            c["f"] = self.f
        return c, streams, columns

    def _run(self, e, kind, name):
        """One call of `kind` -> a list of numpy arrays."""
        c, streams, columns = self.case(name)
        pcm = G._pcm(streams, _samples(c, columns))
        if kind == "device":
            out = G._call(e, c, torch.from_numpy(np.array(pcm)).cuda(), columns)
        elif kind == "host":
            out = G._host(e, c, pcm)
        elif kind == "packed":
            wire, off = e.batch_packed(pcm, *c["shape"], True)
            out = {"wire": wire[:off[-1]].copy(), "offsets": off}
        elif kind == "dump":
            out = dict(zip("pcrq", e.parity_dump_exact(pcm, *c["shape"], True, 0, 6) if self.exact else e.parity_dump(pcm, *c["shape"], True, 0, 6)))
        else:
            assert kind == "live"
            n, hop = c["shape"]
            cols = []
            for j in range(20):
                db, _, col = e.columns(pcm[:, j * hop:j * hop + n], hop, True)
                cols += [db.copy(), col.copy()]
            e.reset()
            out = dict(enumerate(cols))
        e.device_status()
        return [np.ascontiguousarray(v) for v in out.values() if v is not None]

    def long_lived(self, kind, name):
        G._set_budget(self.mp, self.budget)
        return self._run(self.engine, kind, name)

    def on_a_fresh_engine(self, kind, name):
        """The same call with the same settings on an engine of its own, unbudgeted; once per distinct call."""
        key = (kind, name, self.display, self.f, None if self.edges is None else "warped")
        if key not in self.fresh:
            G._set_budget(self.mp, None)
            with self._new() as e:
                self._apply(e)
                self.fresh[key] = self._run(e, kind, name)
        return self.fresh[key]


def _equal(got, want, step):
    assert len(got) == len(want), step
    for i, (a, b) in enumerate(zip(got, want)):
        assert G._same(a, b), (step, G._where(a, b, f"array {i}") if a.ndim >= 3 and a.shape == b.shape else f"array {i} differs")


def test_exact_engine_kept_over_a_script_of_calls(monkeypatch):
    c3, _, col3 = CALLS["records-16384/512-S3"]
    per = K.path(c3, col3)[0][1]
    b = K.budget_for(per)
    assert K.chunks(b, per, 3) == (2, 1) and K.chunks(0, per, 3) == (1, 1, 1)
    warped = emspec.warped_edges_hz(1024, *WARPED)
    script = [
        ("device", "records-16384/512-S3"),      # d_hist and the scatter's low-row scratch in d_xlow grow
        ("device", "lr-1024/64"),                # the no-parking kernel's layout of d_xlow
        ("device", "records-16384/512-S1"),      # d_xlow larger than low_need, d_hist larger than one stream
        ("device", "multi-3x512"),               # d_mres grows
        ("device", "two-8192"),                  # ... and is used smaller
        ("set", "display", G.DISPLAY),
        ("device", "multi-4x128"),               # d_raw / d_peak (d_post: no dB wanted in the next but one)
        ("device", "two-8192"),
        ("device", "index-4096/256"),            # d_post
        ("set", "display", None),
        ("device", "multi-4x128"),
        ("set", "f", 4),
        ("device", "lr-4096/256"),               # d_full: dB + index
        ("set", "f", 1),
        ("device", "peaks-4096/256"),            # d_full: the peaks' dB
        ("set", "f", 64),
        ("device", "index-4096/256"),            # d_full: index only, smaller
        ("set", "f", 1),
        ("set", "budget", b),
        ("device", "records-16384/512-S3"),      # chunks (2, 1) in a d_hist sized for three streams
        ("set", "budget", None),
        ("device", "records-16384/512-S3"),
        ("set", "budget", 0),
        ("device", "records-16384/512-S3"),      # (1, 1, 1)
        ("device", "multi-3x512"),
        ("set", "budget", None),
        ("device", "two-8192"),
        ("refused", "two-8192"),                 # split row 366: INVALID_ARG, nothing run
        ("device", "two-8192"),
        ("live", "lr-4096/256"),                 # a short live session between two batches
        ("device", "lr-4096/256"),
        ("dump", "lr-4096/256"),                 # d_stage: the parity dump, the host pipeline, the packed entry
        ("host", "lr-4096/256"),
        ("packed", "lr-4096/256"),
        ("host", "records-16384/512-S3"),
        ("set", "edges", warped),                # drops the plan and band-plan caches
        ("route", "exact_parked"),
        ("device", "lr-4096/256"),               # (now the kernel with the ring parked under the planes)
        ("device", "records-16384/512-S3"),
        ("device", "multi-3x512"),
        ("device", "two-8192"),
        ("set", "edges", None),
        ("route", "exact_lr"),
        ("device", "lr-4096/256"),
        ("first", "records-16384/512-S3"),       # the first step's call reproduces its first bytes
    ]
    assert sum(s[0] not in ("set", "route") for s in script) >= 20
    s = Session(True, monkeypatch)
    try:
        first = None
        for i, (kind, arg, *rest) in enumerate(script):
            step = f"step {i}: {kind} {arg if isinstance(arg, str) else ''}"
            if kind == "set":
                s.set(arg, rest[0])
            elif kind == "route":
                axis = 0 if s.edges is None else 2
                assert _recorded("exact", n=4096, hop=256, rows=1024, reassign=1, row0=0, axis_rows=1024, axis=axis, parked=0, records=0) == arg
                assert s.engine.fused(4096, 256, True)
            elif kind == "refused":
                c, streams, columns = s.case(arg)
                x = torch.from_numpy(np.array(G._pcm(streams, _samples(c, columns)))).cuda()
                out = torch.full((streams, columns, 1024), 0x5A, dtype=torch.uint8, device="cuda")
                n_low, n_high, hop, _ = c["shape"]
                with pytest.raises(emspec.EmspecError) as ei:
                    s.engine.batch_multires_device(x, n_low, n_high, hop, 366, True, index=out)
                assert ei.value.code == emspec.ERR_INVALID_ARG, step
                torch.cuda.synchronize()
                assert bool((out == 0x5A).all()), step
            elif kind == "first":
                _equal(s.long_lived("device", arg), first, step)
            else:
                got = s.long_lived(kind, arg)
                _equal(got, s.on_a_fresh_engine(kind, arg), step)
                if first is None:
                    first = got
    finally:
        s.close()


def test_fast_engine_kept_over_a_script_of_calls(monkeypatch):
    """FAST sums in arrival order: every call of the script is held to the oracle by the bounds of tests/test_gpu_route.py."""
    script = [("records-16384/512-S3", 1, None), ("multi-3x512", 1, None), ("two-8192", 1, None), ("records-16384/512-S1", 1, None),
              ("lr-4096/256", 4, None), ("multi-4x128", 1, 0), ("lr-4096/256", 64, None), ("two-8192", 1, 1), ("records-16384/512-S3", 1, 0),
              ("multi-3x512", 1, None), ("lr-4096/256", 1, None)]
    calls = dict(CALLS, **{"records-16384/512-S3": (G.case("single", (16384, 128), False, records=True, want=ALL3), 3, 25),
                           "records-16384/512-S1": (G.case("single", (16384, 128), False, records=True, want=ALL3), 1, 25)})
    with emspec.Engine(diag=True) as e:
        assert not e.fused(16384, 128, True)
        for i, (name, f, budget) in enumerate(script):
            c, streams, columns = calls[name]
            c = dict(c, exact=False, **({"f": f} if f > 1 else {}))
            L = _samples(c, columns)
            e.set_time_reduce(f)
            G._set_budget(monkeypatch, budget)
            got = G._call(e, c, torch.from_numpy(np.array(G._pcm(streams, L))).cuda(), columns)
            print(f"step {i}: {name} f = {f} budget {budget}")
            G._check_fast(c, [got], G._reference(G._freeze(c), streams, L), streams * columns * 1024)
