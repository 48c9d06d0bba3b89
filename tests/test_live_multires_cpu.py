"""CPU: the live multi-resolution session's interface (header, export map, Python binding, Node wrapper) and the schedule
DESIGN.md §3.8 rests on, restated in pure Python and swept over every accepted shape.

The schedule: the long band's frame j is samples [j hop, j hop + n_low); the short band's frame j + 2 shift ends on the same
sample, so a call that feeds long frames also feeds the short band's frames up to 2 shift further (frames 0 .. 2 shift all
at once with a stream's first frame).  Composed column c is emitted by the call that feeds long frame c + D_low and takes the
short band's column c + shift.  The short band's ring is indexed by the emitted column (its own column - shift) and holds
mmax + shift + D_low + D_high slots.
"""
import os
import re

import pytest

import emspec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["emspec_columns_multires", "emspec_push_columns_multires", "emspec_push_samples_multires"]


def test_the_three_functions_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "emspec.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in emspec.SYMBOLS
    # the export map lists emspec_* as a pattern
    assert "emspec_*" in open(os.path.join(ROOT, "em-spec_amd", "csrc", "emspec.map")).read()
    assert "#define EMSPEC_ABI_VERSION 2" in header
    for meth in ("columns_multires", "push_samples_multires", "push_columns_multires"):
        assert callable(getattr(emspec.Engine, meth))
    lib = emspec.load()
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_node_wrapper_exports_the_two_methods():
    js = open(os.path.join(ROOT, "em-spec_amd", "js", "index.js")).read()
    for meth in ("computeSpectrogramColumnsMultires", "pushSamplesMultires"):
        assert re.search(r"\b%s\s*\(" % meth, js), meth
    napi = open(os.path.join(ROOT, "em-spec_amd", "js", "emspec_napi.c")).read()
    assert "emspec_columns_multires" in napi and "emspec_push_samples_multires" in napi


# ---- the schedule, restated ----
def latency(n, hop, reassign):
    return (n + 2 * hop - 1) // (2 * hop) if reassign else 0


def shape_ok(n_low, n_high, hop):
    """emspec_multires_shift's rule (include/emspec.h), restated so that this test needs no built library."""
    return n_low in (8192, 16384) and n_high in (1024, 2048, 4096) and 1 <= hop <= n_high and (n_low - n_high) % (2 * hop) == 0


def simulate(n_low, n_high, hop, reassign, frames_per_call):
    """Runs the session call by call.  Per band: frames done, the columns each frame adds to, the column finalised.  Returns
    the largest number of short-band ring slots live at once per call size m (columns touched and not yet finalised)."""
    shift = (n_low - n_high) // (2 * hop)
    Dl, Dh = latency(n_low, hop, reassign), latency(n_high, hop, reassign)
    assert Dl - Dh == (shift if reassign else 0)
    low_done = high_done = 0          # frames done per band
    emitted = 0                       # composed columns emitted: all below are finalised in both rings
    worst = {}
    for m in frames_per_call:
        # the long band's frames low_done .. low_done + m - 1; the short band follows: 0 while the long band has none, else + 2 shift
        new_low = low_done + m
        new_high = new_low + 2 * shift if new_low else 0
        # what the kernel derives from the long band's descriptor (live.hip.inc: LiveBlock::init)
        bj0 = 0 if low_done == 0 else low_done + 2 * shift
        bframes = m + 2 * shift if (low_done == 0 and m > 0) else m
        assert bj0 == high_done and bj0 + bframes == new_high
        # the short band's samples lie inside what the long band's frames cover: frame jh = [jh hop, jh hop + n_high)
        if bframes:
            assert bj0 * hop >= low_done * hop                                             # not older than the oldest long frame
            assert (new_high - 1) * hop + n_high == (new_low - 1) * hop + n_low            # ends on the newest sample
        # ring columns (emitted-column index) the short band touches in this call, dropped below 0 as the kernel does
        touched_hi = (new_high - 1 - shift) + Dh if bframes else None
        touched_lo = max(bj0 - shift - Dh, 0) if bframes else None
        # columns this call emits: c in [max(low_done - Dl, 0), new_low - Dl)
        first, last = max(low_done - Dl, 0), new_low - Dl
        for c in range(first, last):
            # fact 1: the short band's column c + shift is complete - every frame that can add to it (own column within D_high
            # of it) is done: frames up to c + shift + D_high
            assert c + shift + Dh <= new_high - 1, (c, new_high)
            # ... and no LATER frame adds to an emitted column: the next short frame is new_high, its reach new_high - shift - D_high
            assert new_high - shift - Dh > c or not reassign and new_high - shift > c
        if bframes:
            # nothing is added to a column that was already emitted (its slot was cleared and may be reused)
            assert touched_lo >= emitted, (touched_lo, emitted)
            live = touched_hi - emitted + 1                     # columns [emitted, touched_hi] hold energy or may receive it
            worst[m] = max(worst.get(m, 0), live)
        emitted = max(last, emitted)
        low_done, high_done = new_low, new_high
    return worst, shift, Dl, Dh


@pytest.mark.parametrize("reassign", [True, False], ids=["ra", "plain"])
def test_schedule_facts_hold_for_every_accepted_shape(reassign):
    shapes = [(nl, nh, hop) for nl in (8192, 16384) for nh in (1024, 2048, 4096) for hop in (128, 256, 512, 768, 1024)
              if shape_ok(nl, nh, hop)]
    assert (16384, 4096, 256) in shapes and (8192, 2048, 128) in shapes and (16384, 1024, 512) in shapes
    assert (16384, 4096, 768) in shapes and (16384, 2048, 768) not in shapes
    for n_low, n_high, hop in shapes:
        for mmax in (1, 3, 8, 64):
            # calls of mmax frames, of one frame, and mixed, long enough for the ring to wrap several times
            shift = (n_low - n_high) // (2 * hop)
            span = 4 * (mmax + 2 * shift + 2 * latency(n_low, hop, reassign)) + 10
            for pattern in ([mmax] * (span // mmax + 1), [1] * span, [1, mmax, 0, 2 if mmax > 1 else 1] * (span // 4)):
                pattern = [min(m, mmax) for m in pattern]
                worst, shift, Dl, Dh = simulate(n_low, n_high, hop, reassign, pattern)
                slots = mmax + shift + Dl + Dh          # emspec_live_plan.h: live_geometry
                if reassign:
                    assert slots == mmax + 2 * shift + 2 * Dh
                # fact 2: the ring bound is never exceeded
                assert max(worst.values()) <= slots, (n_low, n_high, hop, mmax, worst, slots)
        # the bound is tight for full calls in steady state
        worst, shift, Dl, Dh = simulate(n_low, n_high, hop, reassign, [4] * 200)
        assert worst[4] == 4 + shift + Dl + Dh


def test_library_agrees_on_the_accepted_shapes():
    for nl in (4096, 8192, 16384):
        for nh in (512, 1024, 2048, 4096, 8192):
            for hop in (128, 256, 512, 768, 1024):
                got = emspec.multires_shift(nl, nh, hop)
                assert (got >= 0) == shape_ok(nl, nh, hop)
                if got >= 0:
                    assert got == (nl - nh) // (2 * hop)
