"""CPU: the arithmetic of the live audio history (em-spec_amd/csrc/emspec_audio_plan.h) without a GPU, pinned to
the numpy model tests/audio_ref.py: the slot of a sample, the range a ring holds after a launch, which of a launch's samples are
stored when it ingests more than W (and that no slot is written twice in one launch), the per-frame form's "not yet stored"
rule, the two runs of a range across the wrap, whether a view fits - also with values near 2^62 - the ring's bytes, and the
head / 16-byte body / tail split of a run for every source and destination alignment.

tests/cdriver/audio_plan_driver.cpp is a program of its own that includes only that header and models what the store and view
kernels' threads do to a ring of exactly W entries, built with the host compiler under ASan and UBSan (nothing is preloaded,
nothing is loaded into Python under a sanitizer)."""
import json
import os
import subprocess

import numpy as np
import pytest

import audio_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 3, 4, 1000, 1021, 4096)


def blocks_of(W):
    return sorted({1, 127, 128, 333, W - 1, W, W + 1, 3 * W + 5} - {0})


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("audio_plan")
    exe = str(tmp / "audio_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "audio_plan_driver.cpp"), "-o", exe])
    count = [0]

    def run(lines):
        count[0] += 1
        path = tmp / ("in%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (lines[:3], r.returncode, r.stderr[-2000:])
        return json.loads(r.stdout)
    return run


def words(a0, count):
    """Samples whose bits are their own numbers."""
    return np.arange(a0, a0 + count, dtype=np.int64).astype(np.uint32)


@pytest.mark.parametrize("W", WIDTHS)
def test_blocks_store_their_last_w_samples_each_in_its_own_slot(driver, W):
    """Every block length of the sweep from several fill states, and all of them in a row: what is stored and from where in the
    block, the runs, at most one write per slot and launch, the held range, and a view of everything held."""
    lines, expect = [], []
    for lead in (0, 1, W - 1, W + 3):
        for count in blocks_of(W):
            ring = A.Ring(W)
            lines.append("ring %d" % W)
            expect.append(None)
            if lead:
                lines.append("block 0 %d" % lead)
                ring.launch(words(0, lead), 0)
                expect.append(None)
            lines.append("block %d %d" % (lead, count))
            ring.launch(words(lead, count), lead)
            end, first = ring.held()
            expect.append(("block", lead, count, ring))
            lines.append("view %d %d %d" % (first, end - first, end - first))
            expect.append(("view", first, end - first, ring))
    # one ring through the whole sweep, views at both ends of the held range after each block
    ring = A.Ring(W)
    lines.append("ring %d" % W)
    expect.append(None)
    for count in blocks_of(W) + blocks_of(W)[::-1]:
        a0 = ring.end
        lines.append("block %d %d" % (a0, count))
        ring.launch(words(a0, count), a0)
        expect.append(("block", a0, count, None))
        end, first = ring.held()
        for vf, vc in ((first, 1), (end - 1, 1), (first, end - first), (first + (end - first) // 2, end - first - (end - first) // 2)):
            lines.append("view %d %d %d" % (vf, vc, vc + 3))
            expect.append(("view", vf, vc, (ring.view(vf, vc), end)))
    out = driver(lines)
    assert len(out) == len(expect)
    for got, want in zip(out, expect):
        if want is None:
            continue
        kind, a, b, ring = want
        key = (W, kind, a, b)
        if kind == "block":
            kept = min(b, W)
            assert got["all"] == [0, a, b] and got["kept"] == [b - kept, a + b - kept, kept], key
            slot0, n0, n1 = got["runs"]
            assert [slot0, n0, n1] == list(A.runs(a + b - kept, kept, W)) and slot0 + n0 <= W and n1 <= slot0, key
            assert got["most_writes"] == 1, key
            assert (got["end"], got["first"]) == (a + b, max(0, a + b - W)), key
            if ring is not None and W <= 64:
                assert got["ring"] == ring.holds.tolist(), key
        else:
            assert got["rc"] == 0, key
            if isinstance(ring, tuple):
                assert np.array_equal(np.array(got["samples"], np.int64).astype(np.uint32), ring[0]), key
            else:
                assert np.array_equal(np.array(got["samples"], np.int64).astype(np.uint32), ring.view(a, b)), key
            assert got["samples"] == list(range(a, a + b)), key
            assert got["runs"] == list(A.runs(a, b, W)), key


@pytest.mark.parametrize("W", (1, 3, 4, 1000, 1021))
@pytest.mark.parametrize("n,hop", ((8, 2), (256, 128), (1024, 256), (1024, 1024), (1023, 7)))
def test_frames_store_what_the_ring_does_not_have(driver, W, n, hop):
    """Per-frame form: frame 0 whole, then each frame's last hop; the ring is that of the same samples pushed as blocks."""
    frames = 9
    sess = A.Session(1, n, hop, W, form="frame")
    lines = ["ring %d" % W]
    for j in range(frames):
        lines.append("frame %d %d %d" % (j, n, hop))
        sess.frames(words(j * hop, n)[None])
    end, first = sess.held(0)
    assert end == (frames - 1) * hop + n
    lines.append("view %d %d %d" % (first, end - first, end - first))
    out = driver(lines)
    for j, got in enumerate(out[1:1 + frames]):
        assert got["all"] == ([0, 0, n] if j == 0 else [n - hop, j * hop + n - hop, hop]), (j, got["all"])
        assert got["most_writes"] == 1 and got["end"] == j * hop + n
    assert (out[-1]["end"], out[-1]["first"]) == (end, first)
    assert out[-1]["rc"] == 0 and out[-1]["samples"] == list(range(first, end))
    assert np.array_equal(sess.view(first, end - first)[0], words(first, end - first))


def test_view_validation_at_both_ends_and_near_2_62(driver):
    lines, expect = [], []
    for W in WIDTHS:
        for end in sorted({1, W - 1, W, W + 1, 3 * W + 5} - {0}):
            first = max(0, end - W)
            lines += ["ring %d" % W, "block 0 %d" % end]
            expect += [None, None]
            cases = [(first, 1, 1), (first, end - first, end - first), (end - 1, 1, 1), (first, end - first, end - first + 7),
                     (first - 1, 1, 1), (first - 1, 2, 2), (end, 1, 1), (end - 1, 2, 2), (first, end - first + 1, end - first + 1),
                     (first, 0, 0), (first, -1, 5), (first, 1, 0), (first, end - first, end - first - 1), (-1, 1, 1)]
            for c in cases:
                lines.append("view %d %d %d" % c)
                expect.append((W, end) + c)
    big = 1 << 62
    raw = [  # FIRST COUNT STRIDE END W -> fits
        (big - 5, 5, 5, big, 1 << 28, True), (big - 5, 6, 6, big, 1 << 28, False), (big - (1 << 28), 1 << 28, 1 << 28, big, 1 << 28, True),
        (big - (1 << 28) - 1, 1, 1, big, 1 << 28, False), (big, 1, 1, big, 1 << 28, False), (big - 1, 1, 1, big, 1 << 28, True),
        (big - 1, big, big, big, 1 << 28, False), (big - 1, (1 << 63) - 1, (1 << 63) - 1, big, 1 << 28, False),
        (1, (1 << 63) - 1, (1 << 63) - 1, big, 1 << 28, False), ((1 << 63) - 1, 1, 1, big, 1 << 28, False),
        ((1 << 63) - 2, (1 << 63) - 1, (1 << 63) - 1, (1 << 63) - 1, 1 << 28, False),
        ((1 << 63) - 2, 1, 1, (1 << 63) - 1, 1, True), (big - 3, 3, big, big, 3, True),
    ]
    for r in raw:
        lines.append("check %d %d %d %d %d" % r[:5])
        expect.append(("raw",) + r)
    out = driver(lines)
    checked = 0
    for got, want in zip(out, expect):
        if want is None:
            continue
        if want[0] == "raw":
            assert (got["rc"] == 0) == want[6] == A.view_fits(*want[1:6]), want
        else:
            W, end, first, count, stride = want
            assert (got["rc"] == 0) == A.view_fits(first, count, stride, end, W), (want, got["rc"])
            if got["rc"] == 0:
                assert got["samples"] == list(range(first, first + count)), want
        checked += 1
    assert checked == len(lines) - 2 * sum(len({1, W - 1, W, W + 1, 3 * W + 5} - {0}) for W in WIDTHS)


def test_split_for_every_alignment(driver):
    """Source and destination 0 .. 3 samples behind a 16-byte boundary, every count of the sweep: the split is the model's, it
    copies every sample exactly once, and a 16-byte piece starts on a boundary on both sides."""
    counts = sorted({c for W in WIDTHS for c in blocks_of(W)} | {2, 5, 6, 7, 8, 9})
    cases = [(sa, da, c) for sa in range(4) for da in range(4) for c in counts]
    out = driver(["ring 1"] + ["split %d %d %d" % c for c in cases])[1:]
    for (sa, da, c), got in zip(cases, out):
        head, body, tail = got["split"]
        assert (head, body, tail) == A.split(sa, da, c) and head + 4 * body + tail == c, (sa, da, c)
        assert got["copied"] and got["aligned"] and got["once"], (sa, da, c)
        if sa == da:
            assert head < 4 and tail < 4 and (body > 0 or c < 7), (sa, da, c)   # (the common case moves 16 bytes at a time)
        else:
            assert body == 0, (sa, da, c)


def test_ring_bytes_and_limits(driver):
    out = driver(["ring 1", "bytes 64 524288", "bytes 3 6001", "bytes 65535 268435456", "bytes 1 1"])
    assert (out[1]["bytes"], out[1]["stride"]) == (64 * 524288 * 4, 524288)
    assert (out[2]["bytes"], out[2]["stride"]) == (A.ring_bytes(3, 6001), 6004)
    assert out[3]["bytes"] == 65535 * (1 << 28) * 4                 # (no 32-bit product anywhere)
    assert (out[4]["bytes"], out[4]["stride"]) == (16, 4)
    hdr = open(os.path.join(ROOT, "em-spec_amd", "csrc", "emspec_audio_plan.h")).read()
    assert "kAudioMaxSamples = (int64_t)1 << 28" in hdr and A.MAX_SAMPLES == 1 << 28


def test_model_session_trails_by_less_than_a_frame_then_less_than_a_hop():
    """audio_ref itself: a block session's `end` trails what was pushed by less than a frame before the first frame and by less
    than a hop after; what it holds is what was pushed; a reset stream restarts at 0 and the others keep theirs."""
    rng = np.random.default_rng(11)
    S, n, hop, W = 3, 1024, 256, 6001
    sess = A.Session(S, n, hop, W)
    fed = np.zeros((S, 0), np.uint32)
    for count in (128, 333, 4097, 3 * W + 5, 1, 127):
        block = rng.integers(0, 1 << 32, (S, count), dtype=np.uint64).astype(np.uint32)
        sess.push(block)
        fed = np.concatenate([fed, block], axis=1)
        for s in range(S):
            end, first = sess.held(s)
            pushed = fed.shape[1]
            assert 0 <= pushed - end < (n if pushed < n else hop) and first == max(0, end - W)
            if end > first:
                assert np.array_equal(sess.view(first, end - first, s, 1)[0], fed[s, first:end])
    before = [sess.held(s) for s in range(S)]
    sess.reset_stream(1)
    assert sess.held(1) == (0, 0) and sess.held(0) == before[0] and sess.held(2) == before[2]
