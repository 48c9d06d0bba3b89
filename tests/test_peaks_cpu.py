"""CPU: the spectral peaks.  emspec_peaks_host - plain C++ in the product library, no device, no engine -
against the numpy restatement tests/peaks_ref.py, byte for byte; checks on the restatement itself; emspec_position_hz's
formula; the host call's refusals; the note read-out of the Node binding restated here."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import emspec
import peaks_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = (4, 64, 100, 1024, 4096)
KS = (1, 8, 32)


@pytest.mark.parametrize("R", SHAPES)
def test_peaks_host_equals_the_reference(R):
    """Every case of peaks_ref.cases(R), k = 1, 8 and 32: the raw bytes are equal."""
    seen = 0
    for name, db, min_db in P.cases(R):
        for k in KS:
            got = emspec.peaks_host(db, k, min_db)
            want = P.peaks(db, k, min_db)
            assert got.shape == want.shape == (db.shape[0], k, 2)
            assert np.array_equal(P.bits(got), P.bits(want)), (name, R, k, got[0], want[0])
            seen += 1
    assert seen >= 12 * len(KS)


def test_the_cases_hold_what_their_names_say():
    """The generator really produces the situations of the list (at R = 4096, where all of them exist)."""
    R = 4096
    by = {name: (db, m) for name, db, m in P.cases(R)}
    count = lambda name: int(P.parts(*by[name])[0].sum())
    assert count("below_min_db") == 0 and count("floor_200") == 0 and count("nan_neighbour") == 0
    assert count("sawtooth") == R // 2
    for k in KS:
        assert count(f"exactly_{k}") == k
    assert count("four_values") > 32 and len(np.unique(by["four_values"][0][0, 0::2])) == 4
    cand = P.parts(*by["plateaus"])[0][0]
    assert np.nonzero(cand)[0].tolist() == [3, 9, 11]          # first rows of both plateaus, and the rise behind the second
    assert np.nonzero(P.parts(*by["flat_above"])[0][0])[0].tolist() == [0]
    assert np.nonzero(P.parts(*by["floor_200_all_pass"])[0][0])[0].tolist() == [0]
    assert np.nonzero(P.parts(*by["ends"])[0][0])[0].tolist() == [0, R - 1]
    for at in (3, 4, 255, 256, 1023, 1024):
        assert np.nonzero(P.parts(*by[f"boundary_{at}"])[0][0])[0].tolist() == [at]
    z = P.peaks(*by["signed_zeros"][:1], 2, -1.0)
    assert z[0, :, 0].tolist() == [0.5, 2.5] and z[1, :, 0].tolist() == [0.5, 2.5]                  # the tie goes to the lower row
    assert np.signbit(z[0, 0, 1]) and not np.signbit(z[0, 1, 1]) and np.signbit(z[1, 1, 1])        # and the bits are the cells'
    db, m = by["nan_inf"]
    p = P.peaks(db, 1, m)
    assert np.all(np.isposinf(p[:3, 0, 1]))                     # +inf is the loudest peak where it has two real neighbours
    assert not np.any(np.isnan(p))
    _, _, d, _ = P.parts(*by["one_ulp"])
    assert np.all(np.abs(d[:, 3]) > F(0.49999)) and np.sum(np.abs(d[:, 3]) == F(0.5)) >= 6
    assert np.all(d[0::2, 3] > 0) and np.all(d[1::2, 3] < 0)


@pytest.mark.parametrize("R", SHAPES)
def test_reference_invariants(R):
    """|d| <= 0.5 everywhere; within a column dB descends and equal dB ascend in row; unused slots are (-1, -inf) and come
    last; every used slot's row is a candidate and its dB the cell's."""
    for name, db, min_db in P.cases(R):
        cand, pos, d, _ = P.parts(db, min_db)
        assert np.all(np.abs(d) <= F(0.5)) and not np.any(np.isnan(d)), name
        for k in KS:
            p = P.peaks(db, k, min_db)
            for c in range(db.shape[0]):
                used = p[c, :, 0] >= 0
                n = int(used.sum())
                assert n == min(k, int(cand[c].sum())), (name, c)
                assert np.all(used[:n]) and np.all(p[c, n:, 0] == F(-1.0)) and np.all(np.isneginf(p[c, n:, 1]))
                rows = []
                for pos_t, db_t in zip(p[c, :n, 0], p[c, :n, 1]):
                    # (|d| <= 0.5 keeps pos inside [r, r + 1]; d = 0.5 lands on r + 1 exactly: then row r is the candidate)
                    r = int(np.floor(pos_t))
                    ok = lambda q: 0 <= q < R and cand[c, q] and P.bits(db[c, q]) == P.bits(db_t)
                    if not ok(r) or (pos_t == F(r) and ok(r - 1) and d[c, r - 1] == F(0.5) and r - 1 not in rows):
                        r -= 1
                    assert ok(r) and pos[c, r] == pos_t, (name, c, pos_t)
                    rows.append(r)
                rows = np.array(rows, int)
                assert len(set(rows.tolist())) == n
                v = p[c, :n, 1]
                assert np.all((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (rows[:-1] < rows[1:]))), (name, c)


def test_an_exactly_sampled_parabola_returns_its_vertex():
    """y(r + j) = K - 16 (j - d)^2 with d = +-0.25 has the integer samples K - 25, K - 1, K - 9: every operation of step 3
    is exact, so pos = r + 0.5 + d - negative towards the louder left neighbour."""
    for R, r in ((64, 5), (1024, 256), (4096, 4000)):
        for d, (a, c) in ((0.25, (-25.0, -9.0)), (-0.25, (-9.0, -25.0))):
            x = np.full(R, -80.0, F)
            x[r - 1], x[r], x[r + 1] = -30.0 + a, -30.0 - 1.0, -30.0 + c
            for p in (P.peaks(x, 1, -60.0), emspec.peaks_host(x, 1, -60.0)):
                assert p.shape == (1, 2) and p[0, 0] == F(r + 0.5 + d) and p[0, 1] == F(-31.0)


def _position_hz(edges, pos):
    R = len(edges) - 1
    i = min(max(int(math.floor(pos)), 0), R - 1)
    return float(edges[i]) * (float(edges[i + 1]) / float(edges[i])) ** (pos - i)


def test_position_hz_formula_on_an_edge_table():
    """The formula of emspec_position_hz on a log axis: integer positions are the edges, r + 0.5 the geometric centre of the
    row, to 1e-12 relative (the engine call itself needs a device: tests/test_gpu_peaks.py compares it with this)."""
    edges = emspec.warped_edges_hz(1024, 20.0, 24000.0, 1.0, 1.0)
    for r in (0, 1, 511, 1023):
        assert abs(_position_hz(edges, float(r)) / float(edges[r]) - 1) < 1e-12
        assert abs(_position_hz(edges, r + 0.5) / math.sqrt(float(edges[r]) * float(edges[r + 1])) - 1) < 1e-12
    assert abs(_position_hz(edges, 1024.0) / float(edges[1024]) - 1) < 1e-12


def test_host_call_refusals():
    """k outside 1 .. 32, a NaN min_db, rows breaking the rule, negative columns, null and misaligned pointers:
    EMSPEC_ERR_INVALID_ARG with a message naming the rule; a good call afterwards works; columns = 0 is a no-op."""
    lib = emspec.load()
    db = np.full((3, 64), -80.0, F)
    db[:, 7] = -10.0
    out = np.zeros((3, 8, 2), F)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda d, cols, rows, k, m, o: lib.emspec_peaks_host(d, cols, rows, k, m, o)
    msg = lambda: lib.emspec_last_error(None).decode()
    for k in (0, -1, 33):
        assert call(ptr(db), 3, 64, k, -60.0, ptr(out)) == emspec.ERR_INVALID_ARG and "k must be in [1, 32]" in msg()
    assert call(ptr(db), 3, 64, 8, float("nan"), ptr(out)) == emspec.ERR_INVALID_ARG and "NaN" in msg()
    for rows in (0, 2, 66, 4100, -4):
        assert call(ptr(db), 1, rows, 8, -60.0, ptr(out)) == emspec.ERR_INVALID_ARG and "rows % 4 == 0" in msg()
    assert call(ptr(db), -1, 64, 8, -60.0, ptr(out)) == emspec.ERR_INVALID_ARG and "columns" in msg()
    assert call(None, 3, 64, 8, -60.0, ptr(out)) == emspec.ERR_INVALID_ARG and "null" in msg()
    assert call(ptr(db), 3, 64, 8, -60.0, None) == emspec.ERR_INVALID_ARG and "null" in msg()
    assert call(C.c_void_p(db.ctypes.data + 1), 2, 64, 8, -60.0, ptr(out)) == emspec.ERR_INVALID_ARG and "aligned" in msg()
    assert not out.any()                                        # a refusal writes nothing
    assert call(None, 0, 64, 8, -60.0, None) == emspec.OK       # no columns: nothing is read
    assert call(ptr(db), 3, 64, 8, -60.0, ptr(out)) == emspec.OK
    assert np.array_equal(P.bits(out), P.bits(P.peaks(db, 8, -60.0)))
    with pytest.raises(emspec.EmspecError, match="k must be"):
        emspec.peaks_host(db, 40, -60.0)


NOTE_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")


def note_of(hz):
    """12-TET around A4 = 440 Hz: the nearest semitone, cents in [-50, 50) - what index.js's noteOf computes."""
    semis = 12.0 * math.log2(hz / 440.0)
    n = math.floor(semis + 0.5)
    midi = 69 + n
    return {"name": NOTE_NAMES[midi % 12], "octave": midi // 12 - 1, "cents": 100.0 * (semis - n)}


def test_note_of():
    a4, c4, a0 = note_of(440.0), note_of(261.6256), note_of(27.5)
    assert (a4["name"], a4["octave"]) == ("A", 4) and a4["cents"] == 0.0
    assert (c4["name"], c4["octave"]) == ("C", 4) and abs(c4["cents"]) < 0.01
    assert (a0["name"], a0["octave"]) == ("A", 0) and a0["cents"] == 0.0
    up = note_of(440.0 * 2 ** (49.9 / 1200))
    down = note_of(440.0 * 2 ** (50.0 / 1200) * (1 + 1e-12))
    assert up["name"] == "A" and abs(up["cents"] - 49.9) < 1e-6
    assert down["name"] == "A#" and -50.0 <= down["cents"] < -49.99
    node = shutil.which("node") or shutil.which("nodejs")
    js = os.path.join(ROOT, "em-spec_amd", "js")
    if not node or not os.path.exists(os.path.join(js, "emspec.node")):
        return                                                   # (the binding's own copy is compared where the addon is built)
    hzs = [440.0, 261.6256, 27.5, 452.9, 7040.0, 19.99]
    code = "const m=require('./index.js');process.stdout.write(JSON.stringify(%s.map(m.noteOf)))" % json.dumps(hzs)
    got = json.loads(subprocess.run([node, "-e", code], cwd=js, capture_output=True, text=True, check=True, timeout=60).stdout)
    for hz, g in zip(hzs, got):
        w = note_of(hz)
        assert (g["name"], g["octave"]) == (w["name"], w["octave"]) and abs(g["cents"] - w["cents"]) < 1e-9, (hz, g, w)
