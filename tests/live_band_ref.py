"""The live multi-band session's host arithmetic restated in pure Python, written from the rules and not
from em-spec_amd/csrc/emspec_live_plan.h; tests/test_live_band_plan_cpu.py compares the two field for field.

The rules.  K bands, fft sizes n[0] > ... > n[K-1], one hop.  Band k owns rows [lo_k, hi_k) cut by the K - 1 split rows.  All
bands' frames END on the same sample: band k's frame j + 2 shift_k ends where the long band's frame j ends, shift_k =
(n[0] - n[k]) / (2 hop), so on the emitted column grid band k's frame j is column j - shift_k.  The session is the
single-resolution one at n[0] (tests/live_ref.py: counters, staging, which column a call reports); each band adds a column ring
indexed by the emitted column.  A call that feeds long frames j .. j + m - 1 (m <= mmax) finds emitted columns from j - D on not yet
final, and band k's newest frame sits on emitted column j + m - 1 + shift_k and reaches D_k columns further:
m + shift_k + D + D_k columns are live, so mmax + shift_k + D + D_k slots.  The frame kernel finalises with its plan's latency D_k plus
lat_extra = D - D_k.  A stream's first long frame brings band k's frames 0 .. 2 shift_k at once.  Finalize: a band alone defers to a
second kernel when a launch completes more than 2 columns per stream or its n < 2048; in a multi-band session all bands defer when
any would, and one kernel follows."""
import live_ref as L

SIZES = (1024, 2048, 4096, 8192, 16384)
INLINE = 2


def shape_error(n, hop):
    K = len(n)
    if not 2 <= K <= 4:
        return "bands must be in 2..4"
    if any(v not in SIZES for v in n):
        return "every fft size must be 1024, 2048, 4096, 8192 or 16384"
    if any(b >= a for a, b in zip(n, n[1:])):
        return "fft sizes must be strictly decreasing"
    if not 1 <= hop <= n[-1]:
        return "hop must be in [1, n[bands - 1]]"
    if any((n[0] - v) % (2 * hop) for v in n):
        return "every (n[0] - n[k]) / (2 hop) must be an integer"
    return ""


def split_error(K, split, rows):
    if any(v % 4 for v in split):
        return "every split row must be a multiple of 4"
    if any(b <= a for a, b in zip(split, split[1:])):
        return "split rows must be strictly increasing"
    cuts = [0] + list(split) + [rows]
    if any(b - a < 64 for a, b in zip(cuts, cuts[1:])):
        return "every band must be at least 64 rows high"
    return ""


def geometry(S, hop, reassign, form, R, cell, n, split):
    """-> the dict the driver prints for an accepted shape (without "error" and "two")."""
    g = L.geometry(S, n[0], hop, reassign, form)
    K, D, mmax = len(n), g["D"], g["mmax"]
    cuts = [0] + list(split) + [R]
    shift = [(n[0] - v) // (2 * hop) for v in n]
    Dk = [L.latency(v, hop, reassign) for v in n]
    slots = [mmax + shift[k] + D + Dk[k] for k in range(K)]
    ring = [slots[k] * (cuts[k + 1] - cuts[k]) * cell for k in range(K)]
    small = any(v < 2048 for v in n)
    return dict(S=S, n=n[0], hop=hop, reassign=reassign, D=D, form=form, mmax=mmax, cap=g["cap"], ring_mask=g["ring_mask"],
                bands=K, sring_bytes=S * (g["ring_mask"] + 1) * 4, desc_bytes=32 * S, fresh_bytes=4 * S * g["cap"],
                out1_bytes=4 * S * R, done_bytes=4 * S * K, band_n=list(n), lo=cuts[:-1], hi=cuts[1:], shift=shift,
                band_D=Dk, frame_shift=[2 * v for v in shift], lat_extra=[D - v for v in Dk], slots=slots, ring_bytes=ring,
                rings_bytes=[S * v for v in ring], priming_extra=[2 * v for v in shift],
                defers_1=int(small), defers_2=int(small), defers_3=1)


class Session(L.Session):
    """The calls of a multi-band session: tests/live_ref.py's session at n[0], and per launch what the bands do."""

    def __init__(self, S, hop, reassign, form, R, n, split):
        super().__init__(S, n[0], hop, reassign, form)
        self.n, self.hop = list(n), hop
        self.zero = [set() for _ in n]       # per band: streams whose ring a reset has cleared

    def _steps(self, mlaunch, flush, priming):
        defer = int(not flush and (mlaunch > INLINE or any(v < 2048 for v in self.n)))
        steps = []
        for k, v in enumerate(self.n):       # band 0 carries the ingest; the others follow only when some stream has a frame
            if not flush and (k == 0 or mlaunch > 0):
                steps.append([L.FRAMES, k, mlaunch + (((self.n[0] - v) // self.hop) if priming else 0), 0, defer, int(k == 0)])
        if flush or (defer and mlaunch > 0):  # one kernel for all bands' rows
            steps.append([L.FINALIZE_BANDS, 0, 0, 1 if flush else mlaunch, 0, 0])
        return steps


def run(script):
    def session(o):
        assert o["kind"] == 3 and not o["views"]
        return Session(o["S"], o["hop"], o["reassign"], o["form"], o["R"], o["n"], o["split"])
    return L.run(script, session)
