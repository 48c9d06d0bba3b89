"""The batch entries past 2^31 cells, 2^32 bytes and the stream limits (GPU).

Every other test stays under the bench shape (64 x 16,369 x 1,024 cells: half of 2^31, its dB buffer 3.9 MB short of 2^32
bytes), so a 32-bit product in a cell, byte, sample or record offset, a workspace size or a grid dimension was invisible.
The cases here cross those lines.  The inputs never exist on the host whole (tests/size_ref.py: a small base, the batch built
from it on the device, any slice regenerated bit for bit), and every case is checked twice:

  against the oracle, independent of the library - chosen (stream, column) pairs on the slice of audio that can reach the
      column (frames c-D .. c+D): the column holding each crossed boundary and its two neighbours, the ends of the first and
      last stream, both sides of a segment boundary past the boundary, eight seeded random picks past it.  FAST: |dB error|
      < 8.7e-4, palette index within one step, at most max(8, cells/1000) cells off by one; EXACT: dB bits, index and RGBA
      byte-equal to the binary64 bit model;
  against a small launch, whole streams - every stream that holds a boundary, the last stream and stream 0 (below all of
      them; the record paths: every stream, so both sides of every stream-chunk boundary) equal a call that computes that
      stream alone into a small buffer.  EXACT: torch.equal; FAST: the rule between two launches of tests/test_gpu_host.py
      (|dB difference| < 1e-3, index off by at most 1 on a share of cells < 1e-4).

Each test asserts that the boundaries it is there for lie inside its outputs, frees its tensors before the next one and holds
at most ~28 GB of device memory.  A test that finds too little free device memory skips with the numbers in the reason.

The host-buffer case needs 9 GB of host memory and skips, with the numbers, when the machine cannot give them.

Timeouts: 3 x the measured time of the case on an MI355X, at least 120 s.  Measured: the batch, wire, stream-count and PCM
cases 0.1 - 1.6 s each after their input exists (launches 0.01 - 0.28 s), the post-process, multi-resolution, host-buffer and
gather cases a few seconds with their host-side oracle and arrays; each case prints its own figures in a MEASURED line; the
whole module 45 s including the synthetic bases built on the host.  The kernels are the parent commit's; what changed in the
library is the gather's transfer (pieces of at most 1 GiB), which the gather case here found.
"""
import time

import numpy as np
import pytest

import emspec
import oracle as O
import size_ref as Z
from emspec import synth

pytestmark = pytest.mark.gpu

GB = 1 << 30
_BASES = {}


def _base(B, L):
    if (B, L) not in _BASES:
        _BASES.clear()                      # (one base at a time: at most 64 MB on the host)
        _BASES[(B, L)] = synth.streams(B, L)
    return _BASES[(B, L)]


def _need(nbytes):
    import torch
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < nbytes + 2 * GB:
        pytest.skip(f"needs {nbytes / GB:.1f} GB (+2 GB) of device memory, {free / GB:.1f} of {total / GB:.1f} GB are free")
    torch.cuda.reset_peak_memory_stats()
    _USED0[0] = total - free


_USED0 = [0]


def _held():
    """Device memory taken since the test began, in GB: its tensors, torch's cache and the library's workspaces (read from the
    driver, so the record and band workspaces count; what other processes took meanwhile would count too).  This is the
    figure the 32 GB budget is held against; torch's own peak, printed beside it, leaves the library's workspaces out."""
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free - _USED0[0]) / GB


class Many:
    """S streams of L samples: rolls of a small base (size_ref.build_batch)."""

    def __init__(self, S, L, B=4, copies_of=None):
        self.S, self.L, self.B, self.copies_of = S, L, B, copies_of
        self.base = _base(B, L)

    def _src(self, s):
        return s % self.copies_of if self.copies_of else s

    def device(self, dev, rows=None):
        import torch
        bt = torch.from_numpy(self.base).to(dev)
        rows = range(self.S) if rows is None else rows
        return Z.build_batch(bt, self.S, rows=[self._src(s) for s in rows])

    def slice(self, s, a, b):
        return Z.stream_slice(self.base, self._src(s), a, b)


class Long:
    """S consecutive windows of L samples of one long stream (size_ref.build_long): stream s = samples [s L, (s + 1) L)."""

    def __init__(self, S, L, P=1 << 22):
        self.S, self.L = S, L
        self.base = _base(1, P)[0]

    def device(self, dev, rows=None):
        import torch
        bt = torch.from_numpy(self.base).to(dev)
        if rows is None:
            return Z.build_long(bt, self.L, self.S)
        return torch.cat([Z.build_long(bt, self.L, 1, first=s * self.L) for s in rows])

    def slice(self, s, a, b):
        return Z.long_slice(self.base, s * self.L + a, s * self.L + b)


def _alloc(want, S, Cn, R, dev):
    import torch
    out = {}
    if "db" in want:
        out["db"] = torch.empty((S, Cn, R), dtype=torch.float32, device=dev)
    if "rgba" in want:
        out["rgba"] = torch.empty((S, Cn, R, 4), dtype=torch.uint8, device=dev)
    if "index" in want:
        out["index"] = torch.empty((S, Cn, R), dtype=torch.uint8, device=dev)
    return out


def _oracle_columns(src, pairs, out, n, hop, D, Cn, exact, cfg, lut_t):
    """Chosen columns against the oracle on their slice of audio.  -> (worst |dB error|, cells off by one)."""
    import torch
    worst, off = 0.0, 0
    want = tuple(k for k in ("db", "rgba", "index") if k in out)
    for s, c in pairs:
        f0, f1 = max(0, c - D), min(Cn - 1, c + D)
        seg = src.slice(s, f0 * hop, f1 * hop + n)[None]
        if exact:
            odb, orgba, oidx, _ = O.batch_exact(cfg, seg, want=want, threads=1)
        else:
            odb, orgba, oidx = O.batch_f32(cfg, seg, want=want, threads=1)
        k = c - f0
        if exact:
            if "db" in out:
                assert np.array_equal(out["db"][s, c].cpu().numpy().view(np.uint32), odb[0, k].view(np.uint32)), f"dB bits differ at stream {s} column {c}"
            if "index" in out:
                assert np.array_equal(out["index"][s, c].cpu().numpy(), oidx[0, k]), f"index differs at stream {s} column {c}"
            if "rgba" in out:
                assert np.array_equal(out["rgba"][s, c].cpu().numpy(), orgba[0, k]), f"RGBA differs at stream {s} column {c}"
            continue
        if "db" in out:
            worst = max(worst, float(np.max(np.abs(out["db"][s, c].cpu().numpy() - odb[0, k]))))
        d = np.abs(out["index"][s, c].cpu().numpy().astype(int) - oidx[0, k].astype(int))
        assert d.max() <= 1, f"palette index more than one step off at stream {s} column {c}"
        off += int(np.count_nonzero(d))
        if "rgba" in out:      # the colour is the palette entry of the index the same call wrote, and the oracle's where the indices agree
            g_rgba = out["rgba"][s, c]
            assert torch.equal(g_rgba, lut_t[out["index"][s, c].long()]), f"RGBA is not LUT[index] at stream {s} column {c}"
            assert np.array_equal(g_rgba.cpu().numpy()[d == 0], orgba[0, k][d == 0]), f"RGBA differs from the oracle's at stream {s} column {c}"
    if not exact:
        print(f"MEASURED chosen columns: worst |dB error| {worst:.2e}, cells off by one {off} of {len(pairs) * cfg.rows}")
        assert worst < 8.7e-4, worst
        assert off <= max(8, len(pairs) * cfg.rows // 1000), off
    return worst, off


def _same_as_small(big, small, exact, lut_t, what):
    """One stream of the big launch ([Cn][R] views) against the same columns of a small launch, on the device."""
    import torch
    if exact:
        for k in big:
            assert torch.equal(big[k], small[k]), f"{k} differs from the small launch: {what}"
        return
    if "db" in big:
        dd = float((big["db"] - small["db"]).abs().max())
        assert dd < 1e-3, (what, dd)
    d = (big["index"].to(torch.int16) - small["index"].to(torch.int16)).abs()
    assert int(d.max()) <= 1, what
    share = float((d != 0).float().mean())
    assert share < 1e-4, (what, share)
    if "rgba" in big:
        assert torch.equal(big["rgba"], lut_t[big["index"].long()]), what
        agree = d == 0
        assert torch.equal(big["rgba"][agree], small["rgba"][agree]), f"RGBA differs from the small launch where the indices agree: {what}"


def _run(e, label, src, n, hop, wants, exact=False, cfg_kw=None, need=(), seed=1, every_stream=False, extra_pairs=(),
         itemsizes=None, window=None):
    """One case: a big launch per entry of `wants`, both checks on each.  need: boundary names that must lie inside the outputs
    (size_ref.chosen_columns); window: (first column, columns) - the one-long-stream form of the small launch, a call on
    the samples of that window alone, compared away from its ends."""
    import torch
    dev = torch.device("cuda", 0)
    S, L, R = src.S, src.L, e.rows
    Cn = emspec.num_columns(L, n, hop)
    D = emspec.latency_columns(n, hop, True)
    cfg = O.make_cfg(n, hop, True, rows=R, **(cfg_kw or {}))
    lut_t = torch.from_numpy(O.default_lut()).to(dev)
    t0 = time.time()
    x = src.device(dev)
    assert tuple(x.shape) == (S, L)
    for want in wants:
        t1 = time.time()
        out = _alloc(want, S, Cn, R, dev)
        sizes = itemsizes if itemsizes is not None else sorted({4 if k != "index" else 1 for k in out})
        pairs, where = Z.chosen_columns(S, Cn, R, sizes, seed)
        for name in need:
            assert any(w.startswith(name) for w in where), f"{label}: the shape no longer crosses {name}: {sorted(where)}"
        pairs += [p for p in extra_pairs if p not in pairs]
        e.batch_device(x, n, hop, True, **out)
        torch.cuda.synchronize()
        e.device_status()
        t_launch = time.time() - t1
        held = _held()
        assert held < 32, held
        worst, off = _oracle_columns(src, pairs, out, n, hop, D, Cn, exact, cfg, lut_t)
        # whole streams against a launch of their own
        if window is not None:
            c0, nc = window
            a, b = c0 * hop, (c0 + nc - 1) * hop + n
            xs = x[:, a:b].contiguous()
            small = _alloc(want, S, nc, R, dev)
            e.batch_device(xs, n, hop, True, **small)
            torch.cuda.synchronize()
            e.device_status()
            hi = nc if c0 + nc == Cn else nc - D
            lo = 0 if c0 == 0 else D
            for s in range(S):
                _same_as_small({k: v[s, c0 + lo:c0 + hi] for k, v in out.items()}, {k: v[s, lo:hi] for k, v in small.items()},
                               exact, lut_t, f"{label} stream {s} columns {c0 + lo}..{c0 + hi}")
            streams = [f"window {c0}+{nc}"]
            del xs, small
        else:
            streams = sorted({s for s, _ in where.values()} | {0, S - 1}) if not every_stream else list(range(S))
            for s in streams:
                small = _alloc(want, 1, Cn, R, dev)
                e.batch_device(x[s:s + 1], n, hop, True, **small)
                torch.cuda.synchronize()
                _same_as_small({k: v[s] for k, v in out.items()}, {k: v[0] for k, v in small.items()}, exact, lut_t,
                               f"{label} stream {s}")
                del small
            e.device_status()
        print(f"MEASURED {label} {'+'.join(want)}: cells {S * Cn * R:,} ({S} x {Cn} x {R}), crossed [{', '.join(sorted(where)) or 'none in the outputs'}], "
              f"checked columns {len(pairs)}, whole streams {streams if len(streams) < 12 else len(streams)}, "
              f"worst |dB| error {worst:.2e}, cells off by one {off}, "
              f"peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, {held:.1f} GB taken from the device with the library's workspaces, "
              f"launch {t_launch:.2f} s, case {time.time() - t0:.1f} s")
        del out
        torch.cuda.empty_cache()
    del x
    torch.cuda.empty_cache()


# ---- 1. many streams, FAST fused, FFT 4096 / hop 256 -----------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_many_streams_fast_4096(engine):
    """S = 160 x 2^22 samples: 2,681,896,960 cells, dB and RGBA 10.7 GB each - 2^31 cells in stream 128, 2^32 and 2^33 bytes
    in streams 64 and 128; dB + index in one call, RGBA + index in a second."""
    assert engine.fused(4096, 256, True)
    _need(17 * GB)
    _run(engine, "fast 4096/256 S=160", Many(160, 1 << 22), 4096, 256, [("db", "index"), ("rgba", "index")],
         need=("cell 2^31", "byte 2^32", "byte 2^33"), seed=11)


@pytest.mark.timeout(120)
def test_many_streams_fast_4096_index_past_2_32_cells(engine):
    """S = 264, index only: 4,425,129,984 cells, 2^32 cells (and bytes) in stream 256."""
    _need(10 * GB)
    _run(engine, "fast 4096/256 S=264", Many(264, 1 << 22), 4096, 256, [("index",)], need=("cell 2^31", "cell 2^32"), seed=12)


# ---- 2. the other fused builds, index + dB across 2^31 cells ---------------------------------------------------------------

@pytest.mark.timeout(120)
@pytest.mark.parametrize("n,hop,S,L,B,rows", [(1024, 256, 132, 1 << 22, 4, 1024), (2048, 128, 132, 1 << 22, 4, 512),
                                              (8192, 512, 260, 1 << 22, 4, 1024), (16384, 512, 132, 1 << 23, 2, 1024)])
def test_other_fused_builds_fast(engine, n, hop, S, L, B, rows):
    """fused_small (FFT 1024 / 256; FFT 2048 / 128 at 512 rows, so twice the columns), fused8192 (FFT 8192 / 512) and
    fused16384 (FFT 16384 / 512; 2^23 samples per stream keep the stream count - and the 64 MB base: two streams - down)."""
    _need(16 * GB)
    e = engine if rows == engine.rows else emspec.Engine(rows=rows)
    try:
        assert e.fused(n, hop, True)
        _run(e, f"fast {n}/{hop} S={S} rows={rows}", Many(S, L, B), n, hop, [("db", "index")], need=("cell 2^31", "byte 2^33"), seed=n)
    finally:
        if e is not engine:
            e.close()


# ---- 3. one long stream ----------------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_long_streams_sample_offset_past_2_32_bytes(engine):
    """S = 3 x (2^29 + 4096 + 37) samples, FFT 4096 / hop 512, index only: a stream's samples are 2^31 bytes, so the third
    stream starts past byte 2^32 of the input; each stream has 2^30 + 1024 cells, so cell 2^31 falls at the end of stream 1."""
    L = (1 << 29) + 4096 + 37
    assert 2 * L * 4 >= 1 << 32
    _need(11 * GB)
    _run(engine, "fast 4096/512 S=3 long", Long(3, L), 4096, 512, [("index",)], need=("cell 2^31",), seed=31)


@pytest.mark.timeout(120)
def test_one_stream_sample_index_past_2_31(engine):
    """S = 1, L = 2^31 + 2^20, FFT 4096 / hop 4096, dB + index: frame j >= 524,288 starts at a sample index >= 2^31 (and the
    input passes byte 2^32 at sample 2^30 and 2^33 at 2^31) - where `j * hop` in 32 bits breaks.  524,544 columns: the outputs
    themselves cross nothing, so the chosen columns are those around sample 2^30 and 2^31 (asserted to exist), the ends and
    seeded picks past 2^31; the small launch is a call on the last 2,304 frames' samples alone."""
    n = hop = 4096
    L = (1 << 31) + (1 << 20)
    Cn = emspec.num_columns(L, n, hop)
    j31, j30 = (1 << 31) // hop, (1 << 30) // hop
    assert Cn == 524544 and j31 + 8 < Cn
    rng = np.random.default_rng(32)
    extra = [(0, j) for j in (j30 - 1, j30, j30 + 1, j31 - 2, j31 - 1, j31, j31 + 1, j31 + 2)] + \
        [(0, int(c)) for c in rng.integers(j31 + 1, Cn, 8)]
    _need(14 * GB)
    _run(engine, "fast 4096/4096 S=1 long", Long(1, L), n, hop, [("db", "index")], seed=33, extra_pairs=extra,
         window=(j31 - 2048, Cn - (j31 - 2048)))


# ---- 4. EXACT mode ---------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_many_streams_exact_4096():
    """Case 1 at S = 160 in EXACT mode (the row-split fused kernel; its low-row scratch is sized per launch), dB + index."""
    _need(17 * GB)
    with emspec.Engine(mode=emspec.MODE_EXACT) as x:
        assert x.fused(4096, 256, True)
        _run(x, "exact 4096/256 S=160", Many(160, 1 << 22), 4096, 256, [("db", "index")], exact=True,
             need=("cell 2^31", "byte 2^32", "byte 2^33"), seed=41)


@pytest.mark.timeout(120)
def test_many_streams_exact_4096_warped_axis():
    """The same shape on an axis the row split does not serve (emspec_set_row_edges_hz with the warped table of
    test_exact_custom_axis_and_settings): the parked fused kernel or the record core."""
    _need(26 * GB)
    edges = emspec.warped_edges_hz(1024, 20.0, 24000.0, 2.0, 1.6)
    kw = dict(gain=3.5, db_range=58.0, gate_db=-65.0)
    with emspec.Engine(mode=emspec.MODE_EXACT, **kw) as x:
        x.set_row_edges_hz(edges)
        O.set_custom_edges_hz(edges)
        try:
            _run(x, "exact 4096/256 S=160 warped axis", Many(160, 1 << 22), 4096, 256, [("db", "index")], exact=True, cfg_kw=kw,
                 need=("cell 2^31", "byte 2^33"), seed=42)
        finally:
            O.set_custom_edges_hz(None)


# ---- 4 / 5. record (generic) paths: the workspace is chunked ---------------------------------------------------------------

@pytest.mark.timeout(120)
def test_record_path_exact_16384():
    """EXACT, FFT 16384 / hop 512, S = 132 x 2^23 samples across 2^31 cells: the two-kernel records path (12 B per bin, 1.6 GB
    per stream: five streams fill the 8 GiB workspace, so one chunk's record arrays pass 2^32 bytes and the batch takes some 27
    chunks).  Every stream is compared whole with a call of its own: both sides of every chunk boundary."""
    _need(26 * GB)
    with emspec.Engine(mode=emspec.MODE_EXACT) as x:
        assert not x.fused(16384, 512, True)
        _run(x, "exact records 16384/512 S=132", Many(132, 1 << 23, 2), 16384, 512, [("db", "index")], exact=True,
             need=("cell 2^31", "byte 2^33"), seed=51, every_stream=True)


@pytest.mark.timeout(120)
def test_record_path_fast_rows_2048():
    """FAST, FFT 4096 / 256 at 2,048 rows (no fused kernel: its ring does not fit), S = 80 x 2^22: 2.68e9 cells and several
    4 GiB record chunks (268 MB of records per stream).  Every stream is compared whole with a call of its own."""
    _need(22 * GB)
    with emspec.Engine(rows=2048) as e:
        assert not e.fused(4096, 256, True)
        _run(e, "fast records 4096/256 S=80 rows=2048", Many(80, 1 << 22), 4096, 256, [("db", "index")],
             need=("cell 2^31", "byte 2^32", "byte 2^33"), seed=52, every_stream=True)


# ---- 8. the wire image at its limit ----------------------------------------------------------------------------------------

def _random_index(columns, rows, dev, seed):
    """uint8 [columns][rows] on the device, built in pieces: blocks of 4,096 columns alternate between ~5 % and ~98 % non-zero
    cells (both expand paths: the staged one and the dense-column one; about half the cells in all, so that the payload passes
    offset 2^31 when columns * rows is near 2^32)."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.empty((columns, rows), dtype=torch.uint8, device=dev)
    step = 1 << 15
    for c0 in range(0, columns, step):
        c1 = min(columns, c0 + step)
        dense = ((torch.arange(c0, c1, device=dev) >> 12) & 1).bool()[:, None]
        keep = torch.rand((c1 - c0, rows), device=dev, generator=g) < torch.where(dense, 0.98, 0.05)
        val = torch.randint(1, 256, (c1 - c0, rows), device=dev, generator=g, dtype=torch.int16).to(torch.uint8)
        x[c0:c1] = val * keep
    return x


def _wire_case(e, columns, rows, seed, label, alloc_columns=None):
    import torch
    import wire_ref
    dev = torch.device("cuda", 0)
    t0 = time.time()
    alloc_columns = alloc_columns or columns
    full = _random_index(alloc_columns, rows, dev, seed)
    x = full[:columns]
    wire = torch.zeros(emspec.wire_bound(alloc_columns, rows), dtype=torch.uint8, device=dev)
    nbytes = e.wire_pack(x, wire)
    counts = torch.zeros(columns, dtype=torch.int64, device=dev)
    for c0 in range(0, columns, 1 << 16):
        counts[c0:c0 + (1 << 16)] = (x[c0:c0 + (1 << 16)] != 0).sum(dim=1)
    offs = torch.cumsum(counts, 0) - counts
    payload = int(counts.sum())
    hdr = wire[:32].cpu().numpy().view(np.uint32)
    assert hdr[0] == wire_ref.MAGIC and hdr[1] == rows and (int(hdr[2]) | int(hdr[3]) << 32) == columns
    assert (int(hdr[4]) | int(hdr[5]) << 32) == payload
    fixed = wire_ref.fixed_bytes(columns, rows)
    assert nbytes == fixed + ((payload + 15) & ~15)
    # every column's offset (not a sample): the image's u32 table against the exclusive prefix sum
    got_offs = wire[32:32 + 4 * columns].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got_offs, offs)
    # chosen columns against oracle/wire_ref.py: the ends, around the last 1024-column scan blocks, around payload offset 2^31
    mw = wire_ref.mask_words(rows)
    last_blk = (columns - 1) // 1024 * 1024
    chosen = {0, 1, columns - 1, columns - 2}
    for b in (last_blk, last_blk - 1024, last_blk - 2048):
        chosen |= {b - 1, b, b + 1, b + 1023}
    crossed = payload > (1 << 31)
    if crossed:
        k = int(torch.searchsorted(offs, torch.tensor([1 << 31], device=dev), right=True)[0]) - 1
        chosen |= set(range(k - 4, k + 5))
    rng = np.random.default_rng(seed)
    chosen |= {int(c) for c in rng.integers(0, columns, 12)}
    chosen = sorted(c for c in chosen if 0 <= c < columns)
    for c in chosen:
        col = x[c].cpu().numpy()
        ref = wire_ref.pack(col[None])
        rm = ref[36:36 + 4 * mw]
        rp = ref[36 + 4 * mw:36 + 4 * mw + int(counts[c])]
        m0 = 32 + 4 * columns + 4 * mw * c
        assert np.array_equal(wire[m0:m0 + 4 * mw].cpu().numpy(), rm), f"mask words of column {c}"
        p0 = fixed + int(offs[c])
        assert np.array_equal(wire[p0:p0 + rp.size].cpu().numpy(), rp), f"payload run of column {c}"
    back = torch.full_like(x, 7)
    e.wire_unpack(wire, nbytes, back)
    torch.cuda.synchronize()
    e.device_status()
    assert torch.equal(back, x)
    print(f"MEASURED {label}: cells {columns * rows:,} ({columns} x {rows}), crossed [cell 2^31 of the index, "
          f"{'payload offset 2^31' if crossed else 'payload under 2^31'}], payload {payload:,} B, image {nbytes:,} B, "
          f"checked columns {len(chosen)} against wire_ref (masks, payload run) and all {columns} offsets, round trip byte-equal: "
          f"worst |dB| error n/a, cells off by one 0 (differing cells 0), "
          f"peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, {_held():.1f} GB taken from the device, "
          f"{time.time() - t0:.1f} s")
    del back
    return full, wire, crossed


@pytest.mark.timeout(120)
def test_wire_image_at_its_limit_and_refusal(engine):
    """1,024 rows x (2^22 - 1) columns, one column under the 2^32-cell refusal: pack / unpack round trip on the device, the
    header's payload field, every offset and ~45 chosen columns against oracle/wire_ref.py (the payload passes offset 2^31).
    Then 2^22 columns: emspec_wire_pack and emspec_wire_unpack refuse with EMSPEC_ERR_INVALID_ARG and a message that names
    the limit - on buffers large enough for the refused shape - and the engine still packs afterwards."""
    import torch
    _need(20 * GB)
    cols = (1 << 22) - 1
    full, wire, crossed = _wire_case(engine, cols, 1024, 81, "wire image 1024 rows", alloc_columns=cols + 1)
    assert crossed, "the payload no longer reaches offset 2^31"
    # (the image in `wire` says 2^22 - 1 columns; rewrite its header to 2^22 so that nothing but the size limit can refuse it)
    wire[8:16] = torch.tensor(list((cols + 1).to_bytes(8, "little")), dtype=torch.uint8, device=wire.device)
    for call in (lambda: engine.wire_pack(full, wire), lambda: engine.wire_unpack(wire, wire.numel(), full)):
        with pytest.raises(emspec.EmspecError) as ei:
            call()
        assert ei.value.code == emspec.ERR_INVALID_ARG and "2^32" in str(ei.value)
    small = full[:4096]
    nb = engine.wire_pack(small, wire)
    back = torch.empty_like(small)
    engine.wire_unpack(wire, nb, back)
    torch.cuda.synchronize()
    assert torch.equal(back, small)
    engine.device_status()
    del full, wire, small, back
    torch.cuda.empty_cache()


@pytest.mark.timeout(120)
def test_wire_image_generic_form_near_its_limit():
    """100 rows (the generic, one-wave-per-column kernels) x 42,949,672 columns: 4,294,967,200 cells, 96 under 2^32."""
    import torch
    _need(28 * GB)
    cols = ((1 << 32) - 1) // 100
    assert cols * 100 < 1 << 32 <= (cols + 1) * 100
    with emspec.Engine(rows=100) as e:
        full, wire, crossed = _wire_case(e, cols, 100, 82, "wire image 100 rows")
        assert crossed
        del full, wire
    torch.cuda.empty_cache()


# ---- 9. stream-count limits ------------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode,n,hop", [("fast", 4096, 256), ("exact", 4096, 256), ("fast", 512, 128), ("exact", 512, 128)])
def test_65535_streams_and_the_refusal_of_65536(mode, n, hop):
    """65,535 streams of 4 columns (the C ABI's limit; grid.y of every launcher), copies of 64 distinct ones: every copy equals
    its original, the 64 originals are checked against the oracle; FFT 4096 / 256 runs the fused kernels, FFT 512 / 128 a shape
    without one in either mode (records).  65,536 streams: EMSPEC_ERR_INVALID_ARG, and the engine computes the same bytes
    afterwards."""
    import torch
    S, K = 65535, 64
    L = n + 3 * hop
    exact = mode == "exact"
    dev = torch.device("cuda", 0)
    _need(10 * GB)
    t0 = time.time()
    src = Many(S, L, 4, copies_of=K)
    with emspec.Engine(mode=emspec.MODE_EXACT if exact else emspec.MODE_FAST) as e:
        assert e.fused(n, hop, True) == (n == 4096)
        Cn, R = emspec.num_columns(L, n, hop), e.rows
        assert Cn == 4
        x = torch.empty((S + 1, L), dtype=torch.float32, device=dev)
        x[:S] = src.device(dev)
        x[S] = x[0]
        out = _alloc(("db", "index"), S + 1, Cn, R, dev)
        e.batch_device(x[:S], n, hop, True, db=out["db"][:S], index=out["index"][:S])
        torch.cuda.synchronize()
        e.device_status()
        cfg = O.make_cfg(n, hop, True)
        ref = np.stack([src.slice(s, 0, L) for s in range(K)])
        worst = off = 0
        got_db, got_ix = out["db"][:K].cpu().numpy(), out["index"][:K].cpu().numpy()
        if exact:
            odb, _, oix, _ = O.batch_exact(cfg, ref, want=("db", "index"))
            assert np.array_equal(got_db.view(np.uint32), odb.view(np.uint32)) and np.array_equal(got_ix, oix)
        else:
            odb, _, oix = O.batch_f32(cfg, ref, want=("db", "index"))
            worst = float(np.max(np.abs(got_db - odb)))
            d = np.abs(got_ix.astype(int) - oix.astype(int))
            off = int(np.count_nonzero(d))
            assert worst < 8.7e-4 and d.max() <= 1 and off <= max(8, d.size // 1000), (worst, off)
        # every copy against its original: EXACT bits; FAST the rule between two launches (float sums are order-dependent in
        # the last bits, so equal streams agree to ~1e-5 dB, not bitwise)
        whole = S // K * K
        for k, t in out.items():
            v = t[:whole].view(S // K, K, Cn, R)
            if exact:
                assert torch.equal(v, t[:K].expand_as(v)), k
                assert torch.equal(t[whole:S], t[:S - whole]), k
            else:
                for a, b in ((v, t[:K].expand_as(v)), (t[whole:S], t[:S - whole])):
                    if k == "db":
                        assert float((a - b).abs().max()) < 1e-3
                    else:
                        d = (a.to(torch.int16) - b.to(torch.int16)).abs()
                        assert int(d.max()) <= 1 and float((d != 0).float().mean()) < 1e-4
        first = {k: t[:S].clone() for k, t in out.items()}
        with pytest.raises(emspec.EmspecError) as ei:
            e.batch_device(x, n, hop, True, db=out["db"], index=out["index"])
        assert ei.value.code == emspec.ERR_INVALID_ARG and "65535" in str(ei.value)
        out["db"].zero_(); out["index"].zero_()
        e.batch_device(x[:S], n, hop, True, db=out["db"][:S], index=out["index"][:S])
        torch.cuda.synchronize()
        e.device_status()
        # (the engine after the refusal: EXACT the same bytes; FAST the rule between two launches, as above)
        _same_as_small({k: t[:S] for k, t in out.items()}, first, exact, None, f"{mode} {n}/{hop} after the refusal")
        del first
        print(f"MEASURED {mode} {n}/{hop} S=65535: cells {S * Cn * R:,}, crossed [the stream-count limit], checked columns {K * Cn} "
              f"(64 originals) and every copy, worst |dB| error {worst:.2e}, cells off by one {off}, "
              f"peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, {_held():.1f} GB taken from the device, "
              f"case {time.time() - t0:.1f} s")
        del x, out
    torch.cuda.empty_cache()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sources,views", [(70000, ("mono",)), (66000, ("left", "right", "mid", "side"))])
def test_pcm_decode_past_65535_sources(engine, sources, views):
    """emspec_pcm_decode_device with more sources than grid.y holds (s16 stereo, 300 frames): the kernel's `i += gridDim.y`
    loop.  Bit for bit against tests/pcm_ref.py."""
    import torch
    import pcm_ref
    _need(2 * GB)
    t0 = time.time()
    frames = 300
    fmt = emspec.PcmFormat.make("s16", 2, views)
    rng = np.random.default_rng(sources)
    raw = rng.integers(-32768, 32768, (sources, frames * 2), dtype=np.int16)
    raw[:, :4] = [-32768, 32767, 0, -1]
    src_t = torch.from_numpy(raw).cuda()
    got = engine.pcm_decode_device(src_t, fmt, sources, frames)
    torch.cuda.synchronize()
    engine.device_status()
    ref = pcm_ref.decode(raw.view(np.uint8), pcm_ref.S16, 2, fmt.matrix)
    g = got.cpu().numpy()
    assert g.shape == ref.shape == (sources * len(views), frames)
    assert np.array_equal(g.view(np.uint32), ref.view(np.uint32))
    print(f"MEASURED pcm decode {sources} sources x {len(views)} views: cells n/a ({g.size:,} samples), crossed [65,535 sources: grid.y], "
          f"checked columns n/a (every sample against pcm_ref), worst |dB| error n/a (sample bits equal), cells off by one 0, "
          f"peak memory {torch.cuda.max_memory_allocated() / GB:.2f} GB in torch tensors, {_held():.2f} GB taken from the device, "
          f"{time.time() - t0:.1f} s")
    del src_t, got
    torch.cuda.empty_cache()


# ---- 6. display post-process -----------------------------------------------------------------------------------------------

@pytest.mark.timeout(180)
def test_display_postprocess_exact_4096():
    """Case 1 at S = 160, EXACT, dB + index, with set_display(0.6, 0.5): the raw columns go to a 10.7 GB workspace and
    column_max / agc_scan / smooth_apply run over S * C = 2,619,040 columns.  Whole streams (those holding a boundary, the last
    and stream 0) are byte-equal to a one-stream call; one complete stream past every boundary (the last) is checked against
    O.postprocess over the bit model's raw columns with the project's criteria for this stage (tests/test_gpu_parity.py:
    |dB difference| < 2e-3, palette index within one step)."""
    import torch
    n, hop, S, L = 4096, 256, 160, 1 << 22
    dev = torch.device("cuda", 0)
    _need(28 * GB)
    src = Many(S, L)
    t0 = time.time()
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        e.set_display(0.6, 0.5)
        R, Cn = e.rows, emspec.num_columns(L, n, hop)
        x = src.device(dev)
        out = _alloc(("db", "index"), S, Cn, R, dev)
        pairs, where = Z.chosen_columns(S, Cn, R, [1, 4], 61)
        for name in ("cell 2^31", "byte 2^32", "byte 2^33"):
            assert any(w.startswith(name) for w in where), name
        t1 = time.time()
        e.batch_device(x, n, hop, True, **out)
        torch.cuda.synchronize()
        e.device_status()
        t_launch = time.time() - t1
        held = _held()
        assert held < 32, held
        streams = sorted({s for s, _ in where.values()} | {0, S - 1})
        for s in streams:
            small = _alloc(("db", "index"), 1, Cn, R, dev)
            e.batch_device(x[s:s + 1], n, hop, True, **small)
            torch.cuda.synchronize()
            _same_as_small({k: v[s] for k, v in out.items()}, {k: v[0] for k, v in small.items()}, True, None, f"post-process stream {s}")
            del small
        e.device_status()
        s = S - 1
        cfg = O.make_cfg(n, hop, True)
        raw, _, _, _ = O.batch_exact(cfg, src.slice(s, 0, L)[None], want=("db",))
        pdb, pidx, _ = O.postprocess(raw, 0.6, 0.5, cfg)
        worst = float(np.max(np.abs(out["db"][s].cpu().numpy() - pdb[0])))
        d = np.abs(out["index"][s].cpu().numpy().astype(np.int32) - pidx[0].astype(np.int32))
        off = int(np.count_nonzero(d))
        print(f"MEASURED exact 4096/256 S=160 post-process db+index: cells {S * Cn * R:,} ({S} x {Cn} x {R}), crossed [{', '.join(sorted(where))}], "
              f"checked columns {Cn} (stream {s} whole against O.postprocess), whole streams {streams}, worst |dB| error {worst:.2e}, "
              f"cells off by one {off}, peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, {held:.1f} GB taken "
              f"from the device with the library's workspaces, launch {t_launch:.2f} s, case {time.time() - t0:.1f} s")
        assert worst < 2e-3, worst
        assert d.max() <= 1
        del x, out
    torch.cuda.empty_cache()


# ---- 7. multi-resolution batch, device entry -------------------------------------------------------------------------------

@pytest.mark.timeout(180)
def test_multires_device_exact_across_2_31_cells():
    """emspec_batch_multires_device, 16384 / 4096 / hop 256, split at 250 Hz, EXACT, S = 132 x 2^22 samples: 2,206,076,928
    cells, the bands' workspaces in stream-chunks.  Chosen columns against tests/multires_ref.py on the slice of audio that can
    reach them (low band: frames c-32 .. c+32; the high band's column c + 24 lies inside that slice with its own reach of 8),
    whole streams against the one-stream call: bytes."""
    import torch
    import multires_ref as M
    n_low, n_high, hop, S, L = 16384, 4096, 256, 132, 1 << 22
    dev = torch.device("cuda", 0)
    _need(27 * GB)
    src = Many(S, L)
    t0 = time.time()
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        R, Cn = e.rows, emspec.multires_columns(L, n_low, n_high, hop)
        split = e.split_row_for_hz(250.0)
        D = emspec.latency_columns(n_low, hop, True)
        assert Cn == emspec.num_columns(L, n_low, hop) and D >= emspec.multires_shift(n_low, n_high, hop) + emspec.latency_columns(n_high, hop, True) - 1
        x = src.device(dev)
        out = _alloc(("db", "index"), S, Cn, R, dev)
        pairs, where = Z.chosen_columns(S, Cn, R, [1, 4], 71)
        for name in ("cell 2^31", "byte 2^32", "byte 2^33"):
            assert any(w.startswith(name) for w in where), name
        t1 = time.time()
        e.batch_multires_device(x, n_low, n_high, hop, split, True, **out)
        torch.cuda.synchronize()
        e.device_status()
        t_launch = time.time() - t1
        held = _held()
        assert held < 32, held
        for s, c in pairs:
            f0, f1 = max(0, c - D), min(Cn - 1, c + D)
            ref = M.compose(src.slice(s, f0 * hop, f1 * hop + n_low), n_low, n_high, hop, split, True, exact=True, want=("db", "index"))
            assert np.array_equal(out["db"][s, c].cpu().numpy().view(np.uint32), ref["db"][0, c - f0].view(np.uint32)), f"dB bits differ at stream {s} column {c}"
            assert np.array_equal(out["index"][s, c].cpu().numpy(), ref["index"][0, c - f0]), f"index differs at stream {s} column {c}"
        streams = sorted({s for s, _ in where.values()} | {0, S - 1})
        for s in streams:
            small = _alloc(("db", "index"), 1, Cn, R, dev)
            e.batch_multires_device(x[s:s + 1], n_low, n_high, hop, split, True, **small)
            torch.cuda.synchronize()
            _same_as_small({k: v[s] for k, v in out.items()}, {k: v[0] for k, v in small.items()}, True, None, f"multires stream {s}")
            del small
        e.device_status()
        print(f"MEASURED exact multires 16384/4096/256 S=132 db+index: cells {S * Cn * R:,} ({S} x {Cn} x {R}), crossed [{', '.join(sorted(where))}], "
              f"checked columns {len(pairs)}, whole streams {streams}, worst |dB| error 0.00e+00, cells off by one 0, "
              f"peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, {held:.1f} GB taken from the device with the "
              f"library's workspaces, launch {t_launch:.2f} s, case {time.time() - t0:.1f} s")
        del x, out
    torch.cuda.empty_cache()


# ---- 10 / 8. host buffers: emspec_batch past 2^32 bytes of the caller's array; the gather entry's refusal ---------------------

def _host_available_gb():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / (1 << 20)
    return 0.0


def _host_batch(src):
    """The many-streams batch as a pageable host array (the one case whose input has to live on the host whole)."""
    B, L = src.base.shape
    pcm = np.empty((src.S, L), np.float32)
    for s in range(src.S):
        sh = (s * Z.PRIME) % L
        np.multiply(src.base[s % B][:L - sh], Z.gain(s), out=pcm[s, sh:])
        if sh:
            np.multiply(src.base[s % B][L - sh:], Z.gain(s), out=pcm[s, :sh])
    return pcm


@pytest.mark.timeout(360)
def test_host_batch_index_past_2_32_bytes():
    """emspec_batch (host buffers, pageable: the helper thread and the page-touching threads run), index only, EXACT, S = 66 x
    2^24 samples at FFT 4096 / 256: 4,428,171,264 bytes out, so the caller's array is written past byte 2^32 (stream 64) and
    the input read past it.  Chosen columns against the bit model; the streams holding a boundary, the last and stream 0
    byte-equal to emspec_batch_device on that stream alone.  Needs 9 GB of host memory for the two arrays: skips, with the
    numbers, when MemAvailable is under 14 GB."""
    import torch
    n, hop, S, L = 4096, 256, 66, 1 << 24
    avail = _host_available_gb()
    if avail < 14:
        pytest.skip(f"needs 9 GB of host memory for the caller's arrays (14 GB asked for), {avail:.1f} GB are available")
    _need(8 * GB)
    dev = torch.device("cuda", 0)
    src = Many(S, L, 1)
    t0 = time.time()
    pcm = _host_batch(src)
    assert np.array_equal(pcm[65, 1000:5000].view(np.uint32), src.slice(65, 1000, 5000).view(np.uint32))
    with emspec.Engine(mode=emspec.MODE_EXACT) as e:
        R, Cn = e.rows, emspec.num_columns(L, n, hop)
        D = emspec.latency_columns(n, hop, True)
        pairs, where = Z.chosen_columns(S, Cn, R, [1], 101)
        for name in ("cell 2^31", "cell 2^32", "byte 2^32"):
            assert any(w.startswith(name) for w in where), name
        t1 = time.time()
        idx = e.batch(pcm, n, hop, True, want=("index",))["index"]
        e.device_status()
        t_launch = time.time() - t1
        held = _held()
        assert idx.nbytes > 1 << 32 and held < 32
        cfg = O.make_cfg(n, hop, True)
        for s, c in pairs:
            f0, f1 = max(0, c - D), min(Cn - 1, c + D)
            _, _, oidx, _ = O.batch_exact(cfg, pcm[s, f0 * hop:f1 * hop + n][None], want=("index",), threads=1)
            assert np.array_equal(idx[s, c], oidx[0, c - f0]), f"index differs at stream {s} column {c}"
        streams = sorted({s for s, _ in where.values()} | {0, S - 1})
        for s in streams:
            xs = torch.from_numpy(pcm[s:s + 1]).to(dev)
            small = _alloc(("index",), 1, Cn, R, dev)
            e.batch_device(xs, n, hop, True, **small)
            torch.cuda.synchronize()
            assert np.array_equal(idx[s], small["index"][0].cpu().numpy()), f"host batch differs from the device entry at stream {s}"
            del xs, small
        e.device_status()
        print(f"MEASURED exact host batch 4096/256 S=66 index: cells {S * Cn * R:,} ({S} x {Cn} x {R}), crossed [{', '.join(sorted(where))}], "
              f"checked columns {len(pairs)}, whole streams {streams}, worst |dB| error n/a (index only), cells off by one 0, "
              f"peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, {held:.1f} GB taken from the device with the "
              f"library's staging, host arrays {(pcm.nbytes + idx.nbytes) / GB:.1f} GB, call {t_launch:.2f} s, case {time.time() - t0:.1f} s")
    del pcm, idx
    torch.cuda.empty_cache()


@pytest.mark.timeout(120)
def test_gather_columns_refuses_2_32_cells():
    """The gather's own size check (emspec_gather_columns; a path of its own: the refusal is carried through the size exchange)
    on a single-rank communicator and device buffers: 2^22 columns x 1,024 rows give EMSPEC_ERR_INVALID_ARG with a message
    that names the limit, with and without the loopback; one column fewer is gathered, through the wire image, byte-equal."""
    import torch
    dev = torch.device("cuda", 0)
    _need(22 * GB)
    t0 = time.time()
    with emspec.Engine() as e:
        R, cols = e.rows, 1 << 22
        e.comm_init(emspec.comm_unique_id(), 0, 1)
        try:
            index_t = _random_index(cols, R, dev, 83)
            gathered = torch.empty((cols, R), dtype=torch.uint8, device=dev)
            for loopback in (False, True):
                with pytest.raises(emspec.EmspecError) as ei:
                    e.gather_columns(index_t, 0, out=gathered, loopback=loopback)
                assert ei.value.code == emspec.ERR_INVALID_ARG and "2^32" in str(ei.value), str(ei.value)
            sent = e.gather_columns(index_t[:cols - 1], 0, out=gathered, loopback=True)      # one column under the limit
            torch.cuda.synchronize()
            e.device_status()
            assert sent > 0 and torch.equal(gathered[:cols - 1], index_t[:cols - 1])
            print(f"MEASURED gather_columns refusal: cells {cols * R:,} ({cols} x {R}) refused, {(cols - 1) * R:,} gathered byte-equal "
                  f"({sent:,} B on the wire), crossed [the 2^32-cell limit], checked columns {cols - 1} (all), worst |dB| error n/a, "
                  f"cells off by one 0, peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, "
                  f"{_held():.1f} GB taken from the device, {time.time() - t0:.1f} s")
            del index_t, gathered
        finally:
            e.comm_destroy()
    torch.cuda.empty_cache()


@pytest.mark.timeout(240)
def test_batch_gather_refuses_2_32_cells():
    """The same limit through emspec_batch_gather (host buffers, single-rank communicator): 256 streams of 16,384 columns are
    exactly 2^32 cells; the batch is computed first, the gather then refuses - EMSPEC_ERR_INVALID_ARG, a message that names
    the limit - and the engine gathers a small batch afterwards.  Needs 4.3 GB of host memory for the input (the gathered array
    is never touched): skips, with the numbers, when MemAvailable is under 8 GB."""
    import torch
    n, hop, S = 4096, 256, 256
    L = n + hop * 16383
    avail = _host_available_gb()
    if avail < 8:
        pytest.skip(f"needs 4.3 GB of host memory for the caller's input (8 GB asked for), {avail:.1f} GB are available")
    _need(16 * GB)
    t0 = time.time()
    with emspec.Engine() as e:
        R = e.rows
        assert S * emspec.num_columns(L, n, hop) * R == 1 << 32
        e.comm_init(emspec.comm_unique_id(), 0, 1)
        try:
            base = synth.streams(2, L)
            pcm = np.empty((S, L), np.float32)
            pcm[0::2], pcm[1::2] = base[0], base[1]
            with pytest.raises(emspec.EmspecError) as ei:
                e.batch_gather(pcm, n, hop, True, root=0)
            assert ei.value.code == emspec.ERR_INVALID_ARG and "2^32" in str(ei.value), str(ei.value)
            held = _held()
            small = np.ascontiguousarray(pcm[:3, :n + hop * 40])
            del pcm
            allidx, _, sent = e.batch_gather(small, n, hop, True, root=0)
            ref = e.batch(small, n, hop, True, want=("index",))["index"]
            d = np.abs(allidx[0].astype(int) - ref.astype(int))
            assert d.max() <= 1 and np.mean(d != 0) < 1e-4
            e.device_status()
            print(f"MEASURED batch_gather refusal: cells {1 << 32:,} ({S} x 16384 x {R}) refused after the batch ran, crossed "
                  f"[the 2^32-cell limit], checked columns {3 * 41} (the small batch afterwards), worst |dB| error n/a, cells off by one "
                  f"{int(np.count_nonzero(d))}, peak memory {torch.cuda.max_memory_allocated() / GB:.1f} GB in torch tensors, {held:.1f} GB "
                  f"taken from the device by the library's staging, {time.time() - t0:.1f} s")
        finally:
            e.comm_destroy()
    torch.cuda.empty_cache()
