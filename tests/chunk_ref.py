"""Plain restatement of how the engine cuts a batch into chunks of streams ("Kernel plan": EMSPEC_RECORD_BUDGET_MB).

Six code paths keep an engine workspace bounded by running `chunk` streams at a time (for_stream_chunks / grow_chunked,
em-spec_amd/csrc/emspec_engine.h, emspec_api.cpp).  Each asks the rule of emspec_kernel_plan.h for a chunk with the bytes one
stream needs and a fixed extra; the functions below restate those per-stream sizes, the rule and the list of chunk sizes that
follows, so that a GPU test can say which chunks it expects - and a CPU test (tests/test_chunk_ref_cpu.py) pins every line that
a header states to that header through tests/cdriver/chunk_plan_driver.cpp.

    workspace  path                                per stream                                                   extra
    d_hist     FAST records (run_columns)          C (n/2 + 2) 8          f32_record_bytes, emspec_kernel_plan.h    0
    d_hist     EXACT records (run_columns_exact)   C (n/2 + 4) 12         exact_record_bytes, emspec_kernel_plan.h  kChunkPad
    d_full     time reduction (reduce_streams)     [dB] C R 4 + [index or RGBA] C R      emspec_api.cpp:527-528     kChunkPad
    d_full     emspec_batch_peaks_device           C R 4                                 emspec_peaks.cpp:118       256
    d_mres     two-band batch (multiband_run)      C split 4 + Ch (R - split) 4 + [post] C R 4   band_layout at K = 2   kBandPad
    d_mres     multi-band batch (multiband_run)    band_layout(...).per_stream           emspec_band_plan.h         kBandPad

The two sizes that live in .cpp files cannot be reached from a header; they are cited by line above, and the budgets a GPU test
uses (budget_for) leave a margin of 10 % around them.  multires_bytes stays as the two-band row's own restatement: the CPU tests
compare band_layout at K = 2 against it (tests/test_band_plan_cpu.py, tests/test_chunk_ref_cpu.py).  Lives under tests/ (like multires_ref.py); the product never imports it."""

CHUNK_PAD = 256      # kChunkPad
BAND_PAD = 1024      # kBandPad = 256 * kMaxBands
PEAKS_PAD = 256
FLOOR_MB = 256       # the unbudgeted rule never goes below 256 MiB


def al(v):
    """The host layer's one 256-byte round-up."""
    return (v + 255) & ~255


def num_columns(L, n, hop):
    return (L - n) // hop + 1 if L >= n else 0


# ---- bytes per stream ----
def f32_record_bytes(n, C):
    return C * (n // 2 + 2) * 8


def exact_record_bytes(n, C):
    """(q array, key array, both) per stream: the q array of a chunk comes first, the keys at second_array_offset(q, chunk)."""
    cells = C * (n // 2 + 4)
    return cells * 8, cells * 4, cells * 12


def reduce_bytes(C, R, db, index_or_rgba):
    return (C * R * 4 if db else 0) + (C * R if index_or_rgba else 0)


def peaks_bytes(C, R):
    return C * R * 4


def multires_bytes(C, n_low, n_high, hop, R, split, post):
    Ch = C + (n_low - n_high) // hop          # the high band's own columns: C + 2 shift
    return C * split * 4 + Ch * (R - split) * 4 + (C * R * 4 if post else 0)


def band_planes(n, split_rows, hop, C, R, post):
    """Bytes per stream of each band's plane, then of the raw plane of the display post-process (0 without it)."""
    cuts = [0, *split_rows, R]
    planes = [(C + 2 * ((n[0] - v) // (2 * hop))) * (hi - lo) * 4 for v, lo, hi in zip(n, cuts[:-1], cuts[1:])]
    return planes + [C * R * 4 if post else 0]


def band_bytes(n, split_rows, hop, C, R, post):
    return sum(band_planes(n, split_rows, hop, C, R, post))


def band_offsets(planes, chunk):
    """Where each plane of band_planes starts in the workspace of a chunk: strided by the chunk, each on a 256-byte boundary."""
    out, o = [], 0
    for p in planes:
        out.append(o)
        o += al(p * chunk)
    return out


def second_array_offset(first_per_stream, chunk):
    return al(first_per_stream * chunk)


# ---- the rule ----
def first_chunk(budget_mb, per_stream, S, free_bytes=0, have=0, cap=4 << 30):
    """Streams per chunk.  budget_mb >= 0: the diagnostic build's EMSPEC_RECORD_BUDGET_MB; None: a quarter of what is free
    (counting what the engine holds), at least 256 MiB, at most cap."""
    if budget_mb is None or budget_mb < 0:
        budget = min(max((free_bytes + have) // 4, FLOOR_MB << 20), cap)
    else:
        budget = budget_mb << 20
    return min(max(budget // per_stream, 1), S)


def chunks(budget_mb, per_stream, S):
    """The streams of each chunk in order, e.g. (2, 2, 1)."""
    c = first_chunk(budget_mb, per_stream, S)
    return tuple(min(c, S - s0) for s0 in range(0, S, c))


def halvings(chunk):
    """The chunks tried after a failed allocation (next_chunk), down to one stream."""
    out = []
    while chunk > 1:
        chunk = (chunk + 1) // 2
        out.append(chunk)
    return out


def budget_for(per_stream, chunk=2):
    """An integer budget in MiB that holds chunk + 0.3 .. chunk + 0.65 streams - inside the 2.25 .. 2.75 asked of a GPU case, and
    such that the chunk stays `chunk` when a per-stream size drifts by 10 % either way (2.65 / 0.9 < 3, 2.3 / 1.1 > 2).  None
    when no integer does (the shape is too small or too large: change its frames)."""
    lo, hi = (chunk + 0.3) * per_stream, (chunk + 0.65) * per_stream
    b = -(-int(lo) // (1 << 20))
    while (b << 20) < lo:
        b += 1
    return b if b >= 1 and (b << 20) <= hi else None


def frames_for(per_stream_of_C, lo=25, hi=4096, chunk=2):
    """The fewest columns in [lo, hi] at which budget_for finds a budget: (C, budget in MiB)."""
    for C in range(lo, hi + 1):
        b = budget_for(per_stream_of_C(C), chunk)
        if b is not None:
            return C, b
    raise ValueError("no column count with an integer budget")


# ---- the calls of tests/test_gpu_chunks.py and the workspaces each passes through ----
# A case is a dict: entry "single" (n, hop) / "two" (n_low, n_high, hop, split) / "multi" (sizes, hop, splits); exact; rows;
# f (time reduction); display (the post-process is on); want; peaks (emspec_batch_peaks_device).
def records_for_sure(exact, n, hop, rows=1024):
    """True for the shapes that tests/golden/kernel_plans.json records on the per-bin records path whatever the band: EXACT
    N >= 8192; FAST more than 1024 rows, N = 8192 off hop 512 / 1024, N = 16384 past the register park (D > 16), N = 4096 / 227."""
    if exact:
        return n >= 8192
    D = (n + 2 * hop - 1) // (2 * hop)
    return rows > 1024 or (n == 8192 and hop not in (512, 1024)) or (n == 16384 and D > 16) or (n, hop) == (4096, 227)


def _records(exact, n, C):
    return (f"d_hist (EXACT records, N = {n})", exact_record_bytes(n, C)[2]) if exact else (f"d_hist (FAST records, N = {n})", f32_record_bytes(n, C))


def path(case, C):
    """[(workspace, bytes per stream)] of a call of C full-rate columns, outermost first.  An inner workspace is chunked anew inside
    every chunk of the one before it; a band is listed when records_for_sure says it takes the records path."""
    R, exact, want = case.get("rows", 1024), case["exact"], case.get("want", ("db", "index"))
    post = bool(case.get("display"))
    p = []
    if case.get("peaks"):
        p.append(("d_full (peaks)", peaks_bytes(C, R)))
    elif case.get("f", 1) > 1:
        p.append(("d_full (time reduction)", reduce_bytes(C, R, "db" in want, "index" in want or "rgba" in want)))
    if case["entry"] == "two":
        n_low, n_high, hop, split = case["shape"]
        p.append(("d_mres (two-band)", multires_bytes(C, n_low, n_high, hop, R, split, post)))
        bands = [(n_low, C), (n_high, C + (n_low - n_high) // hop)]
    elif case["entry"] == "multi":
        n, hop, splits = case["shape"]
        p.append(("d_mres (multi-band)", band_bytes(n, splits, hop, C, R, post)))
        bands = [(v, C + (n[0] - v) // hop) for v in n]
    else:
        n, hop = case["shape"]
        bands = [(n, C)]
    for v, Cv in bands:
        if case.get("records") or (case["entry"] != "single" and records_for_sure(exact, v, hop, R)):
            p.append(_records(exact, v, Cv))
    return p


def columns_and_budget(case, lo=25):
    """The fewest columns >= lo at which an integer budget holds 2.25 .. 2.75 streams of the call's OUTERMOST workspace:
    (C, budget in MiB)."""
    return frames_for(lambda C: path(case, C)[0][1], lo)


def outer_chunks(case, C, budget_mb, S):
    """The chunk list of the call's outermost workspace."""
    return chunks(budget_mb, path(case, C)[0][1], S)


def expected(case, C, budget_mb, S):
    """One line per workspace of the call: the chunk list the rule gives at this budget (an inner workspace: per size of the
    chunks around it).  The first line is the outermost workspace's."""
    lines, around = [], (S,)
    for depth, (name, per) in enumerate(path(case, C)):
        lists = {sc: chunks(budget_mb, per, sc) for sc in sorted(set(around), reverse=True)}
        what = lists[S] if depth == 0 else "; ".join(f"inside a chunk of {sc}: {v}" for sc, v in lists.items())
        lines.append(f"{name}: {per} B per stream, budget {budget_mb} MiB -> chunks {what}")
        if not name.startswith("d_hist"):   # (the bands' records all sit inside the same chunks)
            around = tuple(c for v in lists.values() for c in v)
    return lines
