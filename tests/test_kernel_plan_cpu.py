"""CPU: which kernel serves a call and whether it fits in LDS (em-spec_amd/csrc/emspec_kernel_plan.h) - the LDS size of every product
kernel, the FAST and the EXACT route with every diagnostic switch, the record workspaces and the budget and chunk rule - are the
answers recorded in tests/golden/kernel_plans.json.  That file was written once by the statements as they stood beside the six
kernel files and in emspec_api.cpp before the header took them over, which tests/cdriver/kernel_plan_verbatim.h keeps unchanged
for this purpose:

    g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -DKERNEL_PLAN_VERBATIM \
        -I em-spec_amd/csrc tests/cdriver/kernel_plan_driver.cpp -o kernel_plan_verbatim
    ./kernel_plan_verbatim > tests/golden/kernel_plans.json

It is never written by the library's own header (the same command without -DKERNEL_PLAN_VERBATIM): a shape that moves to
another kernel, or a launch that would be refused, shows up here, without a GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_plans.json")
LDS = 160 * 1024


def build_driver(tmp_path, name, *defines):
    """The stand-alone driver, built with the host compiler under ASan and UBSan (a program of its own: nothing is preloaded)."""
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *defines, "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "kernel_plan_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _find(recs, **case):
    hit = [w for w in recs if all(w["case"][k] == v for k, v in case.items())]
    assert len(hit) >= 1, case
    return hit[0]


def test_kernel_plans_match_the_recorded_answers(tmp_path):
    """The header's answers equal the fixture byte for byte; the case list reaches both sides of every boundary; every recorded
    answer has the properties the launchers and the host layer rely on."""
    out = run_driver(build_driver(tmp_path, "kernel_plan_driver"))
    assert out == open(FIXTURE).read()
    want = json.loads(out)
    names = ("fast", "fast_reach", "frames", "exact_frames", "exact", "exact_lr_split", "records", "reduce", "dump", "chunk")
    kinds = {k: [w for w in want if w["kind"] == k] for k in names}
    assert all(kinds.values()) and sum(map(len, kinds.values())) == len(want) >= 600
    fast, exact = kinds["fast"], kinds["exact"]
    plain = [w for w in fast if not w["case"]["no_fused"] and not w["case"]["variant"]]
    xplain = [w for w in exact if not w["case"]["parked"] and not w["case"]["records"]]

    # ---- the three points worked out by hand from the formulas ----
    w = _find(plain, n=4096, hop=228, rows=1024, reassign=1)
    assert (w["D"], w["route"], w["slots"], w["lds"]) == (9, "fused_small", 20, 156640)
    w = _find(plain, n=4096, hop=227, rows=1024, reassign=1)
    assert (w["D"], w["route"], w["small_lds"]) == (10, "records_f32", 164832) and w["small_lds"] > LDS
    w = _find(xplain, n=4096, hop=256, rows=1024, axis=2, axis_rows=1024, reassign=1)          # an axis the no-parking kernel leaves
    assert (w["D"], w["route"], w["lds"]) == (8, "exact_parked", 161328)
    assert _find(xplain, n=4096, hop=255, rows=1024, axis=2, axis_rows=1024)["route"] == "exact_records"   # D = 9 does not fit
    split = {(w["case"]["D"], w["case"]["rh"]): w for w in kinds["exact_lr_split"] if w["case"]["rows"] == 1024}
    assert (split[8, 576]["lds"], split[8, 576]["ok"]) == (163360, 1) and (split[8, 584]["lds"], split[8, 584]["ok"]) == (164512, 0)

    # ---- the list reaches every size, route, switch and both sides of every boundary ----
    sizes = {256, 512, 1024, 2048, 4096, 8192, 16384}
    assert {w["case"]["n"] for w in fast} == sizes == {w["case"]["n"] for w in exact} == {w["case"]["n"] for w in kinds["exact_frames"]}
    assert {w["case"]["log2n"] for w in kinds["frames"]} == set(range(8, 15))
    assert {w["route"] for w in fast} == {"fused_pp", "fused_small", "fused_8192", "fused_16384", "records_f32"}
    assert {w["route"] for w in exact} == {"exact_lr", "exact_parked", "exact_records"}
    assert {w["case"]["rows"] for w in plain} >= {64, 1024, 1028, 4096} <= {w["case"]["rows"] for w in xplain}
    assert {w["case"]["reassign"] for w in plain} == {0, 1} == {w["case"]["reassign"] for w in xplain}
    for n in sizes:
        assert {w["case"]["hop"] for w in plain if w["case"]["n"] == n} >= {1, 256, n}
    assert {w["case"]["variant"] for w in fast} == {0} and any(w["case"]["no_fused"] for w in fast)
    assert {(w["case"]["parked"], w["case"]["records"]) for w in exact} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert {w["case"]["axis"] for w in exact} == {0, 1, 2} and any(w["case"]["row0"] > 0 and w["rl"] > 0 for w in exact)
    # a ring's hop threshold: neighbouring hops, the same rows, one served by fused_small and one not, the size on either side of LDS
    for n in (4096, 2048, 1024):
        by_hop = {w["case"]["hop"]: w for w in plain if w["case"]["n"] == n and w["case"]["rows"] == 1024 and w["case"]["reassign"]}
        assert any(by_hop[h]["route"] == "records_f32" and by_hop[h]["small_lds"] > LDS and h + 1 in by_hop and
                   by_hop[h + 1]["route"] == "fused_small" and by_hop[h + 1]["lds"] <= LDS for h in by_hop), n
        # ... and its rows threshold, four rows apart, at the hop whose rows are swept for it (the sweep of tests/row_grid_cases.py
        # visits other hops at rows on one side only)
        hop = {4096: 200, 2048: 60, 1024: 40}[n]
        by_rows = {w["case"]["rows"]: w for w in plain if w["case"]["n"] == n and w["case"]["hop"] == hop and w["case"]["reassign"]}
        assert len(by_rows) > 2
        assert any(by_rows[r]["route"] == "fused_small" and r + 4 in by_rows and by_rows[r + 4]["route"] == "records_f32" and
                   r + 4 <= 1024 for r in by_rows), (n, hop)
    big = {(w["case"]["hop"], w["case"]["rows"]): w["route"] for w in plain if w["case"]["n"] == 16384 and w["case"]["reassign"]}
    assert big[511, 1024] == "records_f32" and big[512, 1024] == "fused_16384" and big[256, 516] == "fused_16384" and big[256, 520] == "records_f32"
    assert any(w["case"]["reassign"] == 0 and w["route"] == "fused_small" and w["case"]["hop"] == 1 for w in plain)
    # the rows gate: 64, 1024 and the multiples of 4 between them served, 1028 and 4096 not, 62 and 66 not
    for w in plain:
        c = w["case"]
        if c["hop"] == 512 and c["reassign"] and c["n"] >= 1024:
            assert (w["route"] != "records_f32") == (c["rows"] % 4 == 0 and 64 <= c["rows"] <= 1024), c
    assert {64, 68, 1020, 1024, 1028, 4096, 62, 66} <= {w["case"]["rows"] for w in plain if w["case"]["hop"] == 512 and w["case"]["n"] == 4096}
    # the reach check of the kernels built for one hop
    reach = {(w["case"]["n"], w["case"]["hop"], w["case"]["D"]): w["refused"] for w in kinds["fast_reach"]}
    assert reach[4096, 256, 8] == 0 and reach[4096, 256, 9] == 1 and reach[8192, 512, 8] == 0 and reach[8192, 512, 9] == 1
    assert reach[16384, 512, 17] == 0 and reach[4096, 300, 9] == 0   # rings sized at run time take the plan's D
    # EXACT: the no-parking kernel with its whole ring in LDS and with a row split, and the rows where that changes
    by_rows = {w["case"]["rows"]: w for w in xplain if w["case"]["n"] == 4096 and w["case"]["hop"] == 256 and w["case"]["axis"] == 0 and
               w["case"]["row0"] == 0 and w["case"]["reassign"]}
    assert any(by_rows[r]["rl"] == 0 and r + 4 in by_rows and by_rows[r + 4]["rl"] > 0 for r in by_rows)
    parked = {w["case"]["rows"]: w for w in xplain if w["case"]["n"] == 4096 and w["case"]["hop"] == 255 and w["case"]["axis"] == 2}
    assert parked[940]["route"] == "exact_parked" and parked[944]["route"] == "exact_records"
    # the low-share rule: the same shape on the log axis and on the two others; a band plan on either side of it
    on_axis = {a: _find(xplain, n=4096, hop=256, rows=1024, row0=0, axis_rows=1024, reassign=1, axis=a) for a in (0, 1, 2)}
    assert on_axis[0]["route"] == "exact_lr" and on_axis[0]["rl"] > 0 and on_axis[1]["route"] == on_axis[2]["route"] == "exact_parked"
    bands = [w for w in xplain if w["case"]["axis_rows"] == 2048 and w["case"]["rows"] == 1024 and w["case"]["axis"] == 0]
    assert any(w["route"] == "exact_lr" and w["case"]["row0"] > 0 for w in bands) and any(w["route"] == "exact_parked" for w in bands)
    assert all(w["route"] == "exact_records" for w in exact if w["case"]["records"])
    assert all(w["route"] != "exact_lr" for w in exact if w["case"]["parked"]) and any(w["route"] == "exact_parked" for w in exact if w["case"]["parked"])
    xf = kinds["exact_frames"]
    assert {w["form"] for w in xf} == {0, 1, 2} and {w["edges_lds"] for w in xf} == {0, 1} and all(w["ok"] for w in xf)   # (the edges leave LDS first)
    assert any(not w["ok"] for w in kinds["frames"]) and any(w["ok"] and w["case"]["rows"] == 4096 for w in kinds["frames"])
    pers = {(w["case"]["rows"], w["case"]["S"], w["case"]["nframes"], w["case"]["plain"]): w["form"] for w in xf if w["case"]["n"] == 4096}
    assert pers[1024, 2, 40, 1] == 1 and pers[1036, 2, 40, 1] == 1 and pers[1040, 2, 40, 1] == 0 and pers[1024, 2, 40, 0] == 0 and pers[1024, 2, 32, 1] == 1 and pers[1024, 2, 31, 1] == 0

    # ---- properties of every recorded answer ----
    for w in fast:
        # the yes / no answer is "the route is not the records route", and a route that names a kernel has that kernel's LDS fit
        assert w["supported"] == (w["route"] != "records_f32")
        assert (w["route"] == "records_f32") == (w["lds"] == 0) and w["lds"] <= LDS
        assert w["seg_kind"] == {"fused_pp": 0, "fused_8192": 0, "fused_small": 1, "fused_16384": 2, "records_f32": -1}[w["route"]]
        if w["route"] == "fused_small":
            assert w["lds"] == w["small_lds"]
    for w in exact:
        c = w["case"]
        assert w["lds"] <= LDS and (w["route"] == "exact_records") == (w["lds"] == 0) and not w["lr_refused"]
        if w["route"] == "exact_lr":
            assert w["rl"] % 4 == 0 and w["rl"] >= 0 and w["rh"] == c["rows"] - w["rl"] >= 8 and (w["rh"] == c["rows"] or w["rh"] % 8 == 0)
        else:
            assert w["rl"] == 0
        if w["uses_fused"] >= 0:
            assert w["uses_fused"] == (w["route"] != "exact_records")
    for w in kinds["exact_lr_split"]:
        assert w["ok"] == (w["lds"] <= LDS and w["case"]["rh"] >= 8 and (w["case"]["rows"] - w["case"]["rh"]) % 4 == 0)
        if w["case"]["rh"] == w["rows_in_lds"]:
            assert w["ok"]
    for w in kinds["frames"] + kinds["exact_frames"]:
        assert w["ok"] == (w["lds"] <= LDS) or w["kind"] == "exact_frames" and w["form"] == 2
    for w in kinds["records"]:
        c = w["case"]
        assert w["per_stream"] == w["q_per_stream"] + w["key_per_stream"] and w["q_per_stream"] == 2 * w["key_per_stream"]
        assert w["key_offset"] % 256 == 0 and 0 <= w["key_offset"] - w["q_per_stream"] * c["chunk"] < 256
        assert w["key_offset"] + w["key_per_stream"] * c["chunk"] <= w["per_stream"] * c["chunk"] + w["extra"]
        assert w["f32_per_stream"] == c["C"] * (c["n"] // 2 + 2) * 8
    for w in kinds["reduce"]:
        c = w["case"]
        assert w["idx_offset"] % 256 == 0 and 0 <= w["idx_offset"] - w["db_per_stream"] * c["chunk"] < 256
        assert w["idx_offset"] + (w["per_stream"] - w["db_per_stream"]) * c["chunk"] <= w["per_stream"] * c["chunk"] + w["extra"]
    for w in kinds["dump"]:
        c = w["case"]
        sizes_ = [("pcm", w["b_pcm"]), ("power", w["nb"] * (8 if c["exact"] else 4))] + ([("q", w["nb"] * 8)] if c["exact"] else []) + \
                 [("col", w["nb"] * 4), ("row", w["nb"] * 4)]
        end = 0
        for name, size in sizes_:   # 256-aligned, increasing, not overlapping, inside the allocation
            assert w[name] % 256 == 0 and w[name] >= end
            end = w[name] + size
        assert end <= w["bytes"]
    floor_b = 256 << 20
    for w in kinds["chunk"]:
        c = w["case"]
        tries = w["tries"]
        budget = c["budget_mb"] << 20 if c["budget_mb"] >= 0 else min(max((c["free"] + c["have"]) // 4, floor_b), c["cap"])
        assert tries[0][0] == min(max(budget // c["per_stream"], 1), c["S"]) and tries[-1][0] == 1
        for (chunk, nbytes), nxt in zip(tries, tries[1:] + [None]):
            assert 1 <= chunk <= c["S"] and nbytes == chunk * c["per_stream"] + c["extra"]
            assert nxt is None or nxt[0] == (chunk + 1) // 2 < chunk
    ch = kinds["chunk"]
    assert any(w["case"]["free"] // 4 < floor_b and w["case"]["budget_mb"] < 0 and w["tries"][0][0] > 1 for w in ch)           # the floor
    assert any(floor_b < (w["case"]["free"] + w["case"]["have"]) // 4 < w["case"]["cap"] and 1 < w["tries"][0][0] < w["case"]["S"] for w in ch)
    assert any(w["case"]["free"] // 4 > w["case"]["cap"] and 1 < w["tries"][0][0] < w["case"]["S"] for w in ch)                # the cap
    assert any(w["case"]["per_stream"] > w["case"]["cap"] and w["tries"] == [[1, w["case"]["per_stream"] + w["case"]["extra"]]] for w in ch)
    assert any(w["case"]["S"] % w["tries"][0][0] for w in ch) and any(w["tries"][0][0] == w["case"]["S"] for w in ch)
    assert any(w["case"]["have"] and w["tries"][0][0] > _find(ch, **dict(w["case"], have=0))["tries"][0][0] for w in ch)
    assert {w["case"]["budget_mb"] for w in ch} >= {-1, 0, 1, 64}


def test_recorded_answers_are_the_earlier_statements(tmp_path):
    """The fixture is, byte for byte, what the statements from before the header print (the generator command of the module's
    docstring): its provenance can be checked, and it cannot drift with the library's header."""
    assert run_driver(build_driver(tmp_path, "kernel_plan_verbatim", "-DKERNEL_PLAN_VERBATIM")) == open(FIXTURE).read()
