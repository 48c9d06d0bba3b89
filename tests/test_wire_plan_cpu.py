"""CPU: the host arithmetic of the multi-GPU gather and of its wire image (em-spec_amd/csrc/emspec_wire_plan.h) - the sizes of
an image and of the pack workspace, the three header checks, the host expand, the roles and argument rules of a gather, the check
of the announced (bytes, columns) pairs, the root's layout of uneven shards, the transfer pieces and the staging block of
emspec_batch_gather - is the one recorded in tests/golden/gather_plans.json.  That file was written once by the arithmetic as it
stood inside emspec_comm.cpp, emspec_api.cpp, emspec_host.cpp and pack.hip.inc before the header took it over, which
tests/cdriver/wire_plan_verbatim.h keeps unchanged for this purpose:

    g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -DWIRE_PLAN_VERBATIM -I em-spec_amd/csrc \
        tests/cdriver/wire_plan_driver.cpp -o wire_plan_verbatim
    ./wire_plan_verbatim > tests/golden/gather_plans.json

It is never written by the library's own header (the same command without -DWIRE_PLAN_VERBATIM): a change of the arithmetic shows
up here, without a GPU - with world > 1 the only other road to it is the diagnostic build's in-process communicator."""
import json
import os
import subprocess

import numpy as np
import pytest

import wire_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gather_plans.json")
INVALID = -1          # EMSPEC_ERR_INVALID_ARG
GIB = 1 << 30


def al(v):
    return (v + 255) // 256 * 256


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """The stand-alone driver, built with the host compiler under ASan and UBSan (a program of its own: nothing is preloaded), from
    the library's header and from the verbatim one."""
    d = tmp_path_factory.mktemp("wire_plan")
    out = {}
    for name, defines in (("lib", []), ("verbatim", ["-DWIRE_PLAN_VERBATIM"])):
        out[name] = str(d / ("wire_plan_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *defines,
                               "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cdriver", "wire_plan_driver.cpp"), "-o", out[name]])
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _expected_answers(magic_ok, hrows, hcols, hpay, length, columns, rows):
    """[header matches, emspec_wire_unpack accepts, emspec_wire_unpack_host's code, drain() accepts, the bytes drain() copies] from
    the rules as include/emspec.h and pack.hip.inc state them: an image of (columns, rows) carries the magic, these rows and
    columns and at most columns * rows payload bytes; the device expand needs the padded image, the host expand the payload only;
    drain() has the header alone.  Shorter than a header: nothing is read (the driver answers 0 for the header's checks)."""
    fixed = W.fixed_bytes(columns, rows)
    match = length >= 32 and magic_ok and hrows == rows and hcols == columns and hpay <= columns * rows
    padded = fixed + (hpay + 15) // 16 * 16
    host_ok = match and length >= fixed + hpay
    return [int(match), int(match and length >= padded), 0 if host_ok else INVALID, int(match), padded if match else -1]


def _check_damaged(d, columns, rows, payload, nbytes):
    """Every damaged form of one image (the driver's damage_names) against _expected_answers.  (The driver's own images have a
    payload field but no mask bit set: the host expand reads no payload byte of them; a real image whose length passes expands.)"""
    fixed = W.fixed_bytes(columns, rows)
    assert nbytes == fixed + (payload + 15) // 16 * 16
    cases = {"intact": (True, rows, columns, payload, nbytes), "magic": (False, rows, columns, payload, nbytes),
             "rows+4": (True, rows + 4, columns, payload, nbytes), "rows-4": (True, rows - 4, columns, payload, nbytes),
             "columns+1": (True, rows, columns + 1, payload, nbytes), "columns-1": (True, rows, columns - 1, payload, nbytes),
             "payload=cells+1": (True, rows, columns, columns * rows + 1, nbytes),
             "len31": (True, rows, columns, payload, 31), "len32": (True, rows, columns, payload, 32),
             "len=fixed+payload-1": (True, rows, columns, payload, fixed + payload - 1),
             "len=fixed+payload": (True, rows, columns, payload, fixed + payload),
             "len=padded-1": (True, rows, columns, payload, nbytes - 1)}
    assert set(d) == set(cases)
    for name, c in cases.items():
        assert d[name] == _expected_answers(*c, columns, rows), (columns, rows, payload, name, d[name])
    assert d["intact"][:4] == [1, 1, 0, 1] and d["len=fixed+payload"][2] == 0 and d["len=fixed+payload-1"][2] == INVALID
    assert d["len=padded-1"][1] == 0 and d["len=padded-1"][2] == (0 if payload % 16 else INVALID)   # the two length rules differ


def test_wire_plan_matches_the_recorded_plans(drivers):
    """The header's answers equal the fixture field by field; the case list reaches every branch; every recorded layout is sound
    on its own."""
    got = json.loads(_run(drivers["lib"]))
    want = json.load(open(FIXTURE))
    assert list(got) == list(want) == ["sizes", "scratch", "roles", "args", "pairs", "layouts", "pieces", "stage", "headers"]
    for sec in want:
        assert len(got[sec]) == len(want[sec])
        for g, w in zip(got[sec], want[sec]):
            assert g.keys() == w.keys()
            for key in w:
                assert g[key] == w[key], (sec, w.get("case", w), key, g[key], w[key])

    # ---- sizes: the format as oracle/wire_ref.py states it, rows 4 .. 4096, columns up to 2^22 - 1
    assert {w["rows"] for w in want["sizes"]} == {4, 64, 68, 1024, 4096} and max(w["columns"] for w in want["sizes"]) == (1 << 22) - 1
    for w in want["sizes"]:
        C, R = w["columns"], w["rows"]
        assert w["mask_words"] == W.mask_words(R) and w["fixed"] == W.fixed_bytes(C, R) and w["bound"] == W.bound(C, R)
        assert w["padded"] == [w["fixed"] + (p + 15) // 16 * 16 for p in (0, 1, 16, C * R)] and w["padded"][3] <= w["bound"]
    # ---- the pack workspace: local offsets [columns] u32, block sums [ceil(columns / 1024)] u32, the u64 pair of the gather
    for w in want["scratch"]:
        C = w["columns"]
        assert w["local"] == 0 and w["bsum"] % 256 == 0 and w["total"] % 256 == 0
        assert w["bsum"] >= 4 * C and w["total"] >= w["bsum"] + 4 * -(-C // 1024) and w["bytes"] >= w["total"] + 16
        assert w["bytes"] == al(4 * C) + al(4 * -(-C // 1024)) + 256
    # ---- roles
    for w in want["roles"]:
        root, lb, pk = w["rank"] == w["root"], bool(w["flags"] & 1), bool(w["flags"] & 2)
        assert (w["is_root"], w["i_send"], w["i_pack"]) == (int(root), int(not root or lb), int(not root or lb or pk))
    assert {(w["is_root"], w["i_send"], w["i_pack"]) for w in want["roles"]} == {(0, 1, 1), (1, 0, 0), (1, 1, 1), (1, 0, 1)}
    # ---- the argument rules, in precedence order
    texts = ["null argument / no columns", "root out of range", "the root needs the gathered buffer", "at most 2^32 cells per call"]
    for w in want["args"]:
        broken = [not w["index"] or w["columns"] < 1, not 0 <= w["root"] < w["world"], w["is_root"] and not w["gathered"],
                  w["columns"] * w["R"] >= 1 << 32]
        first = broken.index(True) if any(broken) else None
        assert (w["code"], w["msg"]) == ((0, "") if first is None else (INVALID, texts[first])), w
    for i in range(4):   # every rule fires alone, and wins over every later one that is broken with it
        assert any(w["msg"] == texts[i] for w in want["args"])
    assert sum(w["code"] == 0 for w in want["args"]) >= 4
    # ---- the announced pairs
    for w in want["pairs"]:
        pairs, R = np.array(w["pairs"], dtype=object).reshape(-1, 2), w["R"]
        failed = [r for r, (b, c) in enumerate(pairs) if b == (1 << 64) - 1]
        impossible = any(c < 1 or c * R >= 1 << 32 or b > W.bound(c, R) for b, c in pairs)
        if failed:
            assert w["error"] == f"rank {failed[0]} failed before the exchange: no columns were transferred"
        else:
            assert w["error"] == ("a rank announced an impossible wire image (column count / size)" if impossible else "")
    names = {w["name"]: w["error"] for w in want["pairs"]}
    assert names["good"] == names["bytes = bound"] == names["root announces 0"] == names["cols * R = 2^32 - R"] == ""
    assert names["first failed"].startswith("rank 0 ") and names["last failed"].startswith("rank 3 ") and names["two failed"].startswith("rank 1 ")
    assert names["failed behind an impossible pair"].startswith("rank 3 ")
    assert all("impossible" in names[k] for k in ("cols = 0", "cols * R = 2^32", "bytes = bound + 1", "68 rows, bytes = bound + 1"))

    # ---- layouts: sound on their own
    lay = want["layouts"]
    for w in lay:
        c = w["case"]
        world, R, packed = c["world"], c["R"], c["packed"]
        nbytes, cols = c["pairs"][0::2], c["pairs"][1::2]
        assert len(w["off"]) == len(w["dst_off"]) == world + 1 and len(w["dir"]) == 4 * world
        assert w["dir_bytes"] == (al(32 * world) if packed else 0)
        if c["rank"] != c["root"]:    # only the root lays anything out
            assert not any(w["off"]) and not any(w["dst_off"]) and w["fits"] == 1
        else:
            # images: 256-aligned, in rank order, not overlapping, no more than the alignment apart
            assert w["off"][0] == 0 and all(o % 256 == 0 for o in w["off"])
            assert all(nbytes[r] <= w["off"][r + 1] - w["off"][r] < nbytes[r] + 256 for r in range(world))
            # expanded blocks tile [0, sum(cols) * R)
            assert w["dst_off"][0] == 0 and [w["dst_off"][r + 1] - w["dst_off"][r] for r in range(world)] == [k * R for k in cols]
            assert w["dst_off"][world] == sum(cols) * R
            assert w["need"] == (w["dir_bytes"] + w["off"][world] if packed else w["dst_off"][world])
            assert w["fits"] == int(max(c["capacity"], 0) >= w["need"])
        assert w["recv_bytes"] == w["off"][world] + 256
        # the directory: (offset, bytes, columns, 0) with the running 256-aligned offset behind the directory itself
        run = w["dir_bytes"]
        for r in range(world):
            assert w["dir"][4 * r:4 * r + 4] == [run if c["rank"] == c["root"] else w["dir_bytes"], nbytes[r], cols[r], 0]
            run += al(nbytes[r])
    roots = [w for w in lay if w["case"]["rank"] == w["case"]["root"]]
    assert {w["case"]["world"] for w in roots} >= {1, 2, 3, 4, 8} and {w["case"]["root"] for w in roots} >= {0, 1, 2, 3}
    assert {(w["case"]["packed"], w["case"]["loopback"]) for w in roots} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    mock = [w for w in roots if w["case"]["world"] == 8 and w["case"]["name"] == "mock shards"]
    assert mock and all(w["case"]["pairs"][1::2] == [48 * k for k in (3, 1, 2, 4, 2, 1, 3, 2)] and w["case"]["R"] == 1024 for w in mock)
    assert any(w["case"]["pairs"][0] == 0 for w in mock) and any(w["case"]["pairs"][0] > 0 for w in mock)   # the root packs nothing / something
    for packed in (0, 1):
        some = [w for w in roots if w["case"]["packed"] == packed]
        assert any(w["case"]["capacity"] == w["need"] and w["fits"] for w in some)
        assert any(w["case"]["capacity"] == w["need"] - 1 and not w["fits"] for w in some)
        assert any(w["case"]["capacity"] == 0 and not w["fits"] for w in some) and any(w["case"]["capacity"] < 0 and not w["fits"] for w in some)
    big = W.bound((1 << 22) - 1, 1024)
    sizes = {b for w in roots for b in w["case"]["pairs"][0::2]}
    assert sizes >= {0, 1, 255, 256, 257, GIB, GIB + 1, big} and any(2.7e9 < b < 2.8e9 for b in sizes)
    assert any(w["case"]["rank"] != w["case"]["root"] for w in lay)

    # ---- pieces: an image is covered exactly once, in order, by pieces of at most 1 GiB - and by no more than needed
    assert {w["bytes"] for w in want["pieces"]} >= {0, 1, 255, 256, 257, GIB, GIB + 1, big}
    for w in want["pieces"]:
        at = 0
        for off, n in w["pieces"]:
            assert off == at and 0 < n <= GIB
            at += n
        assert at == w["bytes"] and len(w["pieces"]) == -(-w["bytes"] // GIB)
    assert any(len(w["pieces"]) == 3 and 2.7e9 < w["bytes"] < 2.8e9 for w in want["pieces"])

    # ---- the staging block of emspec_batch_gather: samples, index, dB, the root's gathered block, 256 spare bytes
    for w in want["stage"]:
        blocks = [(w["pcm"], w["S"] * w["L"] * 4), (w["idx"], w["cells"])]
        assert (w["db_off"] >= 0) == bool(w["db"]) and (w["all"] >= 0) == bool(w["is_root"])
        if w["db"]:
            blocks.append((w["db_off"], w["cells"] * 4))
        if w["is_root"]:
            blocks.append((w["all"], w["cells"] * w["world"]))
        at = 0
        for off, n in blocks:
            assert off == at and off % 256 == 0
            at += al(n)
        assert w["bytes"] == at + 256
    assert {(w["db"], w["is_root"]) for w in want["stage"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}

    # ---- the header checks
    for w in want["headers"]:
        _check_damaged(w["damaged"], w["columns"], w["rows"], w["payload"], w["bytes"])
    assert any(w["payload"] % 16 for w in want["headers"]) and any(w["payload"] % 16 == 0 for w in want["headers"])


def test_recorded_plans_are_the_earlier_arithmetic(drivers):
    """The fixture is, byte for byte, what the arithmetic from before the header prints (the generator command of the module's
    docstring): its provenance can be checked, and it cannot drift with the library's header."""
    assert _run(drivers["verbatim"]) == open(FIXTURE).read()


def test_host_expand_and_header_checks_on_packed_images(drivers, tmp_path):
    """Images packed by oracle/wire_ref.py (the shapes of test_gather.py::test_wire_ref_round_trip, and one with a column of all
    zeros beside a dense one): the header's host expand reproduces the columns, and the header predicate and the two length
    rules answer to every damaged form of every image what the verbatim code answers and what the format's rules say."""
    rng = np.random.default_rng(20)
    images = []
    for columns, rows, density in [(1, 64, 0.5), (7, 68, 0.3), (300, 256, 0.07), (1025, 1024, 0.06), (5000, 1024, 0.0),
                                   (40, 1024, 1.0), (3, 4096, 0.2), (2049, 100, 0.5)]:
        images.append(((rng.random((columns, rows)) < density) * rng.integers(1, 256, (columns, rows))).astype(np.uint8))
    mixed = images[1][:3].copy()
    mixed[1] = 0
    mixed[2] = rng.integers(1, 256, mixed.shape[1])
    images.append(mixed)
    lines = []
    for i, idx in enumerate(images):
        W.pack(idx).tofile(tmp_path / f"image{i}.bin")
        lines.append(f"{tmp_path / f'image{i}.bin'} {idx.shape[0]} {idx.shape[1]} {tmp_path / f'out{i}.bin'}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    text = _run(drivers["lib"], "images", tmp_path / "list.txt")
    got = json.loads(text)["images"]
    assert len(got) == len(images)
    for i, (idx, g) in enumerate(zip(images, got)):
        assert g["rc"] == 0 and np.array_equal(np.fromfile(tmp_path / f"out{i}.bin", np.uint8).reshape(idx.shape), idx)
        assert (g["columns"], g["rows"], g["payload"]) == (*idx.shape, int((idx != 0).sum()))
        _check_damaged(g["damaged"], g["columns"], g["rows"], g["payload"], g["bytes"])
    assert _run(drivers["verbatim"], "images", tmp_path / "list.txt") == text
