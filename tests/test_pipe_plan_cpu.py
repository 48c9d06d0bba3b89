"""CPU: the plan of the host-buffer pipeline (em-spec_amd/csrc/emspec_pipe_plan.h) - how a batch is cut into units, how a unit's
arrays lie in a staging set, which cells of the caller's arrays each unit delivers - is the one recorded in
tests/golden/pipe_plans.json.  That file was written once by the arithmetic as it stood in emspec_host.cpp before host_batch was
reshaped, which tests/cdriver/pipe_plan_verbatim.h keeps unchanged for this purpose:

    g++ -std=c++17 -O1 -fsanitize=address,undefined -DPIPE_PLAN_VERBATIM -I em-spec_amd/csrc \
        tests/cdriver/pipe_plan_driver.cpp -o pipe_plan_verbatim
    ./pipe_plan_verbatim > tests/golden/pipe_plans.json

It is never written by the library's own header (the same command without -DPIPE_PLAN_VERBATIM): a change of the plan's
arithmetic shows up here, without a GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_driver(tmp_path, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *defines,
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "pipe_plan_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def test_pipe_plan_matches_the_recorded_plans(tmp_path):
    """The stand-alone driver, built with the host compiler under ASan and UBSan (a program of its own: nothing is preloaded),
    prints for every case the unit count, every PipeItem, the Stage's sizes and bytes(), where each delivered array lies in a set,
    every Span, and the per-stream staging bytes and delivered bytes that size the units."""
    got = json.loads(_run_driver(tmp_path, "pipe_plan_driver"))
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "pipe_plans.json")))
    assert len(got) == len(want) >= 36
    for g, w in zip(got, want):
        assert g["case"] == w["case"], (g["case"], w["case"])
        for key in w:
            assert g[key] == w[key], (w["case"], key, g[key], w[key])
        assert g["units"] == len(g["items"]) == len(g["spans"])
    # the list reaches every branch: runs of columns and whole streams, one unit, the staging cap, every kind of array
    assert any(len(w["items"]) == 1 for w in want) and any(w["items"][0][3] != w["items"][-1][2] + w["items"][-1][3] for w in want)
    assert any(w["per_stream"] > 1 << 30 for w in want) and any(w["stage"]["peaks"] for w in want)
    assert any(w["stage"]["reduced"] and w["stage"]["wire"] for w in want) and any(w["stage"]["raw"] for w in want)
    assert all(any(w["out_off"][i] > 0 for w in want) for i in range(4))


def test_recorded_plans_are_the_earlier_arithmetic(tmp_path):
    """The fixture is, byte for byte, what the arithmetic from before the reshaping prints (the generator command of the module's
    docstring): its provenance can be checked, and it cannot drift with the library's header."""
    assert _run_driver(tmp_path, "pipe_plan_verbatim", "-DPIPE_PLAN_VERBATIM") == open(os.path.join(ROOT, "tests", "golden", "pipe_plans.json")).read()
