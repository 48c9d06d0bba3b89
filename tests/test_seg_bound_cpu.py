"""CPU: the longest segment the fused kernels' planner returns (em-spec_amd/csrc/emspec_seg_plan.h) stays inside what
fused4096_pp_kernel's 32-bit column bookkeeping relies on.  The kernel counts half-iterations and remaining samples in int,
relative to its segment's first frame; the launcher refuses a plan whose walk - (seglen + 2D + 5) hop samples - exceeds
kFusedPpMaxWalk = 2^30 (fused_pp_walk_ok).  tests/cdriver/seg_bound_driver.cpp, a stand-alone program built here with the host
compiler under ASan and UBSan (nothing is preloaded), checks

 - every plan of a sweep against the bound the header states for the planner, fused_seglen_max (and that it fits an int), and
 - that on a 256-CU device no batch of up to 2^36 samples - 256 GiB of float32, more than the device holds - gets a plan the
   launcher would refuse for its walk, at hop 256 / 512 / 1024.

The margin is asserted too: the largest walk of the second sweep is at most 2^28 samples (a whole stream as one segment when
the batch has more streams than four rounds of CUs hold: 2^36 / 256), a quarter of the bound."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_segments_stay_inside_the_int_walk(tmp_path):
    exe = str(tmp_path / "seg_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "em-spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cdriver", "seg_bound_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert words[0] == "plans" and words[2] == "max_walk"
    print(f"MEASURED {r.stdout.strip()}")
    assert int(words[1]) > 10000
    assert 0 < int(words[3]) <= (1 << 28) + (2 * 8 + 5 + 2) * 1024
