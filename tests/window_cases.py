"""The device cases of the window walk, shared by tests/test_gpu_wave.py and tests/test_gpu_level.py: the
envelope, the level and the cross kernels are one walk with three reducers, so both suites run it on the same paths - every
team size from one lane (hop 1) to 64 (hop = n = 4096) and the split into pieces over workgroups."""
import wave_ref as W

PATHS = {1, 2, 4, 8, 16, 32, 64, "split"}
# beside the references' shared cases: teams of 2 and 4 lanes (windows of 32 and 64 samples) and one of 32 lanes
DEVICE_CASES = W.CASES + [(256, 32, 4099, 1), (256, 32, 4099, 2), (512, 512, 5001, 2)]
# windows of 76,800 samples (two pieces each) in front of a last one of 2,560, shorter than the split
SPLIT_CASES = [(1024, 256, 1024 + 256 * 609 + 3, 300), (1024, 256, 1024 + 256 * 609 + 3, 65536)]
IDS = dict(ids=lambda c: "n%d-hop%d-L%d-f%d" % c)

# with more than one rule broken every entry reports the same one: the pair's rules (cross), then streams, length, FFT size, hop, factor
PRECEDENCE = [((-1, 1000, 300, 100, 1), "streams"), ((2, -1, 300, 100, 1), "length"), ((2, -1, 256, 0, 1), "length"),
              ((2, 1000, 300, 0, 1), "fft size"), ((2, 1000, 300, 100, 0), "fft size"), ((2, 1000, 256, 0, 0), "hop")]

def _team(n, hop, L, f):
    """The path a launch takes: its team size (emspec_window_plan.h: window_team), or "split" """
    longest = min(f, W.num_columns(L, n, hop)) * hop
    if longest > 16384:
        return "split"
    T = 1
    while T < 64 and T * 32 <= longest:
        T *= 2
    return T
