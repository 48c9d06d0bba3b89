"""CPU: the case table of the stream-order suite (tests/stream_order.py) covers every device entry.

Every function of include/emspec.h with a hip_stream parameter, and every method of emspec.Engine with a `stream` parameter, is a
row of CASES or is excluded with a reason: a device entry added later without a stream-order case fails here, without a GPU.
And every row proves something: the references of the decoy and of the real input differ by more than the comparison allows, in
every output, so an entry that ran on the decoy cannot pass."""
import inspect
import os
import re

import numpy as np
import pytest

import emspec
import stream_order as SO
from test_gpu_route import EXACT, FAST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_entries():
    text = open(os.path.join(ROOT, "include", "emspec.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(emspec_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S) if "hip_stream" in m.group(2)}


def test_every_entry_with_a_hip_stream_is_a_case_or_excluded_with_a_reason():
    entries = _header_entries()
    assert len(entries) == 19 and "emspec_batch_device" in entries and "emspec_gather_columns" in entries, sorted(entries)
    covered = {c.entry for c in SO.CASES}
    assert not covered & set(SO.EXCLUDED_ENTRIES), "an entry is a case and excluded"
    assert all(len(r) > 20 for r in SO.EXCLUDED_ENTRIES.values())
    missing = entries - covered - set(SO.EXCLUDED_ENTRIES)
    assert not missing, f"device entries without a stream-order case (tests/stream_order.py: CASES): {sorted(missing)}"
    assert covered | set(SO.EXCLUDED_ENTRIES) <= entries, "a case names an entry the header does not have"


def test_every_engine_method_with_a_stream_is_a_case_or_excluded_with_a_reason():
    methods = {name for name, f in inspect.getmembers(emspec.Engine, inspect.isfunction)
               if "stream" in inspect.signature(f).parameters} - SO.NOT_A_HIP_STREAM
    covered = {c.method for c in SO.CASES}
    missing = methods - covered - set(SO.EXCLUDED_METHODS)
    assert not missing, f"Engine methods with a stream argument and no stream-order case: {sorted(missing)}"
    assert covered <= methods, sorted(covered - methods)
    # (what is set aside takes a live stream's NUMBER)
    for name in SO.NOT_A_HIP_STREAM:
        assert "cuda_stream" not in inspect.getsource(getattr(emspec.Engine, name))


def test_the_rows_the_table_must_have():
    ids = [c.id for c in SO.CASES]
    assert len(set(ids)) == len(ids)
    assert {c.kind for c in SO.CASES} == {"input", "view", "order"}
    batch = [c for c in SO.INPUT_CASES if c.entry == "emspec_batch_device"]
    assert len([c for c in batch if c.engine[0] == "fast"]) == len(FAST) and len(batch) == len(FAST) + len(EXACT) + 3
    assert {c.id for c in batch} >= {"batch_device-time-reduce-3", "batch_device-display-on", "batch_device-null-stream"}
    assert [c.id for c in SO.CASES if c.null] == ["batch_device-null-stream"]
    for kind in ("wave", "level", "cross"):
        assert {c.id for c in SO.CASES if c.entry == f"emspec_{kind}_device"} == {f"{kind}_device-team", f"{kind}_device-split"}
    assert [c.id for c in SO.CASES if c.kind == "order"] == ["batch_device-exact-scratch-two-streams", "batch_device-exact-scratch-regrow",
                                                             "batch_device-caller-ordered-records", "audio_batch_device-caller-ordered"]
    assert {c.method for c in SO.VIEW_CASES} == {"history_view_device", "history_view_stereo_device", "audio_view_device",
                                                 "audio_batch_device"}
    for c in SO.CASES:
        assert c.shape and c.ref and (not c.blocks or len(c.reason) > 20), c.id
    # EXACT wherever the entry has the mode: FAST only for the FAST routes and the FAST-only parity dump
    assert {c.id for c in SO.CASES if c.engine[0] == "fast"} == ({c.id for c in batch if "-fast-" in c.id}
                                                                 | {"parity_dump_device", "batch_device-caller-ordered-records"})
    assert [c.id for c in SO.CASES if c.blocks] == ["wire_unpack", "batch_device-exact-scratch-regrow"]


@pytest.mark.parametrize("case", SO.INPUT_CASES, ids=repr)
def test_the_decoy_cannot_pass(case):
    real, decoy = case.inputs("real"), case.inputs("decoy")
    assert real.shape == decoy.shape and real.dtype == decoy.dtype and not np.array_equal(SO._bytes(real), SO._bytes(decoy))
    want, other = case.reference(real), case.reference(decoy)
    assert set(want) == set(case.outputs)
    for k, (dtype, shape) in case.outputs.items():
        if case.mismatch is SO.prefix_mismatch:              # (an image at the head of a destination of wire_bound bytes)
            assert want[k].ndim == 1 and 0 < want[k].size <= shape[0]
        else:
            assert want[k].shape == tuple(shape), (k, want[k].shape, shape)
        assert want[k].dtype == np.dtype(dtype) or case.id == "batch_device-display-on", (k, want[k].dtype)   # (a binary64 reference)
    assert case.mismatch(want, want) == {}
    got = {k: np.asarray(v).astype(case.outputs[k][0]) for k, v in other.items()}
    assert set(case.mismatch(got, want)) == set(case.outputs), "an output of the decoy passes for the real input's"
    # ... and neither does the poison
    poison = {k: np.full(np.prod(shape) * np.dtype(dtype).itemsize, SO.POISON, np.uint8).view(dtype).reshape(shape)
              for k, (dtype, shape) in case.outputs.items()}
    assert set(case.mismatch(poison, want)) == set(case.outputs)


def test_delay_rule():
    assert SO.delay_ms_for(0.0001, "a short step") == 50.0 and SO.delay_ms_for(0.01, "a 10 ms step") == 200.0
    with pytest.raises(AssertionError):
        SO.delay_ms_for(0.026, "a step too long for the cap")
