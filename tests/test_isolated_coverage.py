"""
CPU test that ties the isolated layer checks to the call planner: every (layer, form) launch the default rules produce on 256 CUs
for a 1024^2 call of 1 ... 64 frames has an isolated fp64 check that runs it. Layers up to 128^2: the case table of
tests/isolated_small_cases.py (tests/test_isolated_small_layers_gpu.py, on a 128^2 network, which plans those layers identically).
Layers from 256^2 up: the batches of tests/test_isolated_layers_gpu.py. A planner change that produces a new production form fails
here, without a device, until an isolated check reaches it. gance_engine_describe_plan shares plan_call and the name-building code
with the launch loop (tests/test_engine_plan.py).
"""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import isolated_small_cases as cases
from gance_amd import hip_lib

BATCHES = list(range(1, 65))

# The knobs are read once per process: both networks are described in one fresh child with every GANCE_TUNE_* variable stripped.
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
num_cus, max_batch = int(sys.argv[2]), int(sys.argv[3])
out = ctypes.create_string_buffer(1 << 16)
plans = {}
for resolution in json.loads(sys.argv[4]):
    config = (ctypes.c_int32 * 4)(resolution, max_batch, 0, 0)  # gance_engine_config: resolution, max_batch, device, flags (default)
    plans[resolution] = {}
    for batch in range(1, max_batch + 1):
        status = lib.gance_engine_describe_plan(config, ctypes.c_int32(num_cus), ctypes.c_int32(batch), out, ctypes.c_uint64(len(out)))
        assert status == 0, status
        plans[resolution][batch] = out.value.decode().split()
print(json.dumps(plans))
"""


@pytest.fixture(scope="module")
def plans() -> dict:
    """{resolution: {batch: {layer_idx: conv launch name}}} for the 1024^2 and 128^2 networks, default flags, 256 CUs, 1 ... 64 frames."""
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    env = {key: value for key, value in os.environ.items() if not key.startswith("GANCE_TUNE_")}
    child = subprocess.run(
        [sys.executable, "-c", _CHILD, str(hip_lib.LIBRARY_PATH), str(cases.NUM_CUS), str(BATCHES[-1]), json.dumps([1024, 128])],
        check=True, env=env, capture_output=True, text=True, timeout=120,
    )
    return {
        int(resolution): {int(batch): cases.conv_launches(names) for batch, names in by_batch.items()}
        for resolution, by_batch in json.loads(child.stdout).items()
    }


def _reached(by_batch: dict, table) -> set:
    """{(layer_idx, launch name)} that checking the table's layers at the table's batches runs."""
    return {(idx, by_batch[batch][idx]) for batch, layers in table for idx in layers}


def test_the_case_table_is_well_formed() -> None:
    batches = [batch for batch, _ in cases.CASES]
    assert batches == sorted(set(batches)) and batches[0] == 1 and batches[-1] == BATCHES[-1]
    assert sorted(cases.FORMS) == list(range(cases.LAST_SMALL_LAYER + 1))
    assert sum(len(forms) for forms in cases.FORMS.values()) == 25
    for idx, forms in cases.FORMS.items():
        firsts = [first for first, _ in forms]
        assert firsts == sorted(set(firsts)) and firsts[0] == 1, idx
        for first, _ in forms:  # every form is checked at the batch that first selects it
            assert idx in cases.layers_at(first), (idx, first)


def test_every_small_layer_form_the_planner_produces_has_an_isolated_case(plans: dict) -> None:
    small = range(cases.LAST_SMALL_LAYER + 1)
    produced = {(idx, plans[1024][batch][idx]) for batch in BATCHES for idx in small}
    reached = _reached(plans[1024], cases.CASES)
    assert produced == reached, f"not reached: {sorted(produced - reached)}"
    # ... and the names the device test asserts on 256 CUs are the planner's, at every batch
    for batch in BATCHES:
        for idx in small:
            assert plans[1024][batch][idx] == cases.expected_name(idx, batch), (batch, idx)
    assert produced == {(idx, name) for idx, forms in cases.FORMS.items() for _, name in forms}


def test_the_128_network_plans_the_small_layers_like_the_1024_network(plans: dict) -> None:
    for batch, _ in cases.CASES:
        assert sorted(plans[128][batch]) == list(range(cases.LAST_SMALL_LAYER + 1))
        for idx, name in plans[128][batch].items():
            assert name == plans[1024][batch][idx], (batch, idx)


def test_every_large_layer_form_the_planner_produces_is_run_by_the_isolated_layer_test(plans: dict) -> None:
    large = [idx for idx in plans[1024][1] if idx > cases.LAST_SMALL_LAYER]
    assert large == list(range(cases.LAST_SMALL_LAYER + 1, 17))
    produced = {(idx, plans[1024][batch][idx]) for batch in BATCHES for idx in large}
    reached = _reached(plans[1024], [(batch, large) for batch in cases.LARGE_LAYER_BATCHES])
    assert produced == reached, f"not reached: {sorted(produced - reached)}"
