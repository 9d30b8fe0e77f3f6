"""
CPU test of the call planner (gance_amd/csrc/engine_plan.h: plan_call): for every configuration and batch size of
profiles/launch_plan_256cus.txt -- launch names recorded on an MI355X (256 CUs) by tools/gpu_form_table.py --trace from real calls
-- gance_engine_describe_plan returns exactly those names, in that order. The entry shares plan_call and the name-building code
with the launch loop and needs neither a device nor weights.
"""

import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from gance_amd import hip_lib

REPO_ROOT = Path(__file__).resolve().parent.parent
FIXTURE = REPO_ROOT / "profiles" / "launch_plan_256cus.txt"
NUM_CUS = 256

CONV_FLAGS = {
    "auto": 0,
    "direct": hip_lib.GANCE_FLAG_DIRECT_CONV,
    "winograd": hip_lib.GANCE_FLAG_FORCE_WINOGRAD,
    "winograd43": hip_lib.GANCE_FLAG_FORCE_WINOGRAD | hip_lib.GANCE_FLAG_WINOGRAD43,
}
UP_FLAGS = {"auto": 0, "split": hip_lib.GANCE_FLAG_SPLIT_UPFIR, "fused": hip_lib.GANCE_FLAG_FORCE_FUSED_UPFIR}

# The knobs are read once per process, so every configuration is described in a fresh child; ctypes alone keeps that quick.
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
resolution, max_batch, flags, num_cus = (int(v) for v in sys.argv[2:6])
config = (ctypes.c_int32 * 4)(resolution, max_batch, 0, flags)  # gance_engine_config: resolution, max_batch, device, flags
out = ctypes.create_string_buffer(1 << 16)
plans = {}
for batch in json.loads(sys.argv[6]):
    status = lib.gance_engine_describe_plan(config, ctypes.c_int32(num_cus), ctypes.c_int32(batch), out, ctypes.c_uint64(len(out)))
    assert status == 0, status
    plans[batch] = out.value.decode().split()
print(json.dumps(plans))
"""


def _read_fixture():
    """[(header, {batch: [launch names]})] of the committed file."""
    names, sequences, sections = {}, {}, []
    for line in FIXTURE.read_text().splitlines():
        if line.startswith("#") or not line.strip():
            continue
        if line.startswith("N"):
            number, name = line[1:].split()
            names[int(number)] = name
        elif line.startswith("S"):
            tag, steps = line.split(":")
            sequences[tag] = [names[int(step)] for step in steps.split()]
        elif line.startswith("["):
            sections.append((line.strip("[]"), {}))
        else:
            span, tag = line[len("B "):].split(":")
            first, _, last = span.partition("-")
            for batch in range(int(first), int(last or first) + 1):
                sections[-1][1][batch] = sequences[tag.strip()]
    return sections


SECTIONS = _read_fixture()


@pytest.fixture(scope="module")
def library_path() -> Path:
    """The in-tree shared library, built on demand (hipcc cross-compiles without a GPU)."""
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.LIBRARY_PATH


def test_fixture_covers_the_matrix() -> None:
    headers = [header for header, _ in SECTIONS]
    assert len(headers) == len(set(headers)) == 35
    for header, plans in SECTIONS:
        resolution, max_batch, _, _, knob = header.split()
        if knob == "-":
            assert sorted(plans) == list(range(1, int(max_batch) + 1)), header
        elif resolution == "1024":
            assert sorted(plans) == [1, 2, 3, 4, 8, 9, 16, 18, 21, 37, 64], header
        else:
            assert sorted(plans) == [1, 2], header


@pytest.mark.parametrize("header,expected", SECTIONS, ids=[header.replace(" ", "_") for header, _ in SECTIONS])
def test_describe_plan_reproduces_the_recorded_launch_names(library_path: Path, header: str, expected: dict) -> None:
    resolution, max_batch, conv_form, up_form, knob = header.split()
    env = {key: value for key, value in os.environ.items() if not key.startswith("GANCE_TUNE_")}
    if knob != "-":
        name, value = knob.split("=")
        env["GANCE_TUNE_" + name] = value
    flags = CONV_FLAGS[conv_form] | UP_FLAGS[up_form]
    child = subprocess.run(
        [sys.executable, "-c", _CHILD, str(library_path), resolution, max_batch, str(flags), str(NUM_CUS), json.dumps(sorted(expected))],
        check=True, env=env, capture_output=True, text=True, timeout=120,
    )
    plans = {int(batch): names for batch, names in json.loads(child.stdout).items()}
    for batch, names in expected.items():
        assert plans[batch] == names, f"[{header}] B {batch}"


def test_describe_plan_rejects_what_engine_creation_rejects(library_path: Path) -> None:
    lib = ctypes.CDLL(str(library_path))
    out = ctypes.create_string_buffer(1 << 16)
    for resolution, max_batch, batch, capacity in ((1000, 8, 1, len(out)), (256, 8, 9, len(out)), (256, 8, 0, len(out)), (256, 8, 1, 16)):
        config = hip_lib.EngineConfig(resolution, max_batch, 0, 0)
        assert lib.gance_engine_describe_plan(ctypes.byref(config), NUM_CUS, batch, out, ctypes.c_uint64(capacity)) == 1  # GANCE_ERR_INVALID_ARGUMENT
