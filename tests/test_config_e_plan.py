"""
CPU test of the call planner on config-e generators: for every configuration and batch size of
profiles/launch_plan_config_e_256cus.txt -- launch names recorded on an MI355X (256 CUs) by
tools/gpu_form_table.py --fmap-base 8192 --trace from real calls -- gance_engine_describe_plan with GANCE_FLAG_FMAP_BASE_8K returns
exactly those names, in that order. Same format and reader as tests/test_engine_plan.py and its config-f fixture.
"""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import test_engine_plan as plan_helpers
from gance_amd import hip_lib

FIXTURE = plan_helpers.REPO_ROOT / "profiles" / "launch_plan_config_e_256cus.txt"


def _read_fixture():
    saved = plan_helpers.FIXTURE
    plan_helpers.FIXTURE = FIXTURE
    try:
        return plan_helpers._read_fixture()  # pylint: disable=protected-access
    finally:
        plan_helpers.FIXTURE = saved


SECTIONS = _read_fixture()


@pytest.fixture(scope="module")
def library_path() -> Path:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.LIBRARY_PATH


def test_fixture_covers_the_matrix() -> None:
    headers = [header for header, _ in SECTIONS]
    assert len(headers) == len(set(headers))
    for resolution, max_batch in (("1024", 64), ("256", 8), ("64", 8)):
        for conv_form in ("auto", "direct"):
            for up_form in ("auto", "split"):
                assert f"{resolution} {max_batch} {conv_form} {up_form} -" in headers
    for header, plans in SECTIONS:
        assert sorted(plans) == list(range(1, int(header.split()[1]) + 1)), header
        for names in plans.values():  # (config-e channel counts: nothing above 32x32 keeps 512 -> 512)
            assert not [name for name in names if name.endswith("_64x64_512->512")], header


@pytest.mark.parametrize("header,expected", SECTIONS, ids=[header.replace(" ", "_") for header, _ in SECTIONS])
def test_describe_plan_reproduces_the_recorded_launch_names(library_path: Path, header: str, expected: dict) -> None:
    resolution, max_batch, conv_form, up_form, knob = header.split()
    assert knob == "-"
    env = {key: value for key, value in os.environ.items() if not key.startswith("GANCE_TUNE_")}
    flags = plan_helpers.CONV_FLAGS[conv_form] | plan_helpers.UP_FLAGS[up_form] | hip_lib.GANCE_FLAG_FMAP_BASE_8K
    child = subprocess.run(
        [sys.executable, "-c", plan_helpers._CHILD, str(library_path), resolution, max_batch, str(flags), str(plan_helpers.NUM_CUS),  # pylint: disable=protected-access
         json.dumps(sorted(expected))],
        check=True, env=env, capture_output=True, text=True, timeout=120,
    )
    plans = {int(batch): names for batch, names in json.loads(child.stdout).items()}
    for batch, names in expected.items():
        assert plans[batch] == names, f"[{header}] B {batch}"
