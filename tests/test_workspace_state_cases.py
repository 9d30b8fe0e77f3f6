"""
CPU test of tests/workspace_state_cases.py: the launch names tests/test_workspace_state_gpu.py demands of every call it makes are the
ones the call planner gives on 256 CUs (gance_engine_describe_plan, from a child without GANCE_TUNE_* knobs, as
tests/test_isolated_coverage.py asks it), the calls reach every (layer, form) and every image form of the three case tables that
their networks hold, and the border geometry restated there counts what a brute-force walk over a plane counts.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import isolated_config_e_cases as e_cases
import isolated_image_cases as image_cases
import isolated_small_cases as small_cases
import workspace_state_cases as cases
from gance_amd import hip_lib
from test_isolated_coverage import _CHILD

FLAGS = {"f": 0, "e": hip_lib.GANCE_FLAG_FMAP_BASE_8K}


@pytest.fixture(scope="module")
def plans() -> dict:
    """{network: {batch: [launch names]}} of every network of the table, 256 CUs, 1 ... 64 frames."""
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    env = {key: value for key, value in os.environ.items() if not key.startswith("GANCE_TUNE_")}
    wanted = [[network.resolution, FLAGS[network.config]] for network in cases.NETWORKS.values()]
    child = subprocess.run(
        [sys.executable, "-c", _CHILD, str(hip_lib.LIBRARY_PATH), str(cases.NUM_CUS), "64", json.dumps(wanted)],
        check=True, env=env, capture_output=True, text=True, timeout=120,
    )
    by_key = json.loads(child.stdout)
    return {
        name: {int(batch): names for batch, names in by_key[f"{network.resolution}/{FLAGS[network.config]}"].items()}
        for name, network in cases.NETWORKS.items()
    }


def test_the_demanded_names_are_the_planners(plans: dict) -> None:
    for name, network in cases.NETWORKS.items():
        assert set(network.history_batches) <= set(network.batches) and max(network.batches) <= network.max_batch, name
        for batch in network.batches:
            assert cases.name_misses(network.config, network.resolution, batch, plans[name][batch]) == [], (name, batch)
    # ... and the check can fail: another batch's names miss wherever a form changes with the batch
    assert cases.name_misses("f", 128, 1, plans["f-128"][64]) and cases.name_misses("e", 256, 17, plans["e-256"][18])
    assert cases.name_misses("f", 1024, 2, plans["f-1024"][2][:-3])


def test_the_calls_reach_every_form_of_the_three_tables(plans: dict) -> None:
    reached = {config: set() for config in FLAGS}
    for name, network in cases.NETWORKS.items():
        for batch in network.batches:
            reached[network.config] |= set(plans[name][batch])
    for idx, forms in small_cases.FORMS.items():
        for _, launch in forms:
            assert launch in reached["f"], launch
    assert set(small_cases.LARGE_NOISE_FORMS["auto"].values()) <= reached["f"]
    for forms in image_cases.FORMS.values():
        for _, launch, _ in forms:
            assert launch is None or launch in reached["f"], launch
    for idx, forms in e_cases.FORMS.items():
        for _, launch in forms:
            assert launch in reached["e"], launch
    for forms in e_cases.IMAGE_FORMS.values():
        for _, launch, _ in forms:
            assert launch is None or launch in reached["e"], launch


def test_the_call_order_visits_every_batch_twice() -> None:
    for network in cases.NETWORKS.values():
        order = cases.call_order(network.batches)
        half = len(network.batches)
        assert sorted(order[:half]) == sorted(network.batches) and order[half:] == sorted(network.batches, reverse=True)
        assert order == cases.call_order(network.batches)
    assert cases.call_order(cases.NETWORKS["f-128"].batches)[:10] != sorted(cases.NETWORKS["f-128"].batches)
    assert len(cases.FORCED_FORMS) == len(set(cases.FORCED_FORMS)) == 11 and ("auto", "auto") not in cases.FORCED_FORMS


@pytest.mark.parametrize("side", [4, 8, 32])
def test_the_border_counts_are_those_of_a_walk_over_the_plane(side: int) -> None:
    plane = np.ones((side + 2, side + 8), dtype=bool)
    plane[1:side + 1, 4:side + 4] = False
    assert cases.act_border_words(side) == int(plane.sum())
    for py in (0, 1):
        for px in (0, 1):
            plane = np.ones((side + 3, side + 8), dtype=bool)
            # class (py, px) holds T[2y' + py][2x' + px] of the (2 side + 1)^2 transposed-conv result at [y' + 1][x' + 4]
            for y in range(py, 2 * side + 1, 2):
                for x in range(px, 2 * side + 1, 2):
                    plane[y // 2 + 1, x // 2 + 4] = False
            assert cases.parity_border_words(side, py, px) == int(plane.sum()), (py, px)
