"""
CPU test that ties the isolated layer checks to the call planner: every (layer, form) launch the default rules produce on 256 CUs
for a 1024^2 call of 1 ... 64 frames has an isolated fp64 check that runs it. Layers up to 128^2: the case table of
tests/isolated_small_cases.py (tests/test_isolated_small_layers_gpu.py, on a 128^2 network, which plans those layers identically).
Layers from 256^2 up: the batches of tests/test_isolated_layers_gpu.py. A planner change that produces a new production form fails
here, without a device, until an isolated check reaches it. gance_engine_describe_plan shares plan_call and the name-building code
with the launch loop (tests/test_engine_plan.py).

The image branch (ToRGB, skip image, bytes) is tied in the same way: every (ToRGB launch, "+rgb" on the conv in front of it) form the
planner produces at any resolution, for both networks, and the two more of conv_form="direct", is reached by the case table of
tests/isolated_image_cases.py (tests/test_isolated_image_gpu.py).

The checks with a noise plane per sample (tests/test_isolated_noise_gpu.py) have a table of their own, NOISE_CASES, derived from FORMS:
every (layer, form) once, at the last batch of its range. It is held here to the table it must come out as and to the planner, and
the calls of the 256^2 ... 1024^2 layers to every form those layers take over 2 ... 64 frames.

Config-e generators (GANCE_FLAG_FMAP_BASE_8K) are tied in the same way, from the same child: layers 0 ... 6 of a config-e call have
the launch names of the config-f call at every batch, so the config-f checks stand for them; the 27 (layer, form) launches of layers
7 ... 16 and the nine image forms at 64^2 ... 512^2 are the tables of tests/isolated_config_e_cases.py, reached by
tests/test_isolated_config_e_gpu.py (layers 7 ... 12, 256^2 network) and by ISOLATED of tests/test_config_e_gpu.py (layers 13 ... 16).
"""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import isolated_config_e_cases as e_cases
import isolated_image_cases as image_cases
import isolated_small_cases as cases
from gance_amd import hip_lib

BATCHES = list(range(1, 65))
CONFIG_E = hip_lib.GANCE_FLAG_FMAP_BASE_8K

# The knobs are read once per process: both networks are described in one fresh child with every GANCE_TUNE_* variable stripped.
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
num_cus, max_batch = int(sys.argv[2]), int(sys.argv[3])
out = ctypes.create_string_buffer(1 << 16)
plans = {}
for resolution, flags in json.loads(sys.argv[4]):
    config = (ctypes.c_int32 * 4)(resolution, max_batch, 0, flags)  # gance_engine_config: resolution, max_batch, device, flags
    plans[f"{resolution}/{flags}"] = {}
    for batch in range(1, max_batch + 1):
        status = lib.gance_engine_describe_plan(config, ctypes.c_int32(num_cus), ctypes.c_int32(batch), out, ctypes.c_uint64(len(out)))
        assert status == 0, status
        plans[f"{resolution}/{flags}"][batch] = out.value.decode().split()
print(json.dumps(plans))
"""


@pytest.fixture(scope="module")
def launch_names_by_flags() -> dict:
    """{(resolution, flags): {batch: [launch names]}}, 256 CUs, 1 ... 64 frames: config-f, the 1024^2 and 128^2 networks with default
    flags and the 1024^2 one with conv_form="direct"; config-e, the 1024^2 and 256^2 networks with default flags."""
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    env = {key: value for key, value in os.environ.items() if not key.startswith("GANCE_TUNE_")}
    child = subprocess.run(
        [sys.executable, "-c", _CHILD, str(hip_lib.LIBRARY_PATH), str(cases.NUM_CUS), str(BATCHES[-1]),
         json.dumps([[1024, 0], [128, 0], [1024, hip_lib.GANCE_FLAG_DIRECT_CONV], [1024, CONFIG_E], [256, CONFIG_E]])],
        check=True, env=env, capture_output=True, text=True, timeout=120,
    )
    return {
        tuple(int(part) for part in key.split("/")): {int(batch): names for batch, names in by_batch.items()}
        for key, by_batch in json.loads(child.stdout).items()
    }


@pytest.fixture(scope="module")
def launch_names(launch_names_by_flags: dict) -> dict:
    """{(resolution, conv_form): {batch: [launch names]}} of the config-f networks: the 1024^2 and 128^2 ones with default flags and
    the 1024^2 one with conv_form="direct"."""
    forms = {0: "auto", hip_lib.GANCE_FLAG_DIRECT_CONV: "direct"}
    return {(resolution, forms[flags]): by_batch for (resolution, flags), by_batch in launch_names_by_flags.items() if flags in forms}


@pytest.fixture(scope="module")
def config_e_plans(launch_names_by_flags: dict) -> dict:
    """{resolution: {batch: {layer_idx: conv launch name}}} for the config-e 1024^2 and 256^2 networks, default flags."""
    return {
        resolution: {batch: cases.conv_launches(names) for batch, names in by_batch.items()}
        for (resolution, flags), by_batch in launch_names_by_flags.items() if flags == CONFIG_E
    }


@pytest.fixture(scope="module")
def plans(launch_names: dict) -> dict:
    """{resolution: {batch: {layer_idx: conv launch name}}} for the 1024^2 and 128^2 networks, default flags, 256 CUs, 1 ... 64 frames."""
    return {
        resolution: {batch: cases.conv_launches(names) for batch, names in by_batch.items()}
        for (resolution, conv_form), by_batch in launch_names.items() if conv_form == "auto"
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


def test_the_noise_case_table_is_the_one_derived_from_the_forms() -> None:
    assert cases.NOISE_CASES == [
        (1, [3, 10]), (2, [9]), (3, [4, 8, 9]), (5, [5]), (7, [1, 7]), (8, [7]), (15, [2, 6, 7]), (17, [5]), (64, list(range(11))),
    ]
    assert cases.LARGE_NOISE_CASES == [("auto", 9), ("direct", 2)]  # (("auto", 3) was dropped for its time)


def test_the_noise_cases_visit_every_small_layer_form_once_at_the_last_batch_of_its_range(plans: dict) -> None:
    visits = [(idx, cases.expected_name(idx, batch), batch) for batch, layers in cases.NOISE_CASES for idx in layers]
    forms = [(idx, name) for idx, by_first in cases.FORMS.items() for _, name in by_first]
    assert sorted((idx, name) for idx, name, _ in visits) == sorted(forms)  # each exactly once
    for idx, name, batch in visits:
        # the planner's name at that batch is the expected one, on both networks ...
        assert plans[1024][batch][idx] == name and plans[128][batch][idx] == name, (idx, batch)
        # ... and the batch is the last that selects the form: no larger call does
        assert batch <= cases.MAX_BATCH == BATCHES[-1] and all(plans[1024][b][idx] != name for b in BATCHES if b > batch), (idx, batch)


def test_the_large_noise_batches_reach_every_form_of_two_to_64_frames(launch_names: dict) -> None:
    large = list(range(cases.LAST_SMALL_LAYER + 1, 17))
    for conv_form, forms in cases.LARGE_NOISE_FORMS.items():
        by_batch = {batch: cases.conv_launches(names) for batch, names in launch_names[(1024, conv_form)].items()}
        produced = {(idx, by_batch[batch][idx]) for batch in BATCHES[1:] for idx in large}
        assert produced == set(forms.items())  # one form each over 2 ... 64 frames: the names the device test asserts on 256 CUs
        for case_form, batch in cases.LARGE_NOISE_CASES:
            if case_form == conv_form:
                assert batch >= 2 and {(idx, by_batch[batch][idx]) for idx in large} == produced, (conv_form, batch)
    assert sorted({form for form, _ in cases.LARGE_NOISE_CASES}) == sorted(cases.LARGE_NOISE_FORMS)


def test_the_oracle_layer_for_another_plane_follows_from_its_result() -> None:
    """with_other_plane of tests/test_isolated_noise_gpu.py (the sensitivity condition there) against a second call of the oracle layer."""
    import numpy as np  # pylint: disable=import-outside-toplevel
    import torch  # pylint: disable=import-outside-toplevel

    import test_isolated_noise_gpu as noise_checks  # pylint: disable=import-outside-toplevel
    from gance_amd.stylegan2 import spec as sg2_spec  # pylint: disable=import-outside-toplevel
    from oracle import stylegan2_ref as ref  # pylint: disable=import-outside-toplevel

    resolution = 8
    spec = sg2_spec.make_spec(resolution)
    variables = dict(sg2_spec.make_random_variables(resolution, seed=3, perturb=True))
    rng = np.random.RandomState(0)
    w = torch.from_numpy(rng.randn(1, spec.num_layers, 512))
    x = torch.from_numpy(np.asarray(variables["G_synthesis/4x4/Const/const"], dtype=np.float64))
    for conv in spec.convs:  # 4x4 Conv, 8x8 Conv0_up, 8x8 Conv1
        strength = 0.5 * (-1) ** conv.layer_idx
        variables[f"G_synthesis/{conv.scope}/noise_strength"] = np.float32(strength)
        side = 2 ** conv.res_log2
        own, other = rng.randn(2, side, side).astype(np.float32)
        stored = np.asarray(variables[f"G_synthesis/noise{conv.layer_idx}"]).reshape(side, side)
        with torch.no_grad():
            want = ref.synthesis_layer(x, w, variables, conv, noise_override={conv.layer_idx: torch.from_numpy(own[None, None])})
            for plane, override in ((other, {conv.layer_idx: torch.from_numpy(other[None, None])}), (stored, None)):
                again = ref.synthesis_layer(x, w, variables, conv, noise_override=override).numpy()[0]
                worked_out = noise_checks.with_other_plane(want.numpy()[0], own, plane, strength)
                assert np.abs(again - want.numpy()[0]).max() > 0.1 * np.abs(again).max()  # (the planes matter)
                assert np.abs(worked_out - again).max() < 1e-12 * np.abs(again).max()
        x = want


def test_the_image_case_table_is_well_formed() -> None:
    assert sorted(image_cases.FORMS) == [4, 8, 16, 32, 64, 128, 256, 512, 1024]
    assert sum(len(forms) for forms in image_cases.FORMS.values()) == 12
    assert image_cases.NUM_CUS == cases.NUM_CUS
    for resolution, forms in image_cases.FORMS.items():
        firsts = [first for first, _, _ in forms]
        assert firsts == sorted(set(firsts)) and firsts[0] == 1, resolution
        network = 128 if resolution <= 128 else 1024
        for first, name, partials in forms:  # every form is checked at the batch that first selects it, and ...
            assert any(case[:3] == (network, "auto", first) and resolution in case[3] for case in image_cases.CASES), (resolution, first)
            assert (name is None) == (partials == 0)
        # ... in the last sample of a full call (<= 128^2) or of an odd one (the 1024^2 network)
        assert any(case[:3] == (network, "auto", 64 if network == 128 else 3) and resolution in case[3] for case in image_cases.CASES)
    for network, conv_form, batch, resolutions in image_cases.CASES:
        assert network in (128, 1024) and 1 <= batch <= BATCHES[-1] and all(r <= network for r in resolutions)
        assert conv_form == "auto" or resolutions == sorted(image_cases.DIRECT_FORMS)


def test_every_image_form_the_planner_produces_has_an_isolated_case(launch_names: dict) -> None:
    for key, by_batch in launch_names.items():
        network, conv_form = key
        produced = set()
        for batch in BATCHES:
            launches = image_cases.image_launches(by_batch[batch])
            assert sorted(launches) == [r for r in image_cases.FORMS if r <= network], (key, batch)
            for resolution, (torgb, conv) in launches.items():
                if conv_form == "direct" and resolution <= 128:  # (the small kernel after a plain conv: the one-frame form of the table)
                    assert image_cases.form_of(torgb, conv) == (f"torgb_{resolution}x{resolution}", ""), (key, batch, conv)
                    continue
                produced.add((resolution,) + image_cases.form_of(torgb, conv))
                # the names the device test asserts on 256 CUs are the planner's, at every batch
                name, partials = image_cases.expected_form(resolution, batch, conv_form)
                kind, _, channels = conv.split("_")
                if name is None:
                    assert "+" not in kind and torgb != "", (key, batch, conv)
                else:
                    assert conv == name and (torgb == "") == ("+torgb" in name), (key, batch, conv)
                if "+rgb" in kind:  # (F(4x4,3x3): a block holds 32 output channels of a pixel)
                    assert kind.startswith("convV") and partials == int(channels.split("->")[1]) // 32, (key, batch, conv)
                else:
                    assert partials == 0, (key, batch, conv)
        reached = set()
        for case_network, case_form, batch, resolutions in image_cases.CASES:
            if (case_network, case_form) == key:
                launches = image_cases.image_launches(by_batch[batch])
                reached |= {(resolution,) + image_cases.form_of(*launches[resolution]) for resolution in resolutions}
        if key == (1024, "auto"):  # (its first six resolutions are checked on the 128^2 network, which plans them identically: below)
            small = launch_names[(128, "auto")]
            for batch in BATCHES:
                assert {r: v for r, v in image_cases.image_launches(by_batch[batch]).items() if r <= 128} == image_cases.image_launches(small[batch])
            produced = {form for form in produced if form[0] > 128}
        assert produced == reached, f"{key}: not reached: {sorted(produced - reached)}"


def test_the_default_image_forms_are_the_twelve_of_the_table(launch_names: dict) -> None:
    produced = set()
    for batch in BATCHES:
        for resolution, (torgb, conv) in image_cases.image_launches(launch_names[(1024, "auto")][batch]).items():
            produced.add((resolution, conv if "+rgb" in conv.split("_")[0] else None))
    assert produced == {(resolution, name) for resolution, forms in image_cases.FORMS.items() for _, name, _ in forms}
    direct = {(r, conv if "+" in conv.split("_")[0] else None)
              for batch in BATCHES for r, (_, conv) in image_cases.image_launches(launch_names[(1024, "direct")][batch]).items() if r > 128}
    assert direct == set(image_cases.DIRECT_FORMS.items())


# ---- config-e generators ----


def _in_ranges(batch: int, ranges) -> bool:
    return any(first <= batch <= last for first, last in ranges)


def test_the_config_e_case_table_is_well_formed() -> None:
    assert e_cases.NUM_CUS == cases.NUM_CUS and e_cases.MAX_BATCH == BATCHES[-1]
    assert sorted(e_cases.FORMS) == list(range(e_cases.FIRST_LAYER, e_cases.LAST_LAYER + 1)) == e_cases.SMALL_LAYERS + e_cases.LARGE_LAYERS
    assert sum(len(forms) for forms in e_cases.FORMS.values()) == 27
    batches = [batch for batch, _ in e_cases.CASES]
    assert batches == sorted(set(batches)) and batches[0] == 1 and batches[-1] == BATCHES[-1]
    assert e_cases.layers_at(1) == e_cases.layers_at(BATCHES[-1]) == e_cases.SMALL_LAYERS  # all of layers 7 ... 12 at 1 and at 64 frames
    for idx, forms in e_cases.FORMS.items():
        for batch in BATCHES:  # the ranges of a layer's forms partition 1 ... 64
            assert sum(_in_ranges(batch, ranges) for ranges, _ in forms) == 1, (idx, batch)
        for form, (ranges, _) in enumerate(forms):
            assert ranges == sorted(ranges) and all(first <= last for first, last in ranges), (idx, form)
            first = e_cases.first_batch(idx, form)  # every form is checked at the first batch of its range
            table = e_cases.CASES if idx in e_cases.SMALL_LAYERS else e_cases.LARGE_CASES
            assert idx in dict(table).get(first, []), (idx, first)
    assert [batch for batch, _ in e_cases.LARGE_CASES] == list(e_cases.LARGE_LAYER_BATCHES)


def test_the_large_config_e_cases_are_the_rows_of_the_device_test() -> None:
    """LARGE_CASES against ISOLATED of tests/test_config_e_gpu.py: the auto / auto rows (batch 0 there: the smallest batch with the
    fused 32 -> 16 up layer, 2 on 256 CUs), and the layers that test leaves out at 17 frames."""
    import test_config_e_gpu as device_test  # pylint: disable=import-outside-toplevel

    assert device_test.UP_16 == e_cases.expected_name(15, 2) != e_cases.expected_name(15, 1)
    batches = sorted({batch or 2 for _, conv_form, up_form, batch in device_test.ISOLATED if (conv_form, up_form) == ("auto", "auto")})
    assert batches == list(e_cases.LARGE_LAYER_BATCHES)
    for network in ("every_term", "loud"):
        assert (network, "auto", "auto", device_test.PAIR_FORM_BATCH) in device_test.ISOLATED
    for batch, layers in e_cases.LARGE_CASES:
        last = device_test.PAIR_FORM_LAST_LAYER if batch == device_test.PAIR_FORM_BATCH else 17
        assert layers == list(range(device_test.FIRST_LAYER - 1, last)), batch  # (conv layers 14 ... last, 1-based, as layer_idx)
    assert device_test.UP_32_PAIR_FORM == e_cases.expected_name(13, device_test.PAIR_FORM_BATCH)


def test_the_first_seven_config_e_layers_are_planned_like_the_config_f_ones(plans: dict, config_e_plans: dict) -> None:
    for resolution in (1024, 256):
        for batch in BATCHES:
            for idx in range(e_cases.FIRST_LAYER):
                assert config_e_plans[resolution][batch][idx] == plans[1024][batch][idx] == cases.expected_name(idx, batch), (resolution, batch, idx)


def test_every_config_e_layer_form_the_planner_produces_has_an_isolated_case(config_e_plans: dict) -> None:
    by_batch = config_e_plans[1024]
    assert sorted(by_batch[1]) == list(range(e_cases.LAST_LAYER + 1))
    produced = {(idx, by_batch[batch][idx]) for batch in BATCHES for idx in e_cases.FORMS}
    assert produced == {(idx, name) for idx, forms in e_cases.FORMS.items() for _, name in forms}
    assert len(produced) == 27
    # the names the device tests assert on 256 CUs are the planner's, at every batch
    for batch in BATCHES:
        for idx in e_cases.FORMS:
            assert by_batch[batch][idx] == e_cases.expected_name(idx, batch), (batch, idx)
    # layers 7 ... 12 through the table, layers 13 ... 16 through the batches of the 1024^2 device test
    reached = _reached(by_batch, e_cases.CASES) | _reached(by_batch, e_cases.LARGE_CASES)
    assert produced == reached, f"not reached: {sorted(produced - reached)}"
    assert {idx for idx, _ in _reached(by_batch, e_cases.CASES)} == set(e_cases.SMALL_LAYERS)
    assert {idx for idx, _ in _reached(by_batch, e_cases.LARGE_CASES)} == set(e_cases.LARGE_LAYERS)


def test_the_256_config_e_network_plans_layers_7_to_12_like_the_1024_one(config_e_plans: dict) -> None:
    for batch in sorted({batch for batch, _ in e_cases.CASES + e_cases.NOISE_CASES}):
        assert sorted(config_e_plans[256][batch]) == list(range(e_cases.LAST_SMALL_LAYER + 1))
        for idx in e_cases.SMALL_LAYERS:
            assert config_e_plans[256][batch][idx] == config_e_plans[1024][batch][idx], (batch, idx)


def test_the_config_e_noise_cases_visit_every_form_once_at_the_last_batch_of_its_range(config_e_plans: dict) -> None:
    assert e_cases.NOISE_CASES == [
        (1, [10, 12]), (2, [10, 11]), (3, [10]), (4, [8, 9]), (5, [8, 9]), (7, [8]), (15, [7]), (17, [7, 9, 11]), (64, e_cases.SMALL_LAYERS),
    ]
    visits = [(idx, e_cases.expected_name(idx, batch), batch) for batch, layers in e_cases.NOISE_CASES for idx in layers]
    forms = [(idx, name) for idx in e_cases.SMALL_LAYERS for _, name in e_cases.FORMS[idx]]
    assert sorted((idx, name) for idx, name, _ in visits) == sorted(forms)  # each exactly once
    for idx, name, batch in visits:
        assert config_e_plans[1024][batch][idx] == name and config_e_plans[256][batch][idx] == name, (idx, batch)
        # no larger call selects the form
        assert batch <= BATCHES[-1] and all(config_e_plans[1024][b][idx] != name for b in BATCHES if b > batch), (idx, batch)


def test_every_config_e_image_form_the_planner_produces_has_an_isolated_case(launch_names_by_flags: dict) -> None:
    checked = sorted(e_cases.IMAGE_FORMS)
    assert checked == [64, 128, 256, 512] and sum(len(forms) for forms in e_cases.IMAGE_FORMS.values()) == 9
    large, small = launch_names_by_flags[(1024, CONFIG_E)], launch_names_by_flags[(256, CONFIG_E)]
    produced = set()
    for batch in BATCHES:
        launches = e_cases.image_launches(large[batch])
        assert sorted(launches) == sorted(image_cases.FORMS), batch
        # up to 32^2 the image launches are the config-f ones; up to 256^2 the 256^2 network's are the 1024^2 network's
        config_f = image_cases.image_launches(launch_names_by_flags[(1024, 0)][batch])
        assert {r: v for r, v in launches.items() if r < 64} == {r: v for r, v in config_f.items() if r < 64}, batch
        assert {r: v for r, v in launches.items() if r <= 256} == e_cases.image_launches(small[batch]), batch
        for resolution in checked:
            torgb, conv = launches[resolution]
            produced.add((resolution,) + e_cases.form_of(torgb, conv))
            # the names the device test asserts on 256 CUs are the planner's, at every batch
            name, partials = e_cases.expected_form(resolution, batch)
            kind, _, channels = conv.split("_")
            assert torgb == f"torgb_{resolution}x{resolution}", (batch, conv)
            if name is None:
                assert "+" not in kind and partials == 0, (batch, conv)
            else:
                assert conv == name and kind.endswith("+rgb"), (batch, conv)
                cout = int(channels.split("->")[1])  # (a block holds 64 output channels of a pixel in F(2x2,3x3), 32 in F(4x4,3x3))
                assert partials == (cout // 64 if kind.startswith("convW") else cout // 32) and kind[:5] in ("convW", "convV"), (batch, conv)
    assert len(produced) == 9
    reached = set()
    for network, batch, resolutions in e_cases.IMAGE_CASES:
        by_batch = {1024: large, 256: small}[network]
        launches = e_cases.image_launches(by_batch[batch])
        assert all(r in checked and r <= network for r in resolutions)
        assert network == 1024 or 512 not in resolutions
        reached |= {(r,) + e_cases.form_of(*launches[r]) for r in resolutions}
    assert produced == reached, f"not reached: {sorted(produced - reached)}"
    for resolution, forms in e_cases.IMAGE_FORMS.items():
        network = 256 if resolution <= 256 else 1024
        for batch in BATCHES:  # the ranges of a resolution's forms partition 1 ... 64
            assert sum(_in_ranges(batch, ranges) for ranges, _, _ in forms) == 1, (resolution, batch)
        for ranges, _, _ in forms:  # every form at the first batch of its range, ...
            assert any(case[:2] == (network, ranges[0][0]) and resolution in case[2] for case in e_cases.IMAGE_CASES), (resolution, ranges)
        # ... in the last sample of an odd call, and (up to 256^2) of a 64-frame call
        assert any(case[0] == network and case[1] % 2 == 1 and case[1] > 1 and resolution in case[2] for case in e_cases.IMAGE_CASES), resolution
        assert network == 1024 or any(case[:2] == (network, BATCHES[-1]) and resolution in case[2] for case in e_cases.IMAGE_CASES), resolution
    # both F(2x2,3x3) launches with the ToRGB sum are reached in the last sample of an odd call
    for network, batch, resolution in ((256, 7, 64), (256, 3, 128)):
        assert e_cases.expected_form(resolution, batch)[0].startswith("convW")
        assert any(case[:2] == (network, batch) and resolution in case[2] for case in e_cases.IMAGE_CASES)
