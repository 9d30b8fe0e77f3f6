"""
CPU tests of config-e support (fmap_base = 8 << 10: the same skip generator with half the feature maps from 64x64 up): the channel
table, the blob sizes on both sides of the C ABI, network files and legacy pickles, and the call planner's answer for every batch
from 1 to 64 under the form flags tests/test_engine_plan.py uses. The launch names recorded from real calls
(profiles/launch_plan_config_e_256cus.txt) are held in tests/test_config_e_plan.py.
"""

import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

import test_engine_plan as plan_helpers
import test_legacy_import as legacy_helpers
from gance_amd import hip_lib, legacy_import, network_file
from gance_amd.stylegan2 import spec as sg2_spec

CONFIG_E = 8 << 10
NUM_CUS = 256

# (output resolution): (Conv0_up cin -> cout, Conv1 cin -> cout, ToRGB cin)
CONFIG_E_TABLE = {
    64: ((512, 256), (256, 256), 256),
    128: ((256, 128), (128, 128), 128),
    256: ((128, 64), (64, 64), 64),
    512: ((64, 32), (32, 32), 32),
    1024: ((32, 16), (16, 16), 16),
}


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


@pytest.mark.parametrize("resolution", [64, 256, 1024])
def test_channel_table(resolution: int) -> None:
    spec = sg2_spec.make_spec(resolution, fmap_base=CONFIG_E)
    assert spec.fmap_base == CONFIG_E and spec.num_layers == sg2_spec.make_spec(resolution).num_layers
    for side, (up, conv1, rgb_cin) in CONFIG_E_TABLE.items():
        if side > resolution:
            continue
        res_log2 = side.bit_length() - 1
        conv0_up, conv = spec.convs[2 * res_log2 - 5], spec.convs[2 * res_log2 - 4]
        assert conv0_up.up and (conv0_up.cin, conv0_up.cout) == up and conv0_up.scope == f"{side}x{side}/Conv0_up"
        assert not conv.up and (conv.cin, conv.cout) == conv1
        assert spec.torgbs[res_log2 - 2].cin == rgb_cin
    # up to 32x32 the two configs are one network
    assert spec.convs[:7] == sg2_spec.make_spec(resolution).convs[:7]  # (conv layers 0 ... 6: 4x4 ... 32x32)


def test_spec_defaults_and_rejected_values() -> None:
    assert sg2_spec.make_spec(32, fmap_base=CONFIG_E)._replace(fmap_base=sg2_spec.FMAP_BASE) == sg2_spec.make_spec(32)
    assert sg2_spec.make_spec(256) == sg2_spec.make_spec(256, fmap_base=16 << 10) and sg2_spec.make_spec(256).fmap_base == 16 << 10
    for bad in (4 << 10, 32 << 10, 0):
        with pytest.raises(ValueError, match="fmap_base"):
            sg2_spec.make_spec(64, fmap_base=bad)
        with pytest.raises(ValueError, match="fmap_base"):
            sg2_spec.make_random_variables(64, fmap_base=bad)
        with pytest.raises(ValueError, match="fmap_base"):
            sg2_spec.make_stress_variables(64, fmap_base=bad)


def test_fmap_base_of() -> None:
    for resolution in (64, 256):
        assert sg2_spec.fmap_base_of(sg2_spec.make_random_variables(resolution, seed=1, fmap_base=CONFIG_E), resolution) == CONFIG_E
        assert sg2_spec.fmap_base_of(sg2_spec.make_random_variables(resolution, seed=1), resolution) == 16 << 10
    assert sg2_spec.fmap_base_of(sg2_spec.make_random_variables(32, seed=1, fmap_base=CONFIG_E), 32) == 16 << 10  # (one network)
    stress = sg2_spec.make_stress_variables(64, seed=0, fmap_base=CONFIG_E)
    assert stress["G_synthesis/64x64/Conv1/weight"].shape == (3, 3, 256, 256) and sg2_spec.fmap_base_of(stress, 64) == CONFIG_E
    neither = dict(sg2_spec.make_random_variables(64, seed=1))
    neither["G_synthesis/64x64/ToRGB/weight"] = np.zeros((1, 1, 128, 3), dtype=np.float32)
    with pytest.raises(ValueError) as info:
        sg2_spec.fmap_base_of(neither, 64)
    message = str(info.value)
    assert "G_synthesis/64x64/ToRGB/weight" in message and "(1, 1, 512, 3)" in message and "(1, 1, 256, 3)" in message


def test_blob_sizes_agree_across_the_abi(library: ctypes.CDLL) -> None:
    flag = hip_lib.GANCE_FLAG_FMAP_BASE_8K
    assert flag == 128
    for resolution in (8, 64, 256, 1024):
        config_e, config_f = sg2_spec.make_spec(resolution, fmap_base=CONFIG_E), sg2_spec.make_spec(resolution)
        assert library.gance_weight_blob_floats_flags(resolution, flag) == sg2_spec.blob_size(config_e)
        assert library.gance_weight_blob_floats_flags(resolution, 0) == library.gance_weight_blob_floats(resolution) == sg2_spec.blob_size(config_f)
        # (the form flags do not change the count)
        assert library.gance_weight_blob_floats_flags(resolution, flag | hip_lib.GANCE_FLAG_DIRECT_CONV) == sg2_spec.blob_size(config_e)
        assert (sg2_spec.blob_size(config_e) < sg2_spec.blob_size(config_f)) == (resolution > 32)
    assert library.gance_weight_blob_floats_flags(1000, flag) == 0
    assert library.gance_abi_version() == 6 and ctypes.sizeof(hip_lib.EngineConfig) == 16


def test_a_blob_of_the_other_config_is_refused(library: ctypes.CDLL) -> None:
    handle = ctypes.c_void_p()
    for flags, fmap_base in ((hip_lib.GANCE_FLAG_FMAP_BASE_8K, 16 << 10), (0, CONFIG_E)):
        blob = np.zeros(sg2_spec.blob_size(sg2_spec.make_spec(64, fmap_base=fmap_base)), dtype=np.float32)
        config = hip_lib.EngineConfig(64, 1, 0, flags)
        status = library.gance_engine_create(
            ctypes.byref(config), blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_uint64(blob.size), ctypes.byref(handle)
        )
        assert status == 2 and not handle  # GANCE_ERR_BAD_WEIGHTS, before any device is touched


def test_network_file_round_trip(tmp_path: Path) -> None:
    variables = sg2_spec.make_random_variables(64, seed=5, perturb=True, fmap_base=CONFIG_E)
    path = tmp_path / "config_e.pkl"
    network_file.save_network(path, 64, variables)
    loaded = network_file.load_network(path)
    assert loaded.resolution == 64 and loaded.fmap_base == CONFIG_E and set(loaded.variables) == set(variables)
    for name, value in variables.items():
        assert np.array_equal(loaded.variables[name], value)
    network_file.write_random_network(tmp_path / "random_e.pkl", 64, seed=2, fmap_base=CONFIG_E)
    assert network_file.load_network(tmp_path / "random_e.pkl").fmap_base == CONFIG_E
    network_file.write_random_network(tmp_path / "random_f.pkl", 64, seed=2)
    config_f = network_file.load_network(tmp_path / "random_f.pkl")
    assert config_f.fmap_base == 16 << 10 and config_f.variables["G_synthesis/64x64/Conv1/weight"].shape == (3, 3, 512, 512)
    assert network_file.NetworkFile(64, {}).fmap_base == 16 << 10  # (the trailing field has a default)
    # a network that is neither cannot be saved as one of them
    broken = dict(variables)
    broken["G_synthesis/64x64/ToRGB/weight"] = np.zeros((1, 1, 128, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        network_file.save_network(tmp_path / "broken.pkl", 64, broken)


def test_legacy_pickle_round_trip(tmp_path: Path) -> None:
    variables = sg2_spec.make_random_variables(64, seed=6, perturb=True, fmap_base=CONFIG_E)
    path = tmp_path / "legacy_e.pkl"
    legacy_helpers._write_legacy_pickle(path, variables)  # pylint: disable=protected-access
    assert "dnnlib" not in sys.modules
    resolution, loaded = legacy_import.load_legacy_network(path)
    assert resolution == 64 and set(loaded) == set(variables)
    for name, value in variables.items():
        assert np.array_equal(loaded[name], value) and loaded[name].dtype == np.float32
    via_file = network_file.load_network(path)
    assert via_file.resolution == 64 and via_file.fmap_base == CONFIG_E
    assert np.array_equal(via_file.variables["G_synthesis/64x64/Conv1/weight"], variables["G_synthesis/64x64/Conv1/weight"])


def test_legacy_shape_errors_name_the_config(tmp_path: Path) -> None:
    config_f = sg2_spec.make_random_variables(64, seed=1)
    mixed = dict(sg2_spec.make_random_variables(64, seed=1, fmap_base=CONFIG_E))
    mixed["G_synthesis/64x64/Conv1/weight"] = config_f["G_synthesis/64x64/Conv1/weight"]
    path = tmp_path / "mixed.pkl"
    legacy_helpers._write_legacy_pickle(path, mixed)  # pylint: disable=protected-access
    with pytest.raises(ValueError, match=r"G_synthesis/64x64/Conv1/weight.*config-e expects \(3, 3, 256, 256\)"):
        legacy_import.load_legacy_network(path)
    # the other way round, and a top ToRGB that matches neither config: today's words
    mixed = dict(config_f)
    mixed["G_synthesis/64x64/Conv1/weight"] = np.zeros((3, 3, 256, 256), dtype=np.float32)
    legacy_helpers._write_legacy_pickle(path, mixed)  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="config-f expects"):
        legacy_import.load_legacy_network(path)
    neither = dict(config_f)
    neither["G_synthesis/64x64/ToRGB/weight"] = np.zeros((1, 1, 128, 3), dtype=np.float32)
    legacy_helpers._write_legacy_pickle(path, neither)  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="config-f expects"):
        legacy_import.load_legacy_network(path)


def _describe(library: ctypes.CDLL, resolution: int, flags: int, batch: int) -> list:
    out = ctypes.create_string_buffer(1 << 16)
    config = hip_lib.EngineConfig(resolution, 64, 0, flags)
    status = library.gance_engine_describe_plan(ctypes.byref(config), NUM_CUS, batch, out, ctypes.c_uint64(len(out)))
    assert status == 0, (resolution, flags, batch, status)
    return out.value.decode().split()


@pytest.mark.parametrize("resolution", [64, 256, 1024])
def test_every_batch_and_form_flag_gets_a_plan(library: ctypes.CDLL, resolution: int) -> None:
    spec = sg2_spec.make_spec(resolution, fmap_base=CONFIG_E)
    for conv_form, conv_flags in plan_helpers.CONV_FLAGS.items():
        for up_form, up_flags in plan_helpers.UP_FLAGS.items():
            flags = conv_flags | up_flags | hip_lib.GANCE_FLAG_FMAP_BASE_8K
            for batch in range(1, 65):
                names = _describe(library, resolution, flags, batch)
                where = f"{resolution} {conv_form} {up_form} B {batch}"
                convs = [name for name in names if name.startswith("conv")]
                assert len(convs) == len(spec.convs), where
                for name, conv in zip(convs, spec.convs):
                    side = 2 ** conv.res_log2
                    kind, rest = name.split("_", 1)
                    assert "".join(ch for ch in kind.split("+")[0] if ch.isdigit()) == str(conv.layer_idx), f"{where}: {name}"
                    assert rest.split("/")[0] == f"{side}x{side}_{conv.cin}->{conv.cout}", f"{where}: {name}"
                    assert kind.startswith("convT") == conv.up, f"{where}: {name}"
                assert names[:2] == ["styles", "demod"] and names.count(f"torgb_{resolution}x{resolution}") <= 1, where
                if resolution == 1024:
                    # the frame leaves from the last conv launch: no ToRGB pass behind it, no other store of its activation
                    assert convs[-1] == "conv16+torgb_1024x1024_16->16" and names[-1] == convs[-1], where
                    assert not [name for name in names if name.startswith(("finish16", "torgb_1024"))], where
                    # the up layer in front: one fused launch, or the transposed conv and its FIR pass
                    up = convs[-2]
                    assert up in ("convTF15_1024x1024_32->16/16", "convT15_1024x1024_32->16"), f"{where}: {up}"
                    assert ("fir15_1024x1024" in names) == (up == "convT15_1024x1024_32->16"), where
                    if up_form == "split":
                        assert up == "convT15_1024x1024_32->16", where
                    if up_form == "fused":
                        assert up == "convTF15_1024x1024_32->16/16", where


def test_the_flag_describes_the_same_network_up_to_32(library: ctypes.CDLL) -> None:
    for resolution in (8, 32):
        for batch in (1, 5, 64):
            assert _describe(library, resolution, hip_lib.GANCE_FLAG_FMAP_BASE_8K, batch) == _describe(library, resolution, 0, batch)
    assert _describe(library, 64, hip_lib.GANCE_FLAG_FMAP_BASE_8K, 1) != _describe(library, 64, 0, 1)
