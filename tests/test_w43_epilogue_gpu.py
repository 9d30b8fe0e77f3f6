"""
The tile epilogue of the F(4x4,3x3) kernels (gance_amd/csrc/winograd43_conv.hip) after its diet: the ToRGB channel sum as per-lane FMAs
reduced over the four lane rows with v_permlane32_swap / v_permlane16_swap, and the tile decode by shifts.

One-hot ToRGB. In the reduction a lane (n16, g) adds its channels 4 g + r (r = 0 .. 3) for 3 colours x 16 pixels, two swaps add the four
lane rows, and lane row g ends with output row g of the tile. A swapped lane row or colour shows as a wrong or missing plane only when
ONE (channel, colour) coefficient is non-zero; a random network hides it inside the bar. The kernel sees the table style x weight, so the
top ToRGB layer is set up as:
  * weight: zero except colour c (every channel: sqrt(cin) x U(0.5, 1.5), i.e. a runtime coefficient of 0.5 .. 1.5): one engine per colour;
  * mod_weight: zero except [j][k0 + j] = sqrt(512), mod_bias = -1: a ToRGB dlatent row e_j gives the style one-hot at channel k0 + j, so the
    32 channels of a block (both channel tiles = both roles, four lane rows, four r) are 32 dlatents on one engine -- no engine per setting.
The layers below the ToRGB do not depend on the setting: the fp64 oracle chain runs once per geometry (ref.g_synthesis with `collect`, and
once at half the resolution for the previous image), and each setting's image is the oracle's own ref.torgb_layer on that activation.
Geometries: 64^2 with 1 frame per call (the 16 x 64 tile, one tile per block) and 32^2 with 20 frames per call (the 32 x 32 tile of the w32
kernels, blocks of 1 and 2 tiles), as in tests/test_w43_tile_boundaries_gpu.py.

Tile boundaries. 256^2 with 2 and with 5 frames (blocks of 2 / of 2 and 3 tiles at 256^2: a deferred epilogue followed by the re-derived
per-lane values) and 128^2 with 3 frames, each with and without noise and bias (perturb).

Bars: those of tests/test_w43_tile_boundaries_gpu.py, layer-wise 2e-5 and image 1e-4 against the fp64 oracle chain, conv_form="winograd43".
"""

import numpy as np
import pytest
import torch

from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

LAYER_TOLERANCE = 2e-5
IMAGE_TOLERANCE = 1e-4

BLOCK_FIRST_CHANNEL = 5 * 32  # the 32 channels of one block (channel tiles 10 and 11 of the layer)


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    return hip_lib.load_library()


def _w43_rgb_launch_at(names: list, side: int) -> bool:
    return any(n.startswith("convV") and not n.startswith("convVG") and "+rgb" in n and f"_{side}x{side}_" in n for n in names)


def _one_hot_variables(resolution: int, colour: int) -> dict:
    variables = dict(sg2_spec.make_random_variables(resolution, seed=5, perturb=True))
    scope = f"G_synthesis/{resolution}x{resolution}/ToRGB"
    cin = variables[f"{scope}/weight"].shape[2]
    weight = np.zeros((1, 1, cin, 3), dtype=np.float32)
    weight[0, 0, :, colour] = np.sqrt(cin) * np.random.RandomState(40 + colour).uniform(0.5, 1.5, size=cin)
    mod_weight = np.zeros((512, cin), dtype=np.float32)
    for j in range(32):
        mod_weight[j, BLOCK_FIRST_CHANNEL + j] = np.sqrt(512.0)
    variables[f"{scope}/weight"] = weight
    variables[f"{scope}/mod_weight"] = mod_weight
    variables[f"{scope}/mod_bias"] = np.full((cin,), -1.0, dtype=np.float32)
    return variables


# (resolution, frames per call, the channel j of each frame of each call: all 32 are covered)
ONE_HOT_CASES = {
    "64-one-frame": (64, 1, [[j] for j in range(32)]),
    "32-w32-geometry": (32, 20, [list(range(20)), list(range(12, 32))]),
}


@pytest.fixture(scope="module")
def one_hot_base():
    """Per geometry: the base dlatent (one frame) and, from ONE fp64 oracle pass, every layer's activation and the previous image."""
    cache = {}

    def get(case: str):
        if case not in cache:
            resolution = ONE_HOT_CASES[case][0]
            spec = sg2_spec.make_spec(resolution)
            variables = _one_hot_variables(resolution, 0)  # (below the top ToRGB the three colours' networks are the same)
            base = np.random.RandomState(29).randn(1, spec.num_layers, 512).astype(np.float32)
            wants: list = []
            with torch.no_grad():
                ref.g_synthesis(torch.from_numpy(base).double(), variables, resolution, collect=wants)
                y_prev = ref.g_synthesis(torch.from_numpy(base).double(), variables, resolution // 2)
            cache[case] = (spec, base, wants, y_prev)
        return cache[case]

    return get


@pytest.mark.parametrize("colour", [0, 1, 2])
@pytest.mark.parametrize("case", list(ONE_HOT_CASES))
def test_one_hot_torgb_coefficient_lands_in_its_plane(library, one_hot_base, case: str, colour: int) -> None:
    resolution, batch, calls = ONE_HOT_CASES[case]
    spec, base, wants, y_prev = one_hot_base(case)
    res_log2 = int(np.log2(resolution))
    variables = _one_hot_variables(resolution, colour)
    x_last = wants[-1]
    engine = hip_lib.Engine(variables, resolution, max_batch=batch, conv_form="winograd43", profile=True)
    worst, covered = 0.0, set()
    try:
        if colour == 0:  # (the layers below do not depend on the setting: once per geometry)
            dl = np.repeat(base, batch, axis=0)
            for n in range(1, len(spec.convs) + 1):
                got, want = engine.debug_activation_after(dl, n)[0], wants[n - 1].numpy()[0]
                err = float(np.abs(got - want).max() / np.abs(want).max())
                assert err < LAYER_TOLERANCE, f"conv layer {n} ({spec.convs[n - 1].scope}): rel err {err:.2e}"
        for channels in calls:
            assert len(channels) == batch
            dlatents = np.repeat(base, batch, axis=0)
            dlatents[:, res_log2 * 2 - 3, :] = 0.0
            for b, j in enumerate(channels):
                dlatents[b, res_log2 * 2 - 3, j] = 1.0
            with torch.no_grad():
                want = ref.torgb_layer(x_last.repeat(batch, 1, 1, 1), y_prev.repeat(batch, 1, 1, 1), torch.from_numpy(dlatents).double(), variables, res_log2).numpy()
            _, image = engine.synthesize_w(dlatents, want_float=True)
            assert image.shape == want.shape
            for b, j in enumerate(channels):
                err = float(np.abs(image[b] - want[b]).max())
                worst = max(worst, err)
                planes = [f"{float(np.abs(image[b, c] - want[b, c]).max()):.2e}" for c in range(3)]
                assert err < IMAGE_TOLERANCE, f"channel {BLOCK_FIRST_CHANNEL + j}, colour {colour}: max |image - oracle| = {err:.2e}, by plane {planes}"
                covered.add(j)
        names = [step.name for step in engine.steps() if step.name.startswith("conv")]
    finally:
        engine.close()
    print(f"\n{case}, colour {colour}: {len(covered)} channels, worst max |image - oracle| = {worst:.2e}")
    assert covered == set(range(32))
    assert _w43_rgb_launch_at(names, resolution), names


# (resolution, frames, perturb)
BOUNDARY_CASES = [(256, 2), (256, 5), (128, 3)]


@pytest.mark.parametrize("perturb", [True, False])
@pytest.mark.parametrize("resolution,batch", BOUNDARY_CASES)
def test_layers_and_image_across_tile_boundaries(library, resolution: int, batch: int, perturb: bool) -> None:
    spec = sg2_spec.make_spec(resolution)
    variables = sg2_spec.make_random_variables(resolution, seed=7, perturb=perturb)
    dlatents = np.random.RandomState(31).randn(batch, spec.num_layers, 512).astype(np.float32)
    wants: list = []
    with torch.no_grad():
        want_image = ref.g_synthesis(torch.from_numpy(dlatents).double(), variables, resolution, collect=wants).numpy()
    engine = hip_lib.Engine(variables, resolution, max_batch=batch, conv_form="winograd43", profile=True)
    errors = {}
    try:
        for n in range(1, len(spec.convs) + 1):
            got, want = engine.debug_activation_after(dlatents, n), wants[n - 1].numpy()
            assert got.shape == want.shape
            errors[n] = float(np.abs(got - want).max() / np.abs(want).max())
        _, image = engine.synthesize_w(dlatents, want_float=True)
        names = [step.name for step in engine.steps() if step.name.startswith("conv")]
    finally:
        engine.close()
    image_error = float(np.abs(image - want_image).max())
    print(f"\n{resolution}^2, {batch} frames, perturb={perturb}: image {image_error:.2e}, layers " + " ".join(f"{e:.1e}" for e in errors.values()))
    for side in (32, 64, 128, 256):
        if side <= resolution:
            assert _w43_rgb_launch_at(names, side), (side, names)
    for n, err in errors.items():
        assert err < LAYER_TOLERANCE, f"conv layer {n} ({spec.convs[n - 1].scope}): rel err {err:.2e}"
    assert image.shape == want_image.shape
    assert image_error < IMAGE_TOLERANCE, f"max |image - oracle| = {image_error:.2e}"
