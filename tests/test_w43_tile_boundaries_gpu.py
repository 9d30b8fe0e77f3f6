"""
Tile boundaries of the F(4x4,3x3) kernels (gance_amd/csrc/winograd43_conv.hip). A block of that kernel streams its tiles back to back;
both epilogues of a tile (one per channel tile = per wave of a SIMD) run in the first interval of the block's NEXT tile, the ToRGB sums
of the two waves meet in LDS and are added and stored one barrier later, and the block's LAST tile takes a path of its own (no following
interval: epilogues behind the stream, one trailing barrier, then the add). Which of these paths a launch runs depends only on how many
tiles its blocks get, so the cases below are chosen by tile count, with conv_form="winograd43" so that the form does not depend on
the batch (every Conv1 from 32^2 up is a "convV<n>+rgb" launch then).

Grid rule (launch_winograd43_conv, restated in _grid): tiles = (Cout / 32) x pixel tiles x frames, a pixel tile = 16 x 64 pixels (32 x 32
on the 32^2 layer); blocks = min(tiles, CUs x rounds), rounds = 4 (GANCE_TUNE_W43_ROUNDS) lowered while tiles < CUs x rounds x
max(1, 64 / (Cin / 4)); block b takes tiles b, b + blocks, ... On 256 CUs, tiles per frame 16 / 64 / 128 / 256 at 32^2 / 64^2 / 128^2 /
256^2 (Cout 512 / 512 / 256 / 128), so the blocks of a call get:

  case                   32^2 (w32 geometry)   64^2          128^2         256^2
  (a) 256^2, 1 frame     1                     1             1             1              every block has exactly one tile
  (b) 256^2, 2 frames    1                     1             1             2              blocks of two tiles
  (c) 256^2, 5 frames    1                     1 and 2       1 and 2       2 and 3        k and k + 1 tiles side by side (rounds 1 / 2 / 2)
  (d) 32^2, 20 frames    1 and 2                                                          the 32 x 32 geometry across a boundary
  (e) 256^2, 5 frames, GANCE_TUNE_W43_ROUNDS = 1 against the default: 256^2 blocks of 5 tiles against 2 and 3, 128^2 blocks of 2 and 3
      against 1 and 2 -- the same tiles in other blocks. A tile's result must not depend on the block that ran it: EQUAL BYTES.

Bars: the layer-wise 2e-5 (max |got - want| / max |want| per layer against the fp64 oracle chain) and the image bar 1e-4 of
tests/test_synthesis_gpu.py, nothing new. The image goes through the partial ToRGB images the launches write; the layer-wise check
through their activation stores.
"""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

LAYER_TOLERANCE = 2e-5
IMAGE_TOLERANCE = 1e-4


def _grid(cin: int, cout: int, side: int, batch: int, num_cus: int, rounds: int = 4) -> tuple:
    """(tiles, blocks) of an F(4x4,3x3) launch: launch_winograd43_conv's grid rule restated."""
    pixel_tiles = 1 if side == 32 else (side // 64) * (side // 16)
    tiles = (cout // 32) * pixel_tiles * batch
    resident = max(8, num_cus // 8 * 8)
    min_tiles = max(1, 64 // (cin // 4))
    while rounds > 1 and tiles < resident * rounds * min_tiles:
        rounds -= 1
    return tiles, min(tiles, resident * rounds)


def _tiles_per_block(cin: int, cout: int, side: int, batch: int, num_cus: int, rounds: int = 4) -> set:
    tiles, blocks = _grid(cin, cout, side, batch, num_cus, rounds)
    return {tiles // blocks} | ({tiles // blocks + 1} if tiles % blocks else set())


# the Conv1 layers the F(4x4,3x3) kernels run: side -> (Cin, Cout)
W43_LAYERS = {32: (512, 512), 64: (512, 512), 128: (256, 256), 256: (128, 128)}

# (resolution, batch) -> {side: tiles per block} on 256 CUs (the table of the module docstring)
CASES = {
    "a-one-tile": (256, 1, {32: {1}, 64: {1}, 128: {1}, 256: {1}}),
    "b-two-tiles": (256, 2, {32: {1}, 64: {1}, 128: {1}, 256: {2}}),
    "c-k-and-k+1": (256, 5, {32: {1}, 64: {1, 2}, 128: {1, 2}, 256: {2, 3}}),
    "d-w32-geometry": (32, 20, {32: {1, 2}}),
}


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    return hip_lib.load_library()


def test_grid_rule_gives_the_tile_counts_the_cases_are_named_for() -> None:
    for resolution, batch, want in CASES.values():
        for side, counts in want.items():
            assert _tiles_per_block(*W43_LAYERS[side], side, batch, 256) == counts, (resolution, batch, side)
    assert _tiles_per_block(128, 128, 256, 5, 256, rounds=1) == {5} and _tiles_per_block(256, 256, 128, 5, 256, rounds=1) == {2, 3}


@pytest.mark.parametrize("case", list(CASES))
def test_layers_and_image_across_tile_boundaries(library, case: str) -> None:
    resolution, batch, _ = CASES[case]
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    spec = sg2_spec.make_spec(resolution)
    variables = sg2_spec.make_random_variables(resolution, seed=3, perturb=True)
    dlatents = np.random.RandomState(23).randn(batch, spec.num_layers, 512).astype(np.float32)
    wants: list = []
    with torch.no_grad():
        want_image = ref.g_synthesis(torch.from_numpy(dlatents).double(), variables, resolution, collect=wants).numpy()
    engine = hip_lib.Engine(variables, resolution, max_batch=batch, conv_form="winograd43", profile=True)
    errors = {}
    try:
        for n in range(1, len(spec.convs) + 1):
            got = engine.debug_activation_after(dlatents, n)
            want = wants[n - 1].numpy()
            assert got.shape == want.shape
            errors[n] = float(np.abs(got - want).max() / np.abs(want).max())
        _, image = engine.synthesize_w(dlatents, want_float=True)
        names = [step.name for step in engine.steps() if step.name.startswith("conv")]
    finally:
        engine.close()
    image_error = float(np.abs(image - want_image).max())
    print(f"\n{case}: {resolution}^2, {batch} frames, {num_cus} CUs")
    for side, (cin, cout) in W43_LAYERS.items():
        if side <= resolution:
            print(f"  {side}^2: (tiles, blocks) = {_grid(cin, cout, side, batch, num_cus)}, tiles per block {sorted(_tiles_per_block(cin, cout, side, batch, num_cus))}")
    for n, err in errors.items():
        print(f"  conv {n:2d} {spec.convs[n - 1].scope:18s}: {err:.2e}")
    print(f"  image: max |image - oracle| = {image_error:.2e}")
    # the launches the case is about: every Conv1 from 32^2 up in the F(4x4,3x3) form with the ToRGB sum in its epilogue
    for side in W43_LAYERS:
        if side <= resolution:
            assert any(name.startswith("convV") and not name.startswith("convVG") and "+rgb" in name and f"_{side}x{side}_" in name for name in names), (side, names)
    for n, err in errors.items():
        assert err < LAYER_TOLERANCE, f"conv layer {n} ({spec.convs[n - 1].scope}): rel err {err:.2e}"
    assert image.shape == want_image.shape
    assert image_error < IMAGE_TOLERANCE, f"max |image - oracle| = {image_error:.2e}"


_ROUNDS_SCRIPT = """
import sys
import numpy as np
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
res, batch = int(sys.argv[1]), int(sys.argv[2])
spec = sg2_spec.make_spec(res)
variables = sg2_spec.make_random_variables(res, seed=3, perturb=True)
dlatents = np.random.RandomState(23).randn(batch, spec.num_layers, 512).astype(np.float32)
engine = hip_lib.Engine(variables, res, max_batch=batch, conv_form="winograd43")
frames, image = engine.synthesize_w(dlatents, want_float=True)
last = engine.debug_activation_after(dlatents, len(spec.convs) - 1)
engine.close()
np.savez(sys.argv[3], frames=frames, image=image, last=last)
"""


def test_a_tile_does_not_depend_on_the_block_that_runs_it(library, tmp_path) -> None:
    """Case (e): one persistent block per CU against the default rounds, each in its own process (the knob is read once): equal bytes."""
    repo_root = Path(__file__).resolve().parent.parent
    outputs = {}
    for label, env_extra in (("default", {}), ("one_round", {"GANCE_TUNE_W43_ROUNDS": "1"})):
        path = tmp_path / f"{label}.npz"
        env = {k: v for k, v in os.environ.items() if k != "GANCE_TUNE_W43_ROUNDS"}
        env.update(PYTHONPATH=str(repo_root), **env_extra)
        subprocess.run([sys.executable, "-c", _ROUNDS_SCRIPT, "256", "5", str(path)], check=True, env=env, cwd=repo_root, timeout=300)
        outputs[label] = np.load(path)
    for key in ("image", "last", "frames"):
        a, b = outputs["default"][key], outputs["one_round"][key]
        print(f"{key}: {int((a != b).sum())} of {a.size} values differ")
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), key
