"""
The split-operand up kernel's narrow geometries (upfir_split.hip, NT = 2 / 4): the 32^2 and 64^2 Conv0_up layers, inputs 16 and 32 wide,
one block per sample and 64 / W channel tiles of 16, the whole width as one strip. The engine takes them by the fill rule (blocks for
9/16 of the CUs): a 64^2 network at 18 frames has 18 x 8 blocks on the 32^2 layer and 18 x 16 on the 64^2 one, so both are "/s3"
launches (conv layer_idx 5: plain input, the style multiplied in while staging; layer_idx 7: pre-scaled by the F(4x4,3x3) launch
before it in the default form, plain in the direct form).

Bars, on max|got - want| / max|want| per sample:
  * 2e-5 layer-wise against the fp64 oracle chain (tests/test_synthesis_gpu.py's bar), noise on and off, exponent range included;
  * 1.5e-6 in isolation (the layer's own input from the kernels, one fp64 oracle layer): the split bar of
    tests/test_isolated_layers_gpu.py, which a kernel that drops one of its six part products fails.
The oracle runs on two of the 18 samples (the first and the last block of the launch): samples are independent.
"""

import numpy as np
import pytest
import torch

from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

RESOLUTION = 64
BATCH = 18
SAMPLES = [0, BATCH - 1]
TOLERANCE = 2e-5
SPLIT_UP_TOLERANCE = 1.5e-6
NARROW_LAYERS = (5, 7)  # layer_idx of the 32^2 and 64^2 Conv0_up


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    return hip_lib.load_library()


def _launches(engine) -> dict:
    """{layer_idx: launch name} of the up launches of the engine's last call (profiling on)."""
    names = {}
    for step in engine.steps():
        if step.name.startswith("convTF"):
            kind = step.name.split("_")[0]
            names[int("".join(ch for ch in kind if ch.isdigit()))] = step.name
    return names


def _rel(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.abs(got - want).max() / np.abs(want).max())


def _run(variables: dict, conv_form: str, dlatents: np.ndarray, chain: bool) -> None:
    spec = sg2_spec.make_spec(RESOLUTION)
    engine = hip_lib.Engine(variables, RESOLUTION, max_batch=BATCH, conv_form=conv_form, profile=True)
    try:
        engine.synthesize_w(dlatents)
        launches = _launches(engine)
        for idx in NARROW_LAYERS:
            assert launches[idx].endswith("/s3"), launches
        assert launches[7].startswith("convTFp") == (conv_form == "auto"), launches
        wants: list = []
        if chain:
            with torch.no_grad():
                ref.g_synthesis(torch.from_numpy(dlatents[SAMPLES]).double(), variables, RESOLUTION, collect=wants)
        for idx in NARROW_LAYERS:
            n = idx + 1  # (debug taps count conv layers from 1)
            x = engine.debug_activation_after(dlatents, n - 1)[SAMPLES]
            got = engine.debug_activation_after(dlatents, n)[SAMPLES]
            assert np.isfinite(got).all()
            for i, s in enumerate(SAMPLES):
                with torch.no_grad():
                    want = ref.synthesis_layer(torch.from_numpy(x[i:i + 1]).double(), torch.from_numpy(dlatents[s:s + 1]).double(), variables,
                                               spec.convs[n - 1]).numpy()[0]
                iso = _rel(got[i], want)
                print(f"\n{launches[idx]} sample {s}: isolated {iso:.2e}", end="")
                assert iso < SPLIT_UP_TOLERANCE, f"{launches[idx]}, sample {s}: isolated error {iso:.2e}"
                if chain:
                    layer = _rel(got[i], wants[n - 1].numpy()[i])
                    print(f", layer-wise {layer:.2e}", end="")
                    assert layer < TOLERANCE, f"{launches[idx]}, sample {s}: layer-wise error {layer:.2e}"
    finally:
        engine.close()


@pytest.mark.parametrize("conv_form,noise", [("auto", True), ("auto", False), ("direct", True)])
def test_narrow_split_up_layers_match_oracle(library, conv_form: str, noise: bool) -> None:
    variables = sg2_spec.make_random_variables(RESOLUTION, seed=3, perturb=True)
    if not noise:
        variables = {name: (np.zeros_like(value) if name.endswith("/noise_strength") else value) for name, value in variables.items()}
    dlatents = np.random.RandomState(5).randn(BATCH, sg2_spec.make_spec(RESOLUTION).num_layers, 512).astype(np.float32)
    _run(variables, conv_form, dlatents, chain=True)


def test_narrow_split_up_layers_in_isolation_on_the_stress_network(library) -> None:
    variables = sg2_spec.make_stress_variables(RESOLUTION, seed=0)
    dlatents = np.random.RandomState(11).randn(BATCH, sg2_spec.make_spec(RESOLUTION).num_layers, 512).astype(np.float32)
    _run(variables, "auto", dlatents, chain=False)


@pytest.mark.parametrize("log2_scale", [40, -40, -100])
def test_narrow_split_up_layers_keep_the_fp32_exponent_range(library, log2_scale: int) -> None:
    """Both narrow layers' weights x 2^log2_scale (scaled down: their bias and noise zeroed, see test_synthesis_gpu.py)."""
    variables = dict(sg2_spec.make_random_variables(RESOLUTION, seed=7, perturb=True))
    for scope in ("G_synthesis/32x32/Conv0_up", "G_synthesis/64x64/Conv0_up"):
        variables[f"{scope}/weight"] = (variables[f"{scope}/weight"].astype(np.float64) * 2.0 ** log2_scale).astype(np.float32)
        if log2_scale < 0:
            for leaf in ("bias", "noise_strength"):
                variables[f"{scope}/{leaf}"] = np.zeros_like(variables[f"{scope}/{leaf}"])
    dlatents = np.random.RandomState(9).randn(BATCH, sg2_spec.make_spec(RESOLUTION).num_layers, 512).astype(np.float32)
    _run(variables, "auto", dlatents, chain=True)
