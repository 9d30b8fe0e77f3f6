"""
Every 4^2 ... 128^2 conv layer checked IN ISOLATION in each form the product runs it in (default selection: conv_form / up_form "auto",
no GANCE_TUNE_* knob), the way tests/test_isolated_layers_gpu.py checks the 256^2 ... 1024^2 ones: the layer's own input as the kernels
left it (debug_activation_after(n - 1); the 4x4 constant for the first layer), promoted to fp64, goes through ONE oracle layer
(stylegan2_ref.synthesis_layer), and the kernel's output (debug_activation_after(n)) is compared with that. The network is the 128^2
generator, whose eleven conv layers the planner treats exactly as it does layers 0 ... 10 of the 1024^2 one
(tests/test_isolated_coverage.py holds that, and that the case table of tests/isolated_small_cases.py reaches all 25 (layer, form)
launches calls of 1 ... 64 frames produce on 256 CUs). The form of a layer depends on (layer, batch, flags) alone, so a call stopped
after layer n runs layers 1 ... n as the whole call does; the test asserts that from the profiled launch names of both.

Bars, per layer and sample, on error = max|got - want| / max|want|:
  * ceiling: 2e-5 for every form, 1e-4 on the stress network (the layer-wise bars of tests/test_synthesis_gpu.py);
  * split-operand launches ("/s3"): SPLIT_UP_TOLERANCE = 1.5e-6, stress network included: the bar of tests/test_isolated_layers_gpu.py
    (honest <= 8.7e-7 there, a build without the x2 w0 part product >= 2.8e-6);
  * the other fp32 forms that are not Winograd (conv<n> + finish, convT<n> + fir, convTG<n>, convTF<n>/16): FP32_MARGIN = 4 times err32,
    the error of the same oracle layer evaluated in float32 on the CPU from the same fp32 input, against the fp64 result. Kernel and
    float32 restatement sum the same 4608 (2304 at layer 10) fp32 products in different orders, the two-pass up forms also apply the
    FIR to planes already rounded to fp32; the maximum over 1e4 ... 1e6 outputs is a stable statistic, so a factor of four covers the
    difference in order, while an operand or accumulator that loses mantissa bits lands an order of magnitude above it;
  * Winograd launches (convV, convVG): the ceiling only (no tighter bar separates right from subtly wrong there, see
    tests/test_isolated_layers_gpu.py); their error and err32 are printed all the same.

Measured so far, on the CPU alone: err32 of the every-term network at one frame, 3.6e-7 ... 5.0e-7 on the stride-1 layers and
3.9e-7 ... 1.4e-6 on the up layers, so the fp32 bar is 1.4e-6 ... 5.4e-6. NOT YET MEASURED on an MI355X: the error ranges per form
family, the honest "/s3" value of layer 9 (Cin = 512 in the wide geometry, which nobody has measured against 1.5e-6) and the three
"/s3" values of layers 5, 7, 9 of a build without the x2 w0 part product; the test prints one line per (layer, launch, sample) with
error, err32 and their ratio, from which these ranges are to be recorded here.
"""

import os

import numpy as np
import pytest
import torch

import isolated_small_cases as cases
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

RESOLUTION = 128
TOLERANCE = 2e-5
STRESS_TOLERANCE = 1e-4
SPLIT_UP_TOLERANCE = 1.5e-6  # (tests/test_isolated_layers_gpu.py: honest <= 8.7e-7, one dropped part product >= 2.8e-6)
FP32_MARGIN = 4.0  # times the float32 oracle layer's own error: see above


def _family(name: str) -> str:
    """The bar a launch is held to: "split" (/s3), "winograd" (convV, convVG), "fp32" (every other form)."""
    if name.endswith("/s3"):
        return "split"
    return "winograd" if name.startswith("convV") else "fp32"


def _launches(engine) -> dict:
    """{layer_idx: launch name} of the conv launches of the engine's last call (profiling on)."""
    return cases.conv_launches(step.name for step in engine.steps())


def _rel(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.abs(got - want).max() / np.abs(want).max())


_VARIABLES: dict = {}


def _variables(network: str) -> dict:
    """The 128^2 generators, made once per session."""
    if network not in _VARIABLES:
        if network == "stress":
            _VARIABLES[network] = sg2_spec.make_stress_variables(RESOLUTION, seed=0)
        else:
            _VARIABLES[network] = sg2_spec.make_random_variables(RESOLUTION, seed=3, perturb=network == "every_term")
    return _VARIABLES[network]


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    knobs = sorted(key for key in os.environ if key.startswith("GANCE_TUNE_"))
    if knobs:
        pytest.fail(f"{', '.join(knobs)} set: these checks are of the forms the product selects by itself; unset every GANCE_TUNE_* variable")
    return hip_lib.load_library()


# every term on at every batch of the table; StyleGAN2's own init (no noise, no biases: the network bench.py times) at 4 and 16 frames,
# the stress network at 1 and 18
CONFIGS = [("every_term", batch) for batch, _ in cases.CASES] + [("stylegan_init", 4), ("stylegan_init", 16), ("stress", 1), ("stress", 18)]


@pytest.mark.parametrize("network,batch", CONFIGS, ids=[f"{n}-{b}" for n, b in CONFIGS])
def test_layers_4_to_128_in_isolation_on_the_default_kernels(library, network: str, batch: int) -> None:
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    spec = sg2_spec.make_spec(RESOLUTION)
    assert len(spec.convs) == cases.LAST_SMALL_LAYER + 1
    variables = _variables(network)
    ceiling = STRESS_TOLERANCE if network == "stress" else TOLERANCE
    layers = cases.layers_at(batch)
    samples = [batch - 1] if batch == 64 else sorted({0, batch - 1})  # (the GEMM forms' padded last column tile holds the last sample)
    dlatents = np.random.RandomState(11 + batch).randn(batch, spec.num_layers, 512).astype(np.float32)
    const = np.repeat(np.asarray(variables["G_synthesis/4x4/Const/const"], dtype=np.float32), len(samples), axis=0)
    engine = hip_lib.Engine(variables, RESOLUTION, max_batch=batch, profile=True)
    rows: dict = {}  # (layer_idx, sample) -> (isolated error, err32)
    tapped: dict = {}  # layer_idx -> its launch name in the call that stopped after it
    try:
        for idx in layers:
            conv = spec.convs[idx]
            assert conv.layer_idx == idx
            n = idx + 1  # (debug taps count conv layers from 1)
            x = const if idx == 0 else engine.debug_activation_after(dlatents, n - 1)[samples].copy()
            got = engine.debug_activation_after(dlatents, n)[samples].copy()
            tapped[idx] = _launches(engine).get(idx)
            assert np.isfinite(got).all()
            for i, s in enumerate(samples):
                xi, wi = torch.from_numpy(x[i:i + 1]), torch.from_numpy(dlatents[s:s + 1])
                with torch.no_grad():
                    want = ref.synthesis_layer(xi.double(), wi.double(), variables, conv).numpy()[0]
                    want32 = ref.synthesis_layer(xi, wi, variables, conv).numpy()[0]
                assert got[i].shape == want.shape and want32.dtype == np.float32
                rows[(idx, s)] = (_rel(got[i], want), _rel(want32, want))
        engine.synthesize_w(dlatents)
        launches = _launches(engine)
    finally:
        engine.close()

    print(f"\nisolated layers, {network} network, batch {batch} ({num_cus} CUs): error, err32, error / err32")
    for (idx, s), (err, err32) in sorted(rows.items()):
        print(f"  conv {idx + 1:2d} {spec.convs[idx].scope:16s} {launches.get(idx, '?'):30s} {_family(launches.get(idx, '')):8s} sample {s:2d}: "
              f"{err:.2e} {err32:.2e} {err / err32:5.2f}")
    for idx in layers:
        assert tapped[idx] == launches[idx], f"layer {idx}: {tapped[idx]} in the call stopped after it, {launches[idx]} in the whole call"
        if num_cus == cases.NUM_CUS:
            assert launches[idx] == cases.expected_name(idx, batch), f"layer {idx} at {batch} frames: {launches[idx]}"
    for (idx, s), (err, err32) in sorted(rows.items()):
        where = f"conv layer {idx + 1} ({spec.convs[idx].scope}, {launches[idx]}), sample {s}"
        assert err < ceiling, f"{where}: isolated error {err:.2e}"
        family = _family(launches[idx])
        if family == "split":
            assert err < SPLIT_UP_TOLERANCE, f"split-operand up layer, {where}: isolated error {err:.2e}"
        elif family == "fp32":
            assert err <= FP32_MARGIN * err32, f"{where}: isolated error {err:.2e} is {err / err32:.1f} x the float32 oracle layer's {err32:.2e}"
