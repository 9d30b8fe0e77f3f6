"""
GPU tests of the plain 3x3 convolution (gance_amd/csrc/conv3x3.hip, gance::conv3x3) and of `VGG16Lpips(convolution="conv3x3")`.

Isolated op: torch.nn.functional.conv2d on the CPU in float64 is the oracle and in float32 the yardstick, judged with
grad_ref.judge: y within grad_ref.LAYER_BAR of its maximum, grad_x within grad_ref.GRADIENT_BAR_FACTOR x the float32 oracle's
own error. Weights N(0, 1) / sqrt(9 cin), x and the cotangent N(0, 1). The shapes are tests/conv3x3_cases.CASES, which
tests/test_conv3x3.py ties to the dispatcher's forms. The whole chain and the projector are judged exactly as
tests/test_lpips_gpu.py judges the modconv3x3 path, on the same inputs and references. Every figure is printed before it is asserted.

Measured (one MI355X):
    isolated         y 1.9e-7 ... 5.8e-7 of its maximum (bar 2e-5); grad_x 0.78 ... 2.71 x the float32 oracle's own error (bar 8)
    whole chain      activations 2e-7 ... 7e-7 of their maximum; 0 ... 2 masks and selections differ per whole input (cap 8);
                     image gradient 0.84 ... 1.08 (1.3e-6 ... 2.1e-6); distance 0.01 ... 1.00 of the largest float32 own error (1.4e-7)
    projector        30 steps at 64^2 config-e, B = 2: LPIPS 0.0161 -> 0.0075 and 0.0224 -> 0.0058
"""

import functools
from typing import Dict, List, Tuple

import numpy as np
import pytest
import torch

import grad_ref
import lpips_ref
import projection_ref
from conv3x3_cases import CASES
from grad_ref import cuda
from gance_amd import hip_lib, torch_ops
from gance_amd.stylegan2 import lpips
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.stylegan2.projector import Projector

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def inputs(batch: int, cin: int, cout: int, side: int) -> Dict[str, np.ndarray]:
    rng = np.random.RandomState([batch, cin, cout, side])
    return {
        "x": rng.randn(batch, cin, side, side).astype(np.float32),
        "weight": (rng.randn(3, 3, cin, cout) / np.sqrt(9.0 * cin)).astype(np.float32),
        "grad_y": rng.randn(batch, cout, side, side).astype(np.float32),
    }


def oracle(batch: int, cin: int, cout: int, side: int, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, grad_x) of conv2d with padding 1 on the CPU in `dtype`."""
    data = inputs(batch, cin, cout, side)
    x = torch.from_numpy(data["x"]).to(dtype).requires_grad_(True)
    weight = torch.from_numpy(data["weight"]).to(dtype).permute(3, 2, 0, 1).contiguous()  # HWIO -> OIHW
    y = torch.nn.functional.conv2d(x, weight, padding=1)
    (grad_x,) = torch.autograd.grad(y, x, torch.from_numpy(data["grad_y"]).to(dtype))
    return y.detach(), grad_x


def run(batch: int, cin: int, cout: int, side: int, samples: slice = slice(None)) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, grad_x) of gance::conv3x3 on the samples of a case."""
    data = inputs(batch, cin, cout, side)
    weight = cuda(data["weight"])
    x = cuda(data["x"][samples], True)
    y = torch.ops.gance.conv3x3(x, weight, torch_ops.conv3x3_transposed_weight(weight))
    (grad_x,) = torch.autograd.grad(y, x, cuda(data["grad_y"][samples]))
    return y.detach(), grad_x


@pytest.mark.parametrize("batch, cin, cout, side", CASES)
def test_isolated_op(batch: int, cin: int, cout: int, side: int) -> None:
    label = f"conv3x3 B={batch} {cin}->{cout} S={side} form {hip_lib.conv3x3_form(cin, cout, side)} / {hip_lib.conv3x3_form(cout, cin, side)}"
    y, grad_x = run(batch, cin, cout, side)
    assert y.shape == (batch, cout, side, side) and grad_x.shape == (batch, cin, side, side)
    want64, want32 = oracle(batch, cin, cout, side, torch.float64), oracle(batch, cin, cout, side, torch.float32)
    grad_ref.judge(label, ("y", "grad_x"), (y, grad_x), want64, want32)
    # one summation order: a second run gives the same bits
    again_y, again_grad_x = run(batch, cin, cout, side)
    assert torch.equal(again_y, y) and torch.equal(again_grad_x, grad_x)


@pytest.mark.parametrize("batch, cin, cout, side", [case for case in CASES if case[0] == 3])
def test_a_samples_bits_do_not_depend_on_its_batch(batch: int, cin: int, cout: int, side: int) -> None:
    y, grad_x = run(batch, cin, cout, side)
    for sample in range(batch):
        alone_y, alone_grad_x = run(batch, cin, cout, side, slice(sample, sample + 1))
        assert torch.equal(alone_y, y[sample : sample + 1]) and torch.equal(alone_grad_x, grad_x[sample : sample + 1]), sample


@pytest.mark.parametrize("batch, cin, cout, side", CASES)
def test_every_element_is_written(batch: int, cin: int, cout: int, side: int) -> None:
    """The entry point on an output buffer (and a workspace) full of NaN: none is left, at partial tiles too."""
    data = inputs(batch, cin, cout, side)
    x, weight = cuda(data["x"]), cuda(data["weight"])
    y = torch.full((batch, cout, side, side), float("nan"), dtype=torch.float32, device="cuda")
    workspace_bytes = hip_lib.conv3x3_workspace_bytes(batch, cin, cout, side)
    workspace = torch.full((workspace_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    hip_lib.conv3x3_forward_device(
        x.data_ptr(), weight.data_ptr(), batch, cin, cout, side, side, y.data_ptr(), workspace.data_ptr(), workspace_bytes,
        torch.cuda.current_stream().cuda_stream,
    )
    assert not bool(torch.isnan(y).any())
    assert torch.equal(y, torch.ops.gance.conv3x3(x, weight, torch_ops.conv3x3_transposed_weight(weight)))


def test_op_refuses_bad_tensors_and_passes_opcheck() -> None:
    rand = lambda *shape: torch.randn(shape, device="cuda")  # noqa: E731
    x, weight = rand(2, 32, 6, 6), rand(3, 3, 32, 48)
    image = torch_ops.conv3x3_transposed_weight(weight)
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(x.double(), weight, image)
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(x, weight.double(), image)
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(x.cpu(), weight.cpu(), image.cpu())
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(rand(2, 6, 6, 32).permute(0, 3, 1, 2), weight, image)  # not contiguous
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(x, weight, weight)  # weight_transposed of the wrong shape
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(x, weight, weight.flip(0, 1).transpose(2, 3))  # ... and not contiguous
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(rand(2, 32, 6, 8), weight, image)  # not square
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(rand(2, 16, 6, 6), weight, image)  # another channel count than the weight's
    with pytest.raises(ValueError):
        torch.ops.gance.conv3x3(rand(2, 24, 6, 6), rand(3, 3, 24, 48), rand(3, 3, 48, 24))  # no multiple of 16
    torch.library.opcheck(torch.ops.gance.conv3x3.default, (x.clone().requires_grad_(True), weight, image))


# ---- the whole chain, judged as tests/test_lpips_gpu.py::test_whole_chain judges the modconv3x3 path ----


def _run_chain(distance: lpips.VGG16Lpips, images: np.ndarray, targets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
    leaf = cuda(images, True)
    collected: List[torch.Tensor] = []
    total = distance(leaf, targets, collect=collected)
    (gradient,) = torch.autograd.grad(total.sum(), leaf)
    return total.detach(), gradient, [activation.detach() for activation in collected]


@pytest.fixture(scope="module")
def chain_callables():  # type: ignore[no-untyped-def]
    return {
        seed: lpips.VGG16Lpips(lpips_ref.chain_weights(seed), side=lpips_ref.CHAIN_SIDE, device=0, convolution="conv3x3")
        for seed in lpips_ref.CHAIN_SEEDS
    }


@pytest.mark.parametrize("seed, resolution, batch", lpips_ref.CHAIN_CASES)
def test_whole_chain(chain_callables, seed: int, resolution: int, batch: int) -> None:  # type: ignore[no-untyped-def]
    label = f"conv3x3 chain seed {seed} R {resolution} B {batch}"
    images, targets = lpips_ref.chain_inputs(seed, resolution, batch)
    total, gradient, activations = _run_chain(chain_callables[seed], images, torch.from_numpy(targets).cuda())
    assert total.shape == (batch,) and gradient.shape == images.shape and len(activations) == 13
    failures: List[str] = []
    masked, want_total, flips_of_the_input = [], [], 0
    for sample in range(batch):
        ref = lpips_ref.sample64(seed, resolution, sample)
        mine = [activation[sample : sample + 1].cpu() for activation in activations]
        for index, (got, want) in enumerate(zip(mine, ref.activations)):
            error = grad_ref.relative_error(got, want)
            print(f"{label} sample {sample} activation {index}: {error:.3e} (bar {grad_ref.LAYER_BAR:.3e})")
            if not (np.isfinite(error) and error <= grad_ref.LAYER_BAR):
                failures.append(f"sample {sample} activation {index}: {error:.3e} > {grad_ref.LAYER_BAR:.3e}")
        flips = lpips_ref.check_masks(f"{label} sample {sample}", mine, ref.activations)
        flips_of_the_input += flips
        # the float64 gradient of the function the run computed: the mask form built from its own activations
        masked.append(ref.gradient if flips == 0 else lpips_ref.run_sample(seed, resolution, sample, torch.float64, mine).gradient)
        want_total.append(ref.distance)
    lpips_ref.check_cap(label, flips_of_the_input)  # the cap holds for the whole input, not per sample
    own = lpips_ref.gradient_yardstick(seed, resolution, batch)
    error = grad_ref.relative_error(gradient, torch.cat(masked))
    bar = grad_ref.GRADIENT_BAR_FACTOR * own
    print(f"{label} image gradient: error {error:.3e}, float32 restatement {own:.3e}, ratio {error / own:.2f}, bar {bar:.3e}")
    if not (np.isfinite(error) and error <= bar):
        failures.append(f"image gradient: {error:.3e} > {bar:.3e}")
    own = lpips_ref.distance_yardstick()
    error = grad_ref.relative_error(total, torch.cat(want_total))
    bar = grad_ref.GRADIENT_BAR_FACTOR * own
    print(f"{label} distance: error {error:.3e}, largest float32 own error of the cases {own:.3e}, ratio {error / own:.2f}, bar {bar:.3e}")
    if not (np.isfinite(error) and error <= bar):
        failures.append(f"distance: {error:.3e} > {bar:.3e}")
    assert not failures, f"{label}: " + "; ".join(failures)


def test_whole_chain_bits_and_the_kept_target_taps(chain_callables) -> None:  # type: ignore[no-untyped-def]
    distance = chain_callables[1]
    images, targets = lpips_ref.chain_inputs(1, 128, 2)
    device_targets = torch.from_numpy(targets).cuda()
    passes = distance.target_passes
    total, gradient, activations = _run_chain(distance, images, device_targets)
    assert distance.target_passes == passes + 1
    again_total, again_gradient, _ = _run_chain(distance, images, device_targets)
    assert distance.target_passes == passes + 1  # the same tensor, unmodified: the kept taps, no second target pass
    assert torch.equal(again_total, total) and torch.equal(again_gradient, gradient)
    for sample in range(2):  # a sample's bits do not depend on the batch it comes in
        alone_total, alone_gradient, alone_activations = _run_chain(distance, images[sample : sample + 1], device_targets[sample : sample + 1].clone())
        assert torch.equal(alone_total, total[sample : sample + 1]) and torch.equal(alone_gradient, gradient[sample : sample + 1])
        assert all(torch.equal(alone, both[sample : sample + 1]) for alone, both in zip(alone_activations, activations))
    passes = distance.target_passes
    _run_chain(distance, images, device_targets)
    assert distance.target_passes == passes + 1  # another tensor came in between
    _run_chain(distance, images, device_targets.clone())
    assert distance.target_passes == passes + 2  # equal values in another tensor: recomputed


# ---- through the projector ----


def test_projector_with_lpips_on_conv3x3() -> None:
    variables = sg2_spec.make_stress_variables(64, seed=3, fmap_base=sg2_spec.FMAP_BASE_CONFIG_E)
    targets = projection_ref.convergence_targets(variables, 64)
    distance = lpips.VGG16Lpips(lpips.random_lpips_weights(0), side=64, convolution="conv3x3")
    projector = Projector(num_steps=30, distance=distance, seed=0)
    projector.set_network((variables, 64))
    projector.start(targets)
    with torch.no_grad():
        _, distance0, _ = projector.loss_terms()
    terms = []
    while projector.get_cur_step() < projector.num_steps:
        projector.step()
        terms.append(torch.stack([projector.last_distance, projector.last_regularizer]))
    with torch.no_grad():
        _, distance1, _ = projector.loss_terms()
    distance0, distance1 = distance0.cpu().numpy(), distance1.cpu().numpy()
    print(f"projector with LPIPS on conv3x3, 64^2 config-e B=2 30 steps: distance {distance0} -> {distance1} (x {distance1 / distance0})")
    assert projector.get_cur_step() == 30 and bool(torch.isfinite(torch.stack(terms)).all())
    assert distance.target_passes == 1  # one `start`: one pass over the targets for 32 calls
    assert np.all(np.isfinite(distance1)) and np.all(distance1 < distance0), (distance0, distance1)
