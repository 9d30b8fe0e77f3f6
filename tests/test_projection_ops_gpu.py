"""
GPU tests of projection's kernels in isolation: the noise gradient of the layer epilogue
(gance_noise_bias_lrelu_backward_noise, synthesis_grad.hip), the noise regulariser and the pyramid distance (projection.hip),
each forward and backward against float64 autograd of the restatements in tests/projection_ref.py.

Error measure: max|got - ref64| / max|ref64| per tensor. The allowance is grad_ref.GRADIENT_BAR_FACTOR = 8 times the error of
the same restatement in float32 on the CPU on the same inputs (forward outputs of the epilogue keep the project's layer bar).
Every figure is printed before it is asserted.

Measured ratios of the kernels' error to the float32 restatement's (one MI355X; the bar is 8):
    noise gradient   grad_noise 0.56 ... 2.46 (errors 5e-8 ... 2.7e-7), grad_x bit-equal to noise_bias_lrelu_backward, out 1.0
    regulariser      reg 0.26 ... 1.00 (from side 8 up the very float the restatement gives), grad_noise 0.50 ... 1.55 (errors 4e-8 ... 1.5e-7)
    distance         dist 0.01 ... 1.00 (from 256^2 up the very float the restatement gives), grad_image 0.75 ... 1.00 (errors 1.2e-7 ... 1.8e-7)
The scalars (reg, dist) are accumulated in fp64 inside the kernels: the float32 restatement's own error on one number is a
matter of luck (7e-9 at R = 256, 6e-10 at R = 1024), and fp32 partial sums stood at 30 x that.
"""

from typing import Dict, Sequence, Tuple

import numpy as np
import pytest
import torch

import grad_ref
import projection_ref
from grad_ref import cuda
from gance_amd import torch_ops  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu


def judge_all(label: str, names: Sequence[str], got: Sequence[torch.Tensor], want64: Sequence[torch.Tensor], want32: Sequence[torch.Tensor]) -> None:
    """Every tensor against 8 x the float32 restatement's own error."""
    failures = []
    for index, name in enumerate(names):
        error = grad_ref.relative_error(got[index], want64[index])
        own = grad_ref.relative_error(want32[index], want64[index])
        bar = grad_ref.GRADIENT_BAR_FACTOR * own
        print(f"{label} {name}: error {error:.3e}, float32 restatement {own:.3e}, ratio {error / own if own else float('inf'):.2f}, bar {bar:.3e}")
        if not (np.isfinite(error) and error <= bar):
            failures.append(f"{name}: {error:.3e} > {bar:.3e}")
    assert not failures, f"{label}: " + "; ".join(failures)


# ---- the noise gradient ----

NOISE_SHAPES = [
    (batch, channels, side) for side in (4, 8, 66, 130) for channels in (16, 48, 512) for batch in (1, 3) if channels < 512 or side <= 8
] + [(1, 16, 1024)]


def _epilogue_inputs(batch: int, channels: int, side: int, per_sample: bool, negative: bool) -> Dict[str, np.ndarray]:
    inputs = dict(grad_ref.lrelu_inputs(batch, channels, side, batch if per_sample else 1, seed=side + channels + batch))
    if negative:  # the same pre-activations (still away from the kink) through a negative strength
        inputs["strength"], inputs["noise"] = -inputs["strength"], -inputs["noise"]
    return inputs


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("batch, channels, side", NOISE_SHAPES)
def test_noise_gradient(batch: int, channels: int, side: int, per_sample: bool) -> None:
    negative = (batch + channels // 16 + side + per_sample) % 2 == 1
    inputs = _epilogue_inputs(batch, channels, side, per_sample, negative)
    x, noise = cuda(inputs["x"], True), cuda(inputs["noise"], True)
    out = torch.ops.gance.noise_bias_lrelu(x, noise, cuda(inputs["strength"]), cuda(inputs["bias"]))
    grad_x, grad_noise = torch.autograd.grad(out, (x, noise), cuda(inputs["grad"]))
    assert grad_noise.shape == noise.shape
    assert torch.equal(grad_x, torch.ops.gance.noise_bias_lrelu_backward(cuda(inputs["grad"]), out.detach()))  # bit for bit
    label = f"noise gradient B={batch} C={channels} side={side} per_sample={per_sample} strength={float(inputs['strength'][0]):+.2f}"
    grad_ref.judge(label, ("out", "grad_x", "grad_noise"), (out, grad_x, grad_noise),
                   projection_ref.lrelu_noise_oracle(inputs, torch.float64), projection_ref.lrelu_noise_oracle(inputs, torch.float32))
    again = torch.autograd.grad(torch.ops.gance.noise_bias_lrelu(x, noise, cuda(inputs["strength"]), cuda(inputs["bias"])), (x, noise), cuda(inputs["grad"]))
    assert torch.equal(again[0], grad_x) and torch.equal(again[1], grad_noise)  # two runs, the same bits


def test_without_a_noise_gradient_the_path_is_the_old_one() -> None:
    inputs = _epilogue_inputs(3, 48, 8, False, False)
    x = cuda(inputs["x"], True)
    out = torch.ops.gance.noise_bias_lrelu(x, cuda(inputs["noise"]), cuda(inputs["strength"]), cuda(inputs["bias"]))
    (grad_x,) = torch.autograd.grad(out, x, cuda(inputs["grad"]))
    assert torch.equal(grad_x, torch.ops.gance.noise_bias_lrelu_backward(cuda(inputs["grad"]), out.detach()))
    noise = cuda(inputs["noise"], True)
    out = torch.ops.gance.noise_bias_lrelu(x, noise, cuda(inputs["strength"]), cuda(inputs["bias"]))
    assert torch.equal(torch.autograd.grad(out, (x, noise), cuda(inputs["grad"]))[0], grad_x)


# ---- the regulariser ----


def _regularizer_oracle(planes: np.ndarray, cotangent: np.ndarray, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    leaf = torch.from_numpy(planes).to(dtype).requires_grad_(True)
    reg = projection_ref.noise_regularizer(leaf)
    (grad,) = torch.autograd.grad(reg, leaf, torch.from_numpy(cotangent).to(dtype))
    return reg.detach(), grad


@pytest.mark.parametrize("batch, side", [(1, 4), (1, 8), (1, 16), (3, 16), (2, 64), (1, 1024)])
def test_noise_regularizer(batch: int, side: int) -> None:
    planes = projection_ref.smooth_planes(batch, side, seed=side + batch)
    cotangent = np.random.RandomState(side).uniform(0.5, 1.5, size=(batch,)).astype(np.float32)
    leaf = cuda(planes, True)
    reg = torch.ops.gance.noise_regularizer(leaf)
    (grad,) = torch.autograd.grad(reg, leaf, cuda(cotangent))
    assert reg.shape == (batch,) and grad.shape == leaf.shape
    judge_all(f"noise_regularizer B={batch} side={side}", ("reg", "grad_noise"), (reg, grad),
              _regularizer_oracle(planes, cotangent, torch.float64), _regularizer_oracle(planes, cotangent, torch.float32))
    (again,) = torch.autograd.grad(torch.ops.gance.noise_regularizer(leaf), leaf, cuda(cotangent))
    assert torch.equal(again, grad)


# ---- the distance ----


def _distance_oracle(image: np.ndarray, target: np.ndarray, cotangent: np.ndarray, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    leaf = torch.from_numpy(image).to(dtype).requires_grad_(True)
    dist = projection_ref.pyramid_distance(leaf, torch.from_numpy(target).to(dtype))
    (grad,) = torch.autograd.grad(dist, leaf, torch.from_numpy(cotangent).to(dtype))
    return dist.detach(), grad


@pytest.mark.parametrize("batch, resolution", [(1, 8), (1, 32), (3, 32), (1, 256), (1, 512), (1, 1024)])
def test_pyramid_distance(batch: int, resolution: int) -> None:
    image, target = projection_ref.distance_inputs(batch, resolution, seed=resolution + batch)
    cotangent = np.random.RandomState(resolution).uniform(0.5, 1.5, size=(batch,)).astype(np.float32)
    leaf = cuda(image, True)
    dist = torch.ops.gance.pyramid_distance(leaf, cuda(target))
    (grad,) = torch.autograd.grad(dist, leaf, cuda(cotangent))
    assert dist.shape == (batch,) and grad.shape == leaf.shape
    judge_all(f"pyramid_distance B={batch} R={resolution}", ("dist", "grad_image"), (dist, grad),
              _distance_oracle(image, target, cotangent, torch.float64), _distance_oracle(image, target, cotangent, torch.float32))
    (again,) = torch.autograd.grad(torch.ops.gance.pyramid_distance(leaf, cuda(target)), leaf, cuda(cotangent))
    assert torch.equal(again, grad)


def test_pyramid_distance_of_an_image_equal_to_its_target() -> None:
    """(image + 1) * 127.5 == target exactly in float32 (multiples of 1 / 255 * 2 do not survive; quarters do): distance and gradient are 0, finite."""
    levels = np.random.RandomState(0).randint(0, 9, size=(2, 3, 32, 32)).astype(np.float32)  # image = -1 + level / 4
    image = -1.0 + levels / 4.0
    target = (image + 1.0) * np.float32(127.5)
    leaf = cuda(image, True)
    dist = torch.ops.gance.pyramid_distance(leaf, cuda(target))
    (grad,) = torch.autograd.grad(dist.sum(), leaf)
    assert torch.equal(dist, torch.zeros_like(dist)) and torch.equal(grad, torch.zeros_like(grad))
    assert bool(torch.isfinite(dist).all()) and bool(torch.isfinite(grad).all())


def test_shape_checks() -> None:
    with pytest.raises(ValueError, match="power of two"):
        torch.ops.gance.noise_regularizer(torch.zeros((1, 1, 12, 12), device="cuda"))
    with pytest.raises(ValueError, match=r"\[B, 1, S, S\]"):
        torch.ops.gance.noise_regularizer(torch.zeros((1, 2, 8, 8), device="cuda"))
    with pytest.raises(ValueError, match="`target` must be"):
        torch.ops.gance.pyramid_distance(torch.zeros((1, 3, 512, 512), device="cuda"), torch.zeros((1, 3, 512, 512), device="cuda"))
    with pytest.raises(TypeError):
        torch.ops.gance.pyramid_distance(torch.zeros((1, 3, 8, 8), device="cuda"), torch.zeros((1, 3, 8, 8), device="cuda", dtype=torch.float64))
    with pytest.raises(RuntimeError):
        torch.ops.gance.noise_regularizer(torch.zeros((1, 1, 8, 8)))


def test_opcheck() -> None:
    """The four new ops: schema, fake tensors, autograd registration, AOT dispatch."""
    def rand(*shape: int, requires_grad: bool = False) -> torch.Tensor:
        return torch.randn(shape, dtype=torch.float32, device="cuda", requires_grad=requires_grad)

    planes = rand(2, 1, 16, 16, requires_grad=True)
    torch.library.opcheck(torch.ops.gance.noise_regularizer.default, (planes,))
    torch.library.opcheck(torch.ops.gance.noise_regularizer_backward.default, (rand(2), planes.detach()))
    image, target = rand(2, 3, 16, 16, requires_grad=True), rand(2, 3, 16, 16) * 50 + 128
    torch.library.opcheck(torch.ops.gance.pyramid_distance.default, (image, target))
    torch.library.opcheck(torch.ops.gance.pyramid_distance_backward.default, (rand(2), image.detach(), target))
    # (away from the kink, as in test_synthesis_grad_gpu.py)
    pre = (rand(2, 16, 4, 4).abs() + 0.1) * torch.where(rand(2, 16, 4, 4) > 0, 1.0, -1.0)
    strength, bias = torch.full((1,), 0.01, device="cuda"), torch.zeros((16,), device="cuda")
    for noise_batch in (1, 2):
        noise = (rand(noise_batch, 1, 4, 4) * 0.1).requires_grad_(True)
        torch.library.opcheck(torch.ops.gance.noise_bias_lrelu.default, (pre.clone().requires_grad_(True), noise, strength, bias))
        out = torch.ops.gance.noise_bias_lrelu(pre, noise, strength, bias).detach()
        torch.library.opcheck(torch.ops.gance.noise_bias_lrelu_backward_noise.default, (torch.randn_like(out), out, strength, noise_batch))
