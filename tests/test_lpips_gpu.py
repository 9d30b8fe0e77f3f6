"""
GPU tests of LPIPS on VGG16 (gance_amd/csrc/lpips.hip, the gance::lpips_input / bias_relu / bias_relu_pool / lpips_layer /
lpips_normalize ops, gance_amd/stylegan2/lpips.py): every op forward and backward against float64 autograd of the restatement
in tests/lpips_ref.py, the whole chain through `VGG16Lpips`, and the distance inside the projector and the file writer.

Error measure: max|got - ref64| / max|ref64| per tensor. The allowance of a gradient (and of the head's distance) is
grad_ref.GRADIENT_BAR_FACTOR = 8 times the error of the same restatement in float32 on the CPU on the same inputs; forward
activations keep grad_ref.LAYER_BAR. The whole chain's distance is judged against the LARGEST float32 own error over all
whole-chain cases (lpips_ref.distance_yardstick). Every figure is printed before it is asserted.

Measured ratios of the kernels' error to the float32 restatement's (one MI355X; the bar is 8):
    input            grad_image 1.00 ... 1.30 (errors 4e-8 ... 7e-8)
    bias/ReLU(/pool) y, p and grad_x the very bits of the float32 restatement, at every (C, side) named below
    head             dist 0.07 ... 1.00, grad_f 0.37 ... 1.99, normalise 0.32 ... 1.19 (errors up to 1.4e-7, bar 2e-5);
                     all-zero pixels alone 0.58 ... 1.29, the other pixels 0.48 ... 1.08
    whole chain      activations 2.0e-7 ... 7.9e-7 of their maximum (bar 2e-5); 0 ... 2 masks and selections differ per whole input (cap 8);
                     image gradient 0.86 ... 1.34 (1.7e-6 ... 2.4e-6); distance 0.01 ... 0.78 of the largest float32 own error (1.4e-7)
    projector        30 steps at 64^2 config-e, B = 2: LPIPS at the unperturbed w and the current planes 0.0161 -> 0.0075 and 0.0224 -> 0.0058
                     (x 0.46 and x 0.26; the planes are optimised too)
"""

from pathlib import Path
from typing import List, Tuple

import numpy as np
import pytest
import torch

import grad_ref
import lpips_ref
import projection_ref
from grad_ref import cuda
from gance_amd import network_file, torch_ops  # noqa: F401  pylint: disable=unused-import
from gance_amd.projection import projection_file_reader as reader_module
from gance_amd.projection.projector_file_writer import project_video_to_file
from gance_amd.stylegan2 import lpips
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.stylegan2.projector import Projector
from gance_amd.video.mjpeg_avi import MjpegAviWriter

pytestmark = pytest.mark.gpu


def judge(label: str, name: str, got: torch.Tensor, want64: torch.Tensor, want32: torch.Tensor, failures: List[str], bar: float = 0.0) -> None:
    """One tensor against `bar`, or (bar 0) against 8 x the float32 restatement's own error."""
    error = grad_ref.relative_error(got, want64)
    own = grad_ref.relative_error(want32, want64)
    limit = bar if bar else grad_ref.GRADIENT_BAR_FACTOR * own
    print(f"{label} {name}: error {error:.3e}, float32 restatement {own:.3e}, ratio {error / own if own else float('inf'):.2f}, bar {limit:.3e}")
    if not (np.isfinite(error) and error <= limit):
        failures.append(f"{name}: {error:.3e} > {limit:.3e}")


# ---- the input op ----


def _input_reference(image: np.ndarray, cotangent: np.ndarray, side: int, weights: lpips.LpipsWeights, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    leaf = lpips_ref.as_tensor(image, dtype).requires_grad_(True)
    out = lpips_ref.preprocess(leaf, side, weights)
    (gradient,) = torch.autograd.grad(out, leaf, lpips_ref.as_tensor(cotangent[:, :3], dtype))
    return out.detach(), gradient


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("resolution", [64, 128, 192])
def test_input_op(batch: int, resolution: int) -> None:
    side = 64
    rng = np.random.RandomState(resolution + batch)
    weights = lpips_ref.chain_weights(0)
    image = rng.uniform(-1, 1, size=(batch, 3, resolution, resolution)).astype(np.float32)
    cotangent = rng.randn(batch, 16, side, side).astype(np.float32)  # (channels 3 ... 15 must not reach the image)
    leaf = cuda(image, True)
    out = torch.ops.gance.lpips_input(leaf, cuda(weights.shift), cuda(weights.scale), side)
    (gradient,) = torch.autograd.grad(out, leaf, cuda(cotangent))
    assert out.shape == (batch, 16, side, side) and gradient.shape == leaf.shape
    assert float(out.detach()[:, 3:].abs().max()) == 0.0
    want64, want32 = (_input_reference(image, cotangent, side, weights, dtype) for dtype in (torch.float64, torch.float32))
    failures: List[str] = []
    label = f"lpips_input B={batch} R={resolution}"
    judge(label, "out", out[:, :3], want64[0], want32[0], failures, bar=grad_ref.LAYER_BAR)
    judge(label, "grad_image", gradient, want64[1], want32[1], failures)
    assert not failures, f"{label}: " + "; ".join(failures)


# ---- bias + ReLU (+ pool) ----

RELU_SHAPES = [(batch, channels, side, pool) for channels in (16, 48, 512) for side, pool in [(4, True), (10, True), (34, True), (64, True), (130, True), (5, False), (33, False)]
               for batch in (1, 3)]  # fmt: skip


def _relu_reference(x: np.ndarray, bias: np.ndarray, grad_y: np.ndarray, grad_p: np.ndarray, pool: bool, dtype: torch.dtype):  # type: ignore[no-untyped-def]
    leaf = lpips_ref.as_tensor(x, dtype).requires_grad_(True)
    y = lpips_ref.bias_relu(leaf + lpips_ref.as_tensor(bias, dtype).reshape(1, -1, 1, 1))
    if not pool:
        (gradient,) = torch.autograd.grad(y, leaf, lpips_ref.as_tensor(grad_y, dtype))
        return y.detach(), None, gradient
    p = lpips_ref.max_pool(y)
    (gradient,) = torch.autograd.grad((y, p), leaf, (lpips_ref.as_tensor(grad_y, dtype), lpips_ref.as_tensor(grad_p, dtype)))
    return y.detach(), p.detach(), gradient


@pytest.mark.parametrize("batch, channels, side, pool", RELU_SHAPES)
def test_bias_relu_ops(batch: int, channels: int, side: int, pool: bool) -> None:
    rng = np.random.RandomState(channels + side + batch)
    x = rng.randn(batch, channels, side, side).astype(np.float32)
    bias = rng.randn(channels).astype(np.float32)
    if pool:  # by hand: a window with two equal positive maxima (the first in row-major order is selected), and one that is all zero
        bias[1:4] = (0.5, 0.125, -0.25)  # (dyadic: (value - bias) + bias comes back exactly)
        x[0, 1, 0:2, 2:4] = np.array([[0.25, 1.5], [1.5, -3.0]], dtype=np.float32) - bias[1]
        x[-1, 3, 2:4, 0:2] = np.array([[0.5, 0.125], [2.0, 2.0]], dtype=np.float32) - bias[3]
        x[0, 2, 0:2, 0:2] = -5.0
    grad_y = rng.randn(batch, channels, side, side).astype(np.float32)
    grad_p = rng.randn(batch, channels, side // 2, side // 2).astype(np.float32)
    leaf = cuda(x, True)
    if pool:
        y, p = torch.ops.gance.bias_relu_pool(leaf, cuda(bias))
        (gradient,) = torch.autograd.grad((y, p), leaf, (cuda(grad_y), cuda(grad_p)))
    else:
        y, p = torch.ops.gance.bias_relu(leaf, cuda(bias)), None
        (gradient,) = torch.autograd.grad(y, leaf, cuda(grad_y))
    want_y, want_p, want_gradient = _relu_reference(x, bias, grad_y, grad_p, pool, torch.float32)
    # masks and selections are functions of the same float32 inputs on both sides: no flip allowance, and y and p are exact
    assert torch.equal(y.detach().cpu(), want_y)
    if pool:
        assert p is not None and torch.equal(p.detach().cpu(), want_p)
        assert float(want_y[0, 1, 0, 3]) == float(want_y[0, 1, 1, 2]) == 1.5 and float(want_y[-1, 3, 3, 0]) == float(want_y[-1, 3, 3, 1]) == 2.0
        got = gradient.cpu().numpy()
        assert got[0, 1, 0, 3] == grad_y[0, 1, 0, 3] + grad_p[0, 1, 0, 1] and got[0, 1, 1, 2] == grad_y[0, 1, 1, 2]  # the first of the two 1.5
        assert got[0, 1, 0, 2] == grad_y[0, 1, 0, 2] and got[0, 1, 1, 3] == 0.0
        assert got[-1, 3, 3, 0] == grad_y[-1, 3, 3, 0] + grad_p[-1, 3, 1, 0] and got[-1, 3, 3, 1] == grad_y[-1, 3, 3, 1]  # the first of the two 2.0
        assert float(np.abs(got[0, 2, 0:2, 0:2]).max()) == 0.0
    # a sum of two float32 numbers, or one of them, or zero: the float32 restatement gives the very bits
    assert torch.equal(gradient.cpu(), want_gradient)
    want64 = _relu_reference(x, bias, grad_y, grad_p, pool, torch.float64)
    failures: List[str] = []
    judge(f"bias_relu B={batch} C={channels} S={side} pool={pool}", "grad_x", gradient, want64[2], want_gradient, failures)
    assert not failures, "; ".join(failures)
    again = torch.ops.gance.bias_relu_pool_backward(cuda(grad_y), cuda(grad_p), y.detach()) if pool else torch.ops.gance.bias_relu_backward(cuda(grad_y), y.detach())
    assert torch.equal(again, gradient)


# ---- the head and the normalise op ----

HEAD_SHAPES = [(batch, channels, side) for channels in (16, 64, 512) for side in (4, 9, 33, 64) for batch in (1, 3)]


def _head_inputs(batch: int, channels: int, side: int, zero_block: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    rng = np.random.RandomState(7 * channels + side + batch)
    f = np.maximum(rng.randn(batch, channels, side, side), 0).astype(np.float32)  # post-ReLU: half of the entries are zero
    target = np.maximum(rng.randn(batch, channels, side, side), 0).astype(np.float32)
    if zero_block:
        f[:, :, 1:3, 0:3] = 0.0
    lin = (0.1 * np.abs(rng.randn(channels))).astype(np.float32)
    return f, target, lin, rng.uniform(0.5, 1.5, size=batch).astype(np.float32)


def _head_reference(f: np.ndarray, target: np.ndarray, lin: np.ndarray, cotangent: np.ndarray, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    leaf = lpips_ref.as_tensor(f, dtype).requires_grad_(True)
    dist = lpips_ref.layer_distance(leaf, lpips_ref.normalize(lpips_ref.as_tensor(target, dtype)), lpips_ref.as_tensor(lin, dtype))
    (gradient,) = torch.autograd.grad(dist, leaf, lpips_ref.as_tensor(cotangent, dtype))
    return dist.detach(), gradient


@pytest.mark.parametrize("batch, channels, side", HEAD_SHAPES)
def test_head_and_normalize_ops(batch: int, channels: int, side: int) -> None:
    f, target, lin, cotangent = _head_inputs(batch, channels, side)
    label = f"lpips_layer B={batch} C={channels} S={side}"
    failures: List[str] = []
    normalized = torch.ops.gance.lpips_normalize(cuda(target))
    want_normalized = [lpips_ref.normalize(lpips_ref.as_tensor(target, dtype)) for dtype in (torch.float64, torch.float32)]
    judge(label, "normalize", normalized, want_normalized[0], want_normalized[1], failures, bar=grad_ref.LAYER_BAR)
    leaf = cuda(f, True)
    dist = torch.ops.gance.lpips_layer(leaf, normalized, cuda(lin))
    (gradient,) = torch.autograd.grad(dist, leaf, cuda(cotangent))
    assert dist.shape == (batch,) and gradient.shape == leaf.shape
    want64, want32 = (_head_reference(f, target, lin, cotangent, dtype) for dtype in (torch.float64, torch.float32))
    judge(label, "dist", dist, want64[0], want32[0], failures)
    judge(label, "grad_f", gradient, want64[1], want32[1], failures)
    assert not failures, f"{label}: " + "; ".join(failures)
    (again,) = torch.autograd.grad(torch.ops.gance.lpips_layer(leaf, normalized, cuda(lin)), leaf, cuda(cotangent))
    assert torch.equal(again, gradient)  # one fixed summation order
    # the features against their own normalisation: zero to the bit, and a zero gradient
    own = torch.ops.gance.lpips_layer(leaf, torch.ops.gance.lpips_normalize(leaf.detach()), cuda(lin))
    (own_gradient,) = torch.autograd.grad(own, leaf, cuda(cotangent))
    assert float(own.detach().abs().max()) == 0.0 and float(own_gradient.abs().max()) == 0.0


@pytest.mark.parametrize("batch, channels, side", [(1, 16, 4), (3, 64, 9), (1, 512, 33), (3, 64, 64), (1, 512, 64)])
def test_head_with_all_zero_pixels(batch: int, channels: int, side: int) -> None:
    """A block of pixels whose features are all zero, judged on its own: its gradients are of the order 1 / 1e-10."""
    f, target, lin, cotangent = _head_inputs(batch, channels, side, zero_block=True)
    label = f"lpips_layer with zero pixels B={batch} C={channels} S={side}"
    normalized_f = torch.ops.gance.lpips_normalize(cuda(f))
    assert float(normalized_f[:, :, 1:3, 0:3].abs().max()) == 0.0 and bool(torch.isfinite(normalized_f).all())
    leaf = cuda(f, True)
    dist = torch.ops.gance.lpips_layer(leaf, torch.ops.gance.lpips_normalize(cuda(target)), cuda(lin))
    (gradient,) = torch.autograd.grad(dist, leaf, cuda(cotangent))
    assert bool(torch.isfinite(gradient).all()) and bool(torch.isfinite(dist).all())
    want64, want32 = (_head_reference(f, target, lin, cotangent, dtype) for dtype in (torch.float64, torch.float32))
    failures: List[str] = []
    judge(label, "dist", dist, want64[0], want32[0], failures)
    judge(label, "grad_f, the zero pixels", gradient[:, :, 1:3, 0:3], want64[1][:, :, 1:3, 0:3], want32[1][:, :, 1:3, 0:3], failures)
    rest = torch.ones((side, side), dtype=torch.bool)
    rest[1:3, 0:3] = False
    judge(label, "grad_f, the other pixels", gradient[:, :, rest.cuda()], want64[1][:, :, rest], want32[1][:, :, rest], failures)
    assert float(want64[1][:, :, 1:3, 0:3].abs().max()) > 1e3 * float(want64[1][:, :, rest].abs().max())
    assert not failures, f"{label}: " + "; ".join(failures)


def test_ops_refuse_bad_tensors_and_pass_opcheck() -> None:
    rand = lambda *shape: torch.randn(shape, device="cuda")  # noqa: E731
    with pytest.raises(ValueError):
        torch.ops.gance.bias_relu_pool(rand(1, 16, 5, 5), rand(16))  # odd side with pool
    with pytest.raises(ValueError):
        torch.ops.gance.bias_relu(rand(1, 20, 4, 4), rand(20))
    with pytest.raises(ValueError):
        torch.ops.gance.bias_relu(rand(1, 16, 4, 6), rand(16))
    with pytest.raises(ValueError):
        torch.ops.gance.lpips_input(rand(1, 3, 96, 96), rand(3), rand(3), 64)
    with pytest.raises(TypeError):  # (a dtype is a TypeError in every gance op)
        torch.ops.gance.lpips_layer(rand(1, 16, 4, 4), rand(1, 16, 4, 4).double(), rand(16))
    with pytest.raises(ValueError):
        torch.ops.gance.lpips_layer(rand(1, 16, 4, 4), rand(1, 16, 8, 8), rand(16))
    image = rand(2, 3, 128, 128).requires_grad_(True)
    torch.library.opcheck(torch.ops.gance.lpips_input.default, (image, rand(3), rand(3).abs() + 0.5, 64))
    torch.library.opcheck(torch.ops.gance.lpips_input_backward.default, (rand(2, 16, 64, 64), rand(3).abs() + 0.5, 128))
    x = rand(2, 32, 6, 6).requires_grad_(True)
    torch.library.opcheck(torch.ops.gance.bias_relu.default, (x, rand(32)))
    torch.library.opcheck(torch.ops.gance.bias_relu_pool.default, (x, rand(32)))
    y = torch.relu(x.detach())
    torch.library.opcheck(torch.ops.gance.bias_relu_backward.default, (rand(2, 32, 6, 6), y))
    torch.library.opcheck(torch.ops.gance.bias_relu_pool_backward.default, (rand(2, 32, 6, 6), rand(2, 32, 3, 3), y))
    normalized = torch.ops.gance.lpips_normalize(rand(2, 32, 6, 6).abs())
    torch.library.opcheck(torch.ops.gance.lpips_normalize.default, (y,))
    torch.library.opcheck(torch.ops.gance.lpips_layer.default, (y.clone().requires_grad_(True), normalized, rand(32).abs()))
    torch.library.opcheck(torch.ops.gance.lpips_layer_backward.default, (rand(2), y, normalized, rand(32).abs()))


# ---- the whole chain ----


def _run_chain(distance: lpips.VGG16Lpips, images: np.ndarray, targets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
    leaf = cuda(images, True)
    collected: List[torch.Tensor] = []
    total = distance(leaf, targets, collect=collected)
    (gradient,) = torch.autograd.grad(total.sum(), leaf)
    return total.detach(), gradient, [activation.detach() for activation in collected]


@pytest.fixture(scope="module")
def chain_callables():  # type: ignore[no-untyped-def]
    return {seed: lpips.VGG16Lpips(lpips_ref.chain_weights(seed), side=lpips_ref.CHAIN_SIDE, device=0) for seed in lpips_ref.CHAIN_SEEDS}


@pytest.mark.parametrize("seed, resolution, batch", lpips_ref.CHAIN_CASES)
def test_whole_chain(chain_callables, seed: int, resolution: int, batch: int) -> None:  # type: ignore[no-untyped-def]
    label = f"chain seed {seed} R {resolution} B {batch}"
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
    kept = device_targets.clone()
    first_total, _, _ = _run_chain(distance, images, kept)
    passes = distance.target_passes
    kept[0] = kept[1]  # in place: the version counter moves
    moved_total, _, _ = _run_chain(distance, images, kept)
    assert distance.target_passes == passes + 1
    assert float(moved_total[0]) != float(first_total[0]) and float(moved_total[1]) == float(first_total[1])
    with pytest.raises(ValueError):
        distance(cuda(images), device_targets[:1])
    with pytest.raises(ValueError):
        distance(torch.zeros((1, 3, 96, 96), device="cuda"), torch.zeros((1, 96, 96, 3), dtype=torch.uint8, device="cuda"))  # above the side, no multiple


# ---- through the projector and the file writer ----


@pytest.fixture(scope="module")
def stress64():  # type: ignore[no-untyped-def]
    variables = sg2_spec.make_stress_variables(64, seed=3, fmap_base=sg2_spec.FMAP_BASE_CONFIG_E)
    return variables, projection_ref.convergence_targets(variables, 64)


def test_projector_with_lpips(stress64) -> None:  # type: ignore[no-untyped-def]
    variables, targets = stress64
    distance = lpips.VGG16Lpips(lpips.random_lpips_weights(0), side=64)
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
    print(f"projector with LPIPS 64^2 config-e B=2 30 steps: distance {distance0} -> {distance1} (x {distance1 / distance0})")
    assert projector.get_cur_step() == 30 and bool(torch.isfinite(torch.stack(terms)).all())
    assert distance.target_passes == 1  # one `start`: one pass over the targets for 32 calls
    assert np.all(np.isfinite(distance1)) and np.all(distance1 < distance0), (distance0, distance1)


def test_video_to_projection_file_with_lpips(tmp_path: Path, stress64) -> None:  # type: ignore[no-untyped-def]
    from gance_amd.network_interface.network_functions import LoadedNetwork  # pylint: disable=import-outside-toplevel

    variables, _ = stress64
    side, steps = 64, 10
    network_path, video_path, projection_path = tmp_path / "network.pkl", tmp_path / "frames.avi", tmp_path / "projection.npz"
    network_file.save_network(network_path, side, variables)
    network = LoadedNetwork(network_path, max_batch=4)
    try:
        dlatents = np.random.RandomState(6).randn(3, 1, 512).astype(np.float32).repeat(network.engine.num_layers, axis=1)
        frames = network.create_images_matrix(dlatents)
        data, offsets = torch.ops.gance.jpeg_encode(torch.from_numpy(frames).cuda(), 95)
        data, offsets = data.cpu().numpy(), offsets.cpu().numpy()
        with MjpegAviWriter(video_path, side, 30.0) as writer:
            for index in range(3):
                writer.add_frame(data[offsets[index] : offsets[index + 1]].tobytes())
        distance = lpips.VGG16Lpips(lpips.random_lpips_weights(0), side=64)
        project_video_to_file(video_path, network_path, projection_path, steps_per_projection=steps, frames_per_batch=2, distance=distance)
        assert distance.target_passes == 2  # two batches
        with reader_module.ProjectionFileReader(projection_path) as reader:
            attributes = reader.projection_attributes
            assert attributes.complete is True and attributes.steps_in_projection == steps
            assert attributes.projection_frame_count == 3 and attributes.original_frame_count == 3
            assert attributes.original_fps == 30.0 and attributes.projection_fps == 30.0
            assert list(attributes.original_width_height) == [side, side] and list(attributes.projection_width_height) == [side, side]
            assert attributes.original_target_path == str(video_path) and attributes.original_network_path == str(network_path)
            assert attributes.latents_histories_enabled is True
            latents = np.stack(list(reader.final_latents))
            finals, targets = np.stack(list(reader.final_images)), np.stack(list(reader.target_images))
            histories = [np.stack(list(history)) for history in reader.latents_histories]
        assert latents.shape == (3, network.engine.num_layers, 512) and finals.shape == targets.shape == (3, side, side, 3)
        assert [history.shape for history in histories] == [(steps, network.engine.num_layers, 512)] * 3
        assert all(np.array_equal(history[-1], latents[index]) for index, history in enumerate(histories))
        assert np.isfinite(latents).all()
        reader_module.verify_projection_file_assumptions(projection_path)
    finally:
        network.stop()
