"""
GPU tests of differentiable synthesis: the three ops of gance_amd/csrc/synthesis_grad.hip in isolation (forward and every
gradient against the float64 autograd of the oracle's own layer functions), `torch.library.opcheck`, and the whole chain
(gance_amd/stylegan2/differentiable.py) against the float64 oracle, the engine and the sign-injected helper of
tests/grad_ref.py.

Error measure: max|got - ref64| / max|ref64| per tensor; for dlatent gradients per dlatent row, the worst row. Forward bars
are the project's (2e-5 of a layer's maximum, 1e-4 for the image). A gradient's bar is 8 x the error of the ORACLE IN FLOAT32
on the CPU on the same inputs, computed here (grad_ref.GRADIENT_BAR_FACTOR says why 8). Every figure is printed before it
is asserted.
"""

import numpy as np
import pytest
import torch

import grad_ref
from grad_ref import cuda, judge, lrelu_inputs, lrelu_oracle, run_chain
from gance_amd import hip_lib, torch_ops  # noqa: F401  pylint: disable=unused-import
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.stylegan2.differentiable import DifferentiableSynthesis

pytestmark = pytest.mark.gpu


MODCONV_SHAPES = [(False, 4), (False, 8), (False, 32), (True, 4), (True, 8), (True, 16)]  # (up, input side)
CHANNEL_PAIRS = [(16, 16), (32, 16), (16, 48), (512, 256)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("cin, cout", CHANNEL_PAIRS)
@pytest.mark.parametrize("up, side", MODCONV_SHAPES)
def test_modconv3x3_forward_and_gradients(up: bool, side: int, cin: int, cout: int, batch: int) -> None:
    inputs = grad_ref.modconv_inputs(batch, cin, cout, side, up, seed=side + cin + 7 * cout + batch)
    want64 = grad_ref.modconv_oracle(inputs, up, torch.float64)
    want32 = grad_ref.modconv_oracle(inputs, up, torch.float32)
    x, style, demod = cuda(inputs["x"], True), cuda(inputs["style"], True), cuda(inputs["demod"], True)
    y = torch.ops.gance.modconv3x3(x, style, demod, cuda(grad_ref.scaled_weight(inputs["weight"])), up)
    grads = torch.autograd.grad(y, (x, style, demod), cuda(inputs["grad_y"]))
    assert y.shape == want64[0].shape
    judge(f"modconv3x3 up={up} side={side} {cin}->{cout} B={batch}", ("y", "grad_x", "grad_style", "grad_demod"), (y, *grads), want64, want32)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("batch, channels, side", [(1, 16, 4), (3, 48, 9), (2, 32, 32)])
def test_noise_bias_lrelu_forward_and_gradient(batch: int, channels: int, side: int, per_sample: bool) -> None:
    inputs = lrelu_inputs(batch, channels, side, batch if per_sample else 1, seed=side + channels)
    x = cuda(inputs["x"], True)
    out = torch.ops.gance.noise_bias_lrelu(x, cuda(inputs["noise"]), cuda(inputs["strength"]), cuda(inputs["bias"]))
    (grad,) = torch.autograd.grad(out, x, cuda(inputs["grad"]))
    judge(f"noise_bias_lrelu B={batch} C={channels} side={side} per_sample={per_sample}", ("out", "grad_x"), (out, grad),
          lrelu_oracle(inputs, torch.float64), lrelu_oracle(inputs, torch.float32))


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("batch, cin, side", [(1, 16, 4), (3, 48, 8), (2, 512, 32)])
def test_torgb_skip_forward_and_gradients(batch: int, cin: int, side: int, with_prev: bool) -> None:
    inputs = grad_ref.torgb_inputs(batch, cin, side, with_prev, seed=side + cin)
    want64, want32 = grad_ref.torgb_oracle(inputs, torch.float64), grad_ref.torgb_oracle(inputs, torch.float32)
    x, style = cuda(inputs["x"], True), cuda(inputs["style"], True)
    y_prev = cuda(inputs["y_prev"], True) if with_prev else None
    weight = cuda(grad_ref.scaled_weight(inputs["weight"]).reshape(cin, 3))
    y = torch.ops.gance.torgb_skip(x, style, weight, cuda(inputs["bias"]), y_prev)
    leaves = (x, style, y_prev) if with_prev else (x, style)
    grads = torch.autograd.grad(y, leaves, cuda(inputs["grad_y"]))
    names = ("y", "grad_x", "grad_style", "grad_y_prev")[: 1 + len(leaves)]
    judge(f"torgb_skip B={batch} {cin} side={side} prev={with_prev}", names, (y, *grads), want64, want32)


def test_opcheck() -> None:
    """Every op and backward op at its smallest shape: schema, fake tensors, autograd registration, AOT dispatch."""
    def rand(*shape: int, requires_grad: bool = False) -> torch.Tensor:
        return torch.randn(shape, dtype=torch.float32, device="cuda", requires_grad=requires_grad)

    x, style, weight = rand(1, 16, 4, 4, requires_grad=True), rand(1, 16, requires_grad=True), rand(3, 3, 16, 16)
    demod = (rand(1, 16).abs() + 0.1).requires_grad_(True)
    for up in (False, True):
        torch.library.opcheck(torch.ops.gance.modconv3x3.default, (x, style, demod, weight, up))
        y = torch.ops.gance.modconv3x3(x, style, demod, weight, up).detach()
        torch.library.opcheck(torch.ops.gance.modconv3x3_backward.default, (torch.randn_like(y), x.detach(), y, style.detach(), demod.detach(), weight, up))
    # (away from the kink: opcheck compares runs, and a pre-activation at zero is no place for that)
    pre = (rand(1, 16, 4, 4).abs() + 0.1) * torch.where(rand(1, 16, 4, 4) > 0, 1.0, -1.0)
    noise, strength, bias = torch.zeros((1, 1, 4, 4), device="cuda"), torch.zeros((1,), device="cuda"), torch.zeros((16,), device="cuda")
    torch.library.opcheck(torch.ops.gance.noise_bias_lrelu.default, (pre.requires_grad_(True), noise, strength, bias))
    out = torch.ops.gance.noise_bias_lrelu(pre, noise, strength, bias).detach()
    torch.library.opcheck(torch.ops.gance.noise_bias_lrelu_backward.default, (torch.randn_like(out), out))
    rgb_weight, rgb_bias = rand(16, 3), rand(3)
    for y_prev in (None, rand(1, 3, 2, 2, requires_grad=True)):
        torch.library.opcheck(torch.ops.gance.torgb_skip.default, (x, style, rgb_weight, rgb_bias, y_prev))
        torch.library.opcheck(torch.ops.gance.torgb_skip_backward.default, (rand(1, 3, 4, 4), x.detach(), style.detach(), rgb_weight, y_prev is not None))


@pytest.mark.parametrize("name", grad_ref.CASE_NAMES)
def test_whole_chain(name: str) -> None:
    grad_ref.check_whole_chain(name)


def test_backward_is_repeatable() -> None:
    """No atomics, every sum in one order: two backward passes of one case give identical bits."""
    case = grad_ref.case("stress-32-f")
    synthesis = DifferentiableSynthesis(case.variables, case.resolution, fmap_base=case.fmap_base, device=0)
    first, second = run_chain(synthesis, case), run_chain(synthesis, case)
    assert torch.equal(first[0], second[0]) and torch.equal(first[2], second[2])
    assert float(first[2].abs().max()) > 0


def test_noise_override_and_argument_checks() -> None:
    case = grad_ref.case("perturb-16-f")
    synthesis = DifferentiableSynthesis(case.variables, case.resolution, device=0)
    dlatents = cuda(case.dlatents)
    planes = np.random.RandomState(5).randn(2, 1, 8, 8).astype(np.float32)
    with torch.no_grad():
        image = synthesis(dlatents, noise={1: planes})
        want = grad_ref.ref.g_synthesis(torch.from_numpy(case.dlatents).double(), case.variables, 16, noise_override={1: torch.from_numpy(planes)})
    error = grad_ref.relative_error(image, want)
    print(f"per-sample noise override: image error {error:.3e}")
    assert error <= grad_ref.IMAGE_BAR
    assert grad_ref.relative_error(image, case.image64) > 1e-3  # (the override is used)
    with pytest.raises(ValueError):
        synthesis(dlatents[:, :-1])
    with pytest.raises(ValueError):
        synthesis(dlatents, noise={1: planes[:, :, :4]})
    with pytest.raises(ValueError):
        synthesis(dlatents.cpu())


def test_loaded_network_builds_it(tmp_path) -> None:  # type: ignore[no-untyped-def]
    from gance_amd import network_file  # pylint: disable=import-outside-toplevel
    from gance_amd.network_interface.network_functions import LoadedNetwork  # pylint: disable=import-outside-toplevel

    case = grad_ref.case("perturb-16-f")
    path = tmp_path / "network.pkl"
    network_file.save_network(path, case.resolution, case.variables)
    network = LoadedNetwork(path, max_batch=2, device=0)
    try:
        synthesis = network.differentiable()
        with torch.no_grad():
            image = synthesis(cuda(case.dlatents))
    finally:
        network.stop()
    assert grad_ref.relative_error(image, case.image64) <= grad_ref.IMAGE_BAR


def test_full_size() -> None:
    """
    1024^2, one frame: shapes, finiteness, repeatability, and the image against the engine (the float64 oracle is too slow here).
    The gradient is compared with nothing here. What stands for it is in tests/test_synthesis_grad_sizes_gpu.py: the isolated
    ops at the 512^2 and 1024^2 shapes of this chain against the float64 oracle (where a position sum runs its 64 segments), and
    the whole config-e chain up to 256^2. No float64 whole-chain gradient exists at 1024^2.
    """
    resolution = 1024
    variables = sg2_spec.make_random_variables(resolution, seed=3, perturb=True)
    synthesis = DifferentiableSynthesis(variables, resolution, device=0)
    rng = np.random.RandomState(11)
    dlatents = rng.randn(1, synthesis.num_layers, 512).astype(np.float32)
    cotangent = cuda(rng.randn(1, 3, resolution, resolution).astype(np.float32))
    results = []
    for _ in range(2):
        d_dlatents = cuda(dlatents, True)
        image = synthesis(d_dlatents)
        (gradient,) = torch.autograd.grad(image, d_dlatents, cotangent)
        results.append((image.detach(), gradient))
    image, gradient = results[0]
    assert image.shape == (1, 3, resolution, resolution) and gradient.shape == (1, synthesis.num_layers, 512)
    assert bool(torch.isfinite(image).all()) and bool(torch.isfinite(gradient).all())
    assert float(gradient.abs().amax(dim=2).min()) > 0  # every dlatent row reaches the image
    assert torch.equal(image, results[1][0]) and torch.equal(gradient, results[1][1])
    engine = hip_lib.Engine(variables, resolution, max_batch=1, device=0)
    try:
        _, engine_image = engine.synthesize_w(dlatents, want_float=True)
    finally:
        engine.close()
    error = grad_ref.relative_error(image, torch.from_numpy(engine_image).double())
    print(f"1024^2 image against the engine: {error:.3e}")
    assert error <= grad_ref.IMAGE_BAR
