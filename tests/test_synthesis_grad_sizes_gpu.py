"""
GPU tests of differentiable synthesis at the sizes where its position sums split (gance_amd/csrc/synthesis_grad.hip): the
method, measure and bars of tests/test_synthesis_grad_gpu.py (forward output and every gradient against the float64 autograd of
the oracle's own layer functions, max|got - ref64| / max|ref64| per tensor, 2e-5 for the forward tensor, 8 x the float32 CPU
oracle's own error on the same inputs for a gradient, every figure printed before it is asserted), at the shapes that module
leaves out:

- `plane_dot_kernel` + `plane_finish_kernel` (grad_style, grad_demod, grad_x = g * style) run min(64, ceil(positions / 4096))
  segments per plane: one segment up to 64^2, two uneven ones at 65^2, exactly 64 of 4096 at 512^2, 64 of 4225 with a shorter
  last one at 520^2, 64 of 16384 at 1024^2;
- `contract_kernel` on the (2 side + 1)^2 intermediate up to 1025^2, forward (zero-inserted) and backward (stride 2), pixel
  counts that are no multiple of 64, the 32-channel (MT = 2) form as a forward form, K = 128 in 8 chunks;
- the channel pairs of the 128^2 ... 1024^2 layers of both configurations at their own sides.

The whole chain runs at 128^2 and 256^2 config-e (grad_ref.LARGE_CASE_NAMES) through the body of the sibling's test_whole_chain;
the cap on sign flips is grad_ref.sign_flip_cap: the density of 8 per 5 578 752 activations, rounded down (11 and 23).

Measured on one MI355X, smallest ... largest over a group's cases (error = the kernels', oracle = the float32 CPU oracle's own
error on the same inputs, ratio = error / oracle per case and tensor; the bar on a gradient's ratio is 8):

    group (cases)                 tensor        error                 oracle                ratio
    modconv3x3, stride 1 (6)      y             4.3e-7 ... 5.2e-7     4.3e-7 ... 5.1e-7     0.87 ... 1.18
                                  grad_x        3.2e-7 ... 7.4e-7     3.6e-7 ... 5.0e-7     0.83 ... 1.64
                                  grad_style    1.4e-7 ... 5.4e-7     4.0e-7 ... 1.4e-5     0.04 ... 0.53
                                  grad_demod    1.7e-7 ... 3.6e-7     1.9e-7 ... 3.2e-7     0.76 ... 1.31
    modconv3x3, up (5)            y             1.8e-7 ... 2.1e-7     2.6e-7 ... 6.1e-7     0.33 ... 0.83
                                  grad_x        2.8e-7 ... 6.2e-7     3.7e-7 ... 5.9e-7     0.75 ... 1.19
                                  grad_style    2.2e-7 ... 3.8e-7     5.1e-7 ... 3.9e-6     0.06 ... 0.69
                                  grad_demod    1.9e-7 ... 2.6e-7     1.9e-7 ... 4.1e-7     0.53 ... 1.22
    torgb_skip (7)                y             1.1e-7 ... 2.4e-7     1.3e-7 ... 2.5e-7     0.71 ... 1.11
                                  grad_x        8.2e-8 ... 1.3e-7     6.9e-8 ... 2.3e-7     0.48 ... 1.18
                                  grad_style    9.8e-8 ... 5.0e-7     3.2e-7 ... 4.2e-6     0.06 ... 0.54
                                  grad_y_prev   8.5e-8 ... 1.1e-7     1.6e-7 ... 1.9e-7     0.51 ... 0.63
    noise_bias_lrelu (6)          out           8.9e-8 ... 1.2e-7     8.9e-8 ... 1.2e-7     0.97 ... 1.00
                                  grad_x        4.6e-8 ... 7.4e-8     4.6e-8 ... 7.4e-8     1.00
    whole chain, worst row        perturb-128-e 1.13e-6               3.00e-6               0.38
                                  stress-128-e  7.4e-7                1.75e-6               0.42
                                  stress-256-e  1.04e-6               6.24e-6               0.17

The segmented sums are more accurate than the float32 oracle where it matters most: at 1024^2 the oracle's grad_style stands at
0.7e-5 ... 1.4e-5, the kernels' at 4e-7 ... 5e-7 (256 strided running sums, a tree, then at most 64 partials). Whole chain: images
8.7e-7 ... 1.5e-6 from the float64 oracle and 1.7e-6 ... 3.2e-6 from the engine, activations at most 1.1e-6 of their layer.
Sign flips against the float64 oracle, the GPU run / the float32 oracle on the same machine / the cap: perturb-128-e 5 / 8 / 11,
stress-128-e 0 / 0 / 11, stress-256-e 4 / 3 / 23, every flipped value below 1e-4 of its layer's maximum. (The float32 oracle's
count depends on the CPU's summation order: 4 / 3 / 0 were seen on another machine.)
"""

import pytest
import torch

import grad_ref
from grad_ref import cuda, judge, lrelu_inputs, lrelu_oracle
from gance_amd import hip_lib, torch_ops  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

# (up, input side, cin, cout, batch), each the smallest that reaches its path
MODCONV_CASES = [
    (False, 65, 16, 16, 2),  # 4225 positions: 2 uneven segments, pixels no multiple of 64, odd side
    (False, 128, 32, 32, 1),  # 4 even segments; the MT = 2 forward form
    (False, 512, 16, 16, 1),  # exactly 64 segments of 4096: the cap's boundary
    (False, 520, 16, 16, 1),  # just past the cap: segments of ceil(270400 / 64) = 4225, a shorter last one
    (False, 1024, 32, 32, 1),  # the 1024^2 Conv1 of config-f; segments of 16384
    (False, 1024, 16, 16, 2),  # the 1024^2 Conv1 of config-e; batch > 1 at the cap
    (True, 33, 16, 32, 2),  # out 66^2: grad_demod in 2 segments, grad_style in 1; odd input side
    (True, 64, 128, 64, 1),  # out 128^2; K = 128, 8 chunks through the 129^2 intermediate
    (True, 256, 32, 16, 1),  # out 512^2: grad_demod at the cap's boundary, grad_style in 16 segments
    (True, 512, 64, 32, 1),  # the 1024^2 Conv0_up of config-f; the 1025^2 intermediate
    (True, 512, 16, 16, 2),  # the largest intermediate with batch > 1
]


@pytest.mark.parametrize("up, side, cin, cout, batch", MODCONV_CASES)
def test_modconv3x3_forward_and_gradients(up: bool, side: int, cin: int, cout: int, batch: int) -> None:
    inputs = grad_ref.modconv_inputs(batch, cin, cout, side, up, seed=side + cin + 7 * cout + batch)
    want64 = grad_ref.modconv_oracle(inputs, up, torch.float64)
    want32 = grad_ref.modconv_oracle(inputs, up, torch.float32)
    x, style, demod = cuda(inputs["x"], True), cuda(inputs["style"], True), cuda(inputs["demod"], True)
    y = torch.ops.gance.modconv3x3(x, style, demod, cuda(grad_ref.scaled_weight(inputs["weight"])), up)
    grads = torch.autograd.grad(y, (x, style, demod), cuda(inputs["grad_y"]))
    assert y.shape == want64[0].shape
    judge(f"modconv3x3 up={up} side={side} {cin}->{cout} B={batch}", ("y", "grad_x", "grad_style", "grad_demod"), (y, *grads), want64, want32)


# (batch, cin, side, with_prev); 66 is no power of two: grad_ref.torgb_oracle reaches ref.torgb_layer for any even side
TORGB_CASES = [
    (2, 16, 66, True),
    (1, 32, 128, True),
    (1, 32, 128, False),
    (1, 16, 512, True),
    (1, 32, 1024, True),
    (1, 32, 1024, False),
    (2, 16, 1024, True),
]


@pytest.mark.parametrize("batch, cin, side, with_prev", TORGB_CASES)
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
    assert y.shape == want64[0].shape
    judge(f"torgb_skip B={batch} {cin} side={side} prev={with_prev}", names, (y, *grads), want64, want32)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("batch, channels, side", [(2, 16, 130), (1, 32, 1024), (3, 16, 1024)])
def test_noise_bias_lrelu_forward_and_gradient(batch: int, channels: int, side: int, per_sample: bool) -> None:
    inputs = lrelu_inputs(batch, channels, side, batch if per_sample else 1, seed=side + channels)
    x = cuda(inputs["x"], True)
    out = torch.ops.gance.noise_bias_lrelu(x, cuda(inputs["noise"]), cuda(inputs["strength"]), cuda(inputs["bias"]))
    (grad,) = torch.autograd.grad(out, x, cuda(inputs["grad"]))
    judge(f"noise_bias_lrelu B={batch} C={channels} side={side} per_sample={per_sample}", ("out", "grad_x"), (out, grad),
          lrelu_oracle(inputs, torch.float64), lrelu_oracle(inputs, torch.float32))


@pytest.mark.parametrize("name", grad_ref.LARGE_CASE_NAMES)
def test_whole_chain(name: str) -> None:
    """The whole chain beyond 64^2 (config-e), the body of test_synthesis_grad_gpu.test_whole_chain; grad_ref.sign_flip_cap gives the cap on sign flips."""
    grad_ref.check_whole_chain(name)
