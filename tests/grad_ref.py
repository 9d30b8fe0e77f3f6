"""
Reference for the gradients of differentiable synthesis (tests of gance_amd/stylegan2/differentiable.py).

`oracle/stylegan2_ref.py` is plain torch, so it differentiates as it stands, in float64 on the CPU. A whole-chain gradient
still cannot be compared naively: a float32 run puts 0 to 2 pre-activations per case on the other side of leaky ReLU's kink
than the float64 run, and one such flip moves a dlatent row's gradient by 1.5e-5 ... 2e-3 of the row's maximum, against
0.6e-6 ... 1.5e-6 without a flip. `g_synthesis_with_signs` is g_synthesis rebuilt from the oracle's own layer functions
with every leaky ReLU written as pre * where(sign, 1, 0.2) * sqrt(2): `sign` defaults to pre > 0 (then the result IS
g_synthesis, bit for bit), or is GIVEN per layer, taken from the activations of the run being judged (leaky ReLU keeps the
sign, so sign = activation > 0). The run is then compared with the float64 gradient of the function it actually computed.

The yardstick of a gradient bar is the oracle itself in float32 on the CPU, judged the same way (`yardstick`).
"""

import functools
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

SQRT2 = float(np.sqrt(2.0))

# the most activations per case whose sign may differ from the float64 oracle's, and how small each must be (of its layer's maximum)
MAX_SIGN_FLIPS = 8
SIGN_FLIP_MAGNITUDE = 1e-4
# the code under test gets this many times the float32 oracle's own error: the matrix cores add up to 4608 products per output
# in another order than the CPU, through up to ten layers, and the forward kernels sit at 1 ... 3 times the float32 oracle
GRADIENT_BAR_FACTOR = 8.0
LAYER_BAR = 2e-5  # forward, of the layer's maximum
IMAGE_BAR = 1e-4


def g_synthesis_with_signs(
    dlatents: torch.Tensor,
    variables: ref.Variables,
    resolution: int,
    fmap_base: int = sg2_spec.FMAP_BASE,
    signs: Optional[Sequence[torch.Tensor]] = None,
    collect: Optional[list] = None,
) -> torch.Tensor:
    """g_synthesis with the slope mask of conv layer n given by `signs[n]` (bool, the activation's shape) instead of pre > 0."""
    dtype = dlatents.dtype
    x = ref._t(variables, "G_synthesis/4x4/Const/const", dtype).repeat(dlatents.shape[0], 1, 1, 1)  # pylint: disable=protected-access
    y = None
    for index, conv in enumerate(sg2_spec.make_spec(resolution, fmap_base).convs):
        scope = f"G_synthesis/{conv.scope}"
        x = ref.modulated_conv2d_layer(x, dlatents[:, conv.layer_idx], variables, scope, 3, up=conv.up)
        noise = ref._t(variables, f"G_synthesis/noise{conv.layer_idx}", dtype)  # pylint: disable=protected-access
        x = x + noise * ref._t(variables, f"{scope}/noise_strength", dtype)  # pylint: disable=protected-access
        pre = x + ref._t(variables, f"{scope}/bias", dtype).reshape(1, -1, 1, 1)  # pylint: disable=protected-access
        sign = pre > 0 if signs is None else signs[index]
        x = pre * torch.where(sign, torch.tensor(1.0, dtype=dtype), torch.tensor(0.2, dtype=dtype)) * SQRT2
        if collect is not None:
            collect.append(x)
        if not conv.up:
            y = ref.torgb_layer(x, y, dlatents, variables, conv.res_log2)
    return y


def relative_error(got: torch.Tensor, want: torch.Tensor) -> float:
    """max|got - want| / max|want| of one tensor (`want` float64)."""
    want = want.detach().double()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def row_error(got: torch.Tensor, want: torch.Tensor) -> float:
    """The error measure of dlatent gradients [B, W, 512]: relative_error per dlatent row, the worst row."""
    want = want.detach().double()
    difference = (got.detach().double().cpu() - want).abs().amax(dim=2)
    return float((difference / want.abs().amax(dim=2)).max())


class Case(NamedTuple):
    """One whole-chain case: a network, dlatents, a cotangent, and the float64 oracle's image and activations."""

    name: str
    resolution: int
    fmap_base: int
    variables: Dict[str, np.ndarray]
    dlatents: np.ndarray  # [2, W, 512] float32
    cotangent: np.ndarray  # [2, 3, R, R] float32
    image64: torch.Tensor
    activations64: Tuple[torch.Tensor, ...]


# (resolution, fmap_base): 16^2 ... 64^2 config-f and 64^2 config-e, each on the stress network and the perturbed random init
CASE_SHAPES = ((16, sg2_spec.FMAP_BASE), (32, sg2_spec.FMAP_BASE), (64, sg2_spec.FMAP_BASE), (64, sg2_spec.FMAP_BASE_CONFIG_E))
CASE_NAMES = tuple(f"{kind}-{resolution}-{'e' if base == sg2_spec.FMAP_BASE_CONFIG_E else 'f'}" for resolution, base in CASE_SHAPES for kind in ("stress", "perturb"))
# Beyond 64^2, config-e only: every position sum of a real layer sequence in 4 (128^2) and 16 (256^2) segments. Apart from
# CASE_NAMES, so that nothing parametrized over that changes. perturb-256-e is left out: the float32 oracle alone flips 11 of its
# cap of 23 signs there.
LARGE_CASE_NAMES = ("perturb-128-e", "stress-128-e", "stress-256-e")
# MAX_SIGN_FLIPS was set for at most this many activations per sample (64^2 config-f): 512 * (16 + 2 * 64 + 2 * 256 + 2 * 1024 + 2 * 4096)
SIGN_FLIP_ACTIVATIONS = 5_578_752


def activations_per_sample(resolution: int, fmap_base: int) -> int:
    return sum(conv.cout * (1 << conv.res_log2) ** 2 for conv in sg2_spec.make_spec(resolution, fmap_base).convs)


def sign_flip_cap(name: str) -> int:
    """
    MAX_SIGN_FLIPS for the cases it was set for; for the larger ones the same density of flips per activation (the number of
    pre-activations within rounding distance of zero grows with the activation count), rounded down: 11 at 128^2 config-e
    (7 675 904 activations), 23 at 256^2 config-e (16 064 512).
    """
    if name in CASE_NAMES:
        return MAX_SIGN_FLIPS
    _, resolution_text, config = name.split("-")
    count = activations_per_sample(int(resolution_text), sg2_spec.FMAP_BASE_CONFIG_E if config == "e" else sg2_spec.FMAP_BASE)
    return max(MAX_SIGN_FLIPS, MAX_SIGN_FLIPS * count // SIGN_FLIP_ACTIVATIONS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    """A case by name, with its float64 forward pass; computed once per process."""
    kind, resolution_text, config = name.split("-")
    resolution = int(resolution_text)
    fmap_base = sg2_spec.FMAP_BASE_CONFIG_E if config == "e" else sg2_spec.FMAP_BASE
    seed = resolution + (1 if kind == "stress" else 2)
    if kind == "stress":
        variables = sg2_spec.make_stress_variables(resolution, seed=seed, fmap_base=fmap_base)
    else:
        variables = sg2_spec.make_random_variables(resolution, seed=seed, perturb=True, fmap_base=fmap_base)
    rng = np.random.RandomState(1000 + seed)
    num_layers = sg2_spec.make_spec(resolution, fmap_base).num_layers
    dlatents = rng.randn(2, num_layers, 512).astype(np.float32)
    cotangent = rng.randn(2, 3, resolution, resolution).astype(np.float32)
    activations: List[torch.Tensor] = []
    with torch.no_grad():
        image = ref.g_synthesis(torch.from_numpy(dlatents).double(), variables, resolution, collect=activations)
    return Case(name, resolution, fmap_base, variables, dlatents, cotangent, image, tuple(activations))


def gradient64(this: Case, signs: Sequence[torch.Tensor]) -> torch.Tensor:
    """Float64 dlatent gradient [2, W, 512] of <cotangent, image> through the helper with the given slope masks."""
    dlatents = torch.from_numpy(this.dlatents).double().requires_grad_(True)
    image = g_synthesis_with_signs(dlatents, this.variables, this.resolution, this.fmap_base, signs=signs)
    (gradient,) = torch.autograd.grad(image, dlatents, torch.from_numpy(this.cotangent).double())
    return gradient


def check_signs(this: Case, activations: Sequence[torch.Tensor], who: str = "the run") -> List[torch.Tensor]:
    """
    The slope masks of a run (activation > 0 per conv layer) after the conditions on them: at most sign_flip_cap (MAX_SIGN_FLIPS
    for every case up to 64^2) activations differ in sign from the float64 oracle's, each smaller than SIGN_FLIP_MAGNITUDE of
    its layer's largest activation, in the run and in the oracle. A real sign or mask mistake flips ordinary-sized values and
    fails this.
    """
    signs, flips = [], 0
    assert len(activations) == len(this.activations64)
    for index, (got, want) in enumerate(zip(activations, this.activations64)):
        got = got.detach().cpu()
        sign = got > 0
        differ = sign != (want > 0)
        count = int(differ.sum())
        if count:
            limit = SIGN_FLIP_MAGNITUDE * float(want.abs().max())
            largest = max(float(got[differ].abs().max()), float(want[differ].abs().max()))
            assert largest < limit, f"{this.name} layer {index}: an activation of magnitude {largest:.3e} (limit {limit:.3e}) changed sign"
        flips += count
        signs.append(sign)
    cap = sign_flip_cap(this.name)
    print(f"{this.name}: {flips} activations of {who} differ in sign from the float64 oracle (at most {cap})")
    assert flips <= cap, f"{this.name}: {flips} activations differ in sign from the float64 oracle (at most {cap})"
    return signs


@functools.lru_cache(maxsize=None)
def yardstick(name: str) -> float:
    """
    The float32 oracle's own gradient error on a case: the helper in float32 on the CPU (= g_synthesis in float32) against
    the helper in float64 with the float32 run's slope masks, worst dlatent row.
    """
    this = case(name)
    dlatents = torch.from_numpy(this.dlatents).requires_grad_(True)
    activations: List[torch.Tensor] = []
    image = g_synthesis_with_signs(dlatents, this.variables, this.resolution, this.fmap_base, collect=activations)
    (gradient,) = torch.autograd.grad(image, dlatents, torch.from_numpy(this.cotangent))
    return row_error(gradient, gradient64(this, check_signs(this, activations, "the float32 oracle")))


# ---- the three operations in isolation: float64 (or float32) autograd of the oracle's layer functions with style and demod as leaves ----


def modconv_inputs(batch: int, cin: int, cout: int, side: int, up: bool, seed: int) -> Dict[str, np.ndarray]:
    """x, style (with a zero and a negative entry), demod > 0, raw weight, grad_y of one isolated modconv3x3 case (float32)."""
    rng = np.random.RandomState(seed)
    style = (1.0 + 0.5 * rng.randn(batch, cin)).astype(np.float32)
    style[0, 1], style[0, 2] = 0.0, -1.25
    out_side = 2 * side if up else side
    return {
        "x": rng.randn(batch, cin, side, side).astype(np.float32),
        "style": style,
        "demod": rng.uniform(0.05, 0.5, size=(batch, cout)).astype(np.float32),
        "weight": rng.randn(3, 3, cin, cout).astype(np.float32),
        "grad_y": rng.randn(batch, cout, out_side, out_side).astype(np.float32),
    }


def modconv_oracle(inputs: Dict[str, np.ndarray], up: bool, dtype: torch.dtype) -> Tuple[torch.Tensor, ...]:
    """
    (y, grad_x, grad_style, grad_demod) of demod * ref.modulated_conv2d_layer(x, style, demodulate=False) in `dtype`. The layer
    computes its style as dlatent @ mod_weight + mod_bias + 1: with the dlatent `cin` long, mod_weight the identity (after
    its runtime scale) and mod_bias -1, the dlatent IS the style, a leaf.
    """
    cin = inputs["x"].shape[1]
    variables = {
        "L/weight": inputs["weight"],
        "L/mod_weight": np.eye(cin) * np.sqrt(float(cin)),
        "L/mod_bias": -np.ones(cin),
    }
    x = torch.from_numpy(inputs["x"]).to(dtype).requires_grad_(True)
    style = torch.from_numpy(inputs["style"]).to(dtype).requires_grad_(True)
    demod = torch.from_numpy(inputs["demod"]).to(dtype).requires_grad_(True)
    y = demod[:, :, None, None] * ref.modulated_conv2d_layer(x, style, variables, "L", 3, up=up, demodulate=False)
    grads = torch.autograd.grad(y, (x, style, demod), torch.from_numpy(inputs["grad_y"]).to(dtype))
    return (y.detach(), *grads)


def scaled_weight(raw: np.ndarray) -> np.ndarray:
    """The runtime-scaled float32 weight the ops take: raw / sqrt(fan_in), computed in float64."""
    raw = np.asarray(raw, dtype=np.float64)
    return (raw * (1.0 / np.sqrt(float(np.prod(raw.shape[:-1]))))).astype(np.float32)


def torgb_inputs(batch: int, cin: int, side: int, with_prev: bool, seed: int) -> Dict[str, np.ndarray]:
    """x, style, raw weight [1, 1, cin, 3], bias, y_prev (or None) and grad_y of one isolated torgb_skip case (float32)."""
    rng = np.random.RandomState(seed)
    style = (1.0 + 0.5 * rng.randn(batch, cin)).astype(np.float32)
    style[0, 1], style[0, 2] = 0.0, -1.25
    return {
        "x": rng.randn(batch, cin, side, side).astype(np.float32),
        "style": style,
        "weight": rng.randn(1, 1, cin, 3).astype(np.float32),
        "bias": rng.randn(3).astype(np.float32),
        "y_prev": rng.randn(batch, 3, side // 2, side // 2).astype(np.float32) if with_prev else None,
        "grad_y": rng.randn(batch, 3, side, side).astype(np.float32),
    }


def torgb_oracle(inputs: Dict[str, np.ndarray], dtype: torch.dtype) -> Tuple[torch.Tensor, ...]:
    """(y, grad_x, grad_style[, grad_y_prev]) of ref.torgb_layer in `dtype`, the style a leaf as in modconv_oracle."""
    batch, cin, side = inputs["x"].shape[:3]
    # res_log2 only names the scope and the dlatent row that ref.torgb_layer reads: any even side goes under its power of two below
    res_log2 = int(np.log2(side))
    scope = f"G_synthesis/{2 ** res_log2}x{2 ** res_log2}/ToRGB"
    variables = {
        f"{scope}/weight": inputs["weight"],
        f"{scope}/mod_weight": np.eye(cin) * np.sqrt(float(cin)),
        f"{scope}/mod_bias": -np.ones(cin),
        f"{scope}/bias": inputs["bias"],
    }
    x = torch.from_numpy(inputs["x"]).to(dtype).requires_grad_(True)
    style = torch.from_numpy(inputs["style"]).to(dtype).requires_grad_(True)
    leaves = [x, style]
    y_prev = None
    if inputs["y_prev"] is not None:
        y_prev = torch.from_numpy(inputs["y_prev"]).to(dtype).requires_grad_(True)
        leaves.append(y_prev)
    dlatents = torch.zeros((batch, res_log2 * 2 - 2, cin), dtype=dtype)
    dlatents = torch.cat([dlatents[:, : res_log2 * 2 - 3], style[:, None]], dim=1)  # (row res_log2 * 2 - 3 is the one torgb_layer reads)
    y = ref.torgb_layer(x, y_prev, dlatents, variables, res_log2)
    grads = torch.autograd.grad(y, leaves, torch.from_numpy(inputs["grad_y"]).to(dtype))
    return (y.detach(), *grads)


def lrelu_inputs(batch: int, channels: int, side: int, noise_batch: int, seed: int) -> Dict[str, np.ndarray]:
    """Inputs whose pre-activation stays at least 1e-3 away from the kink (values nearer than 2e-3 are moved to +-2e-3 through x)."""
    rng = np.random.RandomState(seed)
    x = rng.randn(batch, channels, side, side).astype(np.float32)
    noise = rng.randn(noise_batch, 1, side, side).astype(np.float32)
    strength, bias = np.float32(0.37), rng.randn(channels).astype(np.float32)
    rest = noise.astype(np.float64) * float(strength) + bias.astype(np.float64)[None, :, None, None]
    pre = x.astype(np.float64) + rest
    near = np.abs(pre) < 2e-3
    x = np.where(near, np.where(pre >= 0, 2e-3, -2e-3) - rest, x).astype(np.float32)
    assert np.abs(x.astype(np.float64) + rest).min() >= 1e-3
    return {"x": x, "noise": noise, "strength": np.reshape(strength, (1,)), "bias": bias, "grad": rng.randn(batch, channels, side, side).astype(np.float32)}


def lrelu_oracle(inputs: Dict[str, np.ndarray], dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    x = torch.from_numpy(inputs["x"]).to(dtype).requires_grad_(True)
    pre = x + torch.from_numpy(inputs["noise"]).to(dtype) * torch.from_numpy(inputs["strength"]).to(dtype)
    out = ref.apply_bias_act(pre, torch.from_numpy(inputs["bias"]).to(dtype), "lrelu")
    (grad,) = torch.autograd.grad(out, x, torch.from_numpy(inputs["grad"]).to(dtype))
    return out.detach(), grad


# ---- what the GPU test modules share ----


def cuda(array: np.ndarray, requires_grad: bool = False) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).cuda().requires_grad_(requires_grad)


def judge(label: str, names: Sequence[str], got: Sequence[torch.Tensor], want64: Sequence[torch.Tensor], want32: Sequence[torch.Tensor]) -> None:
    """tensor 0 is the forward output (bar LAYER_BAR), the others gradients (bar 8 x the float32 oracle's own error)."""
    failures = []
    for index, name in enumerate(names):
        error = relative_error(got[index], want64[index])
        own = relative_error(want32[index], want64[index])
        bar = LAYER_BAR if index == 0 else GRADIENT_BAR_FACTOR * own
        print(f"{label} {name}: error {error:.3e}, float32 oracle {own:.3e}, ratio {error / own if own else float('inf'):.2f}, bar {bar:.3e}")
        if not (np.isfinite(error) and error <= bar):
            failures.append(f"{name}: {error:.3e} > {bar:.3e}")
    assert not failures, f"{label}: " + "; ".join(failures)


def run_chain(synthesis: Any, this: Case) -> Tuple[torch.Tensor, List[torch.Tensor], torch.Tensor]:
    """(image, activations, dlatent gradient) of a DifferentiableSynthesis on a case's dlatents and cotangent."""
    dlatents = cuda(this.dlatents, True)
    activations: List[torch.Tensor] = []
    image = synthesis(dlatents, collect=activations)
    (gradient,) = torch.autograd.grad(image, dlatents, cuda(this.cotangent))
    return image.detach(), [activation.detach() for activation in activations], gradient


def check_whole_chain(name: str) -> None:
    """
    A whole-chain case on the GPU: the image against the float64 oracle and against the engine, every activation against
    LAYER_BAR, the sign conditions, and the dlatent gradient's worst row against GRADIENT_BAR_FACTOR x `yardstick`.
    """
    from gance_amd import hip_lib  # pylint: disable=import-outside-toplevel
    from gance_amd.stylegan2.differentiable import DifferentiableSynthesis  # pylint: disable=import-outside-toplevel

    this = case(name)
    synthesis = DifferentiableSynthesis(this.variables, this.resolution, fmap_base=this.fmap_base, device=0)
    image, activations, gradient = run_chain(synthesis, this)
    assert image.shape == (2, 3, this.resolution, this.resolution) and image.dtype == torch.float32
    failures = []

    def bar(what: str, error: float, limit: float) -> None:
        print(f"{name} {what}: {error:.3e} (bar {limit:.3e})")
        if not (np.isfinite(error) and error <= limit):
            failures.append(f"{what}: {error:.3e} > {limit:.3e}")

    bar("image against the float64 oracle", relative_error(image, this.image64), IMAGE_BAR)
    engine = hip_lib.Engine(this.variables, this.resolution, max_batch=2, device=0)
    try:
        _, engine_image = engine.synthesize_w(this.dlatents, want_float=True)
    finally:
        engine.close()
    bar("image against the engine", relative_error(image, torch.from_numpy(engine_image)), IMAGE_BAR)
    assert len(activations) == len(this.activations64)
    for index, (got, want) in enumerate(zip(activations, this.activations64)):
        bar(f"activation {index}", relative_error(got, want), LAYER_BAR)
    signs = check_signs(this, activations)
    own = yardstick(name)
    error = row_error(gradient, gradient64(this, signs))
    print(f"{name} dlatent gradient: ratio to the float32 oracle {error / own:.2f}")
    bar("dlatent gradient, worst row", error, GRADIENT_BAR_FACTOR * own)
    assert not failures, f"{name}: " + "; ".join(failures)
