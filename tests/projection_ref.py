"""
CPU restatements of projection's arithmetic (tests of gance_amd/csrc/projection.hip, the gance::noise_regularizer /
pyramid_distance / noise_bias_lrelu_backward_noise ops and gance_amd/stylegan2/projector.py), written from the formulas of
the publication (Karras et al. 2020, appendix D) in plain torch, so float64 autograd differentiates them as they stand.

As in tests/grad_ref.py, a whole step is compared through `g_synthesis_with_signs`: the float64 side takes the leaky ReLU
slope masks of the run under judgement. This module's version also takes the noise planes as tensors (leaves).
"""

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import grad_ref
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

REGULARIZE_NOISE_WEIGHT = 1e5


def noise_regularizer(planes: torch.Tensor) -> torch.Tensor:
    """[B, 1, S, S] -> [B]: sum over the 2x2-mean pyramid (down to 8 x 8) of mean(v roll_W v)^2 + mean(v roll_H v)^2."""
    v, total = planes, 0.0
    while True:
        total = total + (v * torch.roll(v, 1, dims=3)).mean(dim=(1, 2, 3)) ** 2 + (v * torch.roll(v, 1, dims=2)).mean(dim=(1, 2, 3)) ** 2
        if v.shape[2] <= 8:
            return total
        v = F.avg_pool2d(v, 2)


def pyramid_distance(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """image [B, 3, R, R] in -1 ... 1, target [B, 3, T, T] in 0 ... 255, T = min(R, 256) -> [B]."""
    batch, _, side, _ = image.shape
    small = min(side, 256)
    factor = side // small
    p = (image + 1.0) * 127.5
    if factor > 1:
        p = p.reshape(batch, 3, small, factor, small, factor).mean(dim=(3, 5))
    d = (p - target) / 255.0
    total = (d * d).mean(dim=(1, 2, 3))
    while d.shape[2] > 8:
        d = F.avg_pool2d(d, 2)
        total = total + (d * d).mean(dim=(1, 2, 3))
    return total


def smooth_planes(batch: int, side: int, seed: int) -> np.ndarray:
    """N(0, 1) planes plus a smooth component, so that the neighbour correlations are not all near zero."""
    rng = np.random.RandomState(seed)
    ramp = np.arange(side, dtype=np.float64) * (2.0 * np.pi / side)
    smooth = np.sin(ramp)[None, None, :, None] * rng.uniform(0.5, 1.5, size=(batch, 1, 1, 1)) + np.cos(2.0 * ramp)[None, None, None, :] * rng.uniform(
        0.5, 1.5, size=(batch, 1, 1, 1)
    )
    return (rng.randn(batch, 1, side, side) + smooth).astype(np.float32)


def distance_inputs(batch: int, resolution: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(image in about -1 ... 1, target in 0 ... 255) with a smooth part, so that the coarse levels carry weight."""
    rng = np.random.RandomState(seed)
    small = min(resolution, 256)
    ramp = np.arange(resolution, dtype=np.float64) * (2.0 * np.pi / resolution)
    image = 0.4 * np.sin(ramp)[None, None, :, None] + 0.3 * np.cos(3.0 * ramp)[None, None, None, :] + 0.3 * rng.randn(batch, 3, resolution, resolution)
    target = rng.randint(0, 256, size=(batch, 3, small, small)).astype(np.float64) * 0.5 + 64.0 * (1.0 + np.sin(ramp[:: resolution // small]))[None, None, None, :]
    return image.astype(np.float32), np.clip(target, 0.0, 255.0).astype(np.float32)


def lrelu_noise_oracle(inputs: Dict[str, np.ndarray], dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(out, grad_x, grad_noise) of the layer epilogue with x and the noise planes as leaves; inputs as grad_ref.lrelu_inputs draws them."""
    x = torch.from_numpy(inputs["x"]).to(dtype).requires_grad_(True)
    noise = torch.from_numpy(inputs["noise"]).to(dtype).requires_grad_(True)
    pre = x + noise * torch.from_numpy(inputs["strength"]).to(dtype)
    out = ref.apply_bias_act(pre, torch.from_numpy(inputs["bias"]).to(dtype), "lrelu")
    grad_x, grad_noise = torch.autograd.grad(out, (x, noise), torch.from_numpy(inputs["grad"]).to(dtype))
    return out.detach(), grad_x, grad_noise


def g_synthesis_with_signs(  # pylint: disable=too-many-arguments,too-many-locals
    dlatents: torch.Tensor,
    variables: ref.Variables,
    resolution: int,
    planes: Sequence[torch.Tensor],
    fmap_base: int = sg2_spec.FMAP_BASE,
    signs: Optional[Sequence[torch.Tensor]] = None,
    collect: Optional[list] = None,
) -> torch.Tensor:
    """grad_ref.g_synthesis_with_signs with conv layer n's noise given by `planes[n]` [B, 1, S, S] (may be a leaf)."""
    dtype = dlatents.dtype
    x = ref._t(variables, "G_synthesis/4x4/Const/const", dtype).repeat(dlatents.shape[0], 1, 1, 1)  # pylint: disable=protected-access
    y = None
    for index, conv in enumerate(sg2_spec.make_spec(resolution, fmap_base).convs):
        scope = f"G_synthesis/{conv.scope}"
        x = ref.modulated_conv2d_layer(x, dlatents[:, conv.layer_idx], variables, scope, 3, up=conv.up)
        x = x + planes[index].to(dtype) * ref._t(variables, f"{scope}/noise_strength", dtype)  # pylint: disable=protected-access
        pre = x + ref._t(variables, f"{scope}/bias", dtype).reshape(1, -1, 1, 1)  # pylint: disable=protected-access
        sign = pre > 0 if signs is None else signs[index]
        x = pre * torch.where(sign, torch.tensor(1.0, dtype=dtype), torch.tensor(0.2, dtype=dtype)) * grad_ref.SQRT2
        if collect is not None:
            collect.append(x)
        if not conv.up:
            y = ref.torgb_layer(x, y, dlatents, variables, conv.res_log2)
    return y


def distance_targets(targets_u8: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """[B, R, R, 3] uint8 -> [B, 3, T, T] in 0 ... 255, area-averaged to T = min(R, 256)."""
    planes = torch.from_numpy(np.ascontiguousarray(targets_u8)).permute(0, 3, 1, 2).to(dtype)
    batch, _, side, _ = planes.shape
    if side > 256:
        factor = side // 256
        planes = planes.reshape(batch, 3, 256, factor, 256, factor).mean(dim=(3, 5))
    return planes


class StepResult:  # pylint: disable=too-few-public-methods
    """One projector step's loss terms and gradients."""

    def __init__(self, loss, distance, regularizer, images, grad_w, grad_planes, activations) -> None:  # type: ignore[no-untyped-def]
        self.loss, self.distance, self.regularizer, self.images = loss, distance, regularizer, images
        self.grad_w, self.grad_planes, self.activations = grad_w, grad_planes, activations


def projector_step(  # pylint: disable=too-many-arguments,too-many-locals
    variables: ref.Variables,
    resolution: int,
    w: np.ndarray,
    planes: Sequence[np.ndarray],
    targets_u8: np.ndarray,
    dtype: torch.dtype,
    fmap_base: int = sg2_spec.FMAP_BASE,
    signs: Optional[Sequence[torch.Tensor]] = None,
) -> StepResult:
    """loss = sum_b [pyramid_distance_b + 1e5 * sum_layers noise_regularizer_b] at w [B, 1, 512] tiled to every row, and its gradients."""
    num_layers = sg2_spec.make_spec(resolution, fmap_base).num_layers
    w_leaf = torch.from_numpy(np.asarray(w)).to(dtype).requires_grad_(True)
    plane_leaves = [torch.from_numpy(np.asarray(plane)).to(dtype).requires_grad_(True) for plane in planes]
    activations: List[torch.Tensor] = []
    images = g_synthesis_with_signs(w_leaf.expand(-1, num_layers, -1), variables, resolution, plane_leaves, fmap_base, signs, activations)
    distance = pyramid_distance(images, distance_targets(targets_u8, dtype))
    regularizer = sum(noise_regularizer(plane) for plane in plane_leaves)
    loss = (distance + REGULARIZE_NOISE_WEIGHT * regularizer).sum()
    grads = torch.autograd.grad(loss, [w_leaf, *plane_leaves])
    return StepResult(loss.detach(), distance.detach(), regularizer.detach(), images.detach(), grads[0], list(grads[1:]), [a.detach() for a in activations])


def check_signs(activations: Sequence[torch.Tensor], activations64: Sequence[torch.Tensor], who: str) -> List[torch.Tensor]:
    """grad_ref.check_signs for a step: at most MAX_SIGN_FLIPS activations differ in sign from the float64 run, each below 1e-4 of its layer's maximum."""
    signs, flips = [], 0
    assert len(activations) == len(activations64)
    for index, (got, want) in enumerate(zip(activations, activations64)):
        got = got.detach().cpu()
        sign = got > 0
        differ = sign != (want > 0)
        count = int(differ.sum())
        if count:
            limit = grad_ref.SIGN_FLIP_MAGNITUDE * float(want.abs().max())
            largest = max(float(got[differ].abs().max()), float(want[differ].abs().max()))
            assert largest < limit, f"layer {index}: an activation of magnitude {largest:.3e} (limit {limit:.3e}) changed sign"
        flips += count
        signs.append(sign)
    print(f"{flips} activations of {who} differ in sign from the float64 step (at most {grad_ref.MAX_SIGN_FLIPS})")
    assert flips <= grad_ref.MAX_SIGN_FLIPS
    return signs


def sample_error(got: torch.Tensor, want: torch.Tensor) -> float:
    """max|got - want| / max|want| per sample (a dlatent row [B, 1, 512], a plane [B, 1, S, S]), the worst sample."""
    want = want.detach().double()
    difference = (got.detach().double().cpu() - want).abs().flatten(1).amax(dim=1)
    return float((difference / want.abs().flatten(1).amax(dim=1)).max())


# ---- the whole loop, for the convergence figures ----


def learning_rate(step: int, num_steps: int) -> float:
    t = step / num_steps
    ramp = min(1.0, (1.0 - t) / 0.25)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    return 0.1 * ramp * min(1.0, t / 0.05)


def noise_strength(step: int, num_steps: int, dlatent_std: float) -> float:
    return dlatent_std * 0.05 * max(0.0, 1.0 - (step / num_steps) / 0.75) ** 2


def w_statistics(variables: ref.Variables, dtype: torch.dtype) -> Tuple[torch.Tensor, float]:
    """(dlatent_avg [1, 1, 512], dlatent_std) from 10 000 z of RandomState(123) through the oracle's mapping network."""
    z = torch.from_numpy(np.random.RandomState(123).randn(10000, 512).astype(np.float32)).to(dtype)
    with torch.no_grad():
        w = ref.g_mapping(z, variables, 1)
    average = w.mean(dim=0, keepdim=True)
    return average, float(torch.sqrt(((w - average) ** 2).sum() / 10000))


def run_projection(  # pylint: disable=too-many-locals
    variables: ref.Variables, resolution: int, targets_u8: np.ndarray, num_steps: int, seed: int, dtype: torch.dtype = torch.float64
) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """
    The projector's loop restated on the CPU with the same draws (gance_amd.stylegan2.projector.frame_draws):
    (distance at step 0 with w alone, final distance with w alone, regulariser sum at step 0, final regulariser sum), each [B].
    """
    from gance_amd.stylegan2 import projector as projector_module  # pylint: disable=import-outside-toplevel

    spec = sg2_spec.make_spec(resolution)
    sides = [1 << conv.res_log2 for conv in spec.convs]
    batch = targets_u8.shape[0]
    draws = [projector_module.frame_draws(seed, frame, num_steps, sides) for frame in range(batch)]
    average, std = w_statistics(variables, dtype)
    w = average.repeat(batch, 1, 1).clone()
    planes = [torch.from_numpy(np.stack([draw.planes[layer] for draw in draws])).to(dtype) for layer in range(len(sides))]
    w_noise = torch.from_numpy(np.stack([draw.w_noise for draw in draws])).to(dtype)
    targets = distance_targets(targets_u8, dtype)
    parameters = [w, *planes]
    first, second = [torch.zeros_like(p) for p in parameters], [torch.zeros_like(p) for p in parameters]

    def terms(offset: Optional[torch.Tensor], leaves: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        w_in = leaves[0] if offset is None else leaves[0] + offset
        images = g_synthesis_with_signs(w_in.expand(-1, spec.num_layers, -1), variables, resolution, leaves[1:])
        return pyramid_distance(images, targets), sum(noise_regularizer(plane) for plane in leaves[1:])

    with torch.no_grad():
        distance0, regularizer0 = terms(None, parameters)
    for step in range(num_steps):
        leaves = [p.detach().requires_grad_(True) for p in parameters]
        distance, regularizer = terms(w_noise[:, step : step + 1] * noise_strength(step, num_steps, std), leaves)
        gradients = torch.autograd.grad((distance + REGULARIZE_NOISE_WEIGHT * regularizer).sum(), leaves)
        count = step + 1
        rate = learning_rate(step, num_steps) * math.sqrt(1.0 - 0.999 ** count) / (1.0 - 0.9 ** count)
        with torch.no_grad():
            for index, gradient in enumerate(gradients):
                first[index] = 0.9 * first[index] + 0.1 * gradient
                second[index] = 0.999 * second[index] + 0.001 * gradient * gradient
                parameters[index] = parameters[index] - rate * first[index] / (torch.sqrt(second[index]) + 1e-8)
            for index in range(1, len(parameters)):
                plane = parameters[index] - parameters[index].mean(dim=(1, 2, 3), keepdim=True)
                parameters[index] = plane * torch.rsqrt((plane * plane).mean(dim=(1, 2, 3), keepdim=True))
    with torch.no_grad():
        distance1, regularizer1 = terms(None, parameters)
    return distance0.numpy(), distance1.numpy(), regularizer0.numpy(), regularizer1.numpy()


def convergence_targets(variables: ref.Variables, resolution: int, seeds: Sequence[int] = (11, 12)) -> np.ndarray:
    """uint8 [B, R, R, 3]: the rounded, clamped 0 ... 255 images of w = mapping(z) for one seeded z per frame (float64 oracle)."""
    num_layers = sg2_spec.make_spec(resolution).num_layers
    z = np.stack([np.random.RandomState(seed).randn(512) for seed in seeds])
    with torch.no_grad():
        images = ref.g_synthesis(ref.g_mapping(torch.from_numpy(z), variables, num_layers), variables, resolution)
    scaled = torch.clamp(torch.round((images + 1.0) * 127.5), 0.0, 255.0)
    return scaled.permute(0, 2, 3, 1).to(torch.uint8).numpy()
