"""
CPU restatement of LPIPS on VGG16 (tests of gance_amd/stylegan2/lpips.py, gance_amd/csrc/lpips.hip and the gance::lpips_* /
bias_relu* ops), in plain torch and generic in dtype, written from the formulas of the publications.

A whole-chain gradient cannot be compared naively: a float32 run may put a pre-activation on the other side of a ReLU's kink,
or pick another element of a max-pool window, than the float64 run. As `grad_ref.g_synthesis_with_signs` does for leaky ReLU,
`taps` takes the thirteen activations of the run being judged: each ReLU is then where(activation > 0, pre, 0) and each pool
gathers the position that is largest in the run's activation. Without given activations the masks and positions are the
restatement's own and the result is the ordinary conv2d / relu / max_pool2d composition, bit for bit.
"""

import functools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

import grad_ref
from gance_amd.stylegan2 import lpips

NORM_EPSILON = 1e-10


def as_tensor(array: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(array)).to(dtype)


def preprocess(images: torch.Tensor, side: int, weights: lpips.LpipsWeights) -> torch.Tensor:
    """images [B, 3, R, R] in -1 ... 1 -> [B, 3, S, S]: the R / side area mean when R > side, then (x - shift) / scale."""
    batch, _, resolution, _ = images.shape
    if resolution > side:
        factor = resolution // side
        images = images.reshape(batch, 3, side, factor, side, factor).mean(dim=(3, 5))
    shift = as_tensor(weights.shift, images.dtype).reshape(1, 3, 1, 1)
    scale = as_tensor(weights.scale, images.dtype).reshape(1, 3, 1, 1)
    return (images - shift) / scale


def target_planes(targets_u8: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """targets [B, R, R, 3] uint8 -> [B, 3, R, R] in -1 ... 1."""
    return targets_u8.permute(0, 3, 1, 2).to(dtype) / 127.5 - 1.0


def bias_relu(pre: torch.Tensor, activation: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ReLU with the mask of `activation` (the run's), or its own."""
    mask = pre > 0 if activation is None else activation > 0
    return torch.where(mask, pre, torch.zeros((), dtype=pre.dtype))


def max_pool(y: torch.Tensor, activation: Optional[torch.Tensor] = None) -> torch.Tensor:
    """2x2 max pool that gathers where `activation` (the run's, upcast), or y itself, is largest: torch's choice among equals."""
    chooser = (y if activation is None else activation.to(y.dtype)).detach()
    _, indices = torch.nn.functional.max_pool2d(chooser, 2, return_indices=True)
    return y.flatten(2).gather(2, indices.flatten(2)).reshape(indices.shape)


def taps(
    x: torch.Tensor, weights: lpips.LpipsWeights, activations: Optional[Sequence[torch.Tensor]] = None, collect: Optional[list] = None
) -> List[torch.Tensor]:
    """The five taps of preprocessed x [B, 3, S, S]; `activations`: the thirteen post-ReLU activations of the run being judged."""
    out = []
    for index, (weight, bias) in enumerate(weights.convs):
        kernel = as_tensor(weight, x.dtype).permute(3, 2, 0, 1)  # HWIO -> OIHW
        pre = torch.nn.functional.conv2d(x, kernel, as_tensor(bias, x.dtype), padding=1)
        given = None if activations is None else activations[index]
        y = bias_relu(pre, given)
        if collect is not None:
            collect.append(y)
        if index in lpips.TAP_LAYERS:
            out.append(y)
        x = max_pool(y, given) if index in lpips.POOL_LAYERS else y
    return out


def normalize(f: torch.Tensor) -> torch.Tensor:
    return f / (torch.linalg.vector_norm(f, dim=1, keepdim=True) + NORM_EPSILON)


def layer_distance(f: torch.Tensor, normalized_target: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """[B]: mean over the pixels of sum_c lin_c (normalize(f)_c - target_c)^2."""
    difference = normalize(f) - normalized_target
    return (lin.reshape(1, -1, 1, 1) * (difference * difference)).sum(dim=1).mean(dim=(1, 2))


def image_distance(
    image: torch.Tensor, other: torch.Tensor, weights: lpips.LpipsWeights, side: int,
    activations: Optional[Sequence[torch.Tensor]] = None, collect: Optional[list] = None,
) -> torch.Tensor:
    """[B]: LPIPS of two float images [B, 3, R, R] in -1 ... 1; the masks of `activations` apply to `image`'s branch only."""
    mine = taps(preprocess(image, side, weights), weights, activations, collect)
    with torch.no_grad():
        theirs = [normalize(tap) for tap in taps(preprocess(other, side, weights), weights)]
    total = None
    for f, target, lin in zip(mine, theirs, weights.lins):
        layer = layer_distance(f, target, as_tensor(lin, image.dtype))
        total = layer if total is None else total + layer
    return total


def distance(
    images: torch.Tensor, targets_u8: torch.Tensor, weights: lpips.LpipsWeights, side: int,
    activations: Optional[Sequence[torch.Tensor]] = None, collect: Optional[list] = None,
) -> torch.Tensor:
    """[B]: the distance `lpips.VGG16Lpips` computes, in images' dtype."""
    return image_distance(images, target_planes(targets_u8, images.dtype), weights, side, activations, collect)


# ---- the whole-chain cases the CPU and the GPU test files share ----

CHAIN_SIDE = 64
CHAIN_SEEDS = (0, 1, 2)
CHAIN_RESOLUTIONS = (64, 128)
CHAIN_BATCHES = (1, 2)
CHAIN_CASES = tuple((seed, resolution, batch) for seed in CHAIN_SEEDS for resolution in CHAIN_RESOLUTIONS for batch in CHAIN_BATCHES)


@functools.lru_cache(maxsize=None)
def chain_weights(seed: int) -> lpips.LpipsWeights:
    return lpips.random_lpips_weights(seed)


def smooth_image(rng: np.random.RandomState, resolution: int) -> np.ndarray:
    """[3, R, R] float32: an 8 x 8 N(0, 1) field enlarged bicubically, plus 0.2 N(0, 1), clamped to -1 ... 1."""
    coarse = torch.from_numpy(rng.randn(1, 3, 8, 8))
    fine = torch.nn.functional.interpolate(coarse, size=(resolution, resolution), mode="bicubic", align_corners=False)[0].numpy()
    return np.clip(fine + 0.2 * rng.randn(3, resolution, resolution), -1.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def chain_sample(seed: int, resolution: int, sample: int) -> Tuple[np.ndarray, np.ndarray]:
    """(image [3, R, R] float32, target [R, R, 3] uint8) of one sample: a function of its three arguments alone."""
    rng = np.random.RandomState([1000 + seed, resolution, sample])
    image = smooth_image(rng, resolution)
    target = np.clip(np.rint(smooth_image(rng, resolution).transpose(1, 2, 0) * 127.5 + 127.5), 0, 255).astype(np.uint8)
    return image, target


def chain_inputs(seed: int, resolution: int, batch: int) -> Tuple[np.ndarray, np.ndarray]:
    """(images [B, 3, R, R] float32, targets [B, R, R, 3] uint8): sample b of any batch is chain_sample(seed, resolution, b)."""
    samples = [chain_sample(seed, resolution, sample) for sample in range(batch)]
    return np.stack([image for image, _ in samples]), np.stack([target for _, target in samples])


class Judged(NamedTuple):
    """One sample through the restatement in one dtype."""

    distance: torch.Tensor  # [1]
    gradient: torch.Tensor  # [1, 3, R, R], of the distance with respect to the image
    activations: Tuple[torch.Tensor, ...]  # thirteen


def run_sample(seed: int, resolution: int, sample: int, dtype: torch.dtype, activations: Optional[Sequence[torch.Tensor]] = None) -> Judged:
    image, target = chain_sample(seed, resolution, sample)
    leaf = as_tensor(image[None], dtype).requires_grad_(True)
    collected: List[torch.Tensor] = []
    total = distance(leaf, torch.from_numpy(target[None]), chain_weights(seed), CHAIN_SIDE, activations, collected)
    (gradient,) = torch.autograd.grad(total.sum(), leaf)
    return Judged(total.detach(), gradient, tuple(activation.detach() for activation in collected))


@functools.lru_cache(maxsize=None)
def sample64(seed: int, resolution: int, sample: int) -> Judged:
    """The float64 restatement with its own masks."""
    return run_sample(seed, resolution, sample, torch.float64)


@functools.lru_cache(maxsize=None)
def sample32(seed: int, resolution: int, sample: int) -> Judged:
    """The float32 restatement with its own masks: the yardstick's run."""
    return run_sample(seed, resolution, sample, torch.float32)


def check_masks(label: str, activations: Sequence[torch.Tensor], want: Sequence[torch.Tensor], who: str = "the run") -> int:
    """
    One sample's part of the flip condition: how many ReLU masks (activation > 0) and pool selections of a run differ from the
    float64 restatement's, after asserting that each differing activation is below grad_ref.SIGN_FLIP_MAGNITUDE of its layer's
    maximum (for a selection: the two values the runs chose between differ by less than that). The cap is on the whole input:
    `check_cap` takes the sum over the samples of a case.
    """
    flips = 0
    assert len(activations) == len(want) == len(lpips.CONV_LAYERS)
    for index, (got, ref) in enumerate(zip(activations, want)):
        got = got.detach().cpu()
        limit = grad_ref.SIGN_FLIP_MAGNITUDE * float(ref.abs().max())
        differ = (got > 0) != (ref > 0)
        count = int(differ.sum())
        if count:
            largest = max(float(got[differ].abs().max()), float(ref[differ].abs().max()))
            assert largest < limit, f"{label} layer {index}: an activation of magnitude {largest:.3e} (limit {limit:.3e}) changed sign"
        flips += count
        if index in lpips.POOL_LAYERS:
            _, mine = torch.nn.functional.max_pool2d(got.double(), 2, return_indices=True)
            pooled, theirs = torch.nn.functional.max_pool2d(ref, 2, return_indices=True)
            moved = mine != theirs
            count = int(moved.sum())
            if count:
                # what the float64 run has at the run's choice is within the limit of its own maximum
                gap = (pooled - ref.flatten(2).gather(2, mine.flatten(2)).reshape(mine.shape))[moved].abs().max()
                assert float(gap) < limit, f"{label} layer {index}: a pool selection moved between values {float(gap):.3e} apart (limit {limit:.3e})"
            flips += count
    print(f"{label}: {flips} masks and selections of {who} differ from the float64 restatement")
    return flips


def check_cap(label: str, flips: int, who: str = "the run") -> None:
    """The cap of the flip condition on one whole-chain input: `flips` is the sum of `check_masks` over its samples."""
    print(f"{label}: {flips} masks and selections of {who} differ from the float64 restatement over the whole input (at most {grad_ref.MAX_SIGN_FLIPS})")
    assert flips <= grad_ref.MAX_SIGN_FLIPS, f"{label}: {flips} masks and selections differ from the float64 restatement (at most {grad_ref.MAX_SIGN_FLIPS})"


@functools.lru_cache(maxsize=None)
def sample_yardstick(seed: int, resolution: int, sample: int) -> Dict[str, torch.Tensor]:
    """
    The float32 restatement of one sample judged as a GPU run is: its flip condition, and the float64 gradient of the mask form
    built from ITS activations. {"distance32", "distance64", "gradient32", "gradient64", "flips" (the count, a tensor)}.
    """
    own, ref = sample32(seed, resolution, sample), sample64(seed, resolution, sample)
    flips = check_masks(f"seed {seed} R {resolution} sample {sample}", own.activations, ref.activations, "the float32 restatement")
    masked = ref if flips == 0 else run_sample(seed, resolution, sample, torch.float64, own.activations)
    return {"distance32": own.distance, "distance64": ref.distance, "gradient32": own.gradient, "gradient64": masked.gradient, "flips": torch.tensor(flips)}


def gradient_yardstick(seed: int, resolution: int, batch: int) -> float:
    """The float32 restatement's own error on the image gradient [B, 3, R, R] of a case; its flips over the whole input meet the cap."""
    parts = [sample_yardstick(seed, resolution, sample) for sample in range(batch)]
    check_cap(f"seed {seed} R {resolution} B {batch}", sum(int(part["flips"]) for part in parts), "the float32 restatement")
    return grad_ref.relative_error(torch.cat([part["gradient32"] for part in parts]), torch.cat([part["gradient64"] for part in parts]))


@functools.lru_cache(maxsize=None)
def distance_yardstick() -> float:
    """The LARGEST float32 own error on the distance over every whole-chain case: one scalar's error on one input is luck."""
    worst = 0.0
    for seed, resolution, batch in CHAIN_CASES:
        parts = [sample_yardstick(seed, resolution, sample) for sample in range(batch)]
        worst = max(worst, grad_ref.relative_error(torch.cat([part["distance32"] for part in parts]), torch.cat([part["distance64"] for part in parts])))
    return worst
