"""
LPIPS on VGG16 (Zhang et al. 2018), the distance StyleGAN2's projector minimises (Karras et al. 2020, appendix D), from
weights the USER supplies: none are shipped, and none were available when this was written. The arithmetic is restated from
the publications, so parity with an upstream run is unpinned.

    images [B, 3, R, R] in -1 ... 1, targets [B, R, R, 3] uint8 -> t / 127.5 - 1
    R > side: both area-averaged by R / side;  (x - shift_c) / scale_c
    VGG16's thirteen 3x3 convolutions + bias + ReLU, 2x2 max pools after conv1_2, 2_2, 3_3 and 4_3
    taps f_l after relu1_2, 2_2, 3_3, 4_3, 5_3:  u = f / (|f|_2 over the channels + 1e-10) per pixel
    distance = sum_l mean over the pixels of sum_c lin_l[c] * (u_c(image) - u_c(target))^2

`VGG16Lpips` is a `projector.Distance`: `Projector(distance=VGG16Lpips(load_lpips_weights(path)))`. The convolutions run
through torch.ops.gance.modconv3x3 with unit style and demodulation or, with `convolution="conv3x3"`, through the plain
convolution torch.ops.gance.conv3x3 (csrc/conv3x3.hip); the rest is csrc/lpips.hip.
"""

from pathlib import Path
from typing import Any, List, Mapping, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from gance_amd import torch_ops  # noqa: F401  pylint: disable=unused-import  (registers torch.ops.gance.*)

# (name, Cin, Cout) of the thirteen convolutions, in order
CONV_LAYERS: Tuple[Tuple[str, int, int], ...] = (
    ("conv1_1", 3, 64), ("conv1_2", 64, 64),
    ("conv2_1", 64, 128), ("conv2_2", 128, 128),
    ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256),
    ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512),
    ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512),
)  # fmt: skip
TAP_LAYERS = (1, 3, 6, 9, 12)  # indices into CONV_LAYERS whose ReLU output is a tap
POOL_LAYERS = (1, 3, 6, 9)  # ... and is max-pooled for the next convolution
TAP_CHANNELS = tuple(CONV_LAYERS[index][2] for index in TAP_LAYERS)
DEFAULT_SHIFT = (-0.030, -0.088, -0.188)
DEFAULT_SCALE = (0.458, 0.448, 0.450)
DEFAULT_SIDE = 256  # upstream's projector judges at 256^2
CONVOLUTIONS = ("modconv3x3", "conv3x3")  # the op the thirteen convolutions run through
# torchvision's vgg16().features: the Sequential indices of the thirteen Conv2d
TORCHVISION_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)


class LpipsWeights(NamedTuple):
    """What LPIPS on VGG16 reads, float32 on the host."""

    convs: Tuple[Tuple[np.ndarray, np.ndarray], ...]  # thirteen (weight [3, 3, Cin, Cout], bias [Cout])
    lins: Tuple[np.ndarray, ...]  # five [C], not negative
    shift: np.ndarray  # [3]
    scale: np.ndarray  # [3]


def _checked(key: str, value: Any, shape: Tuple[int, ...], non_negative: bool = False) -> np.ndarray:
    array = np.asarray(value)
    if tuple(array.shape) != shape:
        raise ValueError(f"`{key}` must be {list(shape)}, got {list(array.shape)}")
    if array.dtype.kind not in "fiu":
        raise ValueError(f"`{key}` must be numeric, got {array.dtype}")
    array = np.ascontiguousarray(array, dtype=np.float32)
    if not np.isfinite(array).all():
        raise ValueError(f"`{key}` holds a value that is not finite")
    if non_negative and (array < 0).any():
        raise ValueError(f"`{key}` holds a negative value")
    return array


def _entries(weights: LpipsWeights) -> List[Tuple[str, np.ndarray, Tuple[int, ...], bool]]:
    """(key, array, shape, must not be negative) of every array, in the file's order."""
    if len(weights.convs) != len(CONV_LAYERS) or len(weights.lins) != len(TAP_LAYERS):
        raise ValueError(f"weights must hold {len(CONV_LAYERS)} convolutions and {len(TAP_LAYERS)} lin vectors")
    entries = []
    for (name, cin, cout), (weight, bias) in zip(CONV_LAYERS, weights.convs):
        entries.append((f"{name}/weight", weight, (3, 3, cin, cout), False))
        entries.append((f"{name}/bias", bias, (cout,), False))
    for index, (channels, lin) in enumerate(zip(TAP_CHANNELS, weights.lins)):
        entries.append((f"lin{index}", lin, (channels,), True))
    entries.append(("shift", weights.shift, (3,), False))
    entries.append(("scale", weights.scale, (3,), False))
    return entries


def validate_lpips_weights(weights: LpipsWeights) -> LpipsWeights:
    """The same weights as contiguous float32 arrays.
    :raises ValueError: a wrong shape, a value that is not finite, a negative lin entry, a zero scale; the message names the key."""
    arrays = {key: _checked(key, array, shape, non_negative) for key, array, shape, non_negative in _entries(weights)}
    if (arrays["scale"] == 0).any():
        raise ValueError("`scale` holds a zero")
    return _from_arrays(arrays)


def _from_arrays(arrays: Mapping[str, np.ndarray]) -> LpipsWeights:
    return LpipsWeights(
        tuple((arrays[f"{name}/weight"], arrays[f"{name}/bias"]) for name, _, _ in CONV_LAYERS),
        tuple(arrays[f"lin{index}"] for index in range(len(TAP_LAYERS))),
        arrays["shift"],
        arrays["scale"],
    )


def save_lpips_weights(path: Union[str, Path], weights: LpipsWeights) -> None:
    """Write an .npz with conv1_1/weight, conv1_1/bias ... conv5_3/bias, lin0 ... lin4, shift and scale (float32)."""
    weights = validate_lpips_weights(weights)
    with open(path, "wb") as file:
        np.savez(file, **{key: array for key, array, _, _ in _entries(weights)})


def load_lpips_weights(path: Union[str, Path]) -> LpipsWeights:
    """
    Read what `save_lpips_weights` wrote (allow_pickle=False).
    :raises ValueError: a missing key, a wrong shape, a value that is not finite or a negative lin entry, naming the key.
    """
    arrays = {}
    with np.load(path, allow_pickle=False) as file:
        for name, _, _ in CONV_LAYERS:
            for key in (f"{name}/weight", f"{name}/bias"):
                arrays[key] = _need(file, key)
        for index in range(len(TAP_LAYERS)):
            arrays[f"lin{index}"] = _need(file, f"lin{index}")
        arrays["shift"], arrays["scale"] = _need(file, "shift"), _need(file, "scale")
    return validate_lpips_weights(_from_arrays(arrays))


def _need(mapping: Any, key: str) -> np.ndarray:
    if key not in mapping:
        raise ValueError(f"`{key}` is missing")
    value = mapping[key]
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    return np.asarray(value)


def lpips_weights_from_state_dicts(vgg_features: Mapping[str, Any], lpips_linear: Mapping[str, Any]) -> LpipsWeights:
    """
    From two mappings of arrays or tensors under the key names of
      * torchvision's `vgg16().features.state_dict()`: `{0,2,5,7,10,12,14,17,19,21,24,26,28}.weight` [Cout, Cin, 3, 3] and `.bias`,
        each optionally prefixed `features.` (the whole model's state dict);
      * the LPIPS package's linear layers: `lin{0..4}.model.1.weight` [1, C, 1, 1].
    Shift and scale are the publication's. The key names are written from those packages' documentation: no file of either was at
    hand to check them against.
    :raises ValueError: a missing key or a wrong shape, naming the key.
    """
    prefix = "features." if any(str(key).startswith("features.") for key in vgg_features) else ""
    convs = []
    for index, (_, cin, cout) in zip(TORCHVISION_CONV_INDICES, CONV_LAYERS):
        weight_key, bias_key = f"{prefix}{index}.weight", f"{prefix}{index}.bias"
        weight = _checked(weight_key, _need(vgg_features, weight_key), (cout, cin, 3, 3))
        bias = _checked(bias_key, _need(vgg_features, bias_key), (cout,))
        convs.append((np.ascontiguousarray(weight.transpose(2, 3, 1, 0)), bias))  # OIHW -> HWIO
    lins = []
    for index, channels in enumerate(TAP_CHANNELS):
        key = f"lin{index}.model.1.weight"
        lins.append(_checked(key, _need(lpips_linear, key), (1, channels, 1, 1), non_negative=True).reshape(channels))
    return validate_lpips_weights(
        LpipsWeights(tuple(convs), tuple(lins), np.asarray(DEFAULT_SHIFT, dtype=np.float32), np.asarray(DEFAULT_SCALE, dtype=np.float32))
    )


def random_lpips_weights(seed: int) -> LpipsWeights:
    """Weights for tests and rate measurements: convolutions N(0, 2 / (9 Cin)), biases N(0, 0.1^2), lin = 0.1 |N(0, 1)|."""
    rng = np.random.RandomState(seed)
    convs = []
    for _, cin, cout in CONV_LAYERS:
        weight = (rng.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9.0 * cin))).astype(np.float32)
        convs.append((weight, (rng.randn(cout) * 0.1).astype(np.float32)))
    lins = tuple((0.1 * np.abs(rng.randn(channels))).astype(np.float32) for channels in TAP_CHANNELS)
    return LpipsWeights(tuple(convs), lins, np.asarray(DEFAULT_SHIFT, dtype=np.float32), np.asarray(DEFAULT_SCALE, dtype=np.float32))


def check_side(side: int) -> int:
    """:raises ValueError: a side that is not a multiple of 16 of at least 64 (conv5 runs at side / 16, the kernels from 4 up)."""
    side = int(side)
    if side < 64 or side > 1024 or side % 16 != 0:
        raise ValueError(f"`side` must be a multiple of 16 in [64, 1024], got {side}")
    return side


class VGG16Lpips:
    """
    The distance as a callable `(images [B, 3, R, R] float32 on the device, targets [B, R, R, 3] uint8) -> [B]` with a graph
    back to `images`. R is a multiple of 16 of at least 64; above `side` it must be a multiple of `side` and both inputs are
    area-averaged to `side`. The target's five normalised taps are kept for as long as the same `targets` tensor, unmodified,
    is handed over (the projector hands one tensor for every step of a `start`).
    """

    def __init__(
        self, weights: LpipsWeights, side: int = DEFAULT_SIDE, device: Optional[Union[int, torch.device]] = None, convolution: str = "modconv3x3"
    ) -> None:
        """
        :param convolution: "modconv3x3" (gance::modconv3x3 with unit style and demodulation) or "conv3x3" (gance::conv3x3).
        :raises ValueError: bad `side`, `convolution` or weights, before a device is touched.
        :raises RuntimeError: no GPU (there is no CPU path).
        """
        self.side = check_side(side)
        if convolution not in CONVOLUTIONS:
            raise ValueError(f"`convolution` must be one of {list(CONVOLUTIONS)}, got {convolution!r}")
        self.convolution = convolution
        weights = validate_lpips_weights(weights)
        if not torch.cuda.is_available():
            raise RuntimeError("VGG16Lpips needs an MI355X: there is no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._convs = []
        for (_, cin, _), (weight, bias) in zip(CONV_LAYERS, weights.convs):
            if cin < torch_ops.LPIPS_INPUT_CHANNELS:  # conv1_1: the input op's zero channels meet zero weights
                weight = np.concatenate([weight, np.zeros((3, 3, torch_ops.LPIPS_INPUT_CHANNELS - cin, weight.shape[3]), dtype=np.float32)], axis=2)
            self._convs.append((torch.from_numpy(np.ascontiguousarray(weight)).to(self.device), torch.from_numpy(bias).to(self.device)))
        # the images under which gance::conv3x3 is its own input gradient, built once
        self._transposed = [torch_ops.conv3x3_transposed_weight(weight) for weight, _ in self._convs] if convolution == "conv3x3" else []
        self._lins = [torch.from_numpy(lin).to(self.device) for lin in weights.lins]
        self._shift, self._scale = torch.from_numpy(weights.shift).to(self.device), torch.from_numpy(weights.scale).to(self.device)
        self._ones: dict = {}
        self._kept: Optional[Tuple[torch.Tensor, int, List[torch.Tensor]]] = None  # (targets, its _version, the normalised taps)
        self.target_passes = 0  # how many times the target's taps were computed

    def _unit(self, batch: int, channels: int) -> torch.Tensor:
        """ones [batch, channels]: the style and the demodulation of a plain convolution."""
        key = (batch, channels)
        if key not in self._ones:
            self._ones[key] = torch.ones(key, dtype=torch.float32, device=self.device)
        return self._ones[key]

    def judged_side(self, resolution: int) -> int:
        """The side an R x R input is judged at.
        :raises ValueError: an R this distance does not take."""
        if resolution < 64 or resolution % 16 != 0:
            raise ValueError(f"the resolution must be a multiple of 16 of at least 64, got {resolution}")
        if resolution <= self.side:
            return resolution
        if resolution % self.side != 0:
            raise ValueError(f"a resolution above the side {self.side} must be a multiple of it, got {resolution}")
        return self.side

    def taps(self, images: torch.Tensor, collect: Optional[List[torch.Tensor]] = None, side: Optional[int] = None) -> List[torch.Tensor]:
        """
        The five tap activations of images [B, 3, R, R] in -1 ... 1; `collect` receives the thirteen post-ReLU activations;
        `side`: `judged_side` of R where the caller has it already.
        """
        batch = int(images.shape[0])
        x = torch.ops.gance.lpips_input(images, self._shift, self._scale, self.judged_side(int(images.shape[2])) if side is None else side)
        taps = []
        for index, (weight, bias) in enumerate(self._convs):
            if self.convolution == "conv3x3":
                x = torch.ops.gance.conv3x3(x, weight, self._transposed[index])
            else:
                x = torch.ops.gance.modconv3x3(x, self._unit(batch, int(weight.shape[2])), self._unit(batch, int(weight.shape[3])), weight, False)
            if index in POOL_LAYERS:
                y, x = torch.ops.gance.bias_relu_pool(x, bias)
            else:
                y = x = torch.ops.gance.bias_relu(x, bias)
            if collect is not None:
                collect.append(y)
            if index in TAP_LAYERS:
                taps.append(y)
        return taps

    def _target_taps(self, targets: torch.Tensor, side: int) -> List[torch.Tensor]:
        if self._kept is not None and self._kept[0] is targets and self._kept[1] == targets._version:  # pylint: disable=protected-access
            return self._kept[2]
        with torch.no_grad():
            planes = targets.to(self.device).permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0
            normalised = [torch.ops.gance.lpips_normalize(tap) for tap in self.taps(planes.contiguous(), side=side)]
        self.target_passes += 1
        self._kept = (targets, targets._version, normalised)  # pylint: disable=protected-access
        return normalised

    def __call__(self, images: torch.Tensor, targets: torch.Tensor, collect: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
            raise ValueError(f"`images` must be [B, 3, R, R], got {list(images.shape)}")
        batch, resolution = int(images.shape[0]), int(images.shape[2])
        if targets.dtype != torch.uint8 or tuple(targets.shape) != (batch, resolution, resolution, 3):
            raise ValueError(f"`targets` must be uint8 {[batch, resolution, resolution, 3]}, got {targets.dtype} {list(targets.shape)}")
        side = self.judged_side(resolution)
        wanted = self._target_taps(targets, side)
        distance = None
        for tap, target, lin in zip(self.taps(images, collect, side), wanted, self._lins):
            layer = torch.ops.gance.lpips_layer(tap, target, lin)
            distance = layer if distance is None else distance + layer
        assert distance is not None
        return distance
