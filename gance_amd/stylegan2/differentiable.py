"""
Differentiable synthesis: the generator's float image with a `torch.autograd` graph back to the dlatents.

The engine (gance_amd.hip_lib.Engine) is forward-only: its kernel forms store activations pre-multiplied by the next
layer's style, do not store the last one, and change with the batch. This is the second, plain-form path through the same
arithmetic (G_synthesis_stylegan2, architecture 'skip', stored noise buffers): every layer is three custom ops whose
forward and backward are HIP kernels (gance_amd/csrc/synthesis_grad.hip through gance_amd.torch_ops),

    x = gance::modconv3x3(x, style, demod, weight, up)          modulated 3x3 conv, demodulation as an input
    x = gance::noise_bias_lrelu(x, noise, strength, bias)       the layer's epilogue
    y = gance::torgb_skip(x, style, weight, bias, y_prev)       the image step of the skip architecture

and the per-layer plumbing is plain torch on the device, because it is tiny:

    style = dlatents[:, row] @ mod_weight + mod_bias + 1        [B, Cin]
    demod = rsqrt(style^2 @ sum_tap(weight^2) + 1e-8)           [B, Cout]

so autograd itself carries the ops' grad_style and grad_demod back to the dlatents. Gradients exist for the dlatents and for
noise planes passed as tensors that require grad (not for weights, noise strengths or biases); the mapping network is not
part of it: projection works in W. What it is for: optimising dlatents against any loss written in PyTorch
(gance_amd/stylegan2/projector.py is the reference's projection, gance/projection/projector.py, built on it).
"""

from typing import Dict, List, Optional, Union

import numpy as np
import torch

from gance_amd import torch_ops  # noqa: F401  pylint: disable=unused-import  (registers torch.ops.gance.*)
from gance_amd.stylegan2 import spec as sg2_spec

NoisePlanes = Dict[int, Union[np.ndarray, torch.Tensor]]


def _runtime_scaled(raw: np.ndarray) -> np.ndarray:
    """`get_weight` with use_wscale=True: raw * 1 / sqrt(fan_in), fan_in = every axis but the last; in float64, rounded once."""
    raw = np.asarray(raw, dtype=np.float64)
    return raw * (1.0 / np.sqrt(float(np.prod(raw.shape[:-1]))))


class _ConvWeights:  # pylint: disable=too-few-public-methods
    """One modulated 3x3 conv layer's tensors on the device."""

    def __init__(self, variables: sg2_spec.Variables, conv: sg2_spec.ConvLayer, device: torch.device) -> None:
        scope = f"G_synthesis/{conv.scope}"
        weight = _runtime_scaled(variables[f"{scope}/weight"])  # [3, 3, Cin, Cout]

        def upload(array: np.ndarray) -> torch.Tensor:
            return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(device)

        self.layer_idx, self.up = conv.layer_idx, conv.up
        self.weight = upload(weight)
        self.weight_squares = upload((weight ** 2).sum(axis=(0, 1)))  # [Cin, Cout]: the demodulation's sum over the taps
        self.mod_weight = upload(_runtime_scaled(variables[f"{scope}/mod_weight"]))  # [512, Cin]
        self.mod_bias = upload(variables[f"{scope}/mod_bias"])
        self.noise = upload(variables[f"G_synthesis/noise{conv.layer_idx}"])  # [1, 1, S, S]
        self.noise_strength = upload(np.reshape(variables[f"{scope}/noise_strength"], (1,)))
        self.bias = upload(variables[f"{scope}/bias"])


class _ToRGBWeights:  # pylint: disable=too-few-public-methods
    """One ToRGB layer's tensors on the device."""

    def __init__(self, variables: sg2_spec.Variables, rgb: sg2_spec.ToRGBLayer, device: torch.device) -> None:
        scope = f"G_synthesis/{rgb.scope}"

        def upload(array: np.ndarray) -> torch.Tensor:
            return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(device)

        self.dlatent_row = rgb.dlatent_row
        self.weight = upload(_runtime_scaled(variables[f"{scope}/weight"]).reshape(rgb.cin, sg2_spec.NUM_CHANNELS))
        self.mod_weight = upload(_runtime_scaled(variables[f"{scope}/mod_weight"]))
        self.mod_bias = upload(variables[f"{scope}/mod_bias"])
        self.bias = upload(variables[f"{scope}/bias"])


class DifferentiableSynthesis:
    """
    dlatents [B, W, 512] (cuda, float32) -> image [B, 3, R, R] float32 with a graph behind it:

        synthesis = DifferentiableSynthesis(variables, 256)
        w = torch.zeros((1, synthesis.num_layers, 512), device="cuda", requires_grad=True)
        loss = my_loss(synthesis(w)); loss.backward(); w.grad ...

    Two backward passes over the same values give the same bits (the kernels use no atomics).
    """

    def __init__(
        self, variables: sg2_spec.Variables, resolution: int, fmap_base: Optional[int] = None, device: Optional[Union[int, torch.device]] = None
    ) -> None:
        """
        Uploads the raw variables once, runtime-scaled as `spec` names and shapes them. `fmap_base` None: told from the
        variables (spec.fmap_base_of); `device` None: the current GPU.
        :raises RuntimeError: no GPU (there is no CPU path).
        """
        if not torch.cuda.is_available():
            raise RuntimeError("DifferentiableSynthesis needs an MI355X: there is no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if fmap_base is None:
            fmap_base = sg2_spec.fmap_base_of(variables, resolution)
        self.spec = sg2_spec.make_spec(resolution, fmap_base)
        sg2_spec.pack_variables(variables, self.spec)  # validates names and shapes
        self.resolution, self.num_layers = self.spec.resolution, self.spec.num_layers
        self.const = torch.from_numpy(np.ascontiguousarray(variables["G_synthesis/4x4/Const/const"], dtype=np.float32)).to(self.device)
        self.convs = [_ConvWeights(variables, conv, self.device) for conv in self.spec.convs]
        self.torgbs = [_ToRGBWeights(variables, rgb, self.device) for rgb in self.spec.torgbs]

    def _noise(self, conv: _ConvWeights, noise: Optional[NoisePlanes], batch: int) -> torch.Tensor:
        if noise is None or conv.layer_idx not in noise:
            return conv.noise
        # (a float32 tensor already on the device passes through both calls as itself: it may be a leaf that requires grad)
        planes = torch.as_tensor(noise[conv.layer_idx], dtype=torch.float32).to(self.device)
        side = conv.noise.shape[2]
        if planes.dim() != 4 or planes.shape[0] not in (1, batch) or tuple(planes.shape[1:]) != (1, side, side):
            raise ValueError(f"noise of layer {conv.layer_idx} must be [1 or {batch}, 1, {side}, {side}], got {list(planes.shape)}")
        return planes

    def __call__(self, dlatents: torch.Tensor, noise: Optional[NoisePlanes] = None, collect: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
        """
        :param dlatents: [B, W, 512] float32 on this object's device; may require grad.
        :param noise: layer index -> planes [1 or B, 1, S, S] replacing that layer's stored buffer.
        :param collect: a list that receives the activation after every conv layer, in order.
        :return: the image [B, 3, R, R] float32 (before any uint8 conversion).
        """
        if dlatents.dim() != 3 or dlatents.shape[1] != self.num_layers or dlatents.shape[2] != sg2_spec.DLATENT_SIZE:
            raise ValueError(f"dlatents must be [B, {self.num_layers}, {sg2_spec.DLATENT_SIZE}], got {list(dlatents.shape)}")
        if dlatents.device != self.device or dlatents.dtype != torch.float32:
            raise ValueError(f"dlatents must be float32 on {self.device}, got {dlatents.dtype} on {dlatents.device}")
        batch = dlatents.shape[0]
        x = self.const.expand(batch, -1, -1, -1).contiguous()
        y: Optional[torch.Tensor] = None
        torgbs = iter(self.torgbs)
        for conv in self.convs:
            style = dlatents[:, conv.layer_idx] @ conv.mod_weight + conv.mod_bias + 1.0
            demod = torch.rsqrt((style * style) @ conv.weight_squares + 1e-8)
            x = torch.ops.gance.modconv3x3(x, style, demod, conv.weight, conv.up)
            x = torch.ops.gance.noise_bias_lrelu(x, self._noise(conv, noise, batch), conv.noise_strength, conv.bias)
            if collect is not None:
                collect.append(x)
            if not conv.up:  # the last conv of its resolution: the image step
                rgb = next(torgbs)
                style = dlatents[:, rgb.dlatent_row] @ rgb.mod_weight + rgb.mod_bias + 1.0
                y = torch.ops.gance.torgb_skip(x, style, rgb.weight, rgb.bias, y)
        assert y is not None
        return y
