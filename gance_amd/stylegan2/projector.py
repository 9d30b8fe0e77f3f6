"""
Project images into W: the optimiser loop of StyleGAN2's `projector.py` (Karras et al. 2020, appendix D) on
DifferentiableSynthesis, for a batch of independent frames at once.

The arithmetic is restated from the publication (the reference drives the upstream class at
gance/projection/projector_file_writer.py:234-235, 576-613; upstream's source is not vendored there), so parity with an
upstream run is unpinned. Per frame: one w [1, 512] tiled to every dlatent row, starting at the mapping network's mean,
and one noise plane per conv layer, optimised together by Adam against

    loss = distance(image, target) + 1e5 * sum over the layers of noise_regularizer(plane)

with w perturbed by Gaussian noise whose strength falls to zero over the first three quarters of the run. Three things
differ from upstream and are meant to:

* The built-in distance is `torch.ops.gance.pyramid_distance`, a weight-free multi-scale squared difference at 256^2 and
  below. It is NOT upstream's LPIPS: no VGG16 weights are shipped. `distance=` takes any torch callable
  `(images [B, 3, R, R] float in -1 ... 1, targets [B, R, R, 3] uint8) -> [B]`; `gance_amd.stylegan2.lpips.VGG16Lpips` is
  upstream's LPIPS on VGG16 as such a callable, from weights the user supplies (`load_lpips_weights`).
* `start` takes B frames; each has its own w, planes, Adam moments and random draws, and the loss is the sum over the
  frames, so the frames do not interact.
* The random numbers of frame k (`frame_draws`) are a function of (seed, k) alone, whatever the batch it is projected in.
"""

import math
from pathlib import Path
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from gance_amd import torch_ops  # noqa: F401  pylint: disable=unused-import  (registers torch.ops.gance.*)
from gance_amd.stylegan2 import spec as sg2_spec

Distance = Callable[[torch.Tensor, torch.Tensor], torch.Tensor]

DISTANCE_SIDE = 256  # the side images and targets are area-averaged to before the built-in distance


def mapping_dlatents(variables: sg2_spec.Variables, z: torch.Tensor) -> torch.Tensor:
    """
    G_mapping without the broadcast to rows: z [N, 512] -> w [N, 512] in z's dtype, on z's device. Normalises z, then 8
    dense layers with lrmul 0.01 (weight * lrmul / sqrt(fan_in), bias * lrmul) and leaky ReLU 0.2 times sqrt(2).
    """
    x = z * torch.rsqrt((z * z).mean(dim=1, keepdim=True) + 1e-8)
    for layer in range(sg2_spec.MAPPING_LAYERS):
        weight = torch.from_numpy(np.asarray(variables[f"G_mapping/Dense{layer}/weight"])).to(device=z.device, dtype=z.dtype)
        bias = torch.from_numpy(np.asarray(variables[f"G_mapping/Dense{layer}/bias"])).to(device=z.device, dtype=z.dtype)
        weight = weight * (1.0 / np.sqrt(weight.shape[0]) * sg2_spec.MAPPING_LRMUL)
        x = torch.nn.functional.leaky_relu(x @ weight + bias * sg2_spec.MAPPING_LRMUL, 0.2) * np.sqrt(2.0)
    return x


class FrameDraws(NamedTuple):
    """The random numbers one frame's projection reads."""

    w_noise: np.ndarray  # [num_steps, 512] float32: step s perturbs w with row s
    planes: Tuple[np.ndarray, ...]  # per conv layer [1, S, S] float32: the initial noise planes


def frame_draws(seed: int, frame: int, num_steps: int, noise_sides: Sequence[int]) -> FrameDraws:
    """The draws of frame `frame` (its index in the whole run, not in its batch): a function of (seed, frame) alone."""
    rng = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(frame) & 0xFFFFFFFF])
    w_noise = rng.randn(num_steps, sg2_spec.DLATENT_SIZE).astype(np.float32)
    return FrameDraws(w_noise, tuple(rng.randn(1, side, side).astype(np.float32) for side in noise_sides))


class Projector:  # pylint: disable=too-many-instance-attributes
    """
    The surface the reference drives: set_network, start, step, get_cur_step, get_dlatents, get_noises, get_images,
    num_steps. Upstream's constants are attributes, as upstream has them.
    """

    def __init__(self, num_steps: Optional[int] = 1000, distance: Optional[Distance] = None, seed: int = 0) -> None:
        self.num_steps = 1000 if num_steps is None else int(num_steps)
        self.dlatent_avg_samples = 10000
        self.initial_learning_rate = 0.1
        self.initial_noise_factor = 0.05
        self.lr_rampdown_length = 0.25
        self.lr_rampup_length = 0.05
        self.noise_ramp_length = 0.75
        self.regularize_noise_weight = 1e5
        self.adam_beta1, self.adam_beta2, self.adam_epsilon = 0.9, 0.999, 1e-8
        self.distance = distance
        self.seed = int(seed)
        self.first_frame = 0  # the run-wide index of the next `start`'s first frame: `start` advances it by its batch

        self._synthesis: Any = None
        self._variables: Optional[sg2_spec.Variables] = None
        self.dlatent_avg: Optional[torch.Tensor] = None  # [1, 1, 512]
        self.dlatent_std: Optional[float] = None
        self._cur_step = 0
        self._w: Optional[torch.Tensor] = None
        self._planes: List[torch.Tensor] = []
        self._moments: Tuple[List[torch.Tensor], List[torch.Tensor]] = ([], [])
        self._w_noise: Optional[torch.Tensor] = None  # [B, num_steps, 512]
        self._targets_u8: Optional[torch.Tensor] = None
        self._targets: Optional[torch.Tensor] = None
        self._images: Optional[torch.Tensor] = None
        self.last_distance: Optional[torch.Tensor] = None  # [B], of the step's perturbed w
        self.last_regularizer: Optional[torch.Tensor] = None  # [B], summed over the layers, unweighted

    # ---- schedules ----

    def noise_strength(self, step: int) -> float:
        """dlatent_std * 0.05 * max(0, 1 - t / 0.75)^2 with t = step / num_steps."""
        t = step / self.num_steps
        assert self.dlatent_std is not None
        return self.dlatent_std * self.initial_noise_factor * max(0.0, 1.0 - t / self.noise_ramp_length) ** 2

    def learning_rate(self, step: int) -> float:
        """0.1 * cosine ramp-down over the last quarter * linear ramp-up over the first twentieth."""
        t = step / self.num_steps
        ramp = min(1.0, (1.0 - t) / self.lr_rampdown_length)
        ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
        ramp = ramp * min(1.0, t / self.lr_rampup_length)
        return self.initial_learning_rate * ramp

    # ---- the network ----

    def set_network(self, network: Any) -> None:
        """
        :param network: a network_functions.LoadedNetwork, or (variables, resolution); config-e is told from the variables.
        Builds the differentiable generator and the W statistics: 10 000 z of RandomState(123) through the mapping network,
        their mean [1, 1, 512] and one scalar sqrt(sum (w - mean)^2 / 10 000).
        """
        from gance_amd.stylegan2.differentiable import DifferentiableSynthesis  # pylint: disable=import-outside-toplevel

        if isinstance(network, tuple):
            variables, resolution = network
            self._synthesis = DifferentiableSynthesis(variables, int(resolution))
        else:
            from gance_amd import network_file  # pylint: disable=import-outside-toplevel

            variables = network_file.load_network(Path(network.network_path)).variables
            self._synthesis = network.differentiable()
        self._variables = variables
        z = torch.from_numpy(np.random.RandomState(123).randn(self.dlatent_avg_samples, sg2_spec.LATENT_SIZE).astype(np.float32))
        with torch.no_grad():
            w = mapping_dlatents(variables, z.to(self._synthesis.device))
            average = w.mean(dim=0, keepdim=True)
            self.dlatent_std = float(torch.sqrt(((w - average) ** 2).sum() / self.dlatent_avg_samples))
            self.dlatent_avg = average[None].contiguous()
        self._w = None

    @property
    def resolution(self) -> int:
        return int(self._synthesis.resolution)

    @property
    def noise_sides(self) -> Tuple[int, ...]:
        """The side of every conv layer's noise plane, in layer order."""
        return tuple(int(conv.noise.shape[2]) for conv in self._synthesis.convs)

    # ---- one projection ----

    def start(self, targets: Union[np.ndarray, torch.Tensor]) -> None:
        """
        Begin projecting `targets` [B, R, R, 3] uint8 (host or device), R the network's resolution. Frame b of the batch is
        frame first_frame + b of the run and reads that frame's draws.
        """
        if self._synthesis is None:
            raise RuntimeError("set_network comes before start")
        device, side = self._synthesis.device, self.resolution
        targets = torch.as_tensor(targets)
        if targets.dtype != torch.uint8 or targets.dim() != 4 or tuple(targets.shape[1:]) != (side, side, 3) or targets.shape[0] < 1:
            raise ValueError(f"targets must be uint8 [B, {side}, {side}, 3], got {targets.dtype} {list(targets.shape)}")
        batch = int(targets.shape[0])
        self._targets_u8 = targets.to(device).contiguous()
        planes_f32 = self._targets_u8.permute(0, 3, 1, 2).to(torch.float32)
        if side > DISTANCE_SIDE:  # upstream's reshape-mean to 256^2
            factor = side // DISTANCE_SIDE
            planes_f32 = planes_f32.reshape(batch, 3, DISTANCE_SIDE, factor, DISTANCE_SIDE, factor).mean(dim=(3, 5))
        self._targets = planes_f32.contiguous()

        draws = [frame_draws(self.seed, self.first_frame + b, self.num_steps, self.noise_sides) for b in range(batch)]
        self.first_frame += batch
        self._w_noise = torch.from_numpy(np.stack([draw.w_noise for draw in draws])).to(device)
        assert self.dlatent_avg is not None
        self._w = self.dlatent_avg.repeat(batch, 1, 1).requires_grad_(True)
        self._planes = [
            torch.from_numpy(np.stack([draw.planes[layer] for draw in draws])).to(device).requires_grad_(True) for layer in range(len(self.noise_sides))
        ]
        parameters = [self._w, *self._planes]
        self._moments = ([torch.zeros_like(p) for p in parameters], [torch.zeros_like(p) for p in parameters])
        self._cur_step = 0
        self._images = None

    def _noise(self) -> Dict[int, torch.Tensor]:
        return {conv.layer_idx: plane for conv, plane in zip(self._synthesis.convs, self._planes)}

    def _distance(self, images: torch.Tensor) -> torch.Tensor:
        if self.distance is not None:
            return self.distance(images, self._targets_u8)
        return torch.ops.gance.pyramid_distance(images, self._targets)

    def set_variables(self, w: torch.Tensor, planes: Sequence[torch.Tensor]) -> None:
        """Replace what is being optimised (after `start`): w [B, 1, 512] and one plane [B, 1, S, S] per conv layer; the Adam moments stay."""
        assert self._w is not None and w.shape == self._w.shape and [p.shape for p in planes] == [p.shape for p in self._planes]
        with torch.no_grad():
            self._w.copy_(w)
            for mine, given in zip(self._planes, planes):
                mine.copy_(given)

    @property
    def variables(self) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """(w [B, 1, 512], the planes): the leaves on the device that `loss_terms` differentiates with respect to."""
        assert self._w is not None
        return self._w, list(self._planes)

    def _regularizer(self, plane: torch.Tensor) -> torch.Tensor:  # pylint: disable=no-self-use
        return torch.ops.gance.noise_regularizer(plane)

    def loss_terms(self, w_offset: Optional[torch.Tensor] = None, collect: Optional[List[torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """
        (images [B, 3, R, R], distance [B], regulariser [B] summed over the layers, unweighted) at the current w (+ `w_offset`
        [B, 1, 512]) and planes, with a graph behind them. loss = (distance + regularize_noise_weight * regulariser).sum().
        `collect` receives the activation after every conv layer.
        """
        assert self._w is not None
        w = self._w if w_offset is None else self._w + w_offset
        images = self._synthesis(w.expand(-1, self._synthesis.num_layers, -1), noise=self._noise(), collect=collect)
        distance = self._distance(images)
        regularizer = self._regularizer(self._planes[0])
        for plane in self._planes[1:]:
            regularizer = regularizer + self._regularizer(plane)
        return images, distance, regularizer

    def step(self) -> None:
        """One optimisation step of every frame of the batch."""
        if self._w is None:
            raise RuntimeError("start comes before step")
        assert self._w_noise is not None
        step = self._cur_step
        offset = self._w_noise[:, step : step + 1] * self.noise_strength(step)
        images, distance, regularizer = self.loss_terms(offset)
        loss = (distance + self.regularize_noise_weight * regularizer).sum()
        parameters = [self._w, *self._planes]
        gradients = list(torch.autograd.grad(loss, parameters))
        self._images, self.last_distance, self.last_regularizer = images.detach(), distance.detach(), regularizer.detach()

        # Adam as TensorFlow 1 writes it: the bias corrections scale the rate, and epsilon is added to sqrt(v) uncorrected.
        # torch.optim.Adam divides by sqrt(v / (1 - beta2^k)) + epsilon instead, which is another update while v is small.
        count = step + 1
        rate = self.learning_rate(step) * math.sqrt(1.0 - self.adam_beta2 ** count) / (1.0 - self.adam_beta1 ** count)
        first, second = self._moments
        with torch.no_grad():
            torch._foreach_mul_(first, self.adam_beta1)  # pylint: disable=protected-access
            torch._foreach_add_(first, gradients, alpha=1.0 - self.adam_beta1)  # pylint: disable=protected-access
            torch._foreach_mul_(second, self.adam_beta2)  # pylint: disable=protected-access
            torch._foreach_addcmul_(second, gradients, gradients, value=1.0 - self.adam_beta2)  # pylint: disable=protected-access
            denominators = torch._foreach_sqrt(second)  # pylint: disable=protected-access
            torch._foreach_add_(denominators, self.adam_epsilon)  # pylint: disable=protected-access
            torch._foreach_addcdiv_(parameters, first, denominators, value=-rate)  # pylint: disable=protected-access
            # every plane of every sample back to zero mean and unit RMS
            for plane in self._planes:
                plane -= plane.mean(dim=(1, 2, 3), keepdim=True)
                plane *= torch.rsqrt((plane * plane).mean(dim=(1, 2, 3), keepdim=True))
        self._cur_step += 1

    def get_cur_step(self) -> int:
        return self._cur_step

    def get_dlatents(self) -> np.ndarray:
        """[B, W, 512] float32: w tiled to every row."""
        assert self._w is not None
        return self._w.detach().expand(-1, self._synthesis.num_layers, -1).cpu().numpy().copy()

    def get_noises(self) -> List[np.ndarray]:
        """Per conv layer [B, 1, S, S] float32."""
        return [plane.detach().cpu().numpy() for plane in self._planes]

    def get_images(self) -> np.ndarray:
        """[B, 3, R, R] float32 in -1 ... 1: the images the last step judged (of the perturbed w)."""
        if self._images is None:
            raise RuntimeError("step comes before get_images")
        return self._images.cpu().numpy()

    def final_images_device(self) -> torch.Tensor:
        """uint8 [B, R, R, 3] on the device: the image of w alone (no perturbation) with the optimised planes, converted as the engine converts."""
        with torch.no_grad():
            images = self.loss_terms()[0]
            return torch.clamp(images.permute(0, 2, 3, 1) * 127.5 + 128.0, 0.0, 255.0).to(torch.uint8).contiguous()
