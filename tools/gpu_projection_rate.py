"""
Cost of one projector step on one GPU (`timeout 900 python tools/gpu_projection_rate.py [--out FILE]`): a whole
`Projector.step()` (synthesis forward and backward with noise gradients, distance, regulariser over every plane, Adam,
plane normalisation) at 256^2 and 1024^2, one and four frames, on a random-init config-f network whose noise strengths are
set to 0.1 so that the noise gradients are not zeros.

Two legs per shape: the HIP forms (gance::pyramid_distance, gance::noise_regularizer, the fused noise gradient of
gance::noise_bias_lrelu) and the same step with those three composed from plain torch ops on the same device (the
distance and the regulariser as avg_pool2d / roll / mean expressions, the noise added to x by a torch broadcast before the
epilogue op so that autograd sums its gradient). Everything else -- the modulated convs, ToRGB, Adam -- is shared. A
warm-up, then rounds that alternate the legs, every leg timed with device events over whole steps; medians are reported
with every round beside them. There is no parent-commit figure: the parent cannot project.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2.differentiable import DifferentiableSynthesis  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2.projector import Projector  # noqa: E402  pylint: disable=wrong-import-position

SHAPES = ((256, 1), (256, 4), (1024, 1), (1024, 4))  # (resolution, batch)
ROUNDS = 3
NUM_STEPS = 1000


class TorchNoiseSynthesis(DifferentiableSynthesis):
    """DifferentiableSynthesis with the caller's noise added in torch: the epilogue op then sees a zero plane that needs no gradient."""

    def __call__(self, dlatents, noise=None, collect=None):  # type: ignore[no-untyped-def]
        batch = dlatents.shape[0]
        x = self.const.expand(batch, -1, -1, -1).contiguous()
        y: Optional[torch.Tensor] = None
        torgbs = iter(self.torgbs)
        for conv in self.convs:
            style = dlatents[:, conv.layer_idx] @ conv.mod_weight + conv.mod_bias + 1.0
            demod = torch.rsqrt((style * style) @ conv.weight_squares + 1e-8)
            x = torch.ops.gance.modconv3x3(x, style, demod, conv.weight, conv.up)
            x = x + noise[conv.layer_idx] * conv.noise_strength
            x = torch.ops.gance.noise_bias_lrelu(x, torch.zeros_like(conv.noise), conv.noise_strength, conv.bias)
            if not conv.up:
                rgb = next(torgbs)
                style = dlatents[:, rgb.dlatent_row] @ rgb.mod_weight + rgb.mod_bias + 1.0
                y = torch.ops.gance.torgb_skip(x, style, rgb.weight, rgb.bias, y)
        return y


class TorchComposedProjector(Projector):
    """The projector with the distance, the regulariser and the noise gradient written in plain torch."""

    def set_network(self, network) -> None:  # type: ignore[no-untyped-def]
        super().set_network(network)
        variables, resolution = network
        self._synthesis = TorchNoiseSynthesis(variables, resolution)

    def _regularizer(self, plane: torch.Tensor) -> torch.Tensor:
        v, total = plane, 0.0
        while True:
            total = total + (v * torch.roll(v, 1, dims=3)).mean(dim=(1, 2, 3)) ** 2 + (v * torch.roll(v, 1, dims=2)).mean(dim=(1, 2, 3)) ** 2
            if v.shape[2] <= 8:
                return total
            v = F.avg_pool2d(v, 2)

    def _distance(self, images: torch.Tensor) -> torch.Tensor:
        p = (images + 1.0) * 127.5
        if p.shape[2] > 256:
            p = F.avg_pool2d(p, p.shape[2] // 256)
        d = (p - self._targets) / 255.0
        total = (d * d).mean(dim=(1, 2, 3))
        while d.shape[2] > 8:
            d = F.avg_pool2d(d, 2)
            total = total + (d * d).mean(dim=(1, 2, 3))
        return total


def timed(step, steps: int) -> float:
    """Milliseconds per call of `step`, device events around `steps` calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def measure(resolution: int, batch: int) -> dict:
    variables = dict(sg2_spec.make_random_variables(resolution, seed=0, perturb=True))
    for name in list(variables):
        if name.endswith("/noise_strength"):
            variables[name] = np.full_like(variables[name], 0.1)
    targets = np.random.RandomState(2).randint(0, 256, size=(batch, resolution, resolution, 3)).astype(np.uint8)
    legs: List[Projector] = [Projector(num_steps=NUM_STEPS), TorchComposedProjector(num_steps=NUM_STEPS)]
    for projector in legs:
        projector.set_network((variables, resolution))
        projector.start(targets)
        projector.step()  # warm-up (step 0 has learning rate 0)
        projector.step()
    torch.cuda.synchronize()
    agreement = float((legs[0].last_distance - legs[1].last_distance).abs().max() / legs[1].last_distance.abs().max())
    steps = 8 if resolution <= 256 else 3
    rounds = []
    for _ in range(ROUNDS):
        rounds.append({"hip_ms": timed(legs[0].step, steps), "torch_composed_ms": timed(legs[1].step, steps)})
    hip_ms = statistics.median(r["hip_ms"] for r in rounds)
    torch_ms = statistics.median(r["torch_composed_ms"] for r in rounds)
    return {
        "resolution": resolution,
        "batch": batch,
        "hip_ms_per_step": hip_ms,
        "torch_composed_ms_per_step": torch_ms,
        "hip_seconds_per_frame_at_1000_steps": hip_ms * NUM_STEPS / 1000.0 / batch,
        "torch_composed_seconds_per_frame_at_1000_steps": torch_ms * NUM_STEPS / 1000.0 / batch,
        "distance_agreement_after_two_steps": agreement,
        "steps_per_round": steps,
        "rounds": rounds,
    }


def measure_ops() -> dict:
    """The three new kernels alone at 1024^2, one frame (ms per call, median of ROUNDS rounds of 20 calls), with the bytes each moves."""
    def rand(*shape: int) -> torch.Tensor:
        return torch.randn(shape, dtype=torch.float32, device="cuda")

    grad_out, out, strength = rand(1, 32, 1024, 1024), rand(1, 32, 1024, 1024), torch.full((1,), 0.1, device="cuda")
    image, target, plane, one = rand(1, 3, 1024, 1024), rand(1, 3, 256, 256) * 40 + 128, rand(1, 1, 1024, 1024), torch.ones((1,), device="cuda")
    tensor_mb = grad_out.numel() * 4 / 1e6
    calls = {
        "noise_bias_lrelu_backward (no noise gradient), 1024^2 x 32": (lambda: torch.ops.gance.noise_bias_lrelu_backward(grad_out, out), 3 * tensor_mb),
        "noise_bias_lrelu_backward_noise, 1024^2 x 32": (
            lambda: torch.ops.gance.noise_bias_lrelu_backward_noise(grad_out, out, strength, 1), 3 * tensor_mb + plane.numel() * 4 / 1e6),
        "pyramid_distance forward, 1024^2": (lambda: torch.ops.gance.pyramid_distance(image, target), (image.numel() + target.numel() * (1 + 4 / 3)) * 4 / 1e6),
        "pyramid_distance_backward (rebuilds the forward), 1024^2": (
            lambda: torch.ops.gance.pyramid_distance_backward(one, image, target), (2 * image.numel() + target.numel() * (1 + 8 / 3)) * 4 / 1e6),
        "noise_regularizer forward, 1024^2": (lambda: torch.ops.gance.noise_regularizer(plane), plane.numel() * (2 + 2 / 3) * 4 / 1e6),
        "noise_regularizer_backward (rebuilds the forward), 1024^2": (
            lambda: torch.ops.gance.noise_regularizer_backward(one, plane), plane.numel() * (5 + 1) * 4 / 1e6),
    }
    result = {}
    for name, (call, megabytes) in calls.items():
        call()
        times = [timed(call, 20) for _ in range(ROUNDS)]
        result[name] = {"ms_per_call": statistics.median(times), "rounds": times, "megabytes_moved": megabytes}
    return result


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "projection_rate.json")
    args = parser.parse_args()
    result = {
        "network": "random init, perturb=True, config-f, noise strengths 0.1",
        "device": torch.cuda.get_device_name(0),
        "shapes": [measure(resolution, batch) for resolution, batch in SHAPES],
        "ops_alone": measure_ops(),
        "note": "one whole Projector.step(); the torch composition replaces the pyramid distance, the noise regulariser and the noise "
        "gradient only; the reference's ~10 min per projected 1024^2 frame is context and includes LPIPS, which neither leg has",
    }
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
