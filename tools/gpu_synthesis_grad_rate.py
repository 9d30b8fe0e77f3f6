"""
Cost of one step of differentiable synthesis on one GPU (`timeout 600 python tools/gpu_synthesis_grad_rate.py [--out FILE]`):
forward + backward of `DifferentiableSynthesis` (image from dlatents, then the dlatents' gradient for a fixed cotangent) at
256^2 and 1024^2, one and four frames, on a random-init config-f network, beside the engine's forward
(`torch.ops.gance.synthesize_w_image`) for the same dlatents as context. Each shape: a warm-up, then three rounds that
alternate the two legs, every leg timed with device events over whole steps; the median round is reported with all three
beside it, and the peak memory torch allocated during one step (the saved activations, the gradients, the workspaces).

Nothing comparable exists on the reference's side except its estimate of about 10 minutes per projected 1024^2 frame, which
includes a perceptual loss and an optimiser loop that are not part of this: the figures are a cost, not a speed-up.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib, torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2.differentiable import DifferentiableSynthesis  # noqa: E402  pylint: disable=wrong-import-position

SHAPES = ((256, 1), (256, 4), (1024, 1), (1024, 4))  # (resolution, batch)
ROUNDS = 3


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
    variables = sg2_spec.make_random_variables(resolution, seed=0, perturb=True)
    synthesis = DifferentiableSynthesis(variables, resolution, device=0)
    engine = hip_lib.Engine(variables, resolution, max_batch=batch, device=0)
    rng = np.random.RandomState(1)
    dlatents = torch.from_numpy(rng.randn(batch, synthesis.num_layers, 512).astype(np.float32)).cuda()
    cotangent = torch.from_numpy(rng.randn(batch, 3, resolution, resolution).astype(np.float32)).cuda()

    def grad_step() -> None:
        leaf = dlatents.clone().requires_grad_(True)
        torch.autograd.grad(synthesis(leaf), leaf, cotangent)

    def engine_step() -> None:
        torch.ops.gance.synthesize_w_image(dlatents, engine.op_handle)

    try:
        grad_step()
        engine_step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        grad_step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        steps = 8 if resolution <= 256 else 2
        rounds = []
        for _ in range(ROUNDS):
            rounds.append({"forward_backward_ms": timed(grad_step, steps), "engine_forward_ms": timed(engine_step, steps)})
    finally:
        engine.close()
    return {
        "resolution": resolution,
        "batch": batch,
        "forward_backward_ms_per_step": statistics.median(r["forward_backward_ms"] for r in rounds),
        "engine_forward_ms_per_call": statistics.median(r["engine_forward_ms"] for r in rounds),
        "peak_step_memory_mb": peak / 2 ** 20,
        "steps_per_round": steps,
        "rounds": rounds,
    }


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "synthesis_grad_rate.json")
    args = parser.parse_args()
    result = {
        "network": "random init, perturb=True, config-f",
        "device": torch.cuda.get_device_name(0),
        "shapes": [measure(resolution, batch) for resolution, batch in SHAPES],
        "note": "forward + backward of the image with respect to the dlatents; the engine's forward is context, not a comparison; "
        "the reference's ~10 min per projected 1024^2 frame includes a loss and a loop this does not have",
    }
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
