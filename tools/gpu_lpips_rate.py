"""
Cost of the VGG16 LPIPS distance on one GPU (`python tools/gpu_lpips_rate.py [--out FILE]`), on random weights and a
random-init config-f 1024^2 network whose noise strengths are set to 0.1:

* ms per whole `Projector.step()` at 1024^2, one and four frames, with (a) the built-in `pyramid_distance`, (b) `VGG16Lpips`
  (gance::modconv3x3 convolutions, csrc/lpips.hip for the rest), (c) the same LPIPS composed of plain torch ops on the same
  device (conv2d, relu, max_pool2d, avg_pool2d, vector_norm), (d) `VGG16Lpips(convolution="conv3x3")` (gance::conv3x3,
  csrc/conv3x3.hip), the leg `hip-conv3x3`;
* forward + backward of the distance alone (images [B, 3, 1024, 1024] -> [B] -> image gradient) for (b), (c) and (d).

Every measurement is a child process of its own under `timeout -k 10`; the first one that fails ends the run. A child warms
up, then runs three rounds that alternate its legs, every leg timed with device events; medians are reported with every
round beside them. No bar is set. `--measure distance --batch 1 --legs hip` (or `hip-conv3x3`) alone is the run to put under a
kernel trace
(`timeout -k 10 400 rocprofv3 --kernel-trace --stats -- python tools/gpu_lpips_rate.py --measure distance --batch 1 --legs hip-conv3x3`).
"""

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path
from typing import Callable, Dict, List

import numpy as np
import torch
import torch.nn.functional as F

REPO_ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO_ROOT))
from gance_amd.stylegan2 import lpips  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2.projector import Projector  # noqa: E402  pylint: disable=wrong-import-position

RESOLUTION = 1024
BATCHES = (1, 4)
ROUNDS = 3
NUM_STEPS = 1000
CHILD_SECONDS = 600
LEGS = ("hip", "torch", "hip-conv3x3")  # the LPIPS legs, alternated in this order in every round


class TorchLpips:
    """The distance of `lpips.VGG16Lpips` from plain torch ops on the device (MIOpen convolutions), the target's taps kept alike."""

    def __init__(self, weights: lpips.LpipsWeights, side: int = lpips.DEFAULT_SIDE) -> None:
        self.side = side
        self.convs = [(torch.from_numpy(weight.transpose(3, 2, 0, 1).copy()).cuda(), torch.from_numpy(bias).cuda()) for weight, bias in weights.convs]
        self.lins = [torch.from_numpy(lin).cuda().reshape(1, -1, 1, 1) for lin in weights.lins]
        self.shift, self.scale = (torch.from_numpy(values).cuda().reshape(1, 3, 1, 1) for values in (weights.shift, weights.scale))
        self._kept = None

    def taps(self, x: torch.Tensor) -> List[torch.Tensor]:
        if x.shape[2] > self.side:
            x = F.avg_pool2d(x, x.shape[2] // self.side)
        x = (x - self.shift) / self.scale
        out = []
        for index, (weight, bias) in enumerate(self.convs):
            x = torch.relu(F.conv2d(x, weight, bias, padding=1))
            if index in lpips.TAP_LAYERS:
                out.append(x)
            if index in lpips.POOL_LAYERS:
                x = F.max_pool2d(x, 2)
        return out

    @staticmethod
    def normalize(f: torch.Tensor) -> torch.Tensor:
        return f / (torch.linalg.vector_norm(f, dim=1, keepdim=True) + 1e-10)

    def __call__(self, images: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        if self._kept is None or self._kept[0] is not targets:
            with torch.no_grad():
                planes = targets.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0
                self._kept = (targets, [self.normalize(tap) for tap in self.taps(planes)])
        total = 0.0
        for tap, target, lin in zip(self.taps(images), self._kept[1], self.lins):
            total = total + (lin * (self.normalize(tap) - target) ** 2).sum(dim=1).mean(dim=(1, 2))
        return total


def timed(call: Callable[[], object], calls: int) -> float:
    """Milliseconds per call, device events around `calls` calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def alternate(legs: Dict[str, Callable[[], object]], calls: int) -> dict:
    for call in legs.values():  # warm-up
        call()
        call()
    torch.cuda.synchronize()
    rounds = [{name: timed(call, calls) for name, call in legs.items()} for _ in range(ROUNDS)]
    return {"ms": {name: statistics.median(r[name] for r in rounds) for name in legs}, "calls_per_round": calls, "rounds": rounds}


def make_distances(names: List[str]) -> Dict[str, object]:
    weights = lpips.random_lpips_weights(0)
    makers = {
        "pyramid": lambda: None,
        "hip": lambda: lpips.VGG16Lpips(weights),
        "torch": lambda: TorchLpips(weights),
        "hip-conv3x3": lambda: lpips.VGG16Lpips(weights, convolution="conv3x3"),
    }
    return {name: makers[name]() for name in names}


def measure_steps(batch: int, names: List[str]) -> dict:
    variables = dict(sg2_spec.make_random_variables(RESOLUTION, seed=0, perturb=True))
    for name in list(variables):
        if name.endswith("/noise_strength"):
            variables[name] = np.full_like(variables[name], 0.1)
    targets = np.random.RandomState(2).randint(0, 256, size=(batch, RESOLUTION, RESOLUTION, 3)).astype(np.uint8)
    legs = {}
    projectors = {}
    for name, distance in make_distances(names).items():
        projector = Projector(num_steps=NUM_STEPS, distance=distance)
        projector.set_network((variables, RESOLUTION))
        projector.start(targets)
        projectors[name], legs[name] = projector, projector.step
    result = alternate(legs, 3)
    result["last_distance"] = {name: projector.last_distance.cpu().tolist() for name, projector in projectors.items()}
    return result


def measure_distance(batch: int, names: List[str]) -> dict:
    rng = np.random.RandomState(3)
    images = torch.from_numpy(rng.uniform(-1, 1, size=(batch, 3, RESOLUTION, RESOLUTION)).astype(np.float32)).cuda().requires_grad_(True)
    targets = torch.from_numpy(rng.randint(0, 256, size=(batch, RESOLUTION, RESOLUTION, 3)).astype(np.uint8)).cuda()
    distances = make_distances(names)
    values = {}

    def leg(name: str) -> Callable[[], object]:
        def call() -> None:
            total = distances[name](images, targets)
            torch.autograd.grad(total.sum(), images)
            values[name] = total.detach()

        return call

    result = alternate({name: leg(name) for name in names}, 5)
    result["distance"] = {name: value.cpu().tolist() for name, value in values.items()}
    return result


def child(measure: str, batch: int, names: List[str]) -> dict:
    command = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, str(Path(__file__).resolve()), "--measure", measure, "--batch", str(batch),
               "--legs", ",".join(names)]  # fmt: skip
    done = subprocess.run(command, stdout=subprocess.PIPE, check=False)
    if done.returncode != 0:
        raise SystemExit(f"{' '.join(command)} ended with status {done.returncode}: nothing more is started")
    return json.loads(done.stdout.decode().strip().splitlines()[-1])


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("--out", type=Path, default=REPO_ROOT / "profiles" / "lpips_conv3x3_rate.json")
    parser.add_argument("--measure", choices=("steps", "distance"), help="run one measurement in this process and print its JSON line")
    parser.add_argument("--batch", type=int, default=1)
    parser.add_argument("--legs", default="", help="comma-separated: pyramid (steps only), hip, torch, hip-conv3x3")
    args = parser.parse_args()
    if args.measure is not None:
        names = args.legs.split(",") if args.legs else (["pyramid"] if args.measure == "steps" else []) + list(LEGS)
        print(json.dumps((measure_steps if args.measure == "steps" else measure_distance)(args.batch, names)))
        return
    result = {
        "network": "random init, perturb=True, config-f, 1024^2, noise strengths 0.1; LPIPS weights random_lpips_weights(0), side 256",
        "device": torch.cuda.get_device_name(0),
        "legs": {
            "pyramid": "gance::pyramid_distance",
            "hip": "VGG16Lpips (gance::modconv3x3 + csrc/lpips.hip)",
            "torch": "plain torch ops (MIOpen conv2d)",
            "hip-conv3x3": "VGG16Lpips(convolution='conv3x3') (gance::conv3x3 + csrc/lpips.hip)",
        },
        "projector_step_ms": {f"B={batch}": child("steps", batch, ["pyramid", *LEGS]) for batch in BATCHES},
        "distance_forward_backward_ms": {f"B={batch}": child("distance", batch, list(LEGS)) for batch in BATCHES},
    }
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
