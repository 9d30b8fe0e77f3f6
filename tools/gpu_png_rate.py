"""
Rate of the HIP PNG encoder and of the still product on one GPU, three legs in one process
(`timeout 600 python tools/gpu_png_rate.py [--out FILE]`):

1. encoder alone: `torch.ops.gance.png_encode` on 64 frames of 1024^2 (a random-init network's output); warm-up, then
   device events over >= 1 s of calls: frames/s, input GB/s, compressed bytes per frame;
2. `images_from_network(num_images=256)` end to end (vector draws, synthesis, encode, copy, the .png and .json files):
   images/s by the wall clock, second run (the first loads the network and warms up);
3. PIL's `Image.save(format="PNG")` of the first of the same frames on this machine's CPU: seconds per frame, bytes;
4. one textured 1024^2 frame (gradients plus sigma = 3 noise, the `scene` of tests/png_ref.py) through both: bytes, and
   PIL's seconds. A random-init network's output is smooth, which favours PIL's match search; trained output is textured.
"""

import argparse
import io
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib, network_file, synthesize_images, torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position

SIDE, BATCH, IMAGES, PIL_FRAMES = 1024, 64, 256, 4


def encoder_leg() -> tuple:
    device = torch.device("cuda", 0)
    engine = hip_lib.Engine(sg2_spec.make_random_variables(SIDE, seed=0), SIDE, max_batch=BATCH, device=0)
    try:
        z = torch.from_numpy(np.random.RandomState(1).randn(BATCH, 512).astype(np.float32)).to(device)
        frames = torch.ops.gance.synthesize_z(z, engine.op_handle, 1.2)
        torch.cuda.synchronize()
    finally:
        engine.close()
    for _ in range(3):
        data, offsets = torch.ops.gance.png_encode(frames)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, elapsed_ms = 0, 0.0
    while elapsed_ms < 1000.0:
        start.record()
        for _ in range(4):
            data, offsets = torch.ops.gance.png_encode(frames)
        end.record()
        torch.cuda.synchronize()
        calls += 4
        elapsed_ms += start.elapsed_time(end)
    compressed = int(offsets[-1].item())
    seconds = elapsed_ms / 1e3
    result = {
        "frames_per_s": calls * BATCH / seconds,
        "input_gb_per_s": calls * frames.numel() / seconds / 1e9,
        "compressed_bytes_per_frame": compressed / BATCH,
        "raw_bytes_per_frame": SIDE * SIDE * 3,
        "compressed_over_raw": compressed / (SIDE * SIDE * 3 * BATCH),
        "calls": calls,
        "ms_per_call": elapsed_ms / calls,
    }
    return result, frames[:PIL_FRAMES].cpu().numpy()


def product_leg() -> dict:
    work = Path(tempfile.mkdtemp(prefix="png_rate_"))
    try:
        (work / "networks").mkdir()
        network_file.write_random_network(work / "networks" / "net.pkl", SIDE, seed=0)
        seconds = []
        for run in range(2):
            clock = time.perf_counter()
            synthesize_images.images_from_network(str(work / "networks"), str(work / f"out{run}"), 0, 0, num_images=IMAGES, frames_per_call=BATCH)
            seconds.append(time.perf_counter() - clock)
        files = sorted((work / "out1" / "net").glob("*.png"))
        return {
            "images": IMAGES,
            "seconds_first_run": seconds[0],
            "seconds": seconds[1],
            "images_per_s": IMAGES / seconds[1],
            "png_bytes_per_image": sum(path.stat().st_size for path in files) / len(files),
            "note": "both runs load the 1024^2 network; the .json of a z vector is about 11 KB of text",
        }
    finally:
        shutil.rmtree(work, ignore_errors=True)


def pil_leg(frames: np.ndarray) -> dict:
    seconds, sizes = [], []
    for frame in frames:
        buffer = io.BytesIO()
        clock = time.perf_counter()
        Image.fromarray(frame).save(buffer, format="PNG")
        seconds.append(time.perf_counter() - clock)
        sizes.append(buffer.tell())
    return {"frames": len(frames), "seconds_per_frame": float(np.median(seconds)), "bytes_per_frame": float(np.mean(sizes))}


def textured_leg() -> dict:
    rs = np.random.RandomState(2)
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    planes = [x * 256.0 / SIDE + 20 * np.sin(y / 30.0), y * 128.0 / SIDE + x * 64.0 / SIDE, 128 + 60 * np.cos((x + y) / 50.0)]
    image = np.clip(np.stack(planes, -1) + rs.randn(SIDE, SIDE, 3) * 3, 0, 255).astype(np.uint8)
    _, offsets = torch.ops.gance.png_encode(torch.from_numpy(image[None]).cuda())
    result = pil_leg(image[None])
    return {"raw_bytes": image.size, "gpu_bytes": int(offsets[-1].item()), "pil_bytes": result["bytes_per_frame"], "pil_seconds": result["seconds_per_frame"]}


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    encoder, frames = encoder_leg()
    result = {"side": SIDE, "batch": BATCH, "encoder": encoder}
    print(json.dumps(result), flush=True)
    result["pil_cpu"] = pil_leg(frames)
    result["encoder"]["frames_per_s_over_pil"] = encoder["frames_per_s"] * result["pil_cpu"]["seconds_per_frame"]
    print(json.dumps(result), flush=True)
    result["textured_frame"] = textured_leg()
    result["images_from_network"] = product_leg()
    print(json.dumps(result), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
