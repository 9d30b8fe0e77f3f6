"""
Rate and sizes of the PNG encoder's match-search mode against the literal-only encoder, both in one process on one GPU
(`timeout -k 10 600 python tools/gpu_png_lz_rate.py [--out profiles/png_lz_rate.json]`):

`torch.ops.gance.png_encode_lz` and `torch.ops.gance.png_encode` on the same 64 frames of 1024^2, for two inputs: a
random-init network's output (smooth gradients) and a plot panel (white, a box, a curve whose phase differs per frame).
Per input a warm-up of both, then three rounds that alternate the two ops, each round timed with device events over 8
calls; the medians of the rounds are reported as ms per 64-frame call, with the compressed bytes per frame and, for the
first frame of each input, the two file sizes beside PIL's. The literal-only op is the yardstick: its rate here should be
the one of profiles/png_encode_rate.json.
"""

import argparse
import io
import json
import sys
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib, torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position

SIDE, BATCH, ROUNDS, CALLS = 1024, 64, 3, 8


def network_frames() -> torch.Tensor:
    engine = hip_lib.Engine(sg2_spec.make_random_variables(SIDE, seed=0), SIDE, max_batch=BATCH, device=0)
    try:
        z = torch.from_numpy(np.random.RandomState(1).randn(BATCH, 512).astype(np.float32)).to(torch.device("cuda", 0))
        frames = torch.ops.gance.synthesize_z(z, engine.op_handle, 1.2)
        torch.cuda.synchronize()
    finally:
        engine.close()
    return frames


def panel_frames() -> torch.Tensor:
    frames = np.full((BATCH, SIDE, SIDE, 3), 255, dtype=np.uint8)
    margin = SIDE // 8
    frames[:, margin, margin : SIDE - margin] = 0
    frames[:, SIDE - margin - 1, margin : SIDE - margin] = 0
    frames[:, margin : SIDE - margin, margin] = 0
    frames[:, margin : SIDE - margin, SIDE - margin - 1] = 0
    x = np.arange(margin + 1, SIDE - margin - 1)
    for index in range(BATCH):
        y = (SIDE / 2 + (SIDE / 4) * np.sin(x * (4 * np.pi / SIDE) + index * 0.1)).astype(np.int64)
        for offset in (0, 1):
            frames[index, y + offset, x] = (31, 119, 180)
    return torch.from_numpy(frames).cuda()


def time_calls(op, frames: torch.Tensor) -> float:  # type: ignore[no-untyped-def]
    """ms per call over CALLS calls, by device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        op(frames)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / CALLS


def file_of(op, frame: torch.Tensor) -> bytes:  # type: ignore[no-untyped-def]
    data, offsets = op(frame[None])
    return data[: int(offsets[-1].item())].cpu().numpy().tobytes()


def measure(frames: torch.Tensor) -> dict:
    ops = {"png_encode": torch.ops.gance.png_encode, "png_encode_lz": torch.ops.gance.png_encode_lz}
    for op in ops.values():  # warm-up
        for _ in range(2):
            op(frames)
    torch.cuda.synchronize()
    rounds = {name: [] for name in ops}
    for _ in range(ROUNDS):
        for name, op in ops.items():
            rounds[name].append(time_calls(op, frames))
    result = {}
    for name, op in ops.items():
        _, offsets = op(frames)
        ms = float(np.median(rounds[name]))
        result[name] = {
            "ms_per_call": ms,
            "ms_per_call_rounds": rounds[name],
            "frames_per_s": BATCH / ms * 1e3,
            "compressed_bytes_per_frame": int(offsets[-1].item()) / BATCH,
        }
    result["lz_over_huffman_time"] = result["png_encode_lz"]["ms_per_call"] / result["png_encode"]["ms_per_call"]
    first = frames[0]
    files = {name: file_of(op, first) for name, op in ops.items()}
    buffer = io.BytesIO()
    Image.fromarray(first.cpu().numpy()).save(buffer, format="PNG")
    for name, file_bytes in files.items():
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(file_bytes))), first.cpu().numpy()), name
    result["first_frame_bytes"] = {"png_encode": len(files["png_encode"]), "png_encode_lz": len(files["png_encode_lz"]), "pil": buffer.tell()}
    return result


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    result = {"side": SIDE, "batch": BATCH, "rounds": ROUNDS, "calls_per_round": CALLS}
    for name, make in (("network", network_frames), ("panel", panel_frames)):
        result[name] = measure(make())
        print(json.dumps(result), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
