"""
Rate of the HIP Motion-JPEG encoder on one GPU, two legs in one process (`python tools/gpu_mjpeg_rate.py [--out FILE]`):

1. encoder alone: 64 frames of 2160^2 per call (a random-init 1024^2 network's frames, bicubic-resized), q 90; warm-up,
   then device events over >= 1 s of calls: frames/s, input GB/s, compressed bytes per frame;
2. the 2160^2 frame stream end to end (a random 1024^2 network, synthetic WAV + projection file): "npy" (raw frames to the
   host) against "avi" (JPEG in HBM, compressed bytes to the host), alternated: frames/s of the stream
   (projection_file_blend_frame_chunks, rank 0's timings) and of the API writing its file.

Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of leg 1 (`--encoder-only`).
"""

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib, network_file, projection_file_blend, synthetic, torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.network_interface.network_functions import MultiNetwork  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.projection import projection_file_reader as pfr  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position

SIDE, BATCH, QUALITY = 2160, 64, 90


def encoder_leg() -> dict:
    device = torch.device("cuda", 0)
    engine = hip_lib.Engine(sg2_spec.make_random_variables(1024, seed=0), 1024, max_batch=BATCH, device=0)
    try:
        w = torch.from_numpy(np.random.RandomState(1).randn(BATCH, engine.num_layers, 512).astype(np.float32)).to(device)
        native = torch.ops.gance.synthesize_w(w, engine.op_handle)
        frames = torch.ops.gance.resize_bicubic(native, SIDE)
        torch.cuda.synchronize()
    finally:
        engine.close()
    for _ in range(3):
        data, offsets = torch.ops.gance.jpeg_encode(frames, QUALITY)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, elapsed_ms = 0, 0.0
    while elapsed_ms < 1000.0:
        start.record()
        for _ in range(8):
            data, offsets = torch.ops.gance.jpeg_encode(frames, QUALITY)
        end.record()
        torch.cuda.synchronize()
        calls += 8
        elapsed_ms += start.elapsed_time(end)
    compressed = int(offsets[-1].item())
    seconds = elapsed_ms / 1e3
    return {
        "frames_per_s": calls * BATCH / seconds,
        "input_gb_per_s": calls * frames.numel() / seconds / 1e9,
        "compressed_bytes_per_frame": compressed / BATCH,
        "raw_bytes_per_frame": SIDE * SIDE * 3,
        "compression_ratio": SIDE * SIDE * 3 * BATCH / compressed,
        "calls": calls,
        "ms_per_call": elapsed_ms / calls,
    }


def stream_leg(rounds: int, num_frames: int) -> dict:
    L, fps_out = 512, 60.0
    work = Path(tempfile.mkdtemp(prefix="mjpeg_rate_"))
    fps_in = fps_out / 2
    num_projection = num_frames // 2
    audio = synthetic.synthetic_audio(num_frames, L, seed=3, frames_per_second=fps_out)
    wav_path = work / "audio.wav"
    wavfile.write(str(wav_path), int(L * fps_out), audio)
    latents = synthetic.synthetic_final_latents(num_projection, L, seed=4)
    projection_path = work / "projection.npz"
    pfr.write_projection_npz(projection_path, latents.reshape(18, num_projection, L).transpose(1, 0, 2), projection_fps=fps_in)
    network_path = work / "net.pkl"
    network_file.write_random_network(network_path, 1024, seed=0)
    args = ([str(wav_path)], [network_path], None, fps_out, SIDE, 0.25, True, (-5, 5), str(projection_path), 12)
    networks = MultiNetwork(network_paths=[network_path], load=True, max_batch=projection_file_blend.DEFAULT_STREAM_BATCH)
    results = {"npy": [], "avi": [], "npy_api": [], "avi_api": [], "bytes_to_host_per_frame": {}}
    try:
        for _ in range(rounds + 1):  # (round 0 warms up)
            for name, quality in (("npy", None), ("avi", QUALITY)):
                timings: dict = {}
                for _first, _total, _chunk in projection_file_blend.projection_file_blend_frame_chunks(
                    *args, networks=networks, timings=timings, jpeg_quality=quality
                ):
                    pass
                results[name].append(timings["frames"] / (timings["synthesis_to_host_ms"] / 1e3))
                results["bytes_to_host_per_frame"][name] = timings["bytes_to_host"] / timings["frames"]
        for _ in range(rounds):
            for name in ("npy", "avi"):
                out = work / f"out.{name}"
                clock = time.perf_counter()
                projection_file_blend.projection_file_blend_api(
                    args[0], str(out), args[1], None, fps_out, SIDE, None, None, None, 0.25, True, (-5, 5), str(projection_path), 12,
                    None, None, None, None, None, output_format=name,
                )
                results[f"{name}_api"].append(num_frames / (time.perf_counter() - clock))
                results[f"{name}_file_bytes"] = out.stat().st_size  # ("out.npy" already ends in .npy: no suffix appended)
                for path in work.glob("out.*"):
                    path.unlink()
    finally:
        networks.unload()
    for name in ("npy", "avi"):
        results[name] = results[name][1:]  # drop the warm-up round
    results["frames"] = num_frames
    return results


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    parser.add_argument("--encoder-only", action="store_true", help="leg 1 only (for the rocprofv3 run)")
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--frames", type=int, default=256)
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    result = {"encoder": encoder_leg()}
    print(json.dumps(result), flush=True)
    if not options.encoder_only:
        result["stream"] = stream_leg(options.rounds, options.frames)
    print(json.dumps(result), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
