"""
What the debug video costs beside the synthesis it accompanies: the 1024^2 one-network blend stream of bench.py's product
leg (1800 frames at 60 fps from a 30 s WAV and 900 projected latents on disk, networks resident, frames drained to the
host), timed by timings["synthesis_to_host_ms"], alternating debug off and debug on (`--debug-side`, default 512) in one
process after a warm-up of both, `--repeats` times each. Prints one JSON record.

    python tools/gpu_debug_video_cost.py [--repeats 3] [--debug-side 512] [--resolution 1024] [--batch 64]
    python tools/gpu_debug_video_cost.py --debug-side 0        # debug off only: also runs on a tree without the feature

For the kernel table: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gpu_debug_video_cost.py --repeats 1 --frames 256
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

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from gance_amd import network_file, projection_file_blend, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.network_interface.network_functions import MultiNetwork  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.projection import projection_file_reader as pfr  # noqa: E402  pylint: disable=wrong-import-position


def main() -> int:  # pylint: disable=too-many-locals
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--debug-side", type=int, default=512)
    parser.add_argument("--resolution", type=int, default=1024)
    parser.add_argument("--batch", type=int, default=64)
    parser.add_argument("--frames", type=int, default=1800)
    parser.add_argument("--quality", type=int, default=90)
    args = parser.parse_args()
    device = torch.device("cuda", 0)
    num_frames, length, fps_in, fps_out = args.frames, 512, 30.0, 60.0
    with tempfile.TemporaryDirectory(prefix="gance_debug_cost_") as holder:
        directory = Path(holder)
        audio, latents = synthetic.benchmark_blend_inputs(num_frames)
        wavfile.write(str(directory / "audio.wav"), int(length * fps_out), audio)
        pfr.write_projection_npz(
            directory / "projection.npz", latents.reshape(18, num_frames // 2, length).transpose(1, 0, 2), projection_fps=fps_in
        )
        network_file.write_random_network(directory / "net.pkl", args.resolution, seed=0)
        networks = MultiNetwork(network_paths=[directory / "net.pkl"], load=True, max_batch=args.batch, device=device.index)

        def run(frames_to_visualize, debug_side: int) -> dict:
            timings: dict = {}
            keywords = {}
            encoded = [0, 0]
            if debug_side:
                from gance_amd.debug_video.compose import DebugVideo  # pylint: disable=import-outside-toplevel

                def on_encoded(_first, chunk) -> None:
                    encoded[0] += len(chunk)
                    encoded[1] += int(chunk.offsets[-1])

                keywords["debug"] = DebugVideo(debug_side, None, on_encoded, jpeg_quality=args.quality)
            start = time.perf_counter()
            received = 0
            for _first, _total, frames in projection_file_blend.projection_file_blend_frame_chunks(
                wav=[str(directory / "audio.wav")], network_paths=[directory / "net.pkl"], frames_to_visualize=frames_to_visualize,
                output_fps=fps_out, output_side_length=args.resolution, alpha=0.25, fft_roll_enabled=True, fft_amplitude_range=(-5, 5),
                projection_file_path=str(directory / "projection.npz"), blend_depth=12, frames_per_call=args.batch, networks=networks,
                timings=timings, **keywords,
            ):
                received += len(frames)
                int(frames[-1, -1, -1, 0])  # the chunk is on the host
            return {
                "frames": received, "seconds": round(time.perf_counter() - start, 4),
                "synthesis_to_host_ms": round(float(timings["synthesis_to_host_ms"]), 2), "debug_frames": encoded[0], "debug_bytes": encoded[1],
            }

        try:
            sides = [0] + ([args.debug_side] if args.debug_side else [])
            for side in sides:  # warm-up of every shape the timed runs use
                run(4 * args.batch, side)
            runs = {side: [] for side in sides}
            for _ in range(args.repeats):
                for side in sides:
                    runs[side].append(run(None, side))
        finally:
            networks.unload()
    record = {"resolution": args.resolution, "frames_per_call": args.batch, "frames": num_frames, "debug_side_length": args.debug_side}
    for side, results in runs.items():
        times = [r["synthesis_to_host_ms"] for r in results]
        record["debug_on" if side else "debug_off"] = {
            "synthesis_to_host_ms": times, "median_ms": float(np.median(times)), "spread_ms": round(max(times) - min(times), 2),
            "frames_per_s_median": round(num_frames / (float(np.median(times)) * 1e-3), 1), "runs": results,
        }
    if args.debug_side:
        off, on = record["debug_off"]["median_ms"], record["debug_on"]["median_ms"]
        record["debug_cost_fraction_of_stream"] = round((on - off) / off, 4)
    print(json.dumps(record))
    return 0


if __name__ == "__main__":
    sys.exit(main())
