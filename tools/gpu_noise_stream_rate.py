"""
The rate of the noise-blend frame stream beside the projection stream it shares its code with: bench.py's product leg
(1024^2, one network resident, 1800 frames at 60 fps from a 30 s WAV on disk, 64 frames per call, chunks drained to the
host), timed by timings["synthesis_to_host_ms"]. The legs are alternated in one process after a warm-up of every one,
`--repeats` times each. Prints one JSON record.

    python tools/gpu_noise_stream_rate.py [--repeats 3] [--debug-side 512] [--quality 90] [--parent-module FILE]

Legs: "projection" (projection_file_blend_frame_chunks of this tree); "projection_parent" (the same generator of another
version of gance_amd/projection_file_blend.py, e.g. `git show HEAD~1:gance_amd/projection_file_blend.py > FILE`, loaded
beside this tree's: what a refactor of the stream cost); "noise_npy" (noise_blend_frame_chunks, raw frames), "noise_seeded"
(the same with noise_seed), "noise_avi" (jpeg_quality: encoded in HBM, only compressed bytes drained), "noise_debug"
(raw frames + the two-panel debug video at --debug-side).

For the kernel table: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gpu_noise_stream_rate.py --repeats 1 --frames 256
"""

import argparse
import importlib.util
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from gance_amd import network_file, noise_blend, projection_file_blend, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.debug_video.compose import DebugVideo  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.network_interface.network_functions import MultiNetwork  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.projection import projection_file_reader as pfr  # noqa: E402  pylint: disable=wrong-import-position


def main() -> int:  # pylint: disable=too-many-locals,too-many-statements
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--debug-side", type=int, default=512)
    parser.add_argument("--resolution", type=int, default=1024)
    parser.add_argument("--batch", type=int, default=64)
    parser.add_argument("--frames", type=int, default=1800)
    parser.add_argument("--quality", type=int, default=90)
    parser.add_argument("--noise-seed", type=int, default=1)
    parser.add_argument("--parent-module", default=None, help="another version of gance_amd/projection_file_blend.py to time beside this tree's")
    parser.add_argument("--legs", default=None, help="comma-separated subset of the legs")
    args = parser.parse_args()
    device = torch.device("cuda", 0)
    num_frames, length, fps_in, fps_out = args.frames, 512, 30.0, 60.0
    parent = None
    if args.parent_module:
        spec = importlib.util.spec_from_file_location("gance_amd._parent_projection_file_blend", args.parent_module)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
    with tempfile.TemporaryDirectory(prefix="gance_noise_rate_") as holder:
        directory = Path(holder)
        audio, latents = synthetic.benchmark_blend_inputs(num_frames)
        wavfile.write(str(directory / "audio.wav"), int(length * fps_out), audio)
        pfr.write_projection_npz(
            directory / "projection.npz", latents.reshape(18, num_frames // 2, length).transpose(1, 0, 2), projection_fps=fps_in
        )
        network_file.write_random_network(directory / "net.pkl", args.resolution, seed=0)
        networks = MultiNetwork(network_paths=[directory / "net.pkl"], load=True, max_batch=args.batch, device=device.index)
        common = dict(
            wav=[str(directory / "audio.wav")], network_paths=[directory / "net.pkl"], output_fps=fps_out, output_side_length=args.resolution,
            alpha=0.25, fft_roll_enabled=True, fft_amplitude_range=(-5, 5), frames_per_call=args.batch, networks=networks,
        )
        projection = dict(projection_file_path=str(directory / "projection.npz"), blend_depth=12)

        def run(leg: str, frames_to_visualize) -> dict:
            timings: dict = {}
            encoded = [0, 0]

            def on_encoded(_first, chunk) -> None:
                encoded[0] += len(chunk)
                encoded[1] += int(chunk.offsets[-1])

            keywords = dict(common, frames_to_visualize=frames_to_visualize, timings=timings)
            if leg == "projection":
                chunks = projection_file_blend.projection_file_blend_frame_chunks(**keywords, **projection)
            elif leg == "projection_parent":
                chunks = parent.projection_file_blend_frame_chunks(**keywords, **projection)
            else:
                if leg == "noise_seeded":
                    keywords["noise_seed"] = args.noise_seed
                if leg == "noise_avi":
                    keywords["jpeg_quality"] = args.quality
                if leg == "noise_debug":
                    keywords["debug"] = DebugVideo(args.debug_side, None, on_encoded, jpeg_quality=args.quality)
                chunks = noise_blend.noise_blend_frame_chunks(**keywords)
            received = 0
            for _first, _total, frames in chunks:
                received += len(frames)
                if leg == "noise_avi":
                    int(frames.frame(len(frames) - 1)[-1])  # the chunk's bytes are on the host
                else:
                    int(frames[-1, -1, -1, 0])
            return {
                "frames": received, "synthesis_to_host_ms": round(float(timings["synthesis_to_host_ms"]), 2),
                "bytes_to_host": int(timings["bytes_to_host"]), "debug_frames": encoded[0], "debug_bytes": encoded[1],
            }

        legs = ["projection"] + (["projection_parent"] if parent is not None else []) + ["noise_npy", "noise_seeded", "noise_avi"]
        legs += ["noise_debug"] if args.debug_side else []
        if args.legs:
            legs = [leg for leg in legs if leg in args.legs.split(",")]
        try:
            for leg in legs:  # warm-up of every shape the timed runs use
                run(leg, 4 * args.batch)
            runs = {leg: [] for leg in legs}
            for _ in range(args.repeats):
                for leg in legs:
                    runs[leg].append(run(leg, None))
        finally:
            networks.unload()
    record = {
        "resolution": args.resolution, "frames_per_call": args.batch, "frames": num_frames, "debug_side_length": args.debug_side,
        "jpeg_quality": args.quality, "legs": {},
    }
    for leg, results in runs.items():
        times = [r["synthesis_to_host_ms"] for r in results]
        record["legs"][leg] = {
            "synthesis_to_host_ms": times, "median_ms": float(np.median(times)), "spread_ms": round(max(times) - min(times), 2),
            "frames_per_s_median": round(num_frames / (float(np.median(times)) * 1e-3), 1), "runs": results,
        }
    print(json.dumps(record))
    return 0


if __name__ == "__main__":
    sys.exit(main())
