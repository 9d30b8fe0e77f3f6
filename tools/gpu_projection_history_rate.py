"""
Rate of the projection-history video on one GPU (`python tools/gpu_projection_history_rate.py [--out FILE]`): a 1024 x 1024
random-init network, a synthetic .npz projection of 4 projected frames x 256 steps, video_height 1024 (frames of
3072 x 1024), 64 frames per chunk. Three legs, each warmed up once, then three alternated rounds in one process:

(a) the same 1024 latents through `synthesize_device_frames` alone: code that predates the video, hence the yardstick;
(b) the composed chunks of `projection_history_frame_chunks` (upload, engine call, latents panel, per-frame title, placing);
(c) `visualize_projection_history`: (b) through the JPEG encoder at quality 90 into the AVI.

A run is timed on the host's clock with a device synchronisation after every chunk. (b) and (c) load the network inside the
run, as a user's call does, so the first chunk of a run carries that; ms per chunk and frames/s are taken over the chunks
after the first, and the whole run's seconds are reported beside them. `--one-chunk` runs (b) for a single chunk only,
for a `rocprofv3 --kernel-trace --stats` run.
"""

import argparse
import itertools
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import network_file, projection_file_blend  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.network_interface.network_functions import MultiNetwork  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.projection import projection_file_reader, projection_visualization  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.video import mjpeg_avi  # noqa: E402  pylint: disable=wrong-import-position

RESOLUTION, FRAMES, STEPS, CHUNK, ROUNDS, QUALITY = 1024, 4, 256, 64, 3, 90


def write_inputs(directory: Path) -> dict:
    network = directory / "network.pkl"
    network_file.write_random_network(network, RESOLUTION, seed=0)
    rs = np.random.RandomState(1)
    finals = rs.standard_normal((FRAMES, 1, 512)).astype(np.float32)
    starts = rs.standard_normal((FRAMES, 1, 512)).astype(np.float32) * 2.0
    weights = ((STEPS - 1 - np.arange(STEPS, dtype=np.float32)) / (STEPS - 1))[None, :, None] ** 2
    rows = finals + (starts - finals) * weights  # [FRAMES, STEPS, 512]
    histories = np.ascontiguousarray(np.broadcast_to(rows[:, :, None, :], (FRAMES, STEPS, 18, 512)))
    images = rs.randint(0, 256, (FRAMES, RESOLUTION, RESOLUTION, 3)).astype(np.uint8)
    projection = directory / "projection.npz"
    projection_file_reader.write_projection_npz(
        projection, histories[:, -1], 30.0, target_images=images, final_images=images, latents_histories=list(histories)
    )
    return dict(network=network, projection=projection, latents=histories.reshape(FRAMES * STEPS, 18, 512), video=directory / "history.avi")


def timed_chunks(chunks) -> dict:
    """Seconds of the whole run and milliseconds of every chunk, the device drained after each."""
    torch.cuda.synchronize()
    start = last = time.perf_counter()
    per_chunk, frames = [], []
    for item in chunks:
        torch.cuda.synchronize()
        now = time.perf_counter()
        per_chunk.append((now - last) * 1e3)
        frames.append(int((item[1] if isinstance(item, tuple) else item).shape[0]))
        last = now
        del item
    steady_ms, steady_frames = sum(per_chunk[1:]), sum(frames[1:])
    return {
        "run_seconds": last - start, "frames": sum(frames), "first_chunk_ms": per_chunk[0],
        "ms_per_chunk": steady_ms / max(1, len(per_chunk) - 1), "frames_per_second": steady_frames / (steady_ms / 1e3) if steady_ms else 0.0,
    }


def main() -> None:  # pylint: disable=too-many-locals
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    parser.add_argument("--one-chunk", action="store_true", help="leg (b) for one chunk only (for the rocprofv3 run)")
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    with tempfile.TemporaryDirectory() as scratch:
        inputs = write_inputs(Path(scratch))

        def composed():
            return projection_visualization.projection_history_frame_chunks(inputs["projection"], inputs["network"], True, RESOLUTION)

        if options.one_chunk:
            print(json.dumps({"one_chunk": timed_chunks(itertools.islice(composed(), 1))}), flush=True)
            return
        networks = MultiNetwork([inputs["network"]], load=True, max_batch=CHUNK)
        d_latents = torch.from_numpy(inputs["latents"]).cuda()
        d_indices = torch.zeros(len(inputs["latents"]), dtype=torch.int32, device="cuda")

        def leg_a() -> dict:
            return timed_chunks(projection_file_blend.synthesize_device_frames(d_latents, d_indices, networks, batch=CHUNK))

        def leg_b() -> dict:
            return timed_chunks(composed())

        def leg_c() -> dict:
            start = time.perf_counter()
            projection_visualization.visualize_projection_history(
                inputs["projection"], inputs["video"], inputs["network"], True, RESOLUTION, jpeg_quality=QUALITY
            )
            torch.cuda.synchronize()
            seconds = time.perf_counter() - start
            with mjpeg_avi.MjpegAviReader(inputs["video"]) as reader:
                frames = reader.frame_count
            return {"run_seconds": seconds, "frames": frames, "frames_per_second_whole_run": frames / seconds, "bytes": inputs["video"].stat().st_size}

        legs = {"a_synthesis_alone": leg_a, "b_composed_chunks": leg_b, "c_avi_q90": leg_c}
        result = {
            "resolution": RESOLUTION, "projected_frames": FRAMES, "steps": STEPS, "chunk": CHUNK, "frame": [3 * RESOLUTION, RESOLUTION],
            "device": torch.cuda.get_device_name(0), "warm_up": {name: leg() for name, leg in legs.items()},
            "rounds": {name: [] for name in legs},
        }
        for _ in range(ROUNDS):
            for name, leg in legs.items():
                result["rounds"][name].append(leg())
        networks.unload()
    print(json.dumps(result), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
