"""
Cost and gain of the JPEG encoder's per-frame optimised Huffman tables on one GPU
(`python tools/gpu_mjpeg_optimized_rate.py [--out profiles/mjpeg_optimized_rate.json] [--previous LIBRARY]`).

Legs, alternated in one process, three rounds after a warm-up of all of them: torch.ops.gance.jpeg_encode_rect ("standard"),
torch.ops.gance.jpeg_encode_optimized ("optimized") and, with --previous, gance_jpeg_encode_rect_u8 of another build of the
library loaded beside this one (the parent commit's: the standard leg must not have got slower; the margin is that leg's own
spread over its rounds). Each call is 64 frames at quality 90, on three inputs:

    network_1024   frames of a random-init 1024^2 generator
    network_2160   the same, bicubic-resized to 2160^2
    debug_1536x512 composed debug frames of projection-file-blend: three panels of 512 (output, final images, synthesis inputs)

Reported per input and leg: ms per call of each round (device events over 8 calls) and bytes per frame; and whether the
optimised file of the input's first frame has the DHT segments and the scan bytes of PIL's
optimize=True, subsampling=1, restart_marker_rows=1 file of that frame. `--only LEG --input NAME` runs one leg on one input a
few times and reports nothing: the command of the separate `rocprofv3 --kernel-trace --stats` run.
"""

import argparse
import ctypes
import io
import json
import struct
import sys
import tempfile
from pathlib import Path
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
from PIL import Image
from scipy.io import wavfile

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib, network_file, projection_file_blend, synthetic, torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.debug_video.compose import DebugVideo  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.projection import projection_file_reader as pfr  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position

BATCH, QUALITY, CALLS_PER_ROUND, ROUNDS = 64, 90, 8, 3


def network_frames() -> Dict[str, torch.Tensor]:
    device = torch.device("cuda", 0)
    engine = hip_lib.Engine(sg2_spec.make_random_variables(1024, seed=0), 1024, max_batch=BATCH, device=0)
    try:
        w = torch.from_numpy(np.random.RandomState(1).randn(BATCH, engine.num_layers, 512).astype(np.float32)).to(device)
        native = torch.ops.gance.synthesize_w(w, engine.op_handle).clone()
        resized = torch.ops.gance.resize_bicubic(native, 2160)
        torch.cuda.synchronize()
    finally:
        engine.close()
    return {"network_1024": native, "network_2160": resized}


def debug_frames() -> torch.Tensor:
    """64 composed debug frames [64, 512, 1536, 3] of a small projection-file-blend run, kept in HBM."""
    L, fps_out = 512, 30.0
    work = Path(tempfile.mkdtemp(prefix="mjpeg_optimized_rate_"))
    audio = synthetic.synthetic_audio(BATCH, L, seed=3, frames_per_second=fps_out)
    wavfile.write(str(work / "audio.wav"), int(L * fps_out), audio)
    latents = synthetic.synthetic_final_latents(BATCH // 2, L, seed=4)
    y, x = np.mgrid[0:128, 0:128]
    final_images = np.stack([  # (a projection's final images are pictures, not the black the stream shows without them)
        np.stack([128 + 100 * np.sin(x / (3.0 + c) + y / 7.0 + 0.2 * k) * np.cos(y / (5.0 + c) - 0.1 * k) for c in range(3)], -1).astype(np.uint8)
        for k in range(BATCH // 2)
    ])
    pfr.write_projection_npz(
        work / "projection.npz", latents.reshape(18, BATCH // 2, L).transpose(1, 0, 2), projection_fps=fps_out / 2, final_images=final_images
    )
    network_file.write_random_network(work / "net.pkl", 128, seed=0)
    composed: List[torch.Tensor] = []
    debug = DebugVideo(512, None, lambda _first, _encoded: None, on_composed=lambda _first, frames: composed.append(frames.clone()))
    for _chunk in projection_file_blend.projection_file_blend_frame_chunks(
        [str(work / "audio.wav")], [work / "net.pkl"], None, fps_out, 128, 0.25, True, (-5, 5), str(work / "projection.npz"), 12, debug=debug
    ):
        pass
    torch.cuda.synchronize()
    frames = torch.cat(composed)
    if tuple(frames.shape) != (BATCH, 512, 1536, 3):
        raise SystemExit(f"unexpected debug frames {tuple(frames.shape)}")
    return frames


def previous_leg(path: Path) -> Callable[[torch.Tensor], torch.Tensor]:
    """gance_jpeg_encode_rect_u8 of the library at `path`, on torch's buffers and current stream; returns the offsets."""
    lib = ctypes.CDLL(str(path))
    for name in ("gance_jpeg_encode_rect_bounds", "gance_jpeg_encode_rect_u8"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = hip_lib.SIGNATURES[name]
    buffers: Dict[tuple, tuple] = {}

    def run(frames: torch.Tensor) -> torch.Tensor:
        batch, height, width = (int(v) for v in frames.shape[:3])
        if (batch, height, width) not in buffers:
            workspace_bytes, capacity = ctypes.c_uint64(), ctypes.c_uint64()
            if lib.gance_jpeg_encode_rect_bounds(batch, width, height, ctypes.byref(workspace_bytes), ctypes.byref(capacity)):
                raise SystemExit("the previous library refuses the shape")
            buffers[(batch, height, width)] = (int(workspace_bytes.value), int(capacity.value))
        workspace_bytes, capacity = buffers[(batch, height, width)]
        # allocated per call, as the ops of this build allocate
        workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=frames.device)
        data = torch.empty((capacity,), dtype=torch.uint8, device=frames.device)
        offsets = torch.empty((batch + 1,), dtype=torch.int64, device=frames.device)
        status = lib.gance_jpeg_encode_rect_u8(
            frames.data_ptr(), batch, width, height, QUALITY, workspace.data_ptr(), workspace_bytes, data.data_ptr(), capacity,
            offsets.data_ptr(), torch.cuda.current_stream(frames.device).cuda_stream,
        )
        if status:
            raise SystemExit(f"the previous library's encode failed with status {status}")
        return offsets

    return run


def scan_and_tables(data: bytes) -> tuple:
    """(the DHT segments' bytes, the bytes from the end of SOS on) of one file."""
    at, tables = 2, b""
    while True:
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        if marker == 0xC4:
            tables += data[at : at + 2 + length]
        at += 2 + length
        if marker == 0xDA:
            return tables, data[at:]


def against_pil(frame: torch.Tensor) -> dict:
    data, offsets = torch.ops.gance.jpeg_encode_optimized(frame[None].contiguous(), QUALITY)
    ours = data[: int(offsets[1].item())].cpu().numpy().tobytes()
    buffer = io.BytesIO()
    Image.fromarray(frame.cpu().numpy()).save(buffer, format="JPEG", quality=QUALITY, subsampling=1, optimize=True, restart_marker_rows=1)
    (our_tables, our_scan), (pil_tables, pil_scan) = scan_and_tables(ours), scan_and_tables(buffer.getvalue())
    return {
        "dht_equal": our_tables == pil_tables, "scan_equal": our_scan == pil_scan, "our_bytes": len(ours), "pil_bytes": len(buffer.getvalue())
    }


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    parser.add_argument("--previous", type=Path, default=None, help="another build of libgance_hip.so for the third leg")
    parser.add_argument("--only", choices=("standard", "optimized"), default=None, help="one leg, a few calls, no report")
    parser.add_argument("--input", default="network_1024", help="the input of --only")
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    inputs = network_frames()
    inputs["debug_1536x512"] = debug_frames()
    legs: Dict[str, Callable[[torch.Tensor], torch.Tensor]] = {
        "standard": lambda frames: torch.ops.gance.jpeg_encode_rect(frames, QUALITY)[1],
        "optimized": lambda frames: torch.ops.gance.jpeg_encode_optimized(frames, QUALITY)[1],
    }
    if options.only is not None:
        for _ in range(4):
            legs[options.only](inputs[options.input])
        torch.cuda.synchronize()
        return
    if options.previous is not None:
        legs["previous_standard"] = previous_leg(options.previous)
    result: Dict[str, dict] = {"batch": BATCH, "quality": QUALITY, "calls_per_round": CALLS_PER_ROUND, "inputs": {}}
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, frames in inputs.items():
        report: Dict[str, dict] = {leg: {"ms_per_call": []} for leg in legs}
        for leg, run in legs.items():  # warm-up of every leg
            for _ in range(3):
                offsets: Optional[torch.Tensor] = run(frames)
            torch.cuda.synchronize()
            report[leg]["bytes_per_frame"] = int(offsets[-1].item()) / BATCH
        for _ in range(ROUNDS):
            for leg, run in legs.items():
                start.record()
                for _ in range(CALLS_PER_ROUND):
                    run(frames)
                end.record()
                torch.cuda.synchronize()
                report[leg]["ms_per_call"].append(start.elapsed_time(end) / CALLS_PER_ROUND)
        report["shape"] = list(frames.shape)
        report["saving"] = 1 - report["optimized"]["bytes_per_frame"] / report["standard"]["bytes_per_frame"]
        report["first_frame_against_pil"] = against_pil(frames[0])
        result["inputs"][name] = report
        print(json.dumps({name: report}), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
