"""
Rate of the HIP Motion-JPEG decoder on one GPU (`python tools/gpu_mjpeg_decode_rate.py [--out FILE]`), the sibling of
tools/gpu_mjpeg_rate.py: 64 frames of 2160^2 per call (a random-init 1024^2 network's frames, bicubic-resized, encoded by
torch.ops.gance.jpeg_encode at q 90). After a warm-up, three rounds alternate

1. the decode call alone (gance_jpeg_decode_u8 with the headers parsed beforehand; device events over 8 calls),
2. torch.ops.gance.jpeg_decode (header read, decode, status read: wall clock),
3. PIL decoding the same 64 files in this process (wall clock): the decode call must be faster than this,
4. file -> HBM: an AVI of the 64 files through frames_in_video_device_chunks (wall clock, page cache warm).

Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of leg 1 (`--decode-only`).
"""

import argparse
import io
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib, torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.video import mjpeg_avi, video_common  # noqa: E402  pylint: disable=wrong-import-position

SIDE, BATCH, QUALITY = 2160, 64, 90


def encoded_frames():
    """(data, offsets on the device, files on the host) of BATCH network frames at SIDE^2."""
    device = torch.device("cuda", 0)
    engine = hip_lib.Engine(sg2_spec.make_random_variables(1024, seed=0), 1024, max_batch=BATCH, device=0)
    try:
        w = torch.from_numpy(np.random.RandomState(1).randn(BATCH, engine.num_layers, 512).astype(np.float32)).to(device)
        frames = torch.ops.gance.resize_bicubic(torch.ops.gance.synthesize_w(w, engine.op_handle), SIDE)
        torch.cuda.synchronize()
    finally:
        engine.close()
    data, offsets = torch.ops.gance.jpeg_encode(frames, QUALITY)
    host_offsets = offsets.cpu().numpy()
    data = data[: int(host_offsets[-1])].clone()
    blob = data.cpu().numpy().tobytes()
    return data, offsets, [blob[host_offsets[i] : host_offsets[i + 1]] for i in range(BATCH)]


class DecodeCall:  # pylint: disable=too-few-public-methods
    """gance_jpeg_decode_u8 on buffers made once."""

    def __init__(self, data: torch.Tensor, files) -> None:
        self.data = data
        self.infos = (hip_lib.JpegInfo * BATCH)()
        for info, blob in zip(self.infos, files):
            hip_lib.jpeg_parse_header(blob, info)
        self.offsets = np.zeros((BATCH + 1,), dtype=np.int64)
        self.offsets[1:] = np.cumsum([len(blob) for blob in files])
        self.workspace_bytes = hip_lib.jpeg_decode_bounds(BATCH, SIDE, SIDE, int(self.offsets[-1]))
        self.workspace = torch.empty((self.workspace_bytes,), dtype=torch.uint8, device=data.device)
        self.out = torch.empty((BATCH, SIDE, SIDE, 3), dtype=torch.uint8, device=data.device)
        self.status = torch.empty((BATCH,), dtype=torch.int32, device=data.device)

    def __call__(self) -> None:
        hip_lib.jpeg_decode_device(
            self.data.data_ptr(), self.offsets, self.infos, self.workspace.data_ptr(), self.workspace_bytes, self.out.data_ptr(),
            self.status.data_ptr(), torch.cuda.current_stream().cuda_stream,
        )


def call_ms(call: DecodeCall, calls: int = 8) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def main() -> None:  # pylint: disable=too-many-locals
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    parser.add_argument("--decode-only", action="store_true", help="leg 1 only (for the rocprofv3 run)")
    parser.add_argument("--rounds", type=int, default=3)
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    data, offsets, files = encoded_frames()
    call = DecodeCall(data, files)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    assert call.status.cpu().tolist() == [0] * BATCH
    assert np.array_equal(call.out[BATCH - 1].cpu().numpy(), np.asarray(Image.open(io.BytesIO(files[-1])).convert("RGB")))
    if options.decode_only:
        print(json.dumps({"decode_call_ms": [call_ms(call) for _ in range(options.rounds)]}), flush=True)
        return

    work = Path(tempfile.mkdtemp(prefix="mjpeg_decode_rate_"))
    avi_path = work / "frames.avi"
    with mjpeg_avi.MjpegAviWriter(avi_path, SIDE, 60.0) as writer:
        for blob in files:
            writer.add_frame(blob)
    torch.ops.gance.jpeg_decode(data, offsets)
    for _chunk in video_common.frames_in_video_device_chunks(avi_path, BATCH):
        pass
    result = {"decode_call_ms": [], "op_ms": [], "pil_ms": [], "file_to_hbm_ms": []}
    for _ in range(options.rounds):
        result["decode_call_ms"].append(call_ms(call))
        clock = time.perf_counter()
        torch.ops.gance.jpeg_decode(data, offsets)
        result["op_ms"].append((time.perf_counter() - clock) * 1e3)
        clock = time.perf_counter()
        for blob in files:
            Image.open(io.BytesIO(blob)).convert("RGB").load()
        result["pil_ms"].append((time.perf_counter() - clock) * 1e3)
        clock = time.perf_counter()
        for _chunk in video_common.frames_in_video_device_chunks(avi_path, BATCH):
            pass
        torch.cuda.synchronize()
        result["file_to_hbm_ms"].append((time.perf_counter() - clock) * 1e3)
    avi_path.unlink()
    work.rmdir()
    compressed = int(call.offsets[-1])
    best = min(result["decode_call_ms"])
    result.update(
        frames_per_call=BATCH, side=SIDE, quality=QUALITY, compressed_bytes_per_frame=compressed / BATCH,
        frames_per_s=BATCH / (best / 1e3), compressed_mb_per_s_in=compressed / (best / 1e3) / 1e6,
        rgb_gb_per_s_out=call.out.numel() / (best / 1e3) / 1e9, file_to_hbm_frames_per_s=BATCH / (min(result["file_to_hbm_ms"]) / 1e3),
        pil_over_decode_call=min(result["pil_ms"]) / max(result["decode_call_ms"]),
        decode_call_faster_than_pil=max(result["decode_call_ms"]) < min(result["pil_ms"]),
        workspace_bytes=call.workspace_bytes,
    )
    print(json.dumps(result), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
