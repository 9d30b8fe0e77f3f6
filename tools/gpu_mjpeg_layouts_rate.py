"""
Rate of the HIP Motion-JPEG decoder per layout on one GPU (`python tools/gpu_mjpeg_layouts_rate.py [--out FILE]`), the
sibling of tools/gpu_mjpeg_decode_rate.py for files from elsewhere: 64 frames of 1024^2 per call (a random-init network's
frames), written by PIL at q 90 as 4:2:2, 4:2:0, 4:4:4 and grey, once with a restart interval per MCU row and once without
restart markers. After a warm-up, the rounds alternate, per layout and form,

1. the decode call alone (gance_jpeg_decode_layouts_u8 with the headers parsed beforehand; device events),
2. PIL decoding the same 64 files in this process (wall clock).

With restart markers the decode call must be faster than PIL for every layout. Without them a frame is one restart
segment, one thread: those figures carry no condition, they are the baseline for a parallel decoder of such files.
`--merge-422 FILE...` adds the per-call series of tools/gpu_mjpeg_decode_rate.py runs (`parent=FILE` / `branch=FILE`, in the
order they were run) to the result: the check that the 4:2:2 path has not slowed.
"""

import argparse
import io
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib, torch_ops  # noqa: E402,F401  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position

SIDE, BATCH, QUALITY = 1024, 64, 90
PIL_SUBSAMPLING = {"4:2:2": 1, "4:2:0": 2, "4:4:4": 0}
FORMS = {"restart_per_mcu_row": {"restart_marker_rows": 1}, "no_restarts": {}}
MCU_PIXELS = {"4:2:2": (16, 8), "4:2:0": (16, 16), "4:4:4": (8, 8), "grey": (8, 8)}


def network_frames() -> np.ndarray:
    """BATCH frames [SIDE][SIDE][3] of a random-init generator, on the host."""
    engine = hip_lib.Engine(sg2_spec.make_random_variables(SIDE, seed=0), SIDE, max_batch=BATCH, device=0)
    try:
        w = torch.from_numpy(np.random.RandomState(1).randn(BATCH, engine.num_layers, 512).astype(np.float32)).to("cuda:0")
        frames = torch.ops.gance.synthesize_w(w, engine.op_handle).cpu().numpy()
    finally:
        engine.close()
    return frames


def pil_files(frames: np.ndarray, layout: str, options: dict):
    files = []
    for frame in frames:
        buffer = io.BytesIO()
        if layout == "grey":
            Image.fromarray(np.ascontiguousarray(frame[..., 0])).save(buffer, format="JPEG", quality=QUALITY, **options)
        else:
            Image.fromarray(frame).save(buffer, format="JPEG", quality=QUALITY, subsampling=PIL_SUBSAMPLING[layout], **options)
        files.append(buffer.getvalue())
    return files


class DecodeCall:  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """gance_jpeg_decode_layouts_u8 on buffers made once."""

    def __init__(self, files) -> None:
        self.files = files
        self.data = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).cuda()
        self.infos = (hip_lib.JpegFrameInfo * BATCH)()
        for info, blob in zip(self.infos, files):
            hip_lib.jpeg_parse_header_layouts(blob, info)
        self.offsets = np.zeros((BATCH + 1,), dtype=np.int64)
        self.offsets[1:] = np.cumsum([len(blob) for blob in files])
        self.workspace_bytes = hip_lib.jpeg_decode_layouts_bounds(BATCH, SIDE, SIDE, self.infos[0].layout, int(self.offsets[-1]))
        self.workspace = torch.empty((self.workspace_bytes,), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((BATCH, SIDE, SIDE, 3), dtype=torch.uint8, device="cuda")
        self.status = torch.empty((BATCH,), dtype=torch.int32, device="cuda")

    def __call__(self) -> None:
        hip_lib.jpeg_decode_layouts_device(
            self.data.data_ptr(), self.offsets, self.infos, self.workspace.data_ptr(), self.workspace_bytes, self.out.data_ptr(),
            self.status.data_ptr(), torch.cuda.current_stream().cuda_stream,
        )


def call_ms(call: DecodeCall, calls: int) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def merged_422(entries) -> dict:
    """The alternated series of tools/gpu_mjpeg_decode_rate.py --decode-only runs, and the verdict the issue asks for."""
    series = {"parent": [], "branch": []}
    for entry in entries:
        side, path = entry.split("=", 1)
        series[side].append(json.loads(Path(path).read_text().strip().splitlines()[-1])["decode_call_ms"])
    parent = [ms for run in series["parent"] for ms in run]
    branch = [ms for run in series["branch"] for ms in run]
    spread = max(parent) - min(parent)
    return {
        "what": "tools/gpu_mjpeg_decode_rate.py --decode-only (2160^2, 64 frames, 4:2:2), parent and branch libraries alternated, ms per call",
        "parent_decode_call_ms": series["parent"], "branch_decode_call_ms": series["branch"],
        "parent_mean_ms": float(np.mean(parent)), "branch_mean_ms": float(np.mean(branch)), "parent_round_to_round_spread_ms": spread,
        "branch_within_parent_spread": float(np.mean(branch)) - float(np.mean(parent)) <= spread,
    }  # fmt: skip


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--merge-422", nargs="*", default=[], metavar="SIDE=FILE", help="parent=FILE / branch=FILE of gpu_mjpeg_decode_rate.py runs")
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    frames = network_frames()
    result = {"frames_per_call": BATCH, "side": SIDE, "quality": QUALITY, "layouts": {}}
    calls = {}
    for layout in hip_lib.JPEG_LAYOUT_NAMES:
        for form, pil_options in FORMS.items():
            call = DecodeCall(pil_files(frames, layout, pil_options))
            call()
            torch.cuda.synchronize()
            assert call.status.cpu().tolist() == [0] * BATCH
            want = np.asarray(Image.open(io.BytesIO(call.files[-1])).convert("RGB"))
            assert np.array_equal(call.out[BATCH - 1].cpu().numpy(), want), (layout, form)
            calls[(layout, form)] = call
            interval = call.infos[0].info.restart_interval
            mcus = (SIDE // MCU_PIXELS[layout][0]) * (SIDE // MCU_PIXELS[layout][1])
            result["layouts"].setdefault(layout, {})[form] = {
                "decode_call_ms": [], "pil_ms": [], "compressed_bytes_per_frame": int(call.offsets[-1]) / BATCH,
                "segments_per_frame": -(-mcus // interval) if interval else 1,
                "workspace_bytes": call.workspace_bytes,
            }  # fmt: skip
    for _ in range(options.rounds):
        for (layout, form), call in calls.items():
            entry = result["layouts"][layout][form]
            entry["decode_call_ms"].append(call_ms(call, 8 if form != "no_restarts" else 2))
            clock = time.perf_counter()
            for blob in call.files:
                Image.open(io.BytesIO(blob)).convert("RGB").load()
            entry["pil_ms"].append((time.perf_counter() - clock) * 1e3)
    for layout, forms in result["layouts"].items():
        for form, entry in forms.items():
            entry["frames_per_s"] = BATCH / (min(entry["decode_call_ms"]) / 1e3)
            entry["pil_over_decode_call"] = min(entry["pil_ms"]) / max(entry["decode_call_ms"])
            if form != "no_restarts":
                entry["decode_call_faster_than_pil"] = max(entry["decode_call_ms"]) < min(entry["pil_ms"])
    result["faster_than_pil_with_restarts_in_every_layout"] = all(
        forms["restart_per_mcu_row"]["decode_call_faster_than_pil"] for forms in result["layouts"].values()
    )
    if options.merge_422:
        result["decode_422_parent_and_branch"] = merged_422(options.merge_422)
    print(json.dumps(result), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
