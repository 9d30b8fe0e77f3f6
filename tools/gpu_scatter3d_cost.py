"""
Cost of the 3-D view of vector_synthesis' visualisation on one GPU (`python tools/gpu_scatter3d_cost.py [--out FILE]`),
HIP events after a warm-up, three alternated rounds in one process:

1. the template build (gance_debug_scatter3d_u8: workspace memset + point pass + resolve pass) for N = 1800 and N = 18000
   vectors of L = 512 at sides 512 and 1024, beside the same call for ONE point (what the memset and the resolve pass cost
   without a cloud); the two passes separately come from a `rocprofv3 --kernel-trace --stats` run of `--template-only`;
2. a chunk of 64 frames at side 1024: the 3-D panel (gance_debug_draw_scatter3d_u8: template copy + marker) against the
   2-D synthesis-inputs panel of the same frames (gance_debug_draw_panels_u8: chrome copy + marks).
"""

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.data_into_network_visualization.visualization_common import DataLabel, ResultLayers, VisualizationInput  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.debug_video import compose, panels, scatter3d  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.vector_sources.vector_types import VectorsLabel  # noqa: E402  pylint: disable=wrong-import-position

LENGTH, CHUNK, ROUNDS, REPEATS = 512, 64, 3, 10
F64 = hip_lib.DEBUG_DTYPES[np.dtype(np.float64)]


def timed(call, repeats: int = REPEATS) -> float:
    """Milliseconds per call over `repeats` calls between two events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / repeats


def template_builder(side: int, values: np.ndarray):
    """A call that builds the template of `values` [N, L] at `side`, and the same for the first point alone."""
    panel = scatter3d.Scatter3dPanel(side, values, "Combined")
    view = panel.view()
    d_values = torch.from_numpy(values).cuda()
    d_chrome, d_lut = torch.from_numpy(panel.chrome()).cuda(), torch.from_numpy(scatter3d.GREENS.copy()).cuda()
    d_keys = torch.empty(side * side, dtype=torch.int64, device="cuda")
    d_template = torch.empty((side, side, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def build(count: int, length: int):
        def call() -> None:
            hip_lib.debug_scatter3d_device(
                d_chrome.data_ptr(), side, view, d_values.data_ptr(), F64, count, length, length, d_lut.data_ptr(), d_keys.data_ptr(),
                d_template.data_ptr(), stream,
            )
        return call

    keep = (d_values, d_chrome, d_lut, d_keys, d_template)
    return build(*values.shape), build(1, 1), panel, view, keep


def template_leg() -> dict:
    out = {}
    for count in (1800, 18000):
        values = np.random.RandomState(count).standard_normal((count, LENGTH))
        for side in (512, 1024):
            whole, one_point, _panel, _view, keep = template_builder(side, values)
            timed(whole, 2), timed(one_point, 2)  # warm-up
            rounds = {"whole_ms": [], "one_point_ms": []}
            for _ in range(ROUNDS):
                rounds["whole_ms"].append(timed(whole))
                rounds["one_point_ms"].append(timed(one_point))
            rounds["points"] = count * LENGTH
            out[f"n{count}_side{side}"] = rounds
            del keep
    return out


def chunk_leg(side: int = 1024, count: int = 1800) -> dict:
    rs = np.random.RandomState(3)
    a, b = rs.uniform(-3, 7, count * LENGTH), rs.uniform(-2, 2, count * LENGTH)
    indices = (np.arange(count) // 40) % 3
    data = VisualizationInput(
        VectorsLabel(a, LENGTH, "A"), VectorsLabel(b, LENGTH, "B"), VectorsLabel(a + b, LENGTH, "Combined"),
        ResultLayers(DataLabel(indices, "Quantized"), [DataLabel(indices + 0.25, "Smoothed")]),
    )
    values = (a + b).reshape(count, LENGTH)
    build, _one, cloud, view, keep = template_builder(side, values)
    build()
    d_template = keep[4]
    synthesis = panels.SynthesisPanel.from_visualization_input(side, data, LENGTH, None)  # windows of 360 frames
    series = {name: torch.from_numpy(member.reshape(count, LENGTH)).cuda() for name, member in (("a", a), ("b", b), ("combined", a + b))}
    series.update({name: torch.from_numpy(np.ascontiguousarray(host)).cuda() for name, host in synthesis.host_series().items()})
    window = synthesis.window(0)
    d_chrome = torch.from_numpy(window.chrome(side)).cuda()
    axes, marks = compose.bind_axes(window.axes), compose.bind_marks(window.marks, series)
    numbers = list(range(100, 100 + CHUNK))
    records_2d = torch.from_numpy(compose.frame_records(numbers, [synthesis.cursor(n) for n in numbers], [0] * CHUNK).view(np.uint8)).cuda()
    records_3d = torch.from_numpy(compose.frame_records(numbers, [cloud.cursor(n) for n in numbers], [0] * CHUNK).view(np.uint8)).cuda()
    out = torch.empty((CHUNK, side, 2 * side, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def panel_2d() -> None:
        hip_lib.debug_draw_panels_device(d_chrome.data_ptr(), side, axes, marks, records_2d.data_ptr(), CHUNK, out.data_ptr(), out.stride(0), out.stride(1), stream)

    def panel_3d() -> None:
        hip_lib.debug_draw_scatter3d_device(
            d_template.data_ptr(), side, view, records_3d.data_ptr(), CHUNK, out.data_ptr() + side * 3, out.stride(0), out.stride(1), stream
        )

    timed(panel_2d, 2), timed(panel_3d, 2)  # warm-up
    result = {"side": side, "chunk": CHUNK, "panel_2d_ms": [], "panel_3d_ms": [], "panel_bytes": CHUNK * side * side * 3}
    for _ in range(ROUNDS):
        result["panel_2d_ms"].append(timed(panel_2d))
        result["panel_3d_ms"].append(timed(panel_3d))
    return result


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", type=Path, default=None, help="also write the JSON result here")
    parser.add_argument("--template-only", action="store_true", help="leg 1 only (for the rocprofv3 run)")
    options = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path")
    result = {"template": template_leg()}
    if not options.template_only:
        result["chunk"] = chunk_leg()
    print(json.dumps(result), flush=True)
    if options.out is not None:
        options.out.parent.mkdir(parents=True, exist_ok=True)
        options.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
