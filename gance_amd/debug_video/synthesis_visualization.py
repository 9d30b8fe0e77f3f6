"""
The visualisation frames of `vector_synthesis` (the reference's matplotlib figure of network_visualization.py:54-157,
254-400, 542-596), composed in HBM: the 2-D "synthesis inputs" panel on the left (`panels.SynthesisPanel` drawn by
gance_debug_draw_panels_u8, exactly as the debug video draws it) and the 3-D view on the right (`scatter3d`:
the cloud rasterised once per run into a template, then a copy and one stamp per frame). Needs no network and no engine.
Nothing is launched, allocated or uploaded before the first chunk is asked for.
"""

from typing import Dict, Iterator, Optional, Tuple

import numpy as np
import torch

from gance_amd import hip_lib
from gance_amd.data_into_network_visualization.visualization_common import VisualizationInput
from gance_amd.debug_video import panels, scatter3d
from gance_amd.debug_video.compose import DebugVideoComposer, _upload, bind_axes, bind_marks, frame_records
from gance_amd.gance_types import RGBInt8ImageType
from gance_amd.vector_sources.vector_sources_common import sub_vectors
from gance_amd.vector_sources.vector_types import is_vector

CHUNK_FRAMES = 64


def validate_height(visualization_height: int) -> int:
    """:raises ValueError: a height the panels cannot take (not a multiple of 16 in [16, 4096])."""
    side = int(visualization_height)
    if side < 16 or side > 4096 or side % 16 != 0:
        raise ValueError(f"visualization_height must be a multiple of 16 in [16, 4096], got {visualization_height}")
    return side


def first_rows(data: np.ndarray, vector_length: int) -> np.ndarray:
    """[N, L] float64: the vectors themselves, or row 0 of every frame's matrix."""
    divided = np.asarray(sub_vectors(data=data, vector_length=vector_length))
    return np.ascontiguousarray(divided if is_vector(data) else divided[:, 0, :], dtype=np.float64)


def visualization_chunks(  # pylint: disable=too-many-arguments,too-many-locals
    data: VisualizationInput, vector_length: int, height: int, enable_2d: bool, enable_3d: bool, frames_to_visualize: Optional[int] = None,
    network_index_window_width: Optional[int] = None, chunk_frames: int = CHUNK_FRAMES, device: Optional[torch.device] = None,
) -> Iterator[Tuple[int, torch.Tensor]]:
    """
    (first frame, frames [n, height, height * (enable_2d + enable_3d), 3] uint8 in HBM) of consecutive chunks of at most
    `chunk_frames` frames, enqueued on the current stream of `device` (default: the current device). The frames do not
    depend on `chunk_frames`. `frames_to_visualize` limits the frames; the 3-D cloud always shows the whole run.
    """
    side = validate_height(height)
    if chunk_frames < 1:
        raise ValueError(f"chunk_frames must be >= 1, got {chunk_frames}")
    if not enable_2d and not enable_3d:
        raise ValueError("Nothing to render!")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())

    def stream() -> int:
        return torch.cuda.current_stream(device).cuda_stream

    combined_rows = first_rows(data.combined.data, vector_length)
    total = int(combined_rows.shape[0])
    count = total if frames_to_visualize is None else max(0, min(total, int(frames_to_visualize)))
    combined = _upload(combined_rows, device)

    synthesis, chrome = None, {}  # the 2-D panel, its series in HBM, the chrome of the window in use
    series: Dict[str, torch.Tensor] = {}
    if enable_2d:
        synthesis = panels.SynthesisPanel.from_visualization_input(side, data, vector_length, network_index_window_width)
        series = {
            "a": _upload(first_rows(data.a_vectors.data, vector_length), device),
            "b": _upload(first_rows(data.b_vectors.data, vector_length), device),
            "combined": combined,
        }
        series.update({name: _upload(values, device) for name, values in synthesis.host_series().items()})

    cloud, view, template = None, None, None
    if enable_3d:
        cloud = scatter3d.Scatter3dPanel(side, combined_rows, data.combined.label)
        view = cloud.view()
        cloud_chrome, lut = _upload(cloud.chrome(), device), _upload(scatter3d.GREENS, device)
        keys = torch.empty(side * side, dtype=torch.int64, device=device)
        template = torch.empty((side, side, 3), dtype=torch.uint8, device=device)
        hip_lib.debug_scatter3d_device(
            cloud_chrome.data_ptr(), side, view, combined.data_ptr(), hip_lib.DEBUG_DTYPES[np.dtype(np.float64)], cloud.num_vectors,
            cloud.vector_length, cloud.vector_length, lut.data_ptr(), keys.data_ptr(), template.data_ptr(), stream(),
        )

    width = side * (int(enable_2d) + int(enable_3d))
    for first in range(0, count, chunk_frames):
        frames_in_chunk = min(chunk_frames, count - first)
        out = torch.empty((frames_in_chunk, side, width, 3), dtype=torch.uint8, device=device)
        if synthesis is not None:
            for window_index, start, frames_in_run in DebugVideoComposer._runs(first, frames_in_chunk, synthesis.width):  # pylint: disable=protected-access
                window = synthesis.window(window_index)
                if window_index not in chrome:
                    chrome.clear()  # (frames come in order: one window is live)
                    chrome[window_index] = _upload(window.chrome(side), device)
                numbers = list(range(start, start + frames_in_run))
                records = _upload(frame_records(numbers, [synthesis.cursor(n) for n in numbers], [0] * frames_in_run).view(np.uint8), device)
                rows = out[start - first :]
                hip_lib.debug_draw_panels_device(
                    chrome[window_index].data_ptr(), side, bind_axes(window.axes), bind_marks(window.marks, series), records.data_ptr(),
                    frames_in_run, rows.data_ptr(), rows.stride(0), rows.stride(1), stream(),
                )
        if cloud is not None:
            numbers = list(range(first, first + frames_in_chunk))
            records = _upload(frame_records(numbers, [cloud.cursor(n) for n in numbers], [0] * frames_in_chunk).view(np.uint8), device)
            hip_lib.debug_draw_scatter3d_device(
                template.data_ptr(), side, view, records.data_ptr(), frames_in_chunk, out.data_ptr() + int(enable_2d) * side * 3,
                out.stride(0), out.stride(1), stream(),
            )
        yield first, out


def visualization_frames(chunks: Iterator[Tuple[int, torch.Tensor]]) -> Iterator[RGBInt8ImageType]:
    """The host frames of device chunks, each chunk brought over through one pinned buffer."""
    for _first, chunk in chunks:
        host = torch.empty(chunk.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(chunk, non_blocking=True)
        torch.cuda.current_stream(chunk.device).synchronize()
        frames = host.numpy()
        for frame in frames:
            yield RGBInt8ImageType(frame)
