"""
GPU tests of the visualisation frames of vector_synthesis (the reference's test/test_network_visualization.py:114-175):
every combination of the 2-D panel, the 3-D view and network / no network; the 2-D half against the debug video's own
path, the 3-D half against the restatement of tests/scatter3d_ref.py; truncation, chunking, and both iterators of a run
with a network.
"""

from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np
import pytest
import torch

import scatter3d_ref as ref
from gance_amd import hip_lib, network_file
from gance_amd.data_into_network_visualization import network_visualization
from gance_amd.data_into_network_visualization.visualization_common import DataLabel, ResultLayers, VisualizationInput
from gance_amd.debug_video import compose, panels, scatter3d
from gance_amd.network_interface import network_functions
from gance_amd.vector_sources.vector_types import MatricesLabel, VectorsLabel

pytestmark = pytest.mark.gpu

FRAMES, LENGTH, HEIGHT, WINDOW = 12, 32, 64, 5
FLAGS = {"2d": (True, False), "3d": (False, True), "both": (True, True)}


def visualization_input(kind: str, num_frames: int = FRAMES, length: int = LENGTH, depth: int = 18) -> VisualizationInput:
    """Vectors, or [depth, N L] matrices whose rows differ (only row 0 may show)."""
    rs = np.random.RandomState(23)
    shape = (num_frames * length,) if kind == "vectors" else (depth, num_frames * length)
    a, b = rs.uniform(-3, 7, shape), rs.uniform(-2, 2, shape)
    label = VectorsLabel if kind == "vectors" else MatricesLabel
    indices = (np.arange(num_frames) // 3) % 3
    return VisualizationInput(
        label(a, length, "A"), label(b, length, "B"), label(a + b, length, "Combined"),
        ResultLayers(DataLabel(indices, "Quantized"), [DataLabel(indices + 0.25, "Smoothed")]),
    )


def first_rows(member, length: int = LENGTH) -> np.ndarray:
    data = np.asarray(member.data, dtype=np.float64)
    return (data if data.ndim == 1 else data[0]).reshape(-1, length)


def run(data: VisualizationInput, enable_2d: bool, enable_3d: bool, **keywords) -> List[np.ndarray]:
    output = network_visualization.vector_synthesis(
        data, None, default_vector_length=LENGTH, visualization_height=HEIGHT, enable_2d=enable_2d, enable_3d=enable_3d,
        network_index_window_width=WINDOW, **keywords,
    )
    assert output.synthesized_images is None
    return [np.array(frame) for frame in output.visualization_images]


@pytest.fixture(scope="module")
def frames() -> Dict[Tuple[str, str], List[np.ndarray]]:
    """(kind, flags) -> the frames of a run without networks: computed once, never changed."""
    return {
        (kind, name): run(visualization_input(kind), *flags) for kind in ("vectors", "matrices") for name, flags in FLAGS.items()
    }


@pytest.mark.parametrize("kind", ["vectors", "matrices"])
def test_frame_shapes_and_halves(frames, kind: str) -> None:
    for name, (enable_2d, enable_3d) in FLAGS.items():
        got = frames[kind, name]
        assert len(got) == FRAMES
        for frame in got:
            assert frame.dtype == np.uint8 and frame.shape == (HEIGHT, HEIGHT * (enable_2d + enable_3d), 3)
    for both, left, right in zip(frames[kind, "both"], frames[kind, "2d"], frames[kind, "3d"]):
        assert np.array_equal(both[:, :HEIGHT], left) and np.array_equal(both[:, HEIGHT:], right)
    assert not np.array_equal(frames[kind, "both"][0], frames[kind, "both"][1])


@pytest.mark.parametrize("kind", ["vectors", "matrices"])
def test_2d_half_is_the_debug_videos_synthesis_panel(frames, kind: str) -> None:
    """SynthesisPanel.from_visualization_input + gance_debug_draw_panels_u8, driven directly, window by window."""
    data = visualization_input(kind)
    panel = panels.SynthesisPanel.from_visualization_input(HEIGHT, data, LENGTH, WINDOW)
    series = {name: torch.from_numpy(first_rows(member)).cuda() for name, member in (("a", data.a_vectors), ("b", data.b_vectors), ("combined", data.combined))}
    series.update({name: torch.from_numpy(np.ascontiguousarray(values)).cuda() for name, values in panel.host_series().items()})
    out = torch.zeros((FRAMES, HEIGHT, HEIGHT, 3), dtype=torch.uint8, device="cuda")
    for index in range((FRAMES + panel.width - 1) // panel.width):
        window = panel.window(index)
        numbers = list(range(window.first_frame, window.first_frame + window.num_frames))
        records = torch.from_numpy(compose.frame_records(numbers, [panel.cursor(n) for n in numbers], [0] * len(numbers)).view(np.uint8)).cuda()
        chrome = torch.from_numpy(window.chrome(HEIGHT)).cuda()
        rows = out[window.first_frame :]
        hip_lib.debug_draw_panels_device(
            chrome.data_ptr(), HEIGHT, compose.bind_axes(window.axes), compose.bind_marks(window.marks, series), records.data_ptr(),
            len(numbers), rows.data_ptr(), rows.stride(0), rows.stride(1), torch.cuda.current_stream().cuda_stream,
        )
        torch.cuda.synchronize()
    want = out.cpu().numpy()
    assert (want != 255).any(axis=-1).mean() > 0.02
    for number, frame in enumerate(frames[kind, "both"]):
        assert np.array_equal(frame[:, :HEIGHT], want[number]), number


@pytest.mark.parametrize("kind", ["vectors", "matrices"])
def test_3d_half_is_the_restated_rule(frames, kind: str) -> None:
    data = visualization_input(kind)
    values = first_rows(data.combined)
    panel = scatter3d.Scatter3dPanel(HEIGHT, values, data.combined.label)
    limits = ref.limits_of(values)
    view = ref.make_view(
        panel.rectangle, limits["x"], limits["y"], limits["z"], limits["colour"], *scatter3d.view_vectors(50, 300),
        point_size=1 + HEIGHT // 512, marker_size=2 + HEIGHT // 128, marker_rgb=(255, 0, 0), marker_x=limits["x"][1], marker_z=0.0,
    )
    want = ref.template(panel.chrome(), view, values, scatter3d.GREENS)
    margin = min(want.smallest_margin, ref.marker_margin(view, [0.0, float(FRAMES - 1)]))
    print(f"{kind}: smallest distance to a rounding boundary {margin:.3e}; {want.reached} pixels reached, {want.contested} contested")
    assert margin > 1e-6 and want.reached > 100
    for number in (0, FRAMES - 1):
        expected = ref.frame(want.image, view, float(number))
        assert (expected != want.image).any(), "the marker does not show"
        assert np.array_equal(frames[kind, "3d"][number], expected), number
        assert np.array_equal(frames[kind, "both"][number][:, HEIGHT:], expected), number


def test_truncation_and_chunking(frames) -> None:
    data = visualization_input("matrices")
    limited = run(data, True, True, frames_to_visualize=5)
    assert len(limited) == 5  # the 3-D half still shows all 12 vectors: it is the full run's
    for got, want in zip(limited, frames["matrices", "both"]):
        assert np.array_equal(got, want)
    for chunk_frames, firsts in ((5, [0, 5, 10]), (64, [0])):
        chunks = list(network_visualization.vector_synthesis_visualization_chunks(
            data, LENGTH, HEIGHT, enable_3d=True, enable_2d=True, network_index_window_width=WINDOW, chunk_frames=chunk_frames,
        ))
        assert [first for first, _ in chunks] == firsts
        assert all(chunk.is_cuda and chunk.dtype == torch.uint8 and chunk.shape[1:] == (HEIGHT, 2 * HEIGHT, 3) for _, chunk in chunks)
        got = torch.cat([chunk for _, chunk in chunks]).cpu().numpy()
        assert np.array_equal(got, np.stack(frames["matrices", "both"])), chunk_frames


def test_with_a_network_both_iterators_drain_in_either_order(tmp_path: Path) -> None:
    resolution, num_frames, length = 32, 6, 512
    path = tmp_path / "network_0.pkl"
    network_file.write_random_network(path, resolution, seed=0)
    data = visualization_input("matrices", num_frames, length, depth=8)  # a 32 x 32 generator takes 8 rows
    with network_functions.MultiNetwork(network_paths=[path, path]) as multi:  # (the indices reach 1)
        assert multi.resolution == resolution
        plain = network_visualization.vector_synthesis(data, multi, enable_2d=False, enable_3d=False)
        assert plain.visualization_images is None
        want = [np.array(frame) for frame in plain.synthesized_images]
        first = network_visualization.vector_synthesis(data, multi, enable_2d=True, enable_3d=True, network_index_window_width=4)
        visualization = [np.array(frame) for frame in first.visualization_images]
        synthesized = [np.array(frame) for frame in first.synthesized_images]
        second = network_visualization.vector_synthesis(data, multi, enable_2d=True, enable_3d=True, network_index_window_width=4)
        synthesized_again = [np.array(frame) for frame in second.synthesized_images]
        visualization_again = [np.array(frame) for frame in second.visualization_images]
    assert len(want) == len(synthesized) == len(visualization) == num_frames
    assert all(frame.shape == (resolution, 2 * resolution, 3) and frame.dtype == np.uint8 for frame in visualization)
    assert all(frame.shape == (resolution, resolution, 3) for frame in synthesized)
    for got in (synthesized, synthesized_again):
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(visualization, visualization_again))
