"""
CPU tests of the 3-D view's host side (gance_amd/debug_video/scatter3d.py), of the argument checks of its two C entries
(which run before any device is touched), and of vector_synthesis' argument rules for the visualisation frames.
"""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import scatter3d_ref as ref
from gance_amd import hip_lib
from gance_amd.data_into_network_visualization import network_visualization
from gance_amd.data_into_network_visualization.visualization_common import DataLabel, ResultLayers, VisualizationInput
from gance_amd.debug_video import scatter3d, synthesis_visualization
from gance_amd.network_interface import network_functions
from gance_amd.vector_sources.vector_types import VectorsLabel


# ---- 1. view, limits, table ----------------------------------------------------------------------------------------------
def test_view_vectors_are_orthonormal() -> None:
    frame = np.array(scatter3d.view_vectors(50, 300))
    assert np.abs(frame @ frame.T - np.eye(3)).max() <= 1e-15
    right, up, toward = scatter3d.view_vectors(50, 300)
    assert right[2] == 0.0 and up[2] > 0 and toward[2] > 0  # z points up the panel and the view is from above
    assert np.allclose(np.cross(right, up), toward, atol=1e-15)  # right-handed: `toward` looks at the viewer


def test_cube_corners_fill_the_axis_rectangle() -> None:
    """The half extents fit the projected unit cube to the rectangle exactly: both extreme columns and rows are reached."""
    values = np.random.RandomState(1).standard_normal((12, 32))
    for side in (64, 96, 512):
        panel = scatter3d.Scatter3dPanel(side, values, "Combined")
        x, y, width, height = panel.rectangle
        assert x >= 0 and y >= 0 and x + width <= side and y + height <= side
        corners = [
            scatter3d.project(tuple(panel.limits[name][bit] for name, bit in zip("xyz", bits)), panel.limits, panel.vectors, width, height)
            for bits in itertools.product((0, 1), repeat=3)
        ]
        columns, rows, levels = (sorted(values) for values in zip(*corners))
        assert (columns[0], columns[-1]) == (0, width - 1) and (rows[0], rows[-1]) == (0, height - 1)
        assert (levels[0], levels[-1]) == (0, 65535)
        # the host projection and the restatement are the same rule
        view = ref.make_view(panel.rectangle, *(panel.limits[name] for name in ("x", "y", "z", "colour")), *panel.vectors)
        column_at, row_at, _ = ref.positions(view, [panel.limits["x"][1]], [3.0], [0.0])
        got = scatter3d.project((panel.limits["x"][1], 3.0, 0.0), panel.limits, panel.vectors, width, height)
        assert got[:2] == (int(np.floor(column_at[0] + 0.5)), height - 1 - int(np.floor(row_at[0] + 0.5)))


def test_limits_follow_the_rule() -> None:
    values = np.array([[1.0, 2.0, 4.0], [3.0, np.nan, 2.5]])
    limits = scatter3d.cloud_limits(values)
    assert limits == {"x": (0.0, 4.0), "y": (0.0, 1.0), "z": (0.0, 4.0), "colour": (1.0, 4.0)}  # ceil(1.1 * 3) = 4; z takes in the marker's 0
    assert limits == ref.limits_of(values)
    constant = scatter3d.cloud_limits(np.full((1, 10), -2.0))
    assert constant == {"x": (0.0, 11.0), "y": (0.0, 1.0), "z": (-2.0, 0.0), "colour": (-2.0, -1.0)}  # widened by span
    assert constant == ref.limits_of(np.full((1, 10), -2.0))
    panel = scatter3d.Scatter3dPanel(1024, values, "c")
    view = panel.view()
    assert (view.point_size, view.marker_size, tuple(view.marker_rgb), view.marker_x, view.marker_z) == (3, 10, (255, 0, 0), 4.0, 0.0)
    assert (view.x, view.y, view.width, view.height) == panel.rectangle and panel.cursor(7) == 7.0
    assert scatter3d.Scatter3dPanel(64, values, "c").view().marker_size == 2


def test_chrome_is_a_white_panel_with_title_cube_and_labels() -> None:
    panel = scatter3d.Scatter3dPanel(128, np.random.RandomState(2).standard_normal((9, 16)), "Combined")
    image = panel.chrome()
    assert image.shape == (128, 128, 3) and image.dtype == np.uint8
    x, y, width, height = panel.rectangle
    inside = image[y : y + height, x : x + width].reshape(-1, 3)
    assert {tuple(pixel) for pixel in inside} == {(255, 255, 255), (220, 220, 220)}  # the cube's edges only
    assert (image[:y] == 0).any() and (image[y + height :] == 0).any()  # the title above, the labels below
    small = scatter3d.Scatter3dPanel(16, np.zeros((2, 4)), "c")
    assert small.chrome().shape == (16, 16, 3) and not small.titled and not small.labelled


def test_greens_table() -> None:
    table = scatter3d.GREENS
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert tuple(table[0]) == (247, 252, 245) and tuple(table[128]) == (115, 195, 117) and tuple(table[255]) == (0, 68, 27)
    assert np.array_equal(table, scatter3d.greens_from_nodes())  # the committed table is the nine nodes' segments


def test_greens_table_is_matplotlibs() -> None:
    matplotlib = pytest.importorskip("matplotlib")
    assert np.array_equal(scatter3d.GREENS, matplotlib.colormaps["Greens"](np.arange(256), bytes=True)[:, :3])


# ---- 2. the C entries refuse bad arguments before touching a device --------------------------------------------------------
@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


INVALID = 1  # GANCE_ERR_INVALID_ARGUMENT
FAKE = 0x10000  # a non-NULL, 16-byte aligned "device pointer": every call below must return before it is looked at
F32, F64, I32 = 0, 1, 2


def good_view(**changes) -> hip_lib.DebugView3d:
    view = scatter3d.Scatter3dPanel(32, np.arange(12.0).reshape(3, 4), "c").view()
    for name, value in changes.items():
        setattr(view, name, (ctypes.c_double * 3)(*value) if name in ("right", "up", "toward") else value)
    return view


BAD_VIEWS = [
    dict(x=-1), dict(y=30), dict(width=0), dict(width=31), dict(height=40),                      # a rectangle outside the panel
    dict(x_min=float("nan")), dict(y_max=float("inf")), dict(z_min=3.0, z_max=3.0), dict(c_min=1.0, c_max=1.0),  # limits
    dict(right=(0.0, 0.0, 0.0)), dict(up=(0.0, 0.0, 0.0)), dict(toward=(0.0, 0.0, 0.0)), dict(up=(float("nan"), 1.0, 0.0)),
    dict(point_size=0), dict(point_size=65), dict(marker_size=0), dict(marker_size=65),
    dict(marker_x=float("inf")),
]


def scatter_arguments(**changes):
    arguments = dict(
        chrome=FAKE, side=32, view=good_view(), values=FAKE, dtype=F64, num_vectors=3, vector_length=4, vector_stride=4, lut=FAKE,
        keys=FAKE, template=FAKE,
    )
    arguments.update(changes)
    return arguments


def call_scatter(library: ctypes.CDLL, **changes) -> int:
    a = scatter_arguments(**changes)
    view = ctypes.byref(a["view"]) if a["view"] is not None else None
    return library.gance_debug_scatter3d_u8(
        a["chrome"], a["side"], view, a["values"], a["dtype"], a["num_vectors"], a["vector_length"], a["vector_stride"], a["lut"], a["keys"],
        a["template"], None,
    )


def call_draw(library: ctypes.CDLL, **changes) -> int:
    a = dict(template=FAKE, side=32, view=good_view(), frames=FAKE, batch=2, out=FAKE, frame_stride=32 * 192, row_stride=192)
    a.update(changes)
    view = ctypes.byref(a["view"]) if a["view"] is not None else None
    return library.gance_debug_draw_scatter3d_u8(a["template"], a["side"], view, a["frames"], a["batch"], a["out"], a["frame_stride"], a["row_stride"], None)


SCATTER_REFUSALS = [
    dict(chrome=None), dict(view=None), dict(values=None), dict(lut=None), dict(keys=None), dict(template=None),      # NULL
    dict(side=0), dict(side=24), dict(side=4112),                                                                      # side
    dict(chrome=FAKE + 8), dict(template=FAKE + 4), dict(keys=FAKE + 4), dict(values=FAKE + 4), dict(values=FAKE + 2, dtype=F32),  # alignment
    dict(dtype=I32), dict(dtype=-1), dict(dtype=7),                                                                    # dtype
    dict(num_vectors=0), dict(vector_length=0), dict(num_vectors=-3), dict(num_vectors=1 << 30, vector_length=1 << 10, vector_stride=1 << 10),
    dict(num_vectors=1 << 62, vector_length=4), dict(vector_stride=3),                                                 # counts
] + [dict(view=good_view(**changes)) for changes in BAD_VIEWS]

DRAW_REFUSALS = [
    dict(template=None), dict(view=None), dict(frames=None), dict(out=None),
    dict(side=8), dict(side=40), dict(side=8192, frame_stride=8192 * 8192 * 3, row_stride=8192 * 3),
    dict(template=FAKE + 8), dict(frames=FAKE + 4), dict(out=FAKE + 8), dict(row_stride=200), dict(frame_stride=32 * 192 + 8),
    dict(row_stride=80), dict(frame_stride=1024), dict(batch=0), dict(batch=70000),
] + [dict(view=good_view(**changes)) for changes in BAD_VIEWS]


def test_the_good_arguments_differ_from_each_refusal_only_in_what_it_names() -> None:
    """(the tables above change one thing each; what they start from passes every check of the host wrappers' view)"""
    view = good_view()
    assert 0 <= view.x and view.x + view.width <= 32 and 0 <= view.y and view.y + view.height <= 32
    assert ctypes.sizeof(hip_lib.DebugView3d) == 4 * 4 + 8 * 8 + 9 * 8 + 2 * 4 + 4 + 4 + 2 * 8


@pytest.mark.parametrize("changes", SCATTER_REFUSALS, ids=lambda changes: ",".join(changes))
def test_scatter3d_refuses(library: ctypes.CDLL, changes: dict) -> None:
    assert call_scatter(library, **changes) == INVALID
    assert b"gance_debug_scatter3d_u8" in library.gance_last_error()


@pytest.mark.parametrize("changes", DRAW_REFUSALS, ids=lambda changes: ",".join(changes))
def test_draw_scatter3d_refuses(library: ctypes.CDLL, changes: dict) -> None:
    assert call_draw(library, **changes) == INVALID
    assert b"gance_debug_draw_scatter3d_u8" in library.gance_last_error()


def test_refusals_name_the_value_and_reach_python_as_value_errors(library: ctypes.CDLL) -> None:
    assert call_scatter(library, side=24) == INVALID and b"24" in library.gance_last_error()
    assert call_scatter(library, view=good_view(point_size=65)) == INVALID and b"65" in library.gance_last_error()
    assert call_draw(library, view=good_view(marker_size=0)) == INVALID and b"marker_size" in library.gance_last_error()
    assert call_scatter(library, num_vectors=1 << 30, vector_length=1 << 10, vector_stride=1 << 10) == INVALID
    assert b"2^40" in library.gance_last_error()
    with pytest.raises(ValueError, match="dtype"):
        hip_lib.debug_scatter3d_device(FAKE, 32, good_view(), FAKE, I32, 3, 4, 4, FAKE, FAKE, FAKE)
    with pytest.raises(ValueError, match="NULL"):
        hip_lib.debug_draw_scatter3d_device(FAKE, 32, None, FAKE, 1, FAKE, 32 * 96, 96)
    with pytest.raises(ValueError, match="16-byte"):
        hip_lib.debug_draw_scatter3d_device(FAKE, 32, good_view(), FAKE, 1, FAKE + 4, 32 * 96, 96)


# ---- 3. vector_synthesis' argument rules -----------------------------------------------------------------------------------
@pytest.fixture
def refuse_everything(monkeypatch) -> None:
    """Neither a network nor the library nor a device may be touched by a call that only builds lazy iterators."""

    def touched(*_args, **_kwargs):
        raise AssertionError("the device was touched before an iterator was pulled")

    monkeypatch.setattr(network_functions, "LoadedNetwork", touched)
    monkeypatch.setattr(hip_lib, "load_library", touched)
    monkeypatch.setattr(torch.cuda, "current_device", touched)
    monkeypatch.setattr(torch.cuda, "current_stream", touched)
    monkeypatch.setattr(synthesis_visualization, "_upload", touched)
    monkeypatch.setattr(torch, "empty", touched)


def visualization_input(num_frames: int = 12, length: int = 32) -> VisualizationInput:
    rs = np.random.RandomState(5)
    a, b = rs.uniform(-3, 7, num_frames * length), rs.uniform(-2, 2, num_frames * length)
    indices = (np.arange(num_frames) // 3) % 3
    return VisualizationInput(
        VectorsLabel(a, length, "A"), VectorsLabel(b, length, "B"), VectorsLabel(a + b, length, "Combined"),
        ResultLayers(DataLabel(indices, "Quantized"), [DataLabel(indices + 0.25, "Smoothed")]),
    )


def test_vector_synthesis_argument_rules(refuse_everything) -> None:  # pylint: disable=unused-argument,redefined-outer-name
    data = visualization_input()
    with pytest.raises(ValueError, match="Nothing to render!"):
        network_visualization.vector_synthesis(data, None, enable_2d=False, enable_3d=False, visualization_height=64)
    for flags in (dict(enable_2d=True), dict(enable_2d=False, enable_3d=True), dict(enable_2d=True, enable_3d=True)):
        with pytest.raises(ValueError, match="visualization_height"):  # neither a height nor networks
            network_visualization.vector_synthesis(data, None, default_vector_length=32, **flags)
        for height in (100, 8, 4112, 0):
            with pytest.raises(ValueError, match="visualization_height must be a multiple of 16.*" + str(height)):
                network_visualization.vector_synthesis(data, None, default_vector_length=32, visualization_height=height, **flags)
    with pytest.raises(ValueError, match="visualization_height"):
        network_visualization.vector_synthesis_visualization_chunks(data, 32, 100)
    with pytest.raises(ValueError, match="Nothing to render!"):
        network_visualization.vector_synthesis_visualization_chunks(data, 32, 64, enable_2d=False, enable_3d=False)


def test_vector_synthesis_is_lazy(refuse_everything) -> None:  # pylint: disable=unused-argument,redefined-outer-name
    data = visualization_input()
    output = network_visualization.vector_synthesis(
        data, None, default_vector_length=32, enable_2d=True, enable_3d=True, visualization_height=64, network_index_window_width=5
    )
    assert output.synthesized_images is None and output.visualization_images is not None
    assert iter(output.visualization_images) is output.visualization_images  # an iterator, not a list
    chunks = network_visualization.vector_synthesis_visualization_chunks(data, 32, 64, enable_3d=True, chunk_frames=5)
    assert iter(chunks) is chunks
    with pytest.raises(AssertionError, match="touched"):  # the work starts with the first pull
        next(output.visualization_images)
