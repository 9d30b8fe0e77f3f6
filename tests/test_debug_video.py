"""
CPU tests of the debug video's host side: the bitmap font, the chrome templates, the rectangular AVI header, the mark
tables of the three plot panels, and the argument checks of the new C entries (which run before any device is touched).
"""

import ctypes
import hashlib
import struct
from pathlib import Path

import numpy as np
import pytest
from scipy.io import wavfile

from gance_amd import hip_lib
from gance_amd.data_into_network_visualization.visualization_common import DataLabel, ResultLayers, VisualizationInput
from gance_amd.debug_video import chrome, font, panels
from gance_amd.overlay.overlay_common import OverlayContext
from gance_amd.vector_sources.vector_types import MatricesLabel, VectorsLabel
from gance_amd.video import mjpeg_avi

GOLDEN = Path(__file__).resolve().parent / "golden"


# ---- 1. font and chrome ------------------------------------------------------------------------------------------------
def test_every_printable_glyph_is_drawn() -> None:
    assert not font.glyph(" ").any()
    for code in range(33, 127):
        bitmap = font.glyph(chr(code))
        assert bitmap.shape == (7, 5) and bitmap.any(), chr(code)
    assert len({font.glyph(chr(code)).tobytes() for code in range(32, 127)}) == 95  # no two glyphs alike
    assert np.array_equal(font.glyph("\x07"), font.glyph("?"))


def test_text_scales_by_whole_pixels_and_clips() -> None:
    assert font.text_size("ab", 1) == (11, 7) and font.text_size("ab", 3) == (33, 21)
    small, large = font.text_mask("Ag", 1), font.text_mask("Ag", 2)
    assert np.array_equal(large, np.kron(small, np.ones((2, 2), dtype=bool)))
    assert [font.scale_for_side(side) for side in (64, 96, 383, 384, 512, 1024)] == [1, 1, 1, 2, 2, 3]
    image = np.zeros((8, 8, 3), dtype=np.uint8)
    font.draw_text(image, 5, -3, "W", (9, 9, 9))  # hangs over the top and the right edge
    font.draw_text(image, 100, 100, "W", (9, 9, 9))
    assert image.any() and image[:, :5].sum() == 0


def test_chrome_matches_golden() -> None:
    """tests/golden/debug_chrome.npz is written by tests/dev/make_debug_chrome_golden.py (our own drawing code)."""
    import importlib.util  # pylint: disable=import-outside-toplevel

    spec = importlib.util.spec_from_file_location("make_debug_chrome_golden", Path(__file__).resolve().parent / "dev" / "make_debug_chrome_golden.py")
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    golden = np.load(GOLDEN / "debug_chrome.npz")
    for side in (96, 400):
        template = chrome.render_chrome(side, maker.golden_axes(side))
        assert template.shape == (side, side, 3) and template.dtype == np.uint8
        assert np.array_equal(template, golden[f"side_{side}"]), side
    # what the template must show: a box one pixel outside the axis, the dotted threshold at the mapped row
    axis = maker.golden_axes(96)[0]
    template = chrome.render_chrome(96, [axis])
    assert (template[axis.y - 1, axis.x - 1 : axis.x + axis.width + 1] == 0).all()
    row = axis.y + (axis.height - 1) - chrome.map_extent(10.0, -5.0, 17.5, axis.height)
    assert tuple(template[row, axis.x]) == chrome.PURPLE and tuple(template[row, axis.x + 2]) != chrome.PURPLE


# ---- 2. the AVI writer with frames that are not square -------------------------------------------------------------------
def tiny_avi(path: Path, tmp_path: Path, **size) -> bytes:
    """
    Five fake JPEG chunks and half a second of 8 kHz int16 audio. The digest below is of this file as written by the
    writer BEFORE it took width= / height= (the parent commit's gance_amd/video/mjpeg_avi.py, called with side=32).
    """
    wav = tmp_path / "a.wav"
    wavfile.write(str(wav), 8000, (np.arange(4000) % 97 * 300 - 14000).astype(np.int16))
    with mjpeg_avi.MjpegAviWriter(path, 32, 30.0, wavs=[wav], **size) as writer:
        for k in range(5):
            writer.add_frame(bytes([0xFF, 0xD8]) + bytes([k]) * (10 + k) + bytes([0xFF, 0xD9]))
    return path.read_bytes()


SIDE_ONLY_SHA256 = "713bad7d78e63dc0cc9555cc9d388b0984490aa49ffd26da71de48a46da7ad88"


def test_avi_side_only_is_byte_identical_to_the_writer_before_width_and_height(tmp_path: Path) -> None:
    blob = tiny_avi(tmp_path / "square.avi", tmp_path)
    assert len(blob) == 17196 and hashlib.sha256(blob).hexdigest() == SIDE_ONLY_SHA256


def test_avi_headers_carry_width_and_height(tmp_path: Path) -> None:
    blob = tiny_avi(tmp_path / "wide.avi", tmp_path, width=96, height=32)
    avih = blob.index(b"avih") + 8
    assert struct.unpack_from("<II", blob, avih + 32) == (96, 32)
    strf = blob.index(b"strf") + 8
    size, width, height, _planes, bits, codec, image_bytes = struct.unpack_from("<IiiHH4sI", blob, strf)
    assert (size, width, height, bits, codec, image_bytes) == (40, 96, 32, 24, b"MJPG", 96 * 32 * 3)
    strh = blob.index(b"strh") + 8
    assert struct.unpack_from("<hhhh", blob, strh + 48) == (0, 0, 96, 32)  # rcFrame
    square = tiny_avi(tmp_path / "square.avi", tmp_path)
    assert len(square) == len(blob)  # only header fields differ
    tall = tiny_avi(tmp_path / "tall.avi", tmp_path, height=64)  # width defaults to side
    assert struct.unpack_from("<II", tall, tall.index(b"avih") + 8 + 32) == (32, 64)


# ---- 3. mark tables ------------------------------------------------------------------------------------------------------
def synthetic_visualization_input(num_frames: int, length: int = 8) -> VisualizationInput:
    rs = np.random.RandomState(4)
    a = rs.uniform(-3, 7, num_frames * length)
    b = rs.uniform(-2, 2, (18, num_frames * length)).astype(np.float32)
    combined = rs.uniform(-9, 5, (18, num_frames * length))
    indices = (np.arange(num_frames) // 3) % 3
    return VisualizationInput(
        VectorsLabel(a, length, "Rolled Audio Spectrogram"), MatricesLabel(b, length, "proj"), MatricesLabel(combined, length, "Combined"),
        ResultLayers(DataLabel(indices, "Quantized"), [DataLabel(indices + 0.25, "Smoothed")]),
    )


def test_synthesis_panel_windows_cursor_and_limits() -> None:
    visualization_input = synthetic_visualization_input(23)
    panel = panels.SynthesisPanel.from_visualization_input(96, visualization_input, 8, None)
    assert panel.width == 5 == int(np.ceil(23 / 5)) and panel.padded == 25  # ceil(N / 5), padded to whole windows
    assert panels.SynthesisPanel.from_visualization_input(96, visualization_input, 8, 7).width == 7
    assert [panel.window_of(f) for f in (0, 4, 5, 22)] == [0, 0, 1, 4] and [panel.cursor(f) for f in (0, 4, 5, 22)] == [0.0, 4.0, 0.0, 2.0]
    series = panel.host_series()
    assert series["indices"].dtype == np.int32 and series["indices"].shape == (25,) and (series["indices"][23:] == 0).all()
    assert series["layer0"].dtype == np.float64 and series["layer0"][22] == visualization_input.network_indices.layers[0].data[22]
    window = panel.window(4)
    assert (window.first_frame, window.num_frames) == (20, 3)
    a_axis, b_axis, c_axis, context_axis, index_axis, bar_axis = window.axes
    # six stacked axes in the 2:2:2:2:1:1 split, top to bottom, none overlapping
    bottoms = [axis.y + axis.height for axis in window.axes]
    assert all(axis.y >= bottom for axis, bottom in zip(window.axes[1:], bottoms))
    assert panels.SynthesisPanel.ROW_SPANS == ((0, 2), (2, 4), (4, 6), (6, 8), (8, 9), (9, 10))
    for axis, (first_row, last_row) in zip(window.axes, panels.SynthesisPanel.ROW_SPANS):  # each inside its rows of the 10-row grid
        assert first_row * 96 // 10 <= axis.y and axis.y + axis.height <= last_row * 96 // 10
    for axis, data in ((a_axis, visualization_input.a_vectors.data), (b_axis, visualization_input.b_vectors.data), (c_axis, visualization_input.combined.data)):
        assert axis.x_limits == (0.0, 8.0) and axis.y_limits == (float(data.min()), float(data.max()))
    assert [axis.title for axis in window.axes[:3]] == ["Input A", "Input B", "Combined Inputs"]
    assert context_axis.title == "Composition of network index selection: Quantized" and bar_axis.title == "network Index"
    assert context_axis.y_limits == (0.25, 2.25) and index_axis.y_limits == (0.0, 2.0) and bar_axis.x_limits == (0.0, 2.0)
    assert context_axis.x_limits == index_axis.x_limits == (0.0, 4.0)
    by_axis = {axis: [mark for mark in window.marks if mark.axis == axis] for axis in range(6)}
    for axis, (name, colour) in enumerate((("a", chrome.RED), ("b", chrome.GREEN), ("combined", chrome.BLUE))):
        (mark,) = by_axis[axis]
        assert (mark.kind, mark.series, mark.colour, mark.count, mark.frame_stride, mark.alpha) == (panels.POINTS, name, colour, 8, 8, 255)
    line, cursor = by_axis[3]
    assert (line.kind, line.series, line.offset, line.count, line.alpha) == (panels.POLYLINE, "layer0", 20, 5, 128)
    assert (cursor.kind, cursor.colour) == (panels.CURSOR, chrome.RED)
    points, cursor = by_axis[4]
    assert (points.kind, points.series, points.offset, points.count, points.colour) == (panels.POINTS, "indices", 20, 5, chrome.CYAN)
    assert cursor.kind == panels.CURSOR
    (bar,) = by_axis[5]
    assert (bar.kind, bar.series, bar.frame_stride, bar.count, bar.colour) == (panels.BAR, "indices", 1, 1, chrome.MAGENTA)
    assert window.chrome(96).shape == (96, 96, 3)
    # a projected row per `frame_multiplier` frames, and the matrices' row 0 at their own stride
    doubled = panels.SynthesisPanel(96, 8, panel.limits, panel.labels, visualization_input.network_indices, 6, frame_multiplier=2, combined_stride=18 * 8)
    marks = doubled.window(0).marks
    assert marks[1].frame_divisor == 2 and marks[2].frame_stride == 144 and marks[0].frame_divisor == 1
    # one network only: the index axes still get limits that can be mapped
    flat = ResultLayers(DataLabel(np.zeros(10, dtype=int), "Q"), [DataLabel(np.zeros(10), "S")])
    axes = panels.SynthesisPanel(64, 8, panel.limits, panel.labels, flat, None).window(0).axes
    assert axes[4].y_limits == (0.0, 1.0) and axes[5].x_limits == (0.0, 1.0)


def test_overlay_panel_limits_cursor_flags_and_the_empty_window() -> None:
    panel = panels.OverlayPanel(96, 4, phash_distance=10, bbox_distance=50.0)
    contexts = [
        OverlayContext(True, None, 6, 12.5), OverlayContext(False, None, 31, 80.0), OverlayContext(), OverlayContext(False, None, 0, None),
    ]
    window, series = panel.window(2, contexts)
    assert (window.first_frame, window.num_frames) == (8, 4) and panel.window_of(9) == 2 and panel.cursor(9) == 1.0
    assert np.array_equal(series["bbox_phash"], [6, 31, np.nan, 0], equal_nan=True) and np.isnan(series["image_phash"]).all()
    hash_axis, box_axis = window.axes
    assert hash_axis.y_limits == (1.0, 36.0)  # min - 5 .. max + 5 without None and 0, as filter(None, ...) leaves them out
    assert box_axis.y_limits == (7.5, 85.0) and hash_axis.x_limits == (0.0, 3.0)
    assert hash_axis.hlines == ((10.0, chrome.PURPLE),) and box_axis.hlines == ((50.0, chrome.PURPLE),)
    assert hash_axis.title == "Overlay Discriminator (Image Hashing)" and box_axis.title == "Overlay Discriminator (Face Tracking)"
    points = [(mark.axis, mark.series, mark.colour) for mark in window.marks if mark.kind == panels.POINTS]
    assert points == [(0, "bbox_phash", chrome.RED), (0, "image_phash", chrome.BLUE), (1, "bbox_distance", chrome.GREEN)]
    cursors = [(mark.axis, mark.colour, mark.flag_mask, mark.flag_value) for mark in window.marks if mark.kind == panels.CURSOR]
    assert cursors == [(0, chrome.GREEN, 1, 1), (0, chrome.RED, 1, 0), (1, chrome.GREEN, 1, 1), (1, chrome.RED, 1, 0)]
    empty, _ = panel.window(0, [OverlayContext(), OverlayContext()])
    assert empty.axes[0].y_limits == (-5.0, 5.0) and empty.axes[1].y_limits == (-5.0, 5.0) and empty.num_frames == 2
    assert panels.overlay_limits([np.array([0.0, np.nan])]) == (-5.0, 5.0)
    with pytest.raises(ValueError, match="debug_window"):
        panels.OverlayPanel(96, None, 10, 50.0)


def test_mask_panel_windows_and_limits() -> None:
    result = np.array([np.nan, np.nan, 4.0, 9.0, 2.0, 30.0, 1.0])
    layers = ResultLayers(DataLabel(result, "rolling sum"), [DataLabel(result - 1.0, "absolute value")])
    panel = panels.MaskPanel(96, layers, 3, threshold=12)
    first, second, last = panel.window(0), panel.window(1), panel.window(2)
    assert (first.num_frames, second.num_frames, last.num_frames) == (3, 3, 1) and last.first_frame == 6
    assert first.axes[0].y_limits == (3.0 - 10.0, 4.0 + 10.0)  # the non-NaN values of result and layers
    assert second.axes[0].y_limits == (1.0 - 10.0, 30.0 + 10.0) and second.axes[0].hlines == ((12.0, chrome.PURPLE),)
    assert first.axes[0].title == "Overlay binary mask" and panel.cursor(7) == 1.0
    line, dashed, cursor = second.marks
    assert (line.kind, line.series, line.offset, line.count, line.colour, line.alpha, line.dash) == (panels.POLYLINE, "result", 3, 3, chrome.RED, 255, (0, 0))
    assert (dashed.series, dashed.alpha) == ("layer0", 128) and dashed.dash[0] > 0 and line.size > dashed.size >= cursor.size
    assert (cursor.kind, cursor.colour) == (panels.CURSOR, chrome.RED)
    all_nan = panels.MaskPanel(96, ResultLayers(DataLabel(np.full(4, np.nan), "r")), 4, None)
    assert all_nan.window(0).axes[0].y_limits == (-10.0, 10.0) and all_nan.window(0).axes[0].hlines == ()


# ---- 4. the new C entries refuse bad arguments before touching a device ----------------------------------------------------
@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


INVALID = 1  # GANCE_ERR_INVALID_ARGUMENT
FAKE = 0x10000  # a non-NULL, 16-byte aligned "device pointer": every call below must return before it is looked at


def test_rect_encode_rejects_bad_sizes_and_an_undersized_workspace(library: ctypes.CDLL) -> None:
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    assert library.gance_jpeg_encode_rect_bounds(1, 40, 32, ctypes.byref(workspace), ctypes.byref(capacity)) == INVALID
    assert b"40 x 32" in library.gance_last_error()
    assert library.gance_jpeg_encode_rect_bounds(1, 32, 0, ctypes.byref(workspace), ctypes.byref(capacity)) == INVALID
    assert library.gance_jpeg_encode_rect_bounds(0, 32, 32, ctypes.byref(workspace), ctypes.byref(capacity)) == INVALID
    assert library.gance_jpeg_encode_rect_bounds(1, 32, 32, None, ctypes.byref(capacity)) == INVALID
    assert library.gance_jpeg_encode_rect_bounds(2, 96, 32, ctypes.byref(workspace), ctypes.byref(capacity)) == 0
    square = hip_lib.jpeg_encode_bounds(2, 48)
    assert hip_lib.jpeg_encode_rect_bounds(2, 48, 48) == square  # the square entry is the rect entry with width = height
    assert hip_lib.jpeg_encode_rect_bounds(2, 96, 32)[0] != hip_lib.jpeg_encode_rect_bounds(2, 32, 96)[0]
    encode = library.gance_jpeg_encode_rect_u8
    assert encode(FAKE, 2, 40, 32, 90, FAKE, workspace.value, FAKE, capacity.value, FAKE, None) == INVALID
    assert encode(FAKE, 2, 96, 0, 90, FAKE, workspace.value, FAKE, capacity.value, FAKE, None) == INVALID
    assert encode(FAKE, 2, 96, 32, 90, FAKE, workspace.value - 1, FAKE, capacity.value, FAKE, None) == INVALID
    assert b"workspace" in library.gance_last_error()
    assert encode(FAKE, 2, 96, 32, 90, FAKE, workspace.value, FAKE, capacity.value - 1, FAKE, None) == INVALID
    assert encode(FAKE, 2, 96, 32, 101, FAKE, workspace.value, FAKE, capacity.value, FAKE, None) == INVALID
    assert encode(None, 2, 96, 32, 90, FAKE, workspace.value, FAKE, capacity.value, FAKE, None) == INVALID
    with pytest.raises(ValueError):
        hip_lib.jpeg_encode_rect_bounds(1, 40, 32)


def one_axis(**changes) -> hip_lib.DebugAxis:
    values = dict(x=2, y=2, width=20, height=20, x_min=0.0, x_max=1.0, y_min=0.0, y_max=1.0)
    values.update(changes)
    return hip_lib.DebugAxis(**values)


def one_mark(**changes) -> hip_lib.DebugMark:
    mark = hip_lib.DebugMark()
    mark.kind, mark.axis, mark.dtype, mark.count, mark.data, mark.limit = hip_lib.DEBUG_MARK_POINTS, 0, 0, 4, FAKE, 4
    mark.frame_divisor, mark.size = 1, 1
    for name, value in changes.items():
        setattr(mark, name, value)
    return mark


def test_draw_panels_rejects_missing_and_bad_tables(library: ctypes.CDLL) -> None:
    def draw(axes, marks, side=32, chrome_pointer=FAKE, frames=FAKE, out=FAKE, frame_stride=32 * 96, row_stride=96, batch=1):
        hip_lib.debug_draw_panels_device(chrome_pointer, side, axes, marks, frames, batch, out, frame_stride, row_stride, 0)

    good_axes, good_marks = [one_axis()], [one_mark()]
    for arguments in (
        dict(axes=None, marks=good_marks),                                    # a NULL axis table
        dict(axes=good_axes, marks=None),                                     # a NULL mark table
        dict(axes=good_axes, marks=good_marks, chrome_pointer=0),
        dict(axes=good_axes, marks=good_marks, frames=0),
        dict(axes=good_axes, marks=good_marks, out=0),
        dict(axes=good_axes, marks=good_marks, side=40),
        dict(axes=good_axes, marks=good_marks, row_stride=90),                # not 16-byte aligned
        dict(axes=good_axes, marks=good_marks, row_stride=80),                # narrower than the panel
        dict(axes=good_axes, marks=good_marks, batch=0),
        dict(axes=[one_axis(width=31)], marks=good_marks),                    # leaves the panel
        dict(axes=[one_axis(x_max=0.0)], marks=good_marks),                   # limits that cannot be mapped
        dict(axes=[one_axis(y_max=float("nan"))], marks=good_marks),
        dict(axes=[one_axis(), one_axis(x=10, y=10, width=5, height=5)], marks=good_marks),  # overlapping axes
        dict(axes=[one_axis()] * 0, marks=good_marks),
        dict(axes=good_axes, marks=[one_mark(axis=1)]),
        dict(axes=good_axes, marks=[one_mark(kind=7)]),
        dict(axes=good_axes, marks=[one_mark(dtype=3)]),
        dict(axes=good_axes, marks=[one_mark(size=0)]),
        dict(axes=good_axes, marks=[one_mark(data=None)]),
        dict(axes=good_axes, marks=[one_mark(frame_divisor=0)]),
        dict(axes=good_axes, marks=[one_mark()] * (hip_lib.DEBUG_MAX_MARKS + 1)),
    ):
        with pytest.raises(ValueError):
            draw(**arguments)
    assert library.gance_debug_draw_panels_u8(FAKE, 32, None, 1, None, 0, FAKE, 1, FAKE, 32 * 96, 96, None) == INVALID
    assert b"NULL" in library.gance_last_error()


def test_place_panels_rejects_sources_out_of_range(library: ctypes.CDLL) -> None:
    place = library.gance_debug_place_panels_u8
    assert place(FAKE, 4, 32, 0, 1, 0, 5, FAKE, 32 * 96, 96, None) == INVALID  # frame 4 reads source 4 of 4
    assert place(FAKE, 4, 32, 2, 2, 2, 2, FAKE, 32 * 96, 96, None) == INVALID  # source -1
    assert place(None, 4, 32, 0, 1, 0, 4, FAKE, 32 * 96, 96, None) == INVALID
    assert place(FAKE, 4, 32, 0, 0, 0, 4, FAKE, 32 * 96, 96, None) == INVALID
    assert place(FAKE, 4, 48, 0, 1, 0, 4, FAKE + 8, 48 * 144, 144, None) == INVALID
