"""
CPU tests of what the projection-file analysis videos stand on: the latent histories of ProjectionFileReader (HDF5
through h5py or hdf5_lite, and the .npz container), the reference's one-shot helpers, projection_convergence, the font
table the library exports, the argument checks of gance_debug_draw_text_u8 (which run before any device is touched), and
the latents panel's host tables. The fixture is a real h5py-written file (tests/dev/make_projection_history_fixture.py).
"""

import ctypes
from pathlib import Path

import numpy as np
import pytest

from gance_amd import hip_lib
from gance_amd.debug_video import chrome, font, latents_panel, panels
from gance_amd.projection import projection_file_reader as pfr
from gance_amd.projection import projection_visualization

STEPS = (11, 3, 3)
LABEL = "history clip.mp4 proj by network-snapshot-000064.pkl"


@pytest.fixture(scope="module")
def expected(golden_dir: Path):
    return np.load(golden_dir / "projection_histories_expected.npz")


@pytest.fixture(scope="module")
def hdf5_path(golden_dir: Path) -> Path:
    return golden_dir / "projection_histories.hdf5"


@pytest.fixture(scope="module")
def npz_path(tmp_path_factory, expected) -> Path:
    path = tmp_path_factory.mktemp("histories") / "projection.npz"
    pfr.write_projection_npz(
        path, expected["final_latents"], 7.5, target_images=expected["target_images"], final_images=expected["final_images"],
        original_target_path="/videos/history clip.mp4", original_network_path="/networks/network-snapshot-000064.pkl",
        latents_histories=[expected[f"history_{frame}"] for frame in range(len(STEPS))],
    )
    return path


def check_histories(path: Path, expected) -> None:
    with pfr.load_projection_file(path) as reader:
        assert reader.projection_attributes.latents_histories_enabled is True
        histories = [list(history) for history in reader.latents_histories]
        finals = list(reader.final_latents)
    assert [len(history) for history in histories] == list(STEPS)
    for frame, history in enumerate(histories):
        assert all(matrix.shape == (18, 512) and matrix.dtype == np.float32 for matrix in history)
        assert np.array_equal(np.stack(history), expected[f"history_{frame}"])  # step 10 is the last of frame 0, not the third
        assert np.array_equal(history[-1], finals[frame])
    assert not np.array_equal(histories[0][2], histories[0][10])


def test_histories_of_a_real_hdf5_file_come_in_step_order(hdf5_path: Path, expected) -> None:
    check_histories(hdf5_path, expected)


def test_histories_through_hdf5_lite(hdf5_path: Path, expected) -> None:
    """The pure-Python reader, whether or not this interpreter has h5py: nested groups, keys sorted by trailing integer."""
    from gance_amd.projection import hdf5_lite  # pylint: disable=import-outside-toplevel

    with hdf5_lite.File(hdf5_path) as file:
        group = file["latents_histories"]
        assert sorted(group.keys(), key=pfr._trailing_int) == [f"latents_histories_{frame}" for frame in range(3)]  # pylint: disable=protected-access
        steps = group["latents_histories_0"]
        names = sorted(steps.keys(), key=pfr._trailing_int)  # pylint: disable=protected-access
        assert names[2] == "latents_histories_0_step_2" and names[-1] == "latents_histories_0_step_10"
        got = np.stack([np.array(steps[name])[0] for name in names])
        assert np.array_equal(got, expected["history_0"])
        assert np.array(steps[names[0]]).shape == (1, 18, 512)
    file.close()  # (twice is fine)


def test_histories_of_the_npz_container(npz_path: Path, expected) -> None:
    check_histories(npz_path, expected)


def test_npz_without_histories_is_what_it_was(tmp_path: Path, expected) -> None:
    pfr.write_projection_npz(tmp_path / "plain.npz", expected["final_latents"], 7.5)
    with np.load(tmp_path / "plain.npz") as plain:
        assert sorted(plain.files) == ["attributes", "final_latents"]
        assert "latents_histories_enabled" not in str(plain["attributes"])
    with pfr.load_projection_file(tmp_path / "plain.npz") as reader:
        assert list(reader.latents_histories) == [] and reader.projection_attributes.latents_histories_enabled is False


def test_existing_fixture_has_no_histories(golden_dir: Path) -> None:
    with pfr.load_projection_file(golden_dir / "projection_v2.hdf5") as reader:
        assert list(reader.latents_histories) == []


@pytest.mark.parametrize("container", ["hdf5", "npz"])
def test_step_labels_stop_at_the_first_short_history(container: str, hdf5_path: Path, npz_path: Path, expected) -> None:
    path = hdf5_path if container == "hdf5" else npz_path
    with pfr.load_projection_file(path) as reader:
        at_two = pfr.projection_history_step_matrices_label(reader, 2)
        at_five = pfr.projection_history_step_matrices_label(reader, 5)
        with pytest.raises(StopIteration):
            pfr.projection_history_step_matrices_label(reader, 11)
    assert at_two.data.shape == (18, 3 * 512) and at_two.vector_length == 512 and at_two.label == LABEL + " step 2"
    assert np.array_equal(at_two.data, np.concatenate([expected[f"history_{frame}"][2] for frame in range(3)], axis=-1))
    assert at_five.data.shape == (18, 512) and at_five.label == LABEL + " step 5"  # frame 1 has three steps: it stops there
    assert np.array_equal(at_five.data, expected["history_0"][5])


def test_one_shot_helpers(hdf5_path: Path, expected) -> None:
    class Network:  # pylint: disable=too-few-public-methods
        @staticmethod
        def create_image_matrix(matrix: np.ndarray) -> np.ndarray:
            return np.full((2, 2, 3), int(abs(float(matrix[0, 0])) * 32) % 256, dtype=np.uint8)

    assert np.array_equal(pfr.final_latents_at_frame(hdf5_path, 1), expected["final_latents"][1])
    assert np.array_equal(np.stack(list(pfr.final_images(hdf5_path))), expected["final_images"])
    assert np.array_equal(np.stack(list(pfr.target_images(hdf5_path))), expected["target_images"])
    attributes = pfr.projection_attributes(hdf5_path)
    assert attributes.network_md5_hash == "00112233445566778899aabbccddeeff" and attributes.projection_fps == 7.5
    at_step = list(pfr.network_outputs_at_projection_step(hdf5_path, Network, 1))
    assert [int(image[0, 0, 0]) for image in at_step] == [int(abs(float(expected[f"history_{f}"][1, 0, 0])) * 32) % 256 for f in range(3)]
    assert len(list(pfr.network_outputs_at_projection_step(hdf5_path, Network, 5))) == 1
    at_final = list(pfr.network_outputs_at_final_latents(hdf5_path, Network))
    assert [int(image[0, 0, 0]) for image in at_final] == [int(abs(float(expected["final_latents"][f, 0, 0])) * 32) % 256 for f in range(3)]


def test_projection_convergence_is_the_references_arithmetic(hdf5_path: Path, golden_dir: Path, expected) -> None:
    got = projection_visualization.projection_convergence(hdf5_path)
    lines = [
        np.array([np.sum(abs(expected["final_latents"][frame] - latent)) for latent in expected[f"history_{frame}"]]) for frame in range(3)
    ]
    points = [np.where(line <= (line.max() - line.min()) * 0.2)[0][0] for line in lines]
    assert len(got.lines) == 3 and all(np.array_equal(a, b) for a, b in zip(got.lines, lines))
    assert got.points_of_interest == [int(point) for point in points]
    assert (got.average, got.standard_deviation) == (int(np.mean(points)), int(np.std(points)))
    assert all(line[-1] == 0 and line[0] == line.max() for line in got.lines) and 0 < got.points_of_interest[0] < 10
    first = projection_visualization.projection_convergence(hdf5_path, consider_first_n_frames=1)
    assert len(first.lines) == 1 and first.average == got.points_of_interest[0] and first.standard_deviation == 0
    with pytest.raises(ValueError, match="File doesn't contain the data to visualize."):
        projection_visualization.projection_convergence(golden_dir / "projection_v2.hdf5")


# ---- the font and the text entry --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


def test_the_librarys_font_is_the_hosts(library: ctypes.CDLL) -> None:
    assert hip_lib.debug_font_columns() == font._COLUMNS  # pylint: disable=protected-access
    table = (ctypes.c_uint8 * 475)()
    assert library.gance_debug_font_columns(table, 474) == INVALID and library.gance_debug_font_columns(None, 475) == INVALID


INVALID = 1  # GANCE_ERR_INVALID_ARGUMENT
FAKE = 0x10000  # a non-NULL, 16-byte aligned "device pointer": every call below must return before it is looked at

TEXT_REFUSALS = [
    dict(text=None), dict(out=None),                                                                       # NULL
    dict(side=0), dict(side=24), dict(side=8), dict(side=4112),                                            # side
    dict(out=FAKE + 8), dict(row_stride=200), dict(frame_stride=32 * 192 + 8),                             # alignment
    dict(row_stride=80), dict(frame_stride=1024), dict(frame_stride=31 * 192 + 80),                        # strides smaller than a panel
    dict(text_stride=0), dict(text_stride=257), dict(text_stride=-4),
    dict(scale=0), dict(scale=65),
    dict(max_width=0), dict(max_width=-5),
    dict(x=-1), dict(x=32), dict(y=-1), dict(y=32),
    dict(batch=0), dict(batch=-2),
]


def call_text(library: ctypes.CDLL, **changes) -> int:
    a = dict(text=FAKE + 3, text_stride=24, x=2, y=0, max_width=20, scale=1, rgb=0, side=32, batch=2, out=FAKE, frame_stride=32 * 192, row_stride=192)
    a.update(changes)
    return library.gance_debug_draw_text_u8(
        a["text"], a["text_stride"], a["x"], a["y"], a["max_width"], a["scale"], a["rgb"], a["side"], a["batch"], a["out"], a["frame_stride"],
        a["row_stride"], None,
    )


@pytest.mark.parametrize("changes", TEXT_REFUSALS, ids=lambda changes: ",".join(f"{k}={v}" for k, v in changes.items()))
def test_draw_text_refuses(library: ctypes.CDLL, changes: dict) -> None:
    assert call_text(library, **changes) == INVALID
    assert b"gance_debug_draw_text_u8" in library.gance_last_error()


def test_draw_text_refusals_reach_python_as_value_errors() -> None:
    with pytest.raises(ValueError, match="scale"):
        hip_lib.debug_draw_text_device(FAKE, 8, 0, 0, 10, 65, (0, 0, 0), 32, 1, FAKE, 32 * 96, 96)
    with pytest.raises(ValueError, match="NULL"):
        hip_lib.debug_draw_text_device(0, 8, 0, 0, 10, 1, (0, 0, 0), 32, 1, FAKE, 32 * 96, 96)


# ---- the latents panel's host tables ------------------------------------------------------------------------------------------
def test_latents_panel_tables() -> None:
    panel = latents_panel.LatentsPanel(64, 512, 18, -2.5, 3.25, "a title")
    window = panel.window()
    (axis,) = window.axes
    assert (axis.x, axis.y, axis.width, axis.height, axis.titled) == chrome.stacked_rectangles(64, [(0, 1)], 1)[0]
    assert axis.x_limits == (0.0, 512.0) and axis.y_limits == (-3.5, 4.25) and axis.title == "a title"
    assert len(window.marks) == 18
    for row, mark in enumerate(window.marks):
        assert (mark.kind, mark.axis, mark.series, mark.count, mark.offset, mark.frame_stride) == (panels.POINTS, 0, "latents", 512, row * 512, 18 * 512)
        assert mark.size == panels.point_size(64) and mark.alpha == panels.OPAQUE and mark.colour == latents_panel.ROW_COLOURS[row]
    assert window.marks[7].colour == (255, 255, 255)  # row 7 is white, as in the reference
    assert latents_panel.LatentsPanel(64, 33, 1, 0.0, 1.0, None).window().axes[0].title == ""
    assert latents_panel.LatentsPanel(96, 8, 20, 0.0, 1.0, "t").colours[18:] == latents_panel.ROW_COLOURS[:2]  # the cycle starts over
    with pytest.raises(ValueError, match="at most 24 rows"):
        latents_panel.LatentsPanel(64, 512, 25, 0.0, 1.0, "t")


def test_per_frame_title_box_keeps_clear_of_the_limits_label() -> None:
    for side in (32, 64, 96, 1024):
        panel = latents_panel.LatentsPanel(side, 512, 18, -2.5, 3.25, None)
        axis = panel.window().axes[0]
        x, y, room, scale = panel.title_box()
        assert (x, y, scale) == (axis.x, axis.y - chrome.title_height(side), font.scale_for_side(side))
        image = chrome.render_chrome(side, [axis])
        line = image[y : y + font.GLYPH_HEIGHT * scale]
        inked = np.nonzero((line != 255).any(axis=(0, 2)))[0]
        inked = inked[inked > axis.x]  # (the box's corner pixel aside)
        if inked.size and inked[0] < axis.x + axis.width - 1:  # the limits label was drawn: the title ends one advance before it
            assert x + room + font.ADVANCE * scale == inked[0]
        else:
            assert room == axis.width
    assert latents_panel.LatentsPanel(16, 4, 1, 0.0, 1.0, None).title_box() is None  # no title line at this side


def test_row_colours_are_matplotlibs() -> None:
    assert len(latents_panel.ROW_COLOURS) == 18 and latents_panel.ROW_COLOURS[:7] == chrome.BASE_COLOURS
    colors = pytest.importorskip("matplotlib.colors")
    names = list(colors.BASE_COLORS.keys()) + list(colors.TABLEAU_COLORS.keys())
    want = tuple(tuple(int(np.floor(255 * channel + 1e-6)) for channel in colors.to_rgb(name)) for name in names)
    assert latents_panel.ROW_COLOURS == want


def test_encode_titles() -> None:
    encoded = latents_panel.encode_titles(["ab", "", "café x"])
    assert encoded.shape == (3, 7) and encoded.dtype == np.uint8
    assert bytes(encoded[0]) == b"ab\0\0\0\0\0" and bytes(encoded[2]) == b"caf? x\0"
    assert latents_panel.encode_titles(["x" * 300]).shape == (1, 256)


def test_per_frame_titles_keep_what_changes() -> None:
    """fit_title cuts the label, never the frame and step; title_glyphs counts whole glyphs of (6 n - 1) * scale columns."""
    assert [latents_panel.title_glyphs(room, 1) for room in (4, 5, 10, 11, 28, 60)] == [0, 1, 1, 2, 4, 10]
    assert latents_panel.title_glyphs(711, 3) == 39 and latents_panel.title_glyphs(33, 3) == 2 and latents_panel.title_glyphs(32, 3) == 1
    label, tail = "clip.mp4 proj by net.pkl", " frame: 3, step: 417"
    assert latents_panel.fit_title(label, tail, "3:417", 44) == label + tail
    assert latents_panel.fit_title(label, tail, "3:417", 43) == "clip.mp4 proj by net." + ".." + tail
    assert latents_panel.fit_title(label, tail, "3:417", 23) == "c.." + tail
    assert latents_panel.fit_title(label, tail, "3:417", 22) == "frame: 3, step: 417"
    assert latents_panel.fit_title(label, tail, "3:417", 19) == "frame: 3, step: 417"
    assert latents_panel.fit_title(label, tail, "3:417", 18) == "3:417" and latents_panel.fit_title(label, tail, "3:417", 2) == "3:417"
    for glyphs in range(5, 60):  # whatever the room, the step is on the line
        assert latents_panel.fit_title(label, tail, "3:417", glyphs).endswith("417")
        assert len(latents_panel.fit_title(label, tail, "3:417", glyphs)) <= glyphs
