"""
Host-side tests of the noise-blend command (no GPU): `noise_blend_api` refuses bad arguments before the library or a
device is touched, the synthesis-inputs panel built from this command's sources reads its series the way the reference
plots them (visualization_inputs.py:153-166: a noise row per OUTPUT frame, the z vectors as the combined series), and the
composer's panel arithmetic with and without the final-images panel.
"""

from pathlib import Path

import numpy as np
import pytest
import torch

from gance_amd import noise_blend, projection_file_blend
from gance_amd.debug_video import chrome, compose


def refuse_everything(monkeypatch) -> None:
    """Neither a network nor the library nor a device may be touched by a call that is refused for its arguments."""

    def touched(*_args, **_kwargs):
        raise AssertionError("the arguments were not checked before the device was touched")

    monkeypatch.setattr(projection_file_blend, "MultiNetwork", touched)
    monkeypatch.setattr(noise_blend, "MultiNetwork", touched)
    monkeypatch.setattr(projection_file_blend.hip_lib, "load_library", touched)
    monkeypatch.setattr(torch.cuda, "current_device", touched)


def api_arguments(tmp_path: Path, **changes):
    """Positional arguments of noise_blend_api in the reference's order, and its keywords."""
    values = dict(
        wav=[str(tmp_path / "missing.wav")], output_path=str(tmp_path / "out"), network_paths=[tmp_path / "missing.pkl"], frames_to_visualize=None,
        output_fps=30.0, output_side_length=64, debug_path=None, debug_window=None, debug_side_length=None, alpha=0.25,
        fft_roll_enabled=True, fft_amplitude_range=(-5, 5),
    )
    keywords = {key: changes.pop(key) for key in ("output_format", "jpeg_quality", "noise_seed", "drain") if key in changes}
    values.update(changes)
    return list(values.values()), keywords


@pytest.mark.parametrize(
    "changes,message",
    [
        (dict(output_format="mp4"), "output_format must be"),
        (dict(output_format="avi", output_side_length=100), "the Motion-JPEG writer needs an output side that is a multiple of 16"),
        (dict(output_format="avi", jpeg_quality=0), "jpeg_quality must be in"),
        (dict(output_format="avi", jpeg_quality=101), "jpeg_quality must be in"),
        (dict(debug_path="debug.avi", debug_side_length=None), "debug_path needs debug_side_length"),
        (dict(debug_path="debug.avi", debug_side_length=100), "debug_side_length must be a multiple of 16"),
        (dict(debug_path="debug.avi", debug_side_length=96, jpeg_quality=0), "jpeg_quality must be in"),
        (dict(output_format="avi", output_fps=0.0), None),
        (dict(output_format="avi", output_fps=-24.0), None),
        (dict(debug_path="debug.avi", debug_side_length=96, output_fps=0.0), None),
    ],
)
def test_bad_arguments_are_refused_before_anything_is_touched(tmp_path: Path, monkeypatch, changes: dict, message) -> None:
    refuse_everything(monkeypatch)
    if "debug_path" in changes:
        changes = dict(changes, debug_path=str(tmp_path / changes["debug_path"]))
    arguments, keywords = api_arguments(tmp_path, **changes)
    with pytest.raises(ValueError, match=message):
        noise_blend.noise_blend_api(*arguments, **keywords)
    assert list(tmp_path.iterdir()) == []  # no output, no debug video, not even an empty one


def test_the_messages_are_the_projection_commands(tmp_path: Path, monkeypatch) -> None:
    """The same mistake, the same words from both commands."""
    refuse_everything(monkeypatch)
    cases = [
        dict(output_format="gif"), dict(output_format="avi", output_side_length=72), dict(output_format="avi", jpeg_quality=200),
        dict(debug_path=str(tmp_path / "d.avi")), dict(debug_path=str(tmp_path / "d.avi"), debug_side_length=8),
        dict(output_format="avi", output_fps=0.0),
    ]
    for changes in cases:
        arguments, keywords = api_arguments(tmp_path, **dict(changes))
        keywords.pop("noise_seed", None)
        with pytest.raises(ValueError) as ours:
            noise_blend.noise_blend_api(*arguments, **keywords)
        projection_arguments = arguments + ["missing.npz", 12, None, None, None, None, None]
        with pytest.raises(ValueError) as theirs:
            projection_file_blend.projection_file_blend_api(*projection_arguments, **keywords)
        assert str(ours.value) == str(theirs.value), changes
    assert list(tmp_path.iterdir()) == []


def noise_sources(num_frames: int, length: int, frames_to_visualize=None, alpha: float = 0.25):
    rs = np.random.RandomState(11)
    spectrogram = rs.uniform(-3, 7, (num_frames, length))
    noise = torch.from_numpy(rs.uniform(-4, 4, (num_frames, length)).astype(np.float32))
    vectors = torch.from_numpy((alpha * spectrogram + (1 - alpha) * noise.numpy()).astype(np.float32))
    indices = ((np.arange(num_frames) // 3) % 2).astype(np.int32)
    sources = noise_blend.noise_debug_sources(
        spectrogram, noise, vectors, indices, indices + 0.25, frames_to_visualize, alpha, torch.device("cpu")
    )
    return sources, spectrogram, noise, vectors


def test_synthesis_panel_of_this_command() -> None:
    length, num_frames = 8, 23
    sources, spectrogram, noise, vectors = noise_sources(num_frames, length)
    assert sources.final_images is None
    assert sources.a_vectors.dtype == torch.float64 and tuple(sources.a_vectors.shape) == (num_frames, length)
    assert sources.b_vectors.dtype == torch.float32 and tuple(sources.b_vectors.shape) == (num_frames, length)  # a row per OUTPUT frame
    panel = compose.synthesis_panel_of(96, None, 1, sources, vectors)
    assert panel.frame_multiplier == 1 and panel.combined_stride == length and panel.width == 5
    window = panel.window(1)
    a_mark, b_mark, combined_mark = window.marks[:3]
    assert (a_mark.series, a_mark.frame_stride, a_mark.frame_divisor, a_mark.count) == ("a", length, 1, length)
    assert (b_mark.series, b_mark.frame_stride, b_mark.frame_divisor, b_mark.count) == ("b", length, 1, length)
    assert (combined_mark.series, combined_mark.frame_stride, combined_mark.frame_divisor, combined_mark.count) == ("combined", length, 1, length)
    # the legend table: the reference's labels for this command, in the series' colours
    assert window.axes[0].legend == (("Audio Spectrogram", chrome.RED),)
    assert window.axes[1].legend == (("Gaussian Smoothed Noise", chrome.GREEN),)
    assert window.axes[2].legend == (("Combined w/ Alpha Blending, a=0.25", chrome.BLUE),)
    assert window.axes[3].legend == (("Savgol Smoothing Filter (window=7, polyorder=3)", chrome.BASE_COLOURS[0]),)
    assert window.axes[3].title == "Composition of network index selection: Savgol Smoothing Filter (window=7, polyorder=3) Scaled, Quantized"
    # limits: each series' global min / max
    for axis, data in zip(window.axes[:3], (spectrogram, noise.numpy(), vectors.numpy())):
        assert axis.y_limits == (float(data.min()), float(data.max())) and axis.x_limits == (0.0, float(length))
    # frames_to_visualize cuts the per-frame series, not the limits (they are the song's)
    cut, _, _, _ = noise_sources(num_frames, length, frames_to_visualize=10)
    assert tuple(cut.a_vectors.shape) == (10, length) and len(cut.network_indices.result.data) == 10 and cut.limits == sources.limits
    assert compose.synthesis_panel_of(96, None, 1, cut, vectors[:10]).width == 2
    # the projection command's strides through the same function: row 0 of [N, 18, L]
    matrices = torch.zeros((num_frames, 18, length))
    doubled = compose.synthesis_panel_of(96, 6, 2, sources, matrices)
    assert doubled.combined_stride == 18 * length and doubled.window(0).marks[1].frame_divisor == 2


def test_panel_arithmetic_with_and_without_final_images() -> None:
    without = compose.panel_layout(final_images=False, overlay=False, mask=False)
    assert without.panel_count == 2 and without.synthesis == 1 and without.final_images is None and without.overlay is None
    side = 96
    assert without.panel_count * side == 2 * side  # the width of a noise-blend debug frame
    # with final images: what the composer and the projection API computed as literals before (3 + 2 + 1; overlay at 3 + 1)
    for overlay, mask in ((False, False), (True, False), (True, True)):
        layout = compose.panel_layout(final_images=True, overlay=overlay, mask=mask)
        assert layout.panel_count == 3 + (2 if overlay else 0) + (1 if mask else 0)
        assert layout.final_images == (2 if overlay else 1) and layout.synthesis == layout.final_images + 1
        assert layout.foreground == (1 if overlay else None)
        assert layout.overlay == (3 + 1 if overlay else None)
        assert layout.mask == (layout.panel_count - 1 if mask else None)
    assert compose.DebugSources._field_defaults == {"final_images": None}
