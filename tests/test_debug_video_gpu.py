"""
GPU tests of the debug video: the rectangular JPEG encode (same bar as tests/test_mjpeg_gpu.py: PIL decodes our files to
the pixels of its own 4:2:2 encode), and `projection_file_blend_api(debug_path=...)` end to end on 64^2 random-init
networks, with and without the overlay, plus the hold-back of composed frames across window and chunk borders.
"""

import io
import struct
from pathlib import Path
from typing import Dict, List

import numpy as np
import pytest
import torch
from PIL import Image
from scipy.io import wavfile

from gance_amd import hip_lib, network_file, projection_file_blend, synthetic, torch_ops  # noqa: F401
from gance_amd.debug_video import chrome, compose, panels
from gance_amd.overlay import overlay_eye_tracking
from gance_amd.projection import projection_file_reader as pfr

pytestmark = pytest.mark.gpu

QUALITIES = (1, 50, 90, 100)


# ---- the rectangular encode ----------------------------------------------------------------------------------------------
def files_of(data: torch.Tensor, offsets: torch.Tensor) -> List[bytes]:
    host = offsets.cpu().numpy()
    blob = data[: int(host[-1])].cpu().numpy().tobytes()
    return [blob[host[i] : host[i + 1]] for i in range(len(host) - 1)]


def rect_contents(width: int, height: int, seed: int) -> np.ndarray:
    """Noise, black, white, a noisy gradient and saturated quadrants of height x width."""
    rs = np.random.RandomState(seed)
    noise = rs.randint(0, 256, (height, width, 3)).astype(np.uint8)
    gradient = np.stack(
        [np.add.outer(np.linspace(0, 255, height), np.linspace(0, 255, width)) / 2, np.tile(np.linspace(255, 0, width), (height, 1)),
         np.tile(np.linspace(0, 255, height)[:, None], (1, width))], -1,
    )
    noisy = np.clip(gradient + rs.randn(height, width, 3) * 12, 0, 255).astype(np.uint8)
    quadrants = np.zeros((height, width, 3), np.uint8)
    quadrants[: height // 2, : width // 2, 0] = 255
    quadrants[: height // 2, width // 2 :, 1] = 255
    quadrants[height // 2 :, : width // 2, 2] = 255
    quadrants[height // 2 :, width // 2 :] = (255, 255, 0)
    return np.stack([noise, np.zeros_like(noise), np.full_like(noise, 255), noisy, quadrants])


def pil_roundtrip(frame: np.ndarray, quality: int) -> Image.Image:
    buffer = io.BytesIO()
    Image.fromarray(frame).save(buffer, format="JPEG", quality=quality, subsampling=1)
    return Image.open(io.BytesIO(buffer.getvalue()))


@pytest.mark.parametrize("width,height", [(96, 32), (32, 96), (480, 80)])
def test_rect_pixels_equal_libjpeg(width: int, height: int) -> None:
    frames = rect_contents(width, height, seed=width + height)
    d_frames = torch.from_numpy(frames).cuda()
    for quality in QUALITIES:
        files = files_of(*torch.ops.gance.jpeg_encode_rect(d_frames, quality))
        for index, (data, frame) in enumerate(zip(files, frames)):
            ours, reference = Image.open(io.BytesIO(data)), pil_roundtrip(frame, quality)
            assert ours.size == (width, height) and ours.mode == "RGB"
            got, want = np.asarray(ours), np.asarray(reference)
            assert np.array_equal(got, want), f"{width}x{height} frame {index} q {quality}: {int(np.abs(got.astype(int) - want).max())} LSB off"
            assert ours.quantization == reference.quantization
        # DRI = width / 16: one restart interval per MCU row
        at = files[0].index(b"\xff\xdd")
        assert struct.unpack_from(">H", files[0], at + 4)[0] == width // 16


def test_rect_op_on_square_frames_gives_the_square_op_bytes() -> None:
    frames = torch.from_numpy(np.concatenate([rect_contents(48, 48, seed=5), rect_contents(48, 48, seed=6)[:2]])).cuda()
    for quality in (35, 90):
        square = files_of(*torch.ops.gance.jpeg_encode(frames, quality))
        assert files_of(*torch.ops.gance.jpeg_encode_rect(frames, quality)) == square
        assert files_of(*torch.ops.gance.jpeg_encode_rect(frames[3:4], quality)) == [square[3]]


def test_rect_torch_op() -> None:
    frames = torch.from_numpy(rect_contents(64, 32, seed=2)).cuda()
    torch.library.opcheck(torch.ops.gance.jpeg_encode_rect.default, (frames, 80), test_utils=("test_schema", "test_faketensor"))
    data, offsets = torch.ops.gance.jpeg_encode_rect(frames, 80)
    assert data.shape == (hip_lib.jpeg_encode_rect_bounds(5, 64, 32)[1],) and offsets.dtype == torch.int64
    with pytest.raises(ValueError):
        torch.ops.gance.jpeg_encode_rect(torch.zeros((1, 32, 40, 3), dtype=torch.uint8, device="cuda"), 80)
    with pytest.raises(ValueError):
        torch.ops.gance.jpeg_encode_rect(torch.zeros((1, 32, 32), dtype=torch.uint8, device="cuda"), 80)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def blend_inputs(tmp_path: Path, num_projection: int, side: int = 64, images: bool = False) -> dict:
    """
    tests/test_mjpeg_gpu.py::blend_inputs restated: WAV + projection file + two random networks on disk, the keyword
    arguments the stream and the API share. With `images` the projection file also holds target and final images.
    """
    L, fps_in, fps_out = 512, 15.0, 30.0
    num_frames = int(num_projection * fps_out / fps_in)
    audio = synthetic.synthetic_audio(num_frames, L, seed=61, frames_per_second=fps_out)
    wav_path = tmp_path / "audio.wav"
    wavfile.write(str(wav_path), int(L * fps_out), audio)
    latents = synthetic.synthetic_final_latents(num_projection, L, seed=62)
    projection_path = tmp_path / "projection.npz"
    extra = {}
    if images:
        rng = np.random.RandomState(63)
        extra["target_images"] = (np.kron(rng.rand(num_projection, 8, 8, 3), np.ones((1, 8, 8, 1))) * 255).astype(np.uint8)
        extra["final_images"] = (np.kron(rng.rand(num_projection, 4, 4, 3), np.ones((1, 8, 8, 1))) * 255).astype(np.uint8)  # 32 x 32
    pfr.write_projection_npz(projection_path, latents.reshape(18, num_projection, L).transpose(1, 0, 2), projection_fps=fps_in, **extra)
    network_paths = []
    for seed in range(2):
        path = tmp_path / f"net_{seed}.pkl"
        network_file.write_random_network(path, side, seed=seed)
        network_paths.append(path)
    inputs = dict(
        wav=[str(wav_path)], network_paths=network_paths, frames_to_visualize=None, output_fps=fps_out, alpha=0.25,
        fft_roll_enabled=True, fft_amplitude_range=(-5, 5), projection_file_path=str(projection_path), blend_depth=12,
    )
    if images:
        inputs["_images"] = extra
    return inputs


def avi_video_and_audio(path: Path):
    """(JPEG files in order, audio bytes, (width, height) of avih) through the super indices of an AVI."""
    blob = path.read_bytes()
    at = blob.index(b"indx")
    streams = {}
    while at >= 0:
        data_at = at + 8
        count, chunk_id = struct.unpack_from("<I4s", blob, data_at + 4)
        chunks = []
        for i in range(count):
            ix_at = struct.unpack_from("<Q", blob, data_at + 24 + 16 * i)[0]
            n, base = struct.unpack_from("<I", blob, ix_at + 12)[0], struct.unpack_from("<Q", blob, ix_at + 20)[0]
            for j in range(n):
                offset, size = struct.unpack_from("<II", blob, ix_at + 32 + 8 * j)
                chunks.append(blob[base + offset : base + offset + size])
        streams[chunk_id] = chunks
        at = blob.find(b"indx", data_at, blob.index(b"movi"))
    size = struct.unpack_from("<II", blob, blob.index(b"avih") + 8 + 32)
    return streams[b"00dc"], b"".join(streams.get(b"01wb", [])), size


def api_arguments(inputs: dict, output_path, debug_path, debug_window, debug_side, overlay=(None, None, None), mask=(None, None), **keywords):
    """Positional arguments of projection_file_blend_api in the reference's order."""
    return (
        [inputs["wav"], output_path, inputs["network_paths"], None, inputs["output_fps"], 64, debug_path, debug_window, debug_side,
         inputs["alpha"], inputs["fft_roll_enabled"], inputs["fft_amplitude_range"], inputs["projection_file_path"], inputs["blend_depth"],
         mask[0], mask[1], overlay[0], overlay[1], overlay[2]],
        keywords,
    )


def raw_debug_frames(inputs: dict, debug_side: int, window, frames_per_call: int, overlay=None, with_output: bool = False):
    """The composed debug frames of a run, before the encode, through the stream's `debug` argument (and, with
    `with_output`, the frames the same run yields)."""
    composed: Dict[int, np.ndarray] = {}
    output: Dict[int, np.ndarray] = {}
    encoded: List[int] = []

    def on_composed(first: int, frames: torch.Tensor) -> None:
        host = frames.cpu().numpy()
        for i, frame in enumerate(host):
            composed[first + i] = frame

    def on_encoded(first: int, chunk) -> None:
        assert chunk.side == debug_side and chunk.width == next(iter(composed.values())).shape[1]
        encoded.extend(range(first, first + len(chunk)))

    debug = compose.DebugVideo(debug_side, window, on_encoded, on_composed, jpeg_quality=80)
    common = {key: value for key, value in inputs.items() if not key.startswith("_")}
    total = 0
    for first, total, frames in projection_file_blend.projection_file_blend_frame_chunks(
        **common, output_side_length=64, frames_per_call=frames_per_call, overlay=overlay, debug=debug
    ):
        for i, frame in enumerate(frames):
            output[first + i] = frame.copy()
    assert sorted(composed) == list(range(total)) and encoded == list(range(total))  # every frame, in frame order
    raw = np.stack([composed[i] for i in range(total)])
    return (raw, np.stack([output[i] for i in range(total)])) if with_output else raw


def test_debug_video_without_overlay(tmp_path: Path) -> None:
    """Fails on the parent commit with NotImplementedError("the matplotlib debug video is out of scope")."""
    inputs = blend_inputs(tmp_path, num_projection=12)
    num_frames, side = 24, 96
    output, debug_path = tmp_path / "out", tmp_path / "debug.avi"
    arguments, keywords = api_arguments(inputs, str(output), str(debug_path), None, side, jpeg_quality=85)
    projection_file_blend.projection_file_blend_api(*arguments, **keywords)
    frames = np.load(str(output) + ".npy")
    assert frames.shape == (num_frames, 64, 64, 3)
    files, audio, size = avi_video_and_audio(debug_path)
    assert len(files) == num_frames and size == (3 * side, side)
    assert audio == wavfile.read(inputs["wav"][0])[1].tobytes()  # the WAV's samples
    raw = raw_debug_frames(inputs, side, None, projection_file_blend.DEFAULT_STREAM_BATCH)  # (the API's frames per call)
    assert raw.shape == (num_frames, side, 3 * side, 3)
    panel0 = torch.ops.gance.resize_bicubic(torch.from_numpy(frames).cuda(), side).cpu().numpy()
    for index, data in enumerate(files):
        assert np.array_equal(raw[index, :, :side], panel0[index]), index  # panel 0 is the resized output frame
        decoded = Image.open(io.BytesIO(data))
        assert decoded.size == (3 * side, side)
        want = np.asarray(pil_roundtrip(raw[index], 85))
        assert np.array_equal(np.asarray(decoded)[:, :side], want[:, :side]), index
        assert np.array_equal(np.asarray(decoded), want), index
    # a projection file without final images: that panel stays black; the synthesis panel is drawn (neither white nor black)
    assert (raw[:, :, side : 2 * side] == 0).all()
    plot = raw[:, :, 2 * side :]
    assert (plot == 255).all(axis=-1).mean() > 0.3 and (plot == np.array(chrome.RED)).all(axis=-1).any()
    # the red cursor of the index axes moves with the frame: window = ceil(24 / 5) = 5 frames
    assert not np.array_equal(plot[0], plot[1]) and (plot[0] != plot[5]).any()


def test_debug_arguments_are_checked_before_any_network_loads(tmp_path: Path, monkeypatch) -> None:
    inputs = blend_inputs(tmp_path, num_projection=4)

    def no_networks(*_args, **_kwargs):
        raise AssertionError("a network was loaded before the debug arguments were checked")

    monkeypatch.setattr(projection_file_blend, "MultiNetwork", no_networks)
    for debug_side in (100, None):
        arguments, keywords = api_arguments(inputs, None, str(tmp_path / "debug.avi"), None, debug_side)
        with pytest.raises(ValueError, match="debug_side_length"):
            projection_file_blend.projection_file_blend_api(*arguments, **keywords)
    arguments, keywords = api_arguments(inputs, None, str(tmp_path / "debug.avi"), None, 96, overlay=(64, 5.0, 3))
    with pytest.raises(ValueError, match="debug_window"):
        projection_file_blend.projection_file_blend_api(*arguments, **keywords)
    assert not (tmp_path / "debug.avi").exists()


class FaceInEverySecondPicture:  # pylint: disable=too-few-public-methods
    """
    A fake landmark finder as in tests/test_overlay_gpu.py and tests/test_blend_api_gpu.py: the same eyes in about half
    of the pictures, decided by a coarse statistic (the mean of the red channel in steps of 4) that one LSB on a few
    pixels does not move.
    """

    @staticmethod
    def face_landmarks(face_image):
        if (int(face_image[:, :, 0].mean()) // 4) % 2:
            return []
        return [{"left_eye": ((12, 20), (24, 26)), "right_eye": ((36, 21), (50, 28))}]


def test_debug_video_with_overlay_and_music_mask(tmp_path: Path, monkeypatch) -> None:
    monkeypatch.setattr(overlay_eye_tracking, "FACE_FINDER_FACTORY", FaceInEverySecondPicture)
    inputs = blend_inputs(tmp_path, num_projection=20, images=True)
    images = inputs.pop("_images")
    num_frames, side, window = 40, 64, 12
    overlay, mask = (64, 5.0, 3), (4, 100000)
    plain, with_debug, debug_path = tmp_path / "plain", tmp_path / "with_debug", tmp_path / "debug.avi"
    arguments, keywords = api_arguments(inputs, str(plain), None, None, None, overlay=overlay, mask=mask)
    projection_file_blend.projection_file_blend_api(*arguments, **keywords)
    arguments, keywords = api_arguments(inputs, str(with_debug), str(debug_path), window, side, overlay=overlay, mask=mask)
    projection_file_blend.projection_file_blend_api(*arguments, **keywords)
    assert Path(str(plain) + ".npy").read_bytes() == Path(str(with_debug) + ".npy").read_bytes()
    files, _audio, size = avi_video_and_audio(debug_path)
    assert len(files) == num_frames and size == (6 * side, side)

    # the raw frames of the same run, and the contexts the overlay stage saw
    contexts: list = []
    original = overlay_eye_tracking.compute_eye_tracking_overlay

    def recording(*args, **kwargs):
        result = original(*args, **kwargs)
        seen = list(result.contexts)
        contexts.extend(seen)
        return result._replace(contexts=iter(seen))

    monkeypatch.setattr(overlay_eye_tracking, "compute_eye_tracking_overlay", recording)
    parameters = projection_file_blend.OverlayParameters(*overlay, *mask)
    raw, blended = raw_debug_frames(inputs, side, window, projection_file_blend.DEFAULT_STREAM_BATCH, overlay=parameters, with_output=True)
    assert raw.shape == (num_frames, side, 6 * side, 3) and len(contexts) == num_frames
    flags = [context.overlay_written for context in contexts]
    assert any(flags) and not all(flags), "the test should see both cursor colours"
    assert np.array_equal(blended, np.load(str(plain) + ".npy"))  # the same run as the API's
    assert np.array_equal(raw[:, :, :side], blended)  # 64 -> 64: no resize
    foreground = np.repeat(images["target_images"], 2, axis=0)
    assert np.array_equal(raw[:, :, side : 2 * side], foreground)
    finals = torch.ops.gance.resize_bicubic(torch.from_numpy(images["final_images"]).cuda(), side).cpu().numpy()
    assert np.array_equal(raw[:, :, 2 * side : 3 * side], np.repeat(finals, 2, axis=0))
    # the overlay panel's cursor: green where the frame's gate flag is set, red otherwise, at frame % window
    overlay_panel = panels.OverlayPanel(side, window, overlay[0], overlay[1])
    for frame in range(num_frames):
        start = (frame // window) * window
        table, _series = overlay_panel.window(frame // window, contexts[start : start + window])
        panel = raw[frame, :, 4 * side : 5 * side]
        for axis in table.axes:
            column = axis.x + chrome.map_extent(frame % window, *axis.x_limits, axis.width)
            want = chrome.GREEN if flags[frame] else chrome.RED
            assert (panel[axis.y : axis.y + axis.height, column] == np.array(want)).all(), (frame, flags[frame])
    # the mask panel is drawn too, and PIL decodes the written video to its own round trip of these frames
    assert (raw[:, :, 5 * side :] == np.array(chrome.RED)).all(axis=-1).any()
    for index in (0, 17, 39):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[index]))), np.asarray(pil_roundtrip(raw[index], 90))), index


def test_composed_frames_do_not_depend_on_the_chunking(tmp_path: Path, monkeypatch) -> None:
    """
    Frames per call 8 and 16 against windows of 12 (overlay, mask) and 8 (synthesis, without overlay) frames: window and
    chunk borders fall differently, so composed chunks are held back, split and released at different points; the whole
    composed frames must not change. The kernel form of an engine call is a function of its batch (1 LSB on a few pixels
    between calls of 8 and of 16 frames, see tests/test_blend_api_gpu.py), so both runs issue their ENGINE calls with 8
    frames: chunking, gather, overlay stage, hold-back and encoder pieces still run at 8 and at 16 frames per call.
    """
    original = projection_file_blend.synthesize_device_frames_network_major

    def engine_calls_of_eight(dlatents, network_indices, networks, output_side_length=None, batch=None, out=None):
        return original(dlatents, network_indices, networks, output_side_length, 8, out=out)

    monkeypatch.setattr(projection_file_blend, "synthesize_device_frames_network_major", engine_calls_of_eight)
    inputs = blend_inputs(tmp_path, num_projection=20, images=True)
    inputs.pop("_images")
    parameters = projection_file_blend.OverlayParameters(64, 5.0, 3, 4, 100000, face_finder=FaceInEverySecondPicture())
    by_eight = raw_debug_frames(inputs, 64, 12, 8, overlay=parameters)
    by_sixteen = raw_debug_frames(inputs, 64, 12, 16, overlay=parameters)
    print("differing bytes per panel:", [int((by_eight[:, :, p * 64 : (p + 1) * 64] != by_sixteen[:, :, p * 64 : (p + 1) * 64]).sum()) for p in range(6)])
    assert np.array_equal(by_eight, by_sixteen)
    without_eight, without_sixteen = raw_debug_frames(inputs, 96, None, 8), raw_debug_frames(inputs, 96, None, 16)
    print("without overlay, differing bytes:", int((without_eight != without_sixteen).sum()))
    assert np.array_equal(without_eight, without_sixteen)
