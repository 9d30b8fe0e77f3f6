"""
GPU tests of the HIP Motion-JPEG decoder (gance_amd/csrc/mjpeg_decode.hip), torch.ops.gance.jpeg_decode and
frames_in_video. The bar is libjpeg itself, as for the encoder (tests/test_mjpeg_gpu.py): every decoded frame equals PIL's
decode of the same bytes, pixel for pixel.
"""

from pathlib import Path
from typing import List, Sequence

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from gance_amd import hip_lib, network_file, projection_file_blend, synthetic, torch_ops  # noqa: F401
from gance_amd.projection import projection_file_reader as pfr
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.video import mjpeg_avi, video_common
from jpeg_decode_ref import binary_grey_noise, gradients, noise, pil_decode, pil_jpeg, without_dht

pytestmark = pytest.mark.gpu

QUALITIES = (1, 50, 90, 100)


def pack(files: Sequence[bytes]):
    """(data on the device, offsets on the host) of files back to back."""
    offsets = np.zeros((len(files) + 1,), dtype=np.int64)
    offsets[1:] = np.cumsum([len(data) for data in files])
    data = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).cuda()
    return data, torch.from_numpy(offsets)


def decode_gpu(files: Sequence[bytes]) -> np.ndarray:
    return torch.ops.gance.jpeg_decode(*pack(files)).cpu().numpy()


def split(data: torch.Tensor, offsets: torch.Tensor) -> List[bytes]:
    host = offsets.cpu().numpy()
    blob = data[: int(host[-1])].cpu().numpy().tobytes()
    return [blob[host[i] : host[i + 1]] for i in range(len(host) - 1)]


def assert_equals_pil(got: np.ndarray, files: Sequence[bytes], what: str) -> None:
    assert got.shape[0] == len(files) and got.dtype == np.uint8
    for index, data in enumerate(files):
        want = pil_decode(data)
        assert got[index].shape == want.shape, (what, index)
        assert np.array_equal(got[index], want), f"{what} frame {index}: {int(np.abs(got[index].astype(int) - want).max())} LSB off"


def contents(side: int, seed: int) -> np.ndarray:
    """Noise, all 0, all 255, saturated primaries, gradients, noisy gradients, binary noise."""
    rs = np.random.RandomState(seed)
    ramp = np.linspace(0, 255, side)
    gradient = np.stack([np.add.outer(ramp, ramp) / 2, np.add.outer(ramp, 255 - ramp) / 2, np.tile(ramp, (side, 1))], -1)
    primaries = np.zeros((side, side, 3), np.uint8)
    half = side // 2
    primaries[:half, :half, 0] = 255
    primaries[:half, half:, 1] = 255
    primaries[half:, :half, 2] = 255
    primaries[half:, half:] = (255, 255, 0)
    flat = np.zeros((side, side, 3), np.uint8)
    return np.stack([
        noise(side, side, seed), flat, flat + 255, primaries, gradient.astype(np.uint8),
        np.clip(gradient + rs.randn(side, side, 3) * 12, 0, 255).astype(np.uint8), binary_grey_noise(side, side, seed),
    ])


@pytest.fixture(scope="module")
def network_frames() -> np.ndarray:
    """Four 64^2 frames of a random-init generator through gance_synthesize_w (as tests/test_mjpeg_gpu.py makes them)."""
    variables = sg2_spec.make_random_variables(64, seed=3, perturb=True)
    engine = hip_lib.Engine(variables, 64, max_batch=4, device=0)
    try:
        w = np.random.RandomState(5).randn(4, engine.num_layers, 512).astype(np.float32)
        frames = engine.synthesize_w(w)
    finally:
        engine.close()
    return frames


# ---- round trip of our own encoder -------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [16, 64, 256])
def test_round_trip_of_the_encoder_equals_pil(side: int, network_frames: np.ndarray) -> None:
    frames = contents(side, seed=side)
    if side == 64:
        frames = np.concatenate([frames, network_frames])
    elif side == 256:
        frames = np.concatenate([frames, torch.ops.gance.resize_bicubic(torch.from_numpy(network_frames).cuda(), 256).cpu().numpy()])
    d_frames = torch.from_numpy(frames).cuda()
    for quality in QUALITIES:
        data, offsets = torch.ops.gance.jpeg_encode(d_frames, quality)
        got = torch.ops.gance.jpeg_decode(data, offsets).cpu().numpy()  # offsets on the device, as the encoder returns them
        assert_equals_pil(got, split(data, offsets), f"side {side} q {quality}")


@pytest.mark.parametrize("width_height", [(48, 32), (32, 48), (16, 1040), (2064, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip_of_rectangles(width_height) -> None:
    """48 x 32 and 32 x 48; 16 x 1040 is 130 restart segments per frame (more than one wave of them), 2064 x 16 has
    segments of 129 MCUs."""
    width, height = width_height
    frames = np.stack([noise(width, height, 7), gradients(width, height), binary_grey_noise(width, height, 8)])
    for quality in (1, 90):
        data, offsets = torch.ops.gance.jpeg_encode_rect(torch.from_numpy(frames).cuda(), quality)
        files = split(data, offsets)
        assert hip_lib.jpeg_parse_header(files[0]).restart_interval == width // 16
        assert_equals_pil(torch.ops.gance.jpeg_decode(data, offsets).cpu().numpy(), files, f"{width}x{height} q {quality}")


def test_round_trip_at_2160() -> None:
    """The product's own geometry: 270 segments of 135 MCUs per frame."""
    frames = np.stack([noise(2160, 2160, 2160), np.clip(gradients(2160, 2160).astype(int) + noise(2160, 2160, 1) // 8, 0, 255).astype(np.uint8)])
    data, offsets = torch.ops.gance.jpeg_encode(torch.from_numpy(frames).cuda(), 90)
    assert_equals_pil(torch.ops.gance.jpeg_decode(data, offsets).cpu().numpy(), split(data, offsets), "2160")


# ---- foreign files ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(21, 50), (17, 33), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pil_written_files(size) -> None:
    width, height = size
    images = [noise(width, height, 1), gradients(width, height), binary_grey_noise(width, height, 2), noise(width, height, 3) // 2]
    for layout in ({"restart_marker_blocks": 3}, {}, {"restart_marker_rows": 1}):
        for quality in QUALITIES:
            files = [pil_jpeg(image, quality, **layout) for image in images]
            assert_equals_pil(decode_gpu(files), files, f"{layout} q {quality}")
    # every frame with its own optimised tables, and one with the standard ones, in ONE batch
    files = [pil_jpeg(image, 60 + 10 * i, optimize=True) for i, image in enumerate(images)] + [pil_jpeg(images[0], 75)]
    assert len({data[: data.index(b"\xff\xda")] for data in files}) == len(files)
    assert_equals_pil(decode_gpu(files), files, "optimize")
    # without DHT: the Annex K tables
    files = [without_dht(pil_jpeg(image, 85, restart_marker_blocks=3)) for image in images]
    assert_equals_pil(decode_gpu(files), files, "without DHT")


def test_noise_at_q1_that_leaves_the_range_limit_table() -> None:
    """The file of tests/test_mjpeg_decode.py on which saturation and libjpeg's range-limit table part: PIL saturates."""
    files = [pil_jpeg(binary_grey_noise(48, 64, 2252), 1, restart_marker_rows=1), pil_jpeg(binary_grey_noise(48, 64, 2252), 1)]
    assert_equals_pil(decode_gpu(files), files, "q 1 binary noise")


# ---- batch independence ------------------------------------------------------------------------------------------------
def test_pixels_do_not_depend_on_the_batch() -> None:
    frames = np.concatenate([contents(48, seed=s) for s in range(10)])[:64]
    data, offsets = torch.ops.gance.jpeg_encode(torch.from_numpy(frames).cuda(), 90)
    files = split(data, offsets)
    assert len(files) == 64
    whole = torch.ops.gance.jpeg_decode(data, offsets).cpu().numpy()
    target = files[63]
    want = pil_decode(target)
    assert np.array_equal(whole[63], want)  # last of 64
    assert np.array_equal(decode_gpu([target])[0], want)  # alone
    assert np.array_equal(decode_gpu([target] + files[:4])[0], want)  # first of 5


# ---- status ------------------------------------------------------------------------------------------------------------
def test_a_truncated_frame_is_reported_and_leaves_its_neighbours_alone() -> None:
    """The middle frame's byte range is shortened by a third inside one buffer, so any over-read would land in the next
    frame's valid bytes: this checks the reporting, it does not set out to provoke a fault."""
    frames = contents(64, seed=11)[[0, 5, 4]]
    files = split(*torch.ops.gance.jpeg_encode(torch.from_numpy(frames).cuda(), 90))
    cut = [files[0], files[1][: len(files[1]) * 2 // 3], files[2]]
    data, offsets = pack(cut)
    with pytest.raises(ValueError, match="frame 1: truncated"):
        torch.ops.gance.jpeg_decode(data, offsets)

    infos = (hip_lib.JpegInfo * 3)()
    for info, blob in zip(infos, cut):
        hip_lib.jpeg_parse_header(blob, info)
    host_offsets = offsets.numpy()
    workspace_bytes = hip_lib.jpeg_decode_bounds(3, 64, 64, int(host_offsets[-1]))
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device="cuda")
    status = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    hip_lib.jpeg_decode_device(data.data_ptr(), host_offsets, infos, workspace.data_ptr(), workspace_bytes, out.data_ptr(), status.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    assert status.cpu().tolist() == [0, 1, 0] and hip_lib.JPEG_STATUS_REASONS[1] == "truncated data"
    host = out.cpu().numpy()
    assert np.array_equal(host[0], pil_decode(files[0])) and np.array_equal(host[2], pil_decode(files[2]))

    # a file without restart markers, cut inside its only segment: found by the entropy decoder
    plain = pil_jpeg(noise(40, 24, 1), 90)
    with pytest.raises(ValueError, match="frame 0: truncated"):
        decode_gpu([plain[: len(plain) * 2 // 3], plain])


def test_unsupported_files_are_refused_by_the_op() -> None:
    good = pil_jpeg(noise(32, 32, 1), 80)
    with pytest.raises(ValueError, match="frame 1: .*4:2:0"):
        decode_gpu([good, pil_jpeg(noise(32, 32, 1), 80, subsampling=2)])
    with pytest.raises(ValueError, match="one size"):
        decode_gpu([good, pil_jpeg(noise(16, 32, 1), 80)])


# ---- frames_in_video -----------------------------------------------------------------------------------------------------
def blend_inputs(tmp_path: Path, num_projection: int, side: int = 64) -> dict:
    """tests/test_mjpeg_gpu.py::blend_inputs restated: WAV + projection file + two random networks on disk."""
    L, fps_in, fps_out = 512, 15.0, 30.0
    num_frames = int(num_projection * fps_out / fps_in)
    audio = synthetic.synthetic_audio(num_frames, L, seed=61, frames_per_second=fps_out)
    wav_path = tmp_path / "audio.wav"
    wavfile.write(str(wav_path), int(L * fps_out), audio)
    latents = synthetic.synthetic_final_latents(num_projection, L, seed=62)
    projection_path = tmp_path / "projection.npz"
    pfr.write_projection_npz(projection_path, latents.reshape(18, num_projection, L).transpose(1, 0, 2), projection_fps=fps_in)
    network_paths = []
    for seed in range(2):
        path = tmp_path / f"net_{seed}.pkl"
        network_file.write_random_network(path, side, seed=seed)
        network_paths.append(path)
    return dict(
        wav=[str(wav_path)], network_paths=network_paths, frames_to_visualize=None, output_fps=fps_out, alpha=0.25,
        fft_roll_enabled=True, fft_amplitude_range=(-5, 5), projection_file_path=str(projection_path), blend_depth=12,
    )


def test_frames_in_video_reads_what_the_blend_wrote(tmp_path: Path) -> None:
    inputs = blend_inputs(tmp_path, num_projection=6)
    num_frames = 12
    video_path, debug_path = tmp_path / "video.avi", tmp_path / "debug.avi"
    projection_file_blend.projection_file_blend_api(
        **inputs, output_path=str(video_path), output_format="avi", jpeg_quality=85, output_side_length=64, debug_path=str(debug_path),
        debug_window=None, debug_side_length=64, complexity_change_rolling_sum_window=None, complexity_change_threshold=None,
        phash_distance=None, bbox_distance=None, track_length=None,
    )
    with mjpeg_avi.MjpegAviReader(video_path) as reader:
        files = reader.read_frame_bytes(0, reader.frame_count)
        rate, audio = reader.read_audio()
    want_rate, want_audio = wavfile.read(inputs["wav"][0])
    assert rate == want_rate and np.array_equal(audio, want_audio)
    want = [pil_decode(data) for data in files]

    video = video_common.frames_in_video(video_path)
    assert (video.original_fps, video.total_frame_count, video.original_resolution) == (30.0, num_frames, (64, 64))
    frames = list(video.frames)
    assert len(frames) == num_frames
    for index, frame in enumerate(frames):
        assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and np.array_equal(frame, want[index]), index

    halved = list(video_common.frames_in_video(video_path, reduce_fps_to=15.0, width_height=(64, 64)).frames)
    assert len(halved) == 6 and all(np.array_equal(frame, want[2 * i]) for i, frame in enumerate(halved))

    chunks = list(video_common.frames_in_video_device_chunks(video_path, frames_per_chunk=5))
    assert [tuple(chunk.shape) for chunk in chunks] == [(5, 64, 64, 3), (5, 64, 64, 3), (2, 64, 64, 3)]
    assert all(chunk.is_cuda and chunk.dtype == torch.uint8 for chunk in chunks)
    assert np.array_equal(torch.cat(chunks).cpu().numpy(), np.stack(want))

    with pytest.raises(NotImplementedError, match="bicubic"):
        video_common.frames_in_video(video_path, width_height=(32, 32))

    # the debug video is a row of panels: not square
    debug = video_common.frames_in_video(debug_path)
    assert debug.original_resolution == (192, 64) and debug.total_frame_count == num_frames
    with mjpeg_avi.MjpegAviReader(debug_path) as reader:
        debug_files = reader.read_frame_bytes(0, num_frames)
    debug_frames = list(debug.frames)
    assert len(debug_frames) == num_frames and debug_frames[0].shape == (64, 192, 3)
    assert all(np.array_equal(frame, pil_decode(data)) for frame, data in zip(debug_frames, debug_files))
