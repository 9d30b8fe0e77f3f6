"""
GPU tests of the HIP Motion-JPEG encoder (gance_amd/csrc/mjpeg.hip) and of `projection_file_blend_api(output_format="avi")`.
The bar is libjpeg itself: PIL decodes every GPU-encoded frame to exactly the pixels it decodes from its own encode of the
same frame at the same quality (4:2:2), and our quantisation tables are PIL's.
"""

import io
import struct
from pathlib import Path
from typing import List

import numpy as np
import pytest
import torch
from PIL import Image
from scipy.io import wavfile

from gance_amd import hip_lib, network_file, projection_file_blend, synthetic, torch_ops  # noqa: F401
from gance_amd.projection import projection_file_reader as pfr
from gance_amd.stylegan2 import spec as sg2_spec

pytestmark = pytest.mark.gpu

QUALITIES = (1, 50, 90, 100)


def encode_gpu(frames: np.ndarray, quality: int) -> List[bytes]:
    """JFIF files of [B, S, S, 3] uint8 frames through the ctypes entry point."""
    batch, side = frames.shape[0], frames.shape[1]
    workspace_bytes, capacity = hip_lib.jpeg_encode_bounds(batch, side)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device="cuda")
    out = torch.empty((capacity,), dtype=torch.uint8, device="cuda")
    offsets = torch.empty((batch + 1,), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    hip_lib.jpeg_encode_device(d_frames.data_ptr(), batch, side, quality, workspace.data_ptr(), workspace_bytes, out.data_ptr(),
                               capacity, offsets.data_ptr(), stream)
    torch.cuda.synchronize()
    host_offsets = offsets.cpu().numpy()
    data = out[: int(host_offsets[-1])].cpu().numpy().tobytes()
    return [data[host_offsets[i] : host_offsets[i + 1]] for i in range(batch)]


def pil_roundtrip(frame: np.ndarray, quality: int) -> Image.Image:
    buffer = io.BytesIO()
    Image.fromarray(frame).save(buffer, format="JPEG", quality=quality, subsampling=1)
    return Image.open(io.BytesIO(buffer.getvalue()))


def contents(side: int, seed: int) -> np.ndarray:
    """Noise (the capacity stress case at q 100), all 0, all 255, saturated primaries, gradients."""
    rs = np.random.RandomState(seed)
    noise = rs.randint(0, 256, (side, side, 3)).astype(np.uint8)
    ramp = np.linspace(0, 255, side)
    gradient = np.stack([np.add.outer(ramp, ramp) / 2, np.add.outer(ramp, 255 - ramp) / 2, np.tile(ramp, (side, 1))], -1)
    noisy_gradient = np.clip(gradient + rs.randn(side, side, 3) * 12, 0, 255)
    primaries = np.zeros((side, side, 3), np.uint8)
    half = side // 2
    primaries[:half, :half, 0] = 255
    primaries[:half, half:, 1] = 255
    primaries[half:, :half, 2] = 255
    primaries[half:, half:] = (255, 255, 0)
    return np.stack([noise, np.zeros_like(noise), np.full_like(noise, 255), primaries, gradient.astype(np.uint8),
                     noisy_gradient.astype(np.uint8)])


@pytest.fixture(scope="module")
def network_frames() -> np.ndarray:
    """Four 64^2 frames of a random-init generator through gance_synthesize_w."""
    variables = sg2_spec.make_random_variables(64, seed=3, perturb=True)
    engine = hip_lib.Engine(variables, 64, max_batch=4, device=0)
    try:
        w = np.random.RandomState(5).randn(4, engine.num_layers, 512).astype(np.float32)
        frames = engine.synthesize_w(w)
    finally:
        engine.close()
    return frames


def assert_decodes_like_pil(files: List[bytes], frames: np.ndarray, quality: int) -> None:
    side = frames.shape[1]
    for index, (data, frame) in enumerate(zip(files, frames)):
        ours = Image.open(io.BytesIO(data))
        reference = pil_roundtrip(frame, quality)
        assert ours.size == (side, side) and ours.mode == "RGB"
        got = np.asarray(ours)
        want = np.asarray(reference)
        assert np.array_equal(got, want), f"frame {index} q {quality}: {int(np.abs(got.astype(int) - want).max())} LSB off"
        assert ours.quantization == reference.quantization


@pytest.mark.parametrize("side", [16, 64, 256])
def test_pixels_equal_libjpeg(side: int, network_frames: np.ndarray) -> None:
    frames = contents(side, seed=side)
    if side == 64:
        frames = np.concatenate([frames, network_frames])
    elif side == 256:
        upscaled = torch.ops.gance.resize_bicubic(torch.from_numpy(network_frames).cuda(), 256).cpu().numpy()
        frames = np.concatenate([frames, upscaled])
    for quality in QUALITIES:
        assert_decodes_like_pil(encode_gpu(frames, quality), frames, quality)


def test_pixels_equal_libjpeg_at_2160() -> None:
    rs = np.random.RandomState(2160)
    noise = rs.randint(0, 256, (1, 2160, 2160, 3)).astype(np.uint8)
    for quality in QUALITIES:
        assert_decodes_like_pil(encode_gpu(noise, quality), noise, quality)


def markers(data: bytes) -> dict:
    """Marker -> payload of the header segments up to SOS."""
    found, at = {}, 2
    while True:
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        found.setdefault(marker, []).append(data[at + 4 : at + 2 + length])
        if marker == 0xDA:
            return found
        at += 2 + length


def test_headers() -> None:
    side = 96
    frames = contents(side, seed=1)[:2]
    data = encode_gpu(frames, 75)[0]
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    found = markers(data)
    sof = found[0xC0][0]
    assert struct.unpack(">BHHB", sof[:6]) == (8, side, side, 3)
    assert sof[6:] == bytes([1, 0x21, 0, 2, 0x11, 1, 3, 0x11, 1])  # Y 2x1, Cb 1x1, Cr 1x1
    assert struct.unpack(">H", found[0xDD][0])[0] == side // 16
    # one restart segment per MCU row: RST0..RST7 cycling between the rows
    scan = data[data.index(b"\xff\xda") :]
    restarts = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert restarts == [0xD0 + (r % 8) for r in range(side // 8 - 1)]
    ours = Image.open(io.BytesIO(data))
    assert ours.layer == pil_roundtrip(frames[0], 75).layer
    assert ours.quantization == pil_roundtrip(frames[0], 75).quantization


def test_deterministic_and_independent_of_batch() -> None:
    frames = np.concatenate([contents(48, seed=7), contents(48, seed=8)[:1]])  # 7 frames
    batch = encode_gpu(frames, 90)
    assert encode_gpu(frames, 90) == batch
    for k in (0, 3, 6):
        assert encode_gpu(frames[k : k + 1], 90) == [batch[k]]


def test_torch_op() -> None:
    frames = torch.from_numpy(contents(32, seed=2)).cuda()
    torch.library.opcheck(torch.ops.gance.jpeg_encode.default, (frames, 80), test_utils=("test_schema", "test_faketensor"))
    data, offsets = torch.ops.gance.jpeg_encode(frames, 80)
    assert data.shape == (hip_lib.jpeg_encode_bounds(6, 32)[1],) and offsets.dtype == torch.int64
    host = offsets.cpu().numpy()
    got = data[: int(host[-1])].cpu().numpy().tobytes()
    assert [got[host[i] : host[i + 1]] for i in range(6)] == encode_gpu(frames.cpu().numpy(), 80)
    with pytest.raises(ValueError):
        torch.ops.gance.jpeg_encode(torch.zeros((1, 40, 40, 3), dtype=torch.uint8, device="cuda"), 80)


def avi_video_and_audio(path: Path):
    """(JPEG files in order, audio bytes, dwRate, dwScale, dmlh frames) through the super indices of an AVI."""
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
    strh = blob.index(b"strh") + 8
    scale, rate = struct.unpack_from("<II", blob, strh + 20)
    frames = struct.unpack_from("<I", blob, blob.index(b"dmlh") + 8)[0]
    return streams[b"00dc"], b"".join(streams.get(b"01wb", [])), rate, scale, frames


def blend_inputs(tmp_path: Path, num_projection: int, side: int = 64) -> dict:
    """WAV + projection file + two random networks on disk: the keyword arguments the stream and the API share."""
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


def test_encoded_ring_returns_every_piece_of_a_chunk_split_across_more_pushes_than_slots() -> None:
    """A gathered chunk of world_size x frames_per_call frames is encoded and pushed piece by piece: with 5 pieces through a
    3-slot ring, every finished piece must be handed out before the push that reuses its slot."""
    frames = np.concatenate([contents(32, seed=s) for s in range(4)])[:20]  # 20 different frames
    want = encode_gpu(frames, 70)
    ring = projection_file_blend._EncodedHostRing(slots=3)  # pylint: disable=protected-access
    reader = torch.cuda.Stream()
    d_frames = torch.from_numpy(frames).cuda()
    torch.cuda.current_stream().synchronize()
    got = {}

    def take(done) -> None:
        first, chunk = done
        assert chunk.side == 32
        for i in range(len(chunk)):
            got[first + i] = chunk.frame(i).tobytes()

    for _moved, done in projection_file_blend.encode_into_ring(ring, 100, d_frames, 70, 4, reader):
        if done is not None:
            take(done)
    take(ring.flush())
    assert sorted(got) == list(range(100, 120))
    assert [got[100 + i] for i in range(20)] == want


def test_encoded_stream_over_several_chunks_and_pieces(tmp_path: Path, monkeypatch) -> None:
    """The stream with 8 frames per chunk over 48 frames, each chunk encoded in 2-frame pieces (four pushes per chunk, as a
    gathered chunk of four ranks takes): every encoded frame decodes like PIL's encode of the raw stream's frame."""
    inputs = blend_inputs(tmp_path, num_projection=24)
    common = dict(output_side_length=96, frames_per_call=8)
    raw = {}
    for first, _total, frames in projection_file_blend.projection_file_blend_frame_chunks(**inputs, **common):
        for i, frame in enumerate(frames):
            raw[first + i] = frame.copy()
    original = projection_file_blend.encode_into_ring

    def in_pieces_of_two(ring, first, frames, quality, _piece_frames, reader_stream):
        return original(ring, first, frames, quality, 2, reader_stream)

    monkeypatch.setattr(projection_file_blend, "encode_into_ring", in_pieces_of_two)
    encoded, timings = {}, {}
    for first, total, chunk in projection_file_blend.projection_file_blend_frame_chunks(**inputs, **common, jpeg_quality=80, timings=timings):
        assert isinstance(chunk, projection_file_blend.EncodedFrames) and total == 48
        for i in range(len(chunk)):
            encoded[first + i] = chunk.frame(i).tobytes()
    assert sorted(encoded) == sorted(raw) == list(range(48))
    for index in range(48):
        got = np.asarray(Image.open(io.BytesIO(encoded[index])))
        assert np.array_equal(got, np.asarray(pil_roundtrip(raw[index], 80))), index
    assert timings["bytes_to_host"] == sum(len(data) for data in encoded.values()) + 8 * (48 + 24)  # bytes + offsets of 24 pieces


def test_projection_file_blend_api_writes_avi(tmp_path: Path) -> None:
    inputs = blend_inputs(tmp_path, num_projection=16)
    num_frames, out_side = 32, 96
    common = dict(
        **inputs, output_side_length=out_side, debug_path=None, debug_window=None, debug_side_length=None,
        complexity_change_rolling_sum_window=None, complexity_change_threshold=None, phash_distance=None, bbox_distance=None,
        track_length=None,
    )
    avi_path = tmp_path / "video.avi"
    projection_file_blend.projection_file_blend_api(output_path=str(avi_path), output_format="avi", jpeg_quality=85, **common)
    npy_path = tmp_path / "frames.npy"
    projection_file_blend.projection_file_blend_api(output_path=str(npy_path), **common)
    raw = np.load(npy_path)
    assert raw.shape == (num_frames, out_side, out_side, 3)

    files, audio_bytes, rate, scale, total = avi_video_and_audio(avi_path)
    assert len(files) == total == num_frames and (rate, scale) == (30, 1)
    for index, data in enumerate(files):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), np.asarray(pil_roundtrip(raw[index], 85))), index
    assert audio_bytes == wavfile.read(inputs["wav"][0])[1].tobytes()

    # no output side: the networks' own (64), as the reference does
    native_path = tmp_path / "native.avi"
    projection_file_blend.projection_file_blend_api(
        output_path=str(native_path), output_format="avi", jpeg_quality=85, **{**common, "output_side_length": None}
    )
    native_files, _, _, _, native_total = avi_video_and_audio(native_path)
    assert native_total == num_frames and Image.open(io.BytesIO(native_files[0])).size == (64, 64)
    with pytest.raises(ValueError):
        projection_file_blend.projection_file_blend_api(
            output_path=str(tmp_path / "bad.avi"), output_format="avi", **{**common, "output_side_length": 100}
        )
