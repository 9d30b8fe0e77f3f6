"""
CPU tests of the Motion-JPEG read path: the numpy restatement of the decoder (tests/jpeg_decode_ref.py) against PIL, the
header parser of the C entry point (host only), `MjpegAviReader` on files `MjpegAviWriter` wrote, and reduce_fps_take_every.
The kernels themselves are tested on the GPU (tests/test_mjpeg_decode_gpu.py).
"""

import struct
from pathlib import Path
from typing import List

import numpy as np
import pytest
from scipy.io import wavfile

import jpeg_decode_ref
from gance_amd import hip_lib
from jpeg_decode_ref import binary_grey_noise, gradients, noise, pil_decode, pil_jpeg, without_dht
from gance_amd.video import mjpeg_avi

SIZES = [(1, 1), (9, 2), (17, 33), (21, 50), (48, 64)]  # width, height
QUALITIES = (1, 50, 90, 100)
LAYOUTS = ({"restart_marker_rows": 1}, {"restart_marker_blocks": 3}, {}, {"optimize": True})
# binary grey noise whose q 1 file decodes to samples more than 512 from mid-grey, where libjpeg's range-limit table wraps
# and a saturating decoder does not (found by a search over 3000 seeds: one file had such samples); the test asserts that
# it still separates the two
WRAPPING_NOISE_SEED, WRAPPING_NOISE_SIZE = 2252, (48, 64)


# ---- the reference decoder against PIL -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_decoder_equals_pil(size) -> None:
    width, height = size
    for name, image in (("noise", noise(width, height, width)), ("gradients", gradients(width, height))):
        for quality in QUALITIES:
            for layout in LAYOUTS:
                data = pil_jpeg(image, quality, **layout)
                assert np.array_equal(jpeg_decode_ref.decode(data), pil_decode(data)), (name, quality, layout)


def test_noise_at_q1_separates_saturation_from_the_range_limit_table() -> None:
    """
    Noise at q 1 is where jidctint.c's range-limit table (sample_range_limit[value & 0x3FF]) and a saturation to 0..255
    part: 3 values of this file. PIL (libjpeg-turbo, whose SIMD IDCT packs with saturation) gives the saturated ones, so
    that is what the decoder restates; the table's would be 255 where PIL has 0.
    """
    data = pil_jpeg(binary_grey_noise(*WRAPPING_NOISE_SIZE, WRAPPING_NOISE_SEED), 1)
    want = pil_decode(data)
    assert np.array_equal(jpeg_decode_ref.decode(data), want)
    wrapped = jpeg_decode_ref.decode(data, limit=jpeg_decode_ref.table_limit)
    assert np.any(wrapped != want), "no sample of this file leaves the table's linear part: the case is vacuous"


def test_reference_decoder_without_dht_uses_annex_k() -> None:
    data = pil_jpeg(noise(21, 50, 3), 90, restart_marker_rows=1)  # PIL's default tables are the Annex K ones
    stripped = without_dht(data)
    assert len(stripped) < len(data) and b"\xff\xc4" not in stripped[: stripped.index(b"\xff\xda")]
    assert np.array_equal(jpeg_decode_ref.decode(stripped), pil_decode(data))


# ---- the header parser, through the C entry ----------------------------------------------------------------------------
def encoder_layout_file(width: int, height: int, quality: int, seed: int) -> bytes:
    """A PIL file in the layout our encoder writes: 4:2:2, standard tables, one restart interval per MCU row."""
    return pil_jpeg(noise(width, height, seed), quality, restart_marker_rows=1)


def test_parse_header_sizes_and_scan_range() -> None:
    for width, height, layout, interval in (
        (64, 48, {"restart_marker_rows": 1}, 4), (17, 33, {"restart_marker_blocks": 3}, 3), (21, 50, {}, 0), (9, 2, {"optimize": True}, 0),
    ):
        data = pil_jpeg(noise(width, height, 1), 75, **layout)
        info = hip_lib.jpeg_parse_header(data)
        assert (info.width, info.height, info.restart_interval, info.has_huffman_tables) == (width, height, interval, 1)
        sos = data.index(b"\xff\xda")
        assert info.scan_offset == sos + 2 + struct.unpack_from(">H", data, sos + 2)[0]
        assert info.scan_offset + info.scan_bytes == len(data)
        reference = jpeg_decode_ref.parse_header(data)
        assert info.scan_offset == reference.scan_offset
        for c in range(3):
            assert list(info.quant[c]) == list(reference.quant[c])
    # the tables of a default PIL file are the Annex K ones, per component
    info = hip_lib.jpeg_parse_header(encoder_layout_file(32, 16, 50, 2))
    for c in range(3):
        for cls in range(2):
            bits, values = jpeg_decode_ref.ANNEX_K[(cls, min(c, 1))]
            assert list(info.huff_bits[c][cls]) == bits and list(info.huff_values[c][cls])[: len(values)] == values


def test_parse_header_without_dht_falls_back_to_annex_k() -> None:
    data = encoder_layout_file(32, 16, 50, 2)
    full, stripped = hip_lib.jpeg_parse_header(data), hip_lib.jpeg_parse_header(without_dht(data))
    assert (full.has_huffman_tables, stripped.has_huffman_tables) == (1, 0)
    assert bytes(stripped.huff_bits) == bytes(full.huff_bits) and bytes(stripped.huff_values) == bytes(full.huff_values)
    assert stripped.scan_bytes == full.scan_bytes and stripped.scan_offset < full.scan_offset


def over_subscribed(data: bytes) -> bytes:
    """Three codes of length 1 in the first DHT."""
    at = data.index(b"\xff\xc4")
    return data[: at + 5] + b"\x03" + data[at + 6 :]


def sixteen_bit_dqt(data: bytes) -> bytes:
    at = data.index(b"\xff\xdb")
    return data[: at + 4] + bytes([0x10 | data[at + 4]]) + data[at + 5 :]


def test_parse_header_refuses_what_the_decoder_does_not_take() -> None:
    image = noise(32, 32, 4)
    good = pil_jpeg(image, 80)
    cases = {
        "progressive": pil_jpeg(image, 80, progressive=True),
        "4:2:0": pil_jpeg(image, 80, subsampling=2),
        "4:4:4": pil_jpeg(image, 80, subsampling=0),
        "grey": pil_jpeg(image[..., 0], 80),
        "cut short": good[: good.index(b"\xff\xda") - 20],
        "over-subscribed": over_subscribed(good),
        "16-bit DQT": sixteen_bit_dqt(good),
    }
    for reason, data in cases.items():
        with pytest.raises(ValueError, match=reason):
            hip_lib.jpeg_parse_header(data)
    with pytest.raises(ValueError, match="SOI"):
        hip_lib.jpeg_parse_header(b"RIFF" + good)


def test_decode_entry_refuses_bad_arguments_before_a_device() -> None:
    """Host-only checks: this machine has no device, and none is asked for."""
    import ctypes

    files = [pil_jpeg(noise(32, 16, 5), 80), pil_jpeg(noise(16, 16, 6), 80)]
    infos = (hip_lib.JpegInfo * 2)()
    for info, data in zip(infos, files):
        hip_lib.jpeg_parse_header(data, info)
    offsets = np.array([0, len(files[0]), len(files[0]) + len(files[1])], dtype=np.int64)
    with pytest.raises(ValueError, match="one size"):
        hip_lib.jpeg_decode_device(16, offsets, infos, 16, 1 << 40, 16, 16)
    one = (hip_lib.JpegInfo * 1)()
    ctypes.memmove(one, infos, ctypes.sizeof(hip_lib.JpegInfo))
    with pytest.raises(ValueError, match="workspace"):
        hip_lib.jpeg_decode_device(16, offsets[:2], one, 16, 64, 16, 16)
    with pytest.raises(ValueError, match="scan range"):
        hip_lib.jpeg_decode_device(16, offsets[:2] + np.array([0, 7]), one, 16, 1 << 40, 16, 16)
    assert hip_lib.jpeg_decode_bounds(1, 32, 16, len(files[0])) > 32 * 16 * 3
    for width, height in ((0, 16), (16, 8193)):
        with pytest.raises(ValueError):
            hip_lib.jpeg_decode_bounds(1, width, height, 1000)


# ---- MjpegAviReader ----------------------------------------------------------------------------------------------------
def jpegs(count: int, width: int = 32, height: int = 32) -> List[bytes]:
    return [pil_jpeg(noise(width, height, 100 + i), 60 + i % 30) for i in range(count)]


def write_avi(path: Path, files: List[bytes], fps: float = 30.0, wavs=None, **options) -> None:
    with mjpeg_avi.MjpegAviWriter(path, 32, fps, wavs=wavs, **options) as writer:
        for data in files:
            writer.add_frame(data)


@pytest.mark.parametrize("segment_limit", [mjpeg_avi.DEFAULT_SEGMENT_LIMIT, 16384], ids=["one_segment", "many_segments"])
@pytest.mark.parametrize("dtype", [None, np.int16, np.float32], ids=["silent", "int16", "float32"])
def test_reader_returns_what_the_writer_was_given(tmp_path: Path, segment_limit: int, dtype) -> None:
    files = jpegs(40)
    wavs, samples = None, None
    if dtype is not None:
        rs = np.random.RandomState(9)
        values = rs.randn(2 * 8000 + 123, 2)
        samples = (values * 8000).astype(np.int16) if dtype == np.int16 else values.astype(np.float32)
        wavfile.write(str(tmp_path / "a.wav"), 8000, samples[:9000])
        wavfile.write(str(tmp_path / "b.wav"), 8000, samples[9000:])
        wavs = [tmp_path / "a.wav", tmp_path / "b.wav"]
    path = tmp_path / "video.avi"
    write_avi(path, files, 29.97, wavs, segment_limit=segment_limit)
    if segment_limit < mjpeg_avi.DEFAULT_SEGMENT_LIMIT:
        assert path.read_bytes().count(b"AVIX") > 2
    with mjpeg_avi.MjpegAviReader(path) as reader:
        assert reader.frame_count == 40 and (reader.width, reader.height) == (32, 32)
        assert reader.fps_fraction == mjpeg_avi.Fraction(2997, 100) and reader.fps == 29.97
        assert reader.read_frame_bytes(0, 40) == files
        assert reader.read_frame_bytes(37, 3) == files[37:] and reader.read_frame_bytes(5, 0) == []
        assert reader.frame_sizes(3, 2) == [len(files[3]), len(files[4])]
        with pytest.raises(IndexError):
            reader.read_frame_bytes(39, 2)
        audio = reader.read_audio()
        if dtype is None:
            assert audio is None
        else:
            want_rate, want = mjpeg_avi.read_concatenated_wavs(wavs)
            assert audio[0] == want_rate == 8000 and audio[1].dtype == want.dtype and np.array_equal(audio[1], want)


def test_reader_mono_audio_keeps_its_shape(tmp_path: Path) -> None:
    samples = (np.random.RandomState(1).randn(5000) * 3000).astype(np.int16)
    wavfile.write(str(tmp_path / "mono.wav"), 4000, samples)
    write_avi(tmp_path / "video.avi", jpegs(10), 10.0, [tmp_path / "mono.wav"])
    with mjpeg_avi.MjpegAviReader(tmp_path / "video.avi") as reader:
        rate, audio = reader.read_audio()
    assert rate == 4000 and audio.shape == (5000,) and np.array_equal(audio, samples)


def test_reader_falls_back_to_idx1(tmp_path: Path) -> None:
    files = jpegs(12)
    samples = (np.random.RandomState(2).randn(3000) * 3000).astype(np.int16)
    wavfile.write(str(tmp_path / "a.wav"), 4000, samples)
    write_avi(tmp_path / "video.avi", files, 24.0, [tmp_path / "a.wav"])
    blob = bytearray((tmp_path / "video.avi").read_bytes())
    at = blob.find(b"indx")
    while 0 <= at < blob.index(b"movi"):  # both streams' super indices: no entries in use, the entries zeroed
        size = struct.unpack_from("<I", blob, at + 4)[0]
        blob[at + 8 + 4 : at + 8 + 8] = bytes(4)
        blob[at + 8 + 24 : at + 8 + size] = bytes(size - 24)
        at = blob.find(b"indx", at + 8)
    (tmp_path / "old.avi").write_bytes(bytes(blob))
    with mjpeg_avi.MjpegAviReader(tmp_path / "old.avi") as reader:
        assert reader.frame_count == 12 and reader.read_frame_bytes(0, 12) == files
        assert np.array_equal(reader.read_audio()[1], samples)


def test_reader_repeats_the_previous_frame_for_an_empty_chunk(tmp_path: Path) -> None:
    files = jpegs(6)
    dropped = list(files)
    dropped[3] = b""
    write_avi(tmp_path / "video.avi", dropped)
    with mjpeg_avi.MjpegAviReader(tmp_path / "video.avi") as reader:
        assert reader.frame_count == 6
        assert reader.read_frame_bytes(0, 6) == files[:3] + [files[2]] + files[4:]
    write_avi(tmp_path / "first.avi", [b""] + files)
    with pytest.raises(ValueError, match="first frame"):
        mjpeg_avi.MjpegAviReader(tmp_path / "first.avi")


def test_reader_refuses_other_files(tmp_path: Path) -> None:
    (tmp_path / "frame.jpg").write_bytes(jpegs(1)[0])
    with pytest.raises(ValueError, match="not a RIFF / AVI"):
        mjpeg_avi.MjpegAviReader(tmp_path / "frame.jpg")
    wavfile.write(str(tmp_path / "riff.wav"), 4000, np.zeros(100, np.int16))
    with pytest.raises(ValueError, match="not a RIFF / AVI"):
        mjpeg_avi.MjpegAviReader(tmp_path / "riff.wav")
    write_avi(tmp_path / "video.avi", jpegs(3))
    blob = bytearray((tmp_path / "video.avi").read_bytes())
    strf = blob.index(b"strf")
    assert blob[strf + 8 + 16 : strf + 8 + 20] == b"MJPG"
    blob[strf + 8 + 16 : strf + 8 + 20] = b"H264"
    (tmp_path / "h264.avi").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="only MJPG"):
        mjpeg_avi.MjpegAviReader(tmp_path / "h264.avi")


# ---- video_common ------------------------------------------------------------------------------------------------------
def test_reduce_fps_take_every() -> None:
    from gance_amd.video import video_common

    assert video_common.reduce_fps_take_every(60, 30) == 2
    assert video_common.reduce_fps_take_every(30, 30) is None
    assert video_common.reduce_fps_take_every(60, None) is None
    with pytest.raises(ValueError):
        video_common.reduce_fps_take_every(60, 25)


def test_frames_in_video_checks_before_a_device(tmp_path: Path, caplog) -> None:
    from gance_amd.video import video_common

    with pytest.raises(ValueError, match="Couldn't open video file"):
        video_common.frames_in_video(tmp_path / "missing.avi")
    (tmp_path / "frame.jpg").write_bytes(jpegs(1)[0])
    with pytest.raises(ValueError, match="Couldn't open video file"):
        video_common.frames_in_video(tmp_path / "frame.jpg")
    write_avi(tmp_path / "video.avi", jpegs(4), 30.0)
    with pytest.raises(NotImplementedError, match="bicubic"):
        video_common.frames_in_video(tmp_path / "video.avi", width_height=(64, 64))
    with pytest.raises(ValueError):
        video_common.frames_in_video(tmp_path / "video.avi", reduce_fps_to=25.0)
    with caplog.at_level("WARNING", logger="gance_amd"):
        result = video_common.frames_in_video(tmp_path / "video.avi", video_fps=60.0, width_height=(32, 32))
    assert "Override FPS of: 60.0 fps did not match the fps from the file of: 30.0 fps." in caplog.text
    assert (result.original_fps, result.total_frame_count, result.original_resolution) == (30.0, 4, (32, 32))
    assert result.original_resolution.width == 32


def test_jpeg_decode_op_has_a_fake_tensor_registration() -> None:
    """The frame size is in the bytes, so the fake output has two data-dependent extents."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv

    from gance_amd import torch_ops  # noqa: F401  pylint: disable=unused-import

    with FakeTensorMode(shape_env=ShapeEnv()):
        frames = torch.ops.gance.jpeg_decode(torch.empty((1000,), dtype=torch.uint8, device="cuda"), torch.empty((5,), dtype=torch.int64))
        assert frames.shape[0] == 4 and frames.shape[3] == 3 and frames.dtype == torch.uint8 and frames.device.type == "cuda"
