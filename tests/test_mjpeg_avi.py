"""
CPU tests of the Motion-JPEG AVI writer (gance_amd/video/mjpeg_avi.py) and of the argument checks of the GPU JPEG encoder's
C entry point. Frames come from PIL's own JPEG encoder; a small RIFF walker checks the OpenDML structure.
"""

import ctypes
import io
import struct
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np
import pytest
from PIL import Image
from scipy.io import wavfile

from gance_amd import hip_lib
from gance_amd.video import mjpeg_avi


# ---- RIFF walker ---------------------------------------------------------------------------------------------------
class Chunk:  # pylint: disable=too-few-public-methods
    """One chunk or list: fourcc, list type (None for a plain chunk), offset of the header, data offset, size, children."""

    def __init__(self, fourcc: bytes, offset: int, size: int, kind: bytes = None) -> None:
        self.fourcc, self.offset, self.size, self.kind = fourcc, offset, size, kind
        self.data_at = offset + 8
        self.children: List["Chunk"] = []

    def find(self, fourcc: bytes) -> List["Chunk"]:
        """Every descendant with this fourcc (or list type), depth first."""
        found = []
        for child in self.children:
            if child.fourcc == fourcc or child.kind == fourcc:
                found.append(child)
            found.extend(child.find(fourcc))
        return found


def walk(blob: bytes, start: int, end: int) -> List[Chunk]:
    """Chunks in blob[start:end]; every size must land exactly on `end`."""
    chunks, at = [], start
    while at < end:
        fourcc, size = blob[at : at + 4], struct.unpack_from("<I", blob, at + 4)[0]
        assert at + 8 + size <= end, f"{fourcc} at {at} overruns its parent"
        if fourcc in (b"RIFF", b"LIST"):
            chunk = Chunk(fourcc, at, size, blob[at + 8 : at + 12])
            chunk.children = walk(blob, at + 12, at + 8 + size)
        else:
            chunk = Chunk(fourcc, at, size)
        chunks.append(chunk)
        at += 8 + size + (size & 1)
    assert at == end, f"chunk sizes end at {at}, not {end}"
    return chunks


def parse(path: Path) -> Tuple[bytes, List[Chunk]]:
    blob = path.read_bytes()
    return blob, walk(blob, 0, len(blob))


def chunk_at(blob: bytes, data_at: int) -> Tuple[bytes, int]:
    """(fourcc, size) of the chunk whose data starts at `data_at`."""
    return blob[data_at - 8 : data_at - 4], struct.unpack_from("<I", blob, data_at - 4)[0]


def read_indices(blob: bytes, riffs: List[Chunk]) -> Dict[bytes, List[Tuple[int, int]]]:
    """Per stream, (data offset, size) of every chunk through indx -> ix00 / ix01, checked against the chunks they name."""
    hdrl = riffs[0].find(b"hdrl")[0]
    result = {}
    for indx in hdrl.find(b"indx"):
        longs, subtype, kind, count, chunk_id = struct.unpack_from("<HBBI4s", blob, indx.data_at)
        assert (longs, subtype, kind) == (4, 0, 0)
        entries = []
        for i in range(count):
            ix_at, ix_size, duration = struct.unpack_from("<QII", blob, indx.data_at + 24 + 16 * i)
            assert blob[ix_at : ix_at + 2] == b"ix" and struct.unpack_from("<I", blob, ix_at + 4)[0] + 8 == ix_size
            longs, subtype, kind, n, ix_chunk, base = struct.unpack_from("<HBBI4sQ", blob, ix_at + 8)
            assert (longs, kind, ix_chunk) == (2, 1, chunk_id)
            for j in range(n):
                offset, size = struct.unpack_from("<II", blob, ix_at + 32 + 8 * j)
                assert chunk_at(blob, base + offset) == (chunk_id, size & 0x7FFFFFFF)
                entries.append((base + offset, size & 0x7FFFFFFF))
            if chunk_id == b"00dc":
                assert duration == n
        result[chunk_id] = entries
    return result


def jpeg_frames(count: int, side: int = 32, seed: int = 0) -> List[bytes]:
    rs = np.random.RandomState(seed)
    frames = []
    for _ in range(count):
        buffer = io.BytesIO()
        Image.fromarray(rs.randint(0, 256, (side, side, 3)).astype(np.uint8)).save(buffer, format="JPEG", quality=75, subsampling=1)
        frames.append(buffer.getvalue())
    return frames


def write_avi(path: Path, frames: List[bytes], fps: float, wavs=None, segment_limit: int = mjpeg_avi.DEFAULT_SEGMENT_LIMIT) -> None:
    with mjpeg_avi.MjpegAviWriter(path, 32, fps, wavs=wavs, segment_limit=segment_limit) as writer:
        for frame in frames:
            writer.add_frame(frame)


# ---- tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_opendml_layout_and_contents(tmp_path: Path, dtype) -> None:
    rate, fps = 8000, 30.0
    rs = np.random.RandomState(1)
    pieces = []
    for i, seconds in enumerate((0.7, 1.9)):
        samples = rs.randint(-20000, 20000, (int(rate * seconds), 2)).astype(dtype)
        if dtype == np.float32:
            samples = (samples / 32768).astype(np.float32)
        wavfile.write(str(tmp_path / f"{i}.wav"), rate, samples)
        pieces.append(samples)
    frames = jpeg_frames(75)
    path = tmp_path / "out.avi"
    write_avi(path, frames, fps, wavs=[tmp_path / "0.wav", tmp_path / "1.wav"], segment_limit=64 * 1024)
    blob, top = parse(path)
    assert [chunk.kind for chunk in top][:1] == [b"AVI "] and all(chunk.kind == b"AVIX" for chunk in top[1:])
    assert len(top) >= 4, "a 64 KiB segment limit must give at least three AVIX segments"
    assert all(chunk.size + 8 <= 64 * 1024 for chunk in top[1:])
    dmlh = top[0].find(b"dmlh")[0]
    assert struct.unpack_from("<I", blob, dmlh.data_at)[0] == len(frames)

    # every frame and every audio chunk through the OpenDML indices, in order
    indices = read_indices(blob, top)
    video = [blob[at : at + size] for at, size in indices[b"00dc"]]
    assert video == frames
    audio = b"".join(blob[at : at + size] for at, size in indices[b"01wb"])
    assert audio == np.concatenate(pieces).tobytes()
    # the chunks in file order say the same
    movi_chunks = [chunk for riff in top for movi in riff.find(b"movi") for chunk in movi.children]
    assert [blob[c.data_at : c.data_at + c.size] for c in movi_chunks if c.fourcc == b"00dc"] == frames
    assert b"".join(blob[c.data_at : c.data_at + c.size] for c in movi_chunks if c.fourcc == b"01wb") == audio

    # idx1 of the first segment: offsets from the 'movi' fourcc
    movi0 = top[0].find(b"movi")[0]
    idx1 = [c for c in top[0].children if c.fourcc == b"idx1"][0]
    first_riff_chunks = [c for c in movi0.children if c.fourcc in (b"00dc", b"01wb")]
    assert idx1.size == 16 * len(first_riff_chunks)
    for i, chunk in enumerate(first_riff_chunks):
        fourcc, flags, offset, size = struct.unpack_from("<4sIII", blob, idx1.data_at + 16 * i)
        assert (fourcc, size) == (chunk.fourcc, chunk.size) and flags & 0x10
        assert movi0.offset + 8 + offset == chunk.offset

    # stream headers
    strf_audio = top[0].find(b"strl")[1].children[1]
    tag, channels, sample_rate, _, align, bits = struct.unpack_from("<HHIIHH", blob, strf_audio.data_at)
    assert (tag, channels, sample_rate, align, bits) == (3 if dtype == np.float32 else 1, 2, rate, 2 * np.dtype(dtype).itemsize, 8 * np.dtype(dtype).itemsize)
    strf_video = top[0].find(b"strl")[0].children[1]
    assert struct.unpack_from("<Iii", blob, strf_video.data_at) == (40, 32, 32)
    assert blob[strf_video.data_at + 16 : strf_video.data_at + 20] == b"MJPG"


@pytest.mark.parametrize("fps,rate,scale", [(60, 60, 1), (30.0, 30, 1), (29.97, 2997, 100), (23.976, 2997, 125)])
def test_frame_rate_is_exact(tmp_path: Path, fps, rate, scale) -> None:
    path = tmp_path / "out.avi"
    write_avi(path, jpeg_frames(3), fps)
    blob, top = parse(path)
    strh = top[0].find(b"strl")[0].children[0]
    assert blob[strh.data_at : strh.data_at + 8] == b"vidsMJPG"
    got_scale, got_rate = struct.unpack_from("<II", blob, strh.data_at + 20)
    assert (got_rate, got_scale) == (rate, scale)
    assert struct.unpack_from("<I", blob, strh.data_at + 32)[0] == 3  # dwLength


def test_single_segment_without_audio(tmp_path: Path) -> None:
    frames = jpeg_frames(5)
    path = tmp_path / "out.avi"
    write_avi(path, frames, 60)
    blob, top = parse(path)
    assert len(top) == 1 and len(top[0].find(b"strl")) == 1
    assert [blob[at : at + size] for at, size in read_indices(blob, top)[b"00dc"]] == frames


def test_rates_that_do_not_fit_are_refused(tmp_path: Path) -> None:
    with pytest.raises(ValueError):
        mjpeg_avi.MjpegAviWriter(tmp_path / "a.avi", 32, 1 / 3)  # 0.333...: a denominator past 32 bits
    with pytest.raises(ValueError):
        mjpeg_avi.frame_rate_fraction(0)


@pytest.mark.parametrize("second", ["rate", "channels", "dtype"])
def test_mismatched_wavs_are_refused(tmp_path: Path, second: str) -> None:
    first = np.zeros((800, 2), dtype=np.int16)
    other = {
        "rate": (16000, first),
        "channels": (8000, np.zeros(800, dtype=np.int16)),
        "dtype": (8000, np.zeros((800, 2), dtype=np.float32)),
    }[second]
    wavfile.write(str(tmp_path / "a.wav"), 8000, first)
    wavfile.write(str(tmp_path / "b.wav"), other[0], other[1])
    with pytest.raises(ValueError):
        mjpeg_avi.MjpegAviWriter(tmp_path / "out.avi", 32, 30, wavs=[tmp_path / "a.wav", tmp_path / "b.wav"])


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


def test_jpeg_encoder_rejects_bad_arguments_before_touching_a_device(library: ctypes.CDLL) -> None:
    """Fake device pointers: every case must be refused on the host, before any HIP call could see them."""
    workspace, capacity = hip_lib.jpeg_encode_bounds(2, 64)
    fake = 0x1000

    def encode(side=64, quality=90, workspace_bytes=workspace, out_capacity=capacity):
        return library.gance_jpeg_encode_u8(fake, 2, side, quality, fake, workspace_bytes, fake, out_capacity, fake, None)

    for status in (encode(side=100), encode(quality=0), encode(quality=101), encode(out_capacity=capacity - 1),
                   encode(workspace_bytes=workspace - 1)):
        assert status == 1  # GANCE_ERR_INVALID_ARGUMENT
    assert encode(out_capacity=10) == 1 and b"capacity" in library.gance_last_error()
    with pytest.raises(ValueError):
        hip_lib.jpeg_encode_bounds(1, 100)


def test_encoder_bounds_cover_the_worst_case_block() -> None:
    """1660 bits per block before stuffing (DC 16 + 11, 63 x AC 16 + 10), every byte 0xFF after: the capacity covers it."""
    side, batch = 64, 3
    _, capacity = hip_lib.jpeg_encode_bounds(batch, side)
    blocks = side * side // 32
    assert capacity >= batch * (blocks * 2 * 1660 // 8 + 2 * (side // 8))
