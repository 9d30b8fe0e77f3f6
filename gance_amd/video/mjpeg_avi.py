"""
Motion-JPEG AVI with the song muxed in: what write_source_to_disk_forward + add_wavs_to_video
(gance/image_sources/video_common.py:67-79, 301-376) produce through ffmpeg, written here without it.

The frames arrive already encoded (JFIF byte strings, e.g. from torch.ops.gance.jpeg_encode) and stream to disk; only the
indices are held until `close()`. The layout is AVI 2.0 / OpenDML, because real outputs pass 1 GB:

    RIFF 'AVI '  LIST hdrl (avih, strl video {strh, strf, indx}, strl audio {strh, strf, indx}, LIST odml {dmlh})
                 LIST movi (00dc / 01wb chunks, then ix00 / ix01 for them)  idx1
    RIFF 'AVIX'  LIST movi (chunks, ix00 / ix01) ...

`indx` is a super index per stream pointing at the standard indices (`ix00`, `ix01`) of every RIFF segment; `idx1`
covers the first segment for AVI 1.0 readers; `dmlh` holds the total frame count. The audio is the input WAVs
concatenated (as add_wavs_to_video's ffmpeg concat does), stored as PCM (format tag 1) or IEEE float (3), in chunks of
about one second interleaved between the video frames.

`MjpegAviReader` reads such a file back (and other Motion-JPEG AVIs): frame locations from the OpenDML indices, or from
`idx1` when there are none; the JFIF bytes go to torch.ops.gance.jpeg_decode_layouts undecoded (gance_amd/video/video_common.py).
"""

import struct
from fractions import Fraction
from pathlib import Path
from typing import BinaryIO, Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
from scipy.io import wavfile

DEFAULT_SEGMENT_LIMIT = 1 << 30  # bytes per RIFF segment
SUPER_INDEX_ENTRIES = 256  # RIFF segments an `indx` has room for (256 GiB at the default limit)
_AVIF_HASINDEX = 0x10
_AVIIF_KEYFRAME = 0x10
_MAX_U32 = (1 << 32) - 1


def frame_rate_fraction(output_fps: float) -> Tuple[int, int]:
    """
    (dwRate, dwScale) of `output_fps` exactly as written: Fraction(str(fps)) (29.97 -> 2997 / 100).
    :raises ValueError: a rate that is not positive or whose terms do not fit in 32 bits.
    """
    rate = Fraction(str(output_fps))
    if rate <= 0 or rate.numerator > _MAX_U32 or rate.denominator > _MAX_U32:
        raise ValueError(f"frame rate {output_fps!r} = {rate} cannot be written as dwRate / dwScale in 32 bits")
    return rate.numerator, rate.denominator


def read_concatenated_wavs(paths: Sequence[Union[str, Path]]) -> Tuple[int, np.ndarray]:
    """
    (sample rate, samples [n] or [n, channels]) of the WAVs one after another, read without conversion.
    :raises ValueError: WAVs that differ in sample rate, channel count or sample type (the reference refuses mixed rates,
    music.read_wavs_scale_for_video), or a sample type AVI cannot carry.
    """
    rate, parts = None, []
    for path in paths:
        this_rate, data = wavfile.read(str(path))
        if data.dtype.kind not in "iuf":
            raise ValueError(f"{path}: unsupported sample type {data.dtype}")
        if parts and (this_rate != rate or data.dtype != parts[0].dtype or data.shape[1:] != parts[0].shape[1:]):
            raise ValueError(
                f"{path}: {this_rate} Hz {data.dtype} x {data.shape[1:] or 1} does not match the first WAV's "
                f"{rate} Hz {parts[0].dtype} x {parts[0].shape[1:] or 1}"
            )
        rate = this_rate
        parts.append(data)
    if not parts:
        raise ValueError("no WAV given")
    return int(rate), np.concatenate(parts)


def _chunk_header(fourcc: bytes, size: int) -> bytes:
    return fourcc + struct.pack("<I", size)


class MjpegAviWriter:  # pylint: disable=too-many-instance-attributes
    """
    `add_frame(jpeg_bytes)` in frame order, then `close()` (or use as a context manager). The file is complete only
    after `close()`.
    :param segment_limit: bytes per RIFF segment (default 1 GiB); a test can force many segments with a small one.
    :param width: :param height: (keyword only) frames that are not square, e.g. the debug video's row of panels; each
    defaults to `side`.
    """

    def __init__(  # pylint: disable=too-many-arguments
        self,
        path: Union[str, Path],
        side: int,
        output_fps: float,
        wavs: Optional[Sequence[Union[str, Path]]] = None,
        segment_limit: int = DEFAULT_SEGMENT_LIMIT,
        *,
        width: Optional[int] = None,
        height: Optional[int] = None,
    ) -> None:
        self._rate, self._scale = frame_rate_fraction(output_fps)
        self._width = int(side if width is None else width)
        self._height = int(side if height is None else height)
        self._segment_limit = int(segment_limit)
        self._audio: Optional[np.ndarray] = None
        self._audio_rate = 0
        if wavs:
            self._audio_rate, samples = read_concatenated_wavs(wavs)
            channels = 1 if samples.ndim == 1 else samples.shape[1]
            self._audio = np.ascontiguousarray(samples).reshape(-1, channels)
        self._file: BinaryIO = open(path, "wb")  # pylint: disable=consider-using-with
        self._frames = 0
        self._audio_written = 0  # sample frames
        self._max_chunk = {b"00dc": 0, b"01wb": 0}
        self._super: dict = {b"00dc": [], b"01wb": []}  # per stream: (offset of ix chunk, its size, duration)
        self._idx1: List[Tuple[bytes, int, int]] = []  # first segment: (fourcc, offset from 'movi', size)
        self._frames_in_first = 0
        self._write_headers()
        self._segment_index = 0
        self._open_segment()

    # ---- headers ----------------------------------------------------------------------------------------------
    def _audio_format(self) -> Tuple[int, int, int]:
        """(format tag, channels, bytes per sample)."""
        assert self._audio is not None
        return (3 if self._audio.dtype.kind == "f" else 1), self._audio.shape[1], self._audio.dtype.itemsize

    def _write_headers(self) -> None:
        f = self._file
        f.write(b"RIFF\0\0\0\0AVI ")
        hdrl = f.tell()
        f.write(b"LIST\0\0\0\0hdrl")
        self._avih_at = f.tell() + 8
        f.write(_chunk_header(b"avih", 56) + bytes(56))
        self._strh_at, self._indx_at = {}, {}
        streams = [b"00dc"] + ([b"01wb"] if self._audio is not None else [])
        for fourcc in streams:
            strl = f.tell()
            f.write(b"LIST\0\0\0\0strl")
            self._strh_at[fourcc] = f.tell() + 8
            f.write(_chunk_header(b"strh", 56) + bytes(56))
            if fourcc == b"00dc":
                strf = struct.pack(
                    "<IiiHH4sIiiII", 40, self._width, self._height, 1, 24, b"MJPG", self._width * self._height * 3, 0, 0, 0, 0
                )
            else:
                tag, channels, width = self._audio_format()
                align = channels * width
                strf = struct.pack("<HHIIHHH", tag, channels, self._audio_rate, self._audio_rate * align, align, 8 * width, 0)
            f.write(_chunk_header(b"strf", len(strf)) + strf)
            self._indx_at[fourcc] = f.tell()
            size = 24 + 16 * SUPER_INDEX_ENTRIES
            f.write(_chunk_header(b"indx", size) + bytes(size))
            self._patch_size(strl)
        odml = f.tell()
        f.write(b"LIST\0\0\0\0odml")
        self._dmlh_at = f.tell() + 8
        f.write(_chunk_header(b"dmlh", 248) + bytes(248))
        self._patch_size(odml)
        self._patch_size(hdrl)
        self._streams = streams

    def _patch_size(self, start: int) -> None:
        """Size field of the chunk / list that starts at `start`, from the current end of the file."""
        end = self._file.tell()
        self._file.seek(start + 4)
        self._file.write(struct.pack("<I", end - start - 8))
        self._file.seek(end)

    # ---- segments -----------------------------------------------------------------------------------------------
    def _open_segment(self) -> None:
        f = self._file
        if self._segment_index > 0:
            self._riff_at = f.tell()
            f.write(b"RIFF\0\0\0\0AVIX")
        else:
            self._riff_at = 0
        self._movi_at = f.tell()
        f.write(b"LIST\0\0\0\0movi")
        self._entries: dict = {fourcc: [] for fourcc in self._streams}  # (offset of chunk data, size)

    def _index_overhead(self, extra_chunks: int) -> int:
        """Bytes the indices of the open segment will take if it gets `extra_chunks` more chunks."""
        count = sum(len(entries) for entries in self._entries.values()) + extra_chunks
        overhead = 8 * count + 32 * len(self._streams) + 8
        if self._segment_index == 0:
            overhead += 8 + 16 * count  # idx1
        return overhead

    def _close_segment(self) -> None:
        f = self._file
        for stream_number, fourcc in enumerate(self._streams):
            entries = self._entries[fourcc]
            if not entries:
                continue
            base = self._movi_at
            at = f.tell()
            ix = struct.pack("<HBBI4sQI", 2, 0, 1, len(entries), fourcc, base, 0)
            ix += b"".join(struct.pack("<II", offset - base, size) for offset, size in entries)
            f.write(_chunk_header(b"ix%02d" % stream_number, len(ix)) + ix)
            duration = len(entries) if fourcc == b"00dc" else sum(size for _, size in entries) // self._block_align()
            self._super[fourcc].append((at, len(ix) + 8, duration))
            if len(self._super[fourcc]) > SUPER_INDEX_ENTRIES:
                raise RuntimeError(f"more than {SUPER_INDEX_ENTRIES} RIFF segments: raise segment_limit")
        self._patch_size(self._movi_at)
        if self._segment_index == 0:
            self._frames_in_first = len(self._entries[b"00dc"])
            idx1 = b"".join(struct.pack("<4sIII", fourcc, _AVIIF_KEYFRAME, offset, size) for fourcc, offset, size in self._idx1)
            f.write(_chunk_header(b"idx1", len(idx1)) + idx1)
        self._patch_size(self._riff_at)
        self._segment_index += 1

    def _block_align(self) -> int:
        _, channels, width = self._audio_format()
        return channels * width

    def _write_chunk(self, fourcc: bytes, data: bytes) -> None:
        f = self._file
        size = len(data)
        padded = size + (size & 1)
        if any(self._entries.values()):  # (a segment always takes at least one chunk)
            if f.tell() - self._riff_at + 8 + padded + self._index_overhead(1) > self._segment_limit:
                self._close_segment()
                self._open_segment()
        at = f.tell()
        f.write(_chunk_header(fourcc, size))
        f.write(data)
        if size & 1:
            f.write(b"\0")
        self._entries[fourcc].append((at + 8, size))
        if self._segment_index == 0:
            self._idx1.append((fourcc, at - (self._movi_at + 8), size))
        self._max_chunk[fourcc] = max(self._max_chunk[fourcc], size)

    def _write_audio_until(self, sample_frames: int) -> None:
        """Audio chunks of at most one second until `sample_frames` sample frames are written (or the audio ends)."""
        if self._audio is None:
            return
        stop = min(sample_frames, self._audio.shape[0])
        while self._audio_written < stop:
            end = min(stop, self._audio_written + self._audio_rate)
            self._write_chunk(b"01wb", self._audio[self._audio_written : end].tobytes())
            self._audio_written = end

    # ---- public ---------------------------------------------------------------------------------------------------
    def add_frame(self, jpeg: Union[bytes, bytearray, memoryview, np.ndarray]) -> None:
        """The next frame, one JFIF file. Audio up to one second ahead of the video is interleaved before it."""
        data = jpeg.tobytes() if isinstance(jpeg, np.ndarray) else bytes(jpeg)
        if self._audio is not None:
            # one second of audio ahead of the frame's start time: written in one-second chunks at whole seconds
            seconds_ahead = self._frames * self._scale // self._rate + 1
            if self._audio_written < seconds_ahead * self._audio_rate:
                self._write_audio_until(seconds_ahead * self._audio_rate)
        self._write_chunk(b"00dc", data)
        self._frames += 1

    @property
    def frames_written(self) -> int:
        """Frames added so far."""
        return self._frames

    def close(self) -> None:
        """Rest of the audio, the last segment's indices, and every header field that depends on the totals."""
        if self._file.closed:
            return
        if self._audio is not None:
            self._write_audio_until(self._audio.shape[0])
        self._close_segment()
        f = self._file
        end = f.tell()
        micro = round(1e6 * self._scale / self._rate)
        max_bytes = max(self._max_chunk.values())
        f.seek(self._avih_at)
        f.write(
            struct.pack(
                "<IIIIIIIIII16x", micro, min(_MAX_U32, max_bytes * self._rate // self._scale + 1), 0, _AVIF_HASINDEX, self._frames_in_first, 0,
                len(self._streams), max_bytes, self._width, self._height,
            )
        )
        f.seek(self._strh_at[b"00dc"])
        f.write(
            struct.pack(
                "<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, self._scale, self._rate, 0, self._frames,
                self._max_chunk[b"00dc"], 0xFFFFFFFF, 0, 0, 0, self._width, self._height,
            )
        )
        if self._audio is not None:
            align = self._block_align()
            f.seek(self._strh_at[b"01wb"])
            f.write(
                struct.pack(
                    "<4s4sIHHIIIIIIIIhhhh", b"auds", b"\0\0\0\0", 0, 0, 0, 0, align, self._audio_rate * align, 0,
                    self._audio_written, self._max_chunk[b"01wb"], 0xFFFFFFFF, align, 0, 0, 0, 0,
                )
            )
        for fourcc in self._streams:
            entries = self._super[fourcc]
            f.seek(self._indx_at[fourcc] + 8)
            f.write(struct.pack("<HBBI4s12x", 4, 0, 0, len(entries), fourcc))
            for offset, size, duration in entries:
                f.write(struct.pack("<QII", offset, size, duration))
        f.seek(self._dmlh_at)
        f.write(struct.pack("<I", self._frames))
        f.seek(end)
        f.close()

    def __enter__(self) -> "MjpegAviWriter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class _Stream:  # pylint: disable=too-few-public-methods
    """What `hdrl` says about one stream."""

    def __init__(self) -> None:
        self.kind = b""
        self.scale, self.rate, self.length = 1, 0, 0
        self.format = b""
        self.super_index: Optional[bytes] = None


class MjpegAviReader:  # pylint: disable=too-many-instance-attributes
    """
    The frames (as JFIF byte strings) and the audio of a Motion-JPEG AVI, e.g. one `MjpegAviWriter` wrote. Frame locations
    come from the OpenDML indices (`indx` -> `ix00` of every RIFF segment), or from `idx1` (AVI 1.0: the first segment only)
    when the file has none. A context manager; `close()` releases the file.
    :raises ValueError: not a RIFF / AVI file, no video stream, a video stream that is not MJPG, a frame count (`dmlh`) that
    the index does not bear out, or a first frame of zero length.
    """

    def __init__(self, path: Union[str, Path]) -> None:
        self._path = Path(path)
        self._file: BinaryIO = open(self._path, "rb")  # pylint: disable=consider-using-with
        try:
            self._parse()
        except (struct.error, IndexError) as error:
            self._file.close()
            raise ValueError(f"{self._path}: damaged AVI headers ({error})") from None
        except Exception:
            self._file.close()
            raise

    # ---- RIFF ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _children(blob: bytes, at: int, end: int) -> Iterator[Tuple[bytes, int, int]]:
        """(fourcc, start of data, size) of the chunks in blob[at:end]."""
        while at + 8 <= end:
            fourcc, size = struct.unpack_from("<4sI", blob, at)
            yield fourcc, at + 8, size
            at += 8 + size + (size & 1)

    def _parse(self) -> None:  # pylint: disable=too-many-locals,too-many-branches,too-many-statements
        f = self._file
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:] != b"AVI ":
            raise ValueError(f"{self._path} is not a RIFF / AVI file")
        riff_end = 8 + struct.unpack_from("<I", head, 4)[0]
        streams: List[_Stream] = []
        total_frames: Optional[int] = None
        movi_at: Optional[int] = None  # of the 'movi' fourcc: what idx1 offsets count from
        idx1: Optional[bytes] = None
        at = 12
        while at + 8 <= riff_end:
            f.seek(at)
            header = f.read(12)
            if len(header) < 8:
                break
            fourcc, size = struct.unpack_from("<4sI", header)
            if fourcc == b"LIST" and header[8:] == b"hdrl":
                blob = f.read(size - 4)
                for child, start, child_size in self._children(blob, 0, len(blob)):
                    if child != b"LIST":
                        continue
                    kind = blob[start : start + 4]
                    if kind == b"strl":
                        stream = _Stream()
                        for sub, sub_start, sub_size in self._children(blob, start + 4, start + child_size):
                            if sub == b"strh":
                                stream.kind = blob[sub_start : sub_start + 4]
                                stream.scale, stream.rate = struct.unpack_from("<II", blob, sub_start + 20)
                                stream.length = struct.unpack_from("<I", blob, sub_start + 32)[0]
                            elif sub == b"strf":
                                stream.format = blob[sub_start : sub_start + sub_size]
                            elif sub == b"indx":
                                stream.super_index = blob[sub_start : sub_start + sub_size]
                        streams.append(stream)
                    elif kind == b"odml":
                        for sub, sub_start, _ in self._children(blob, start + 4, start + child_size):
                            if sub == b"dmlh":
                                total_frames = struct.unpack_from("<I", blob, sub_start)[0]
            elif fourcc == b"LIST" and header[8:] == b"movi":
                movi_at = at + 8
            elif fourcc == b"idx1":
                f.seek(at + 8)
                idx1 = f.read(size)
            at += 8 + size + (size & 1)

        video = next((n for n, stream in enumerate(streams) if stream.kind == b"vids"), None)
        if video is None:
            raise ValueError(f"{self._path} has no video stream")
        strf = streams[video].format
        _, self.width, self.height, _, _, compression = struct.unpack_from("<IiiHH4s", strf)
        if compression.upper() != b"MJPG":
            raise ValueError(f"{self._path}: the video stream is {compression!r}, only MJPG (Motion-JPEG) can be read")
        self.height = abs(self.height)
        if streams[video].rate == 0 or streams[video].scale == 0:
            raise ValueError(f"{self._path}: frame rate {streams[video].rate} / {streams[video].scale}")
        self.fps_fraction = Fraction(streams[video].rate, streams[video].scale)
        self.fps = float(self.fps_fraction)

        chunks = self._indexed_chunks(streams[video], video, b"dc", movi_at, idx1)
        from_opendml = chunks is not None and self._has_super_index(streams[video])
        if chunks is None:
            raise ValueError(f"{self._path} has neither OpenDML indices nor idx1")
        self._frames: List[Tuple[int, int]] = []
        for offset, size in chunks:
            if size == 0:  # a dropped frame: the previous one shows again
                if not self._frames:
                    raise ValueError(f"{self._path}: the first frame has no data")
                self._frames.append(self._frames[-1])
            else:
                self._frames.append((offset, size))
        if from_opendml and total_frames is not None and total_frames != len(self._frames):
            raise ValueError(f"{self._path}: dmlh counts {total_frames} frames, the indices hold {len(self._frames)}")
        self.frame_count = len(self._frames)

        self._audio_format: Optional[Tuple[int, int, int, int]] = None  # tag, channels, rate, bits per sample
        self._audio_chunks: List[Tuple[int, int]] = []
        audio = next((n for n, stream in enumerate(streams) if stream.kind == b"auds"), None)
        if audio is not None:
            tag, channels, rate, _, _, bits = struct.unpack_from("<HHIIHH", streams[audio].format)
            self._audio_format = (tag, channels, rate, bits)
            self._audio_chunks = self._indexed_chunks(streams[audio], audio, b"wb", movi_at, idx1) or []

    @staticmethod
    def _has_super_index(stream: _Stream) -> bool:
        return stream.super_index is not None and len(stream.super_index) >= 24 and struct.unpack_from("<I", stream.super_index, 4)[0] > 0

    def _indexed_chunks(
        self, stream: _Stream, number: int, suffix: bytes, movi_at: Optional[int], idx1: Optional[bytes]
    ) -> Optional[List[Tuple[int, int]]]:
        """(offset of the data, size) of the stream's chunks in order, or None without any index."""
        f = self._file
        if self._has_super_index(stream):
            indx = stream.super_index
            assert indx is not None
            _, _, index_type, entries = struct.unpack_from("<HBBI", indx)
            chunks: List[Tuple[int, int]] = []
            if index_type == 1:  # the indx is itself a chunk index
                return self._standard_index(indx)
            for i in range(entries):
                offset, size, _ = struct.unpack_from("<QII", indx, 24 + 16 * i)
                f.seek(offset + 8)
                chunks += self._standard_index(f.read(size - 8))
            return chunks
        if idx1 is None or movi_at is None:
            return None
        wanted = b"%02d" % number + suffix
        entries = [struct.unpack_from("<4sIII", idx1, 16 * i) for i in range(len(idx1) // 16)]
        # offsets count from the 'movi' fourcc; some writers count from the start of the file instead
        base = movi_at
        if entries:
            f.seek(movi_at + entries[0][2])
            if f.read(4) != entries[0][0]:
                base = 0
        return [(base + offset + 8, size) for fourcc, _, offset, size in entries if fourcc == wanted]

    @staticmethod
    def _standard_index(body: bytes) -> List[Tuple[int, int]]:
        """AVISTDINDEX (without its chunk header): (offset of the data, size) per entry."""
        _, _, _, entries, _, base, _ = struct.unpack_from("<HBBI4sQI", body)
        return [
            (base + offset, size & 0x7FFFFFFF)  # bit 31: not a key frame
            for offset, size in (struct.unpack_from("<II", body, 24 + 8 * i) for i in range(entries))
        ]

    # ---- public ---------------------------------------------------------------------------------------------------
    def frame_sizes(self, first: int, count: int) -> List[int]:
        """Byte counts of frames [first, first + count)."""
        return [size for _, size in self._frames[first : first + count]]

    def read_frame_into(self, index: int, out: np.ndarray) -> None:
        """Frame `index`'s JFIF file into the uint8 array `out` of exactly its size (e.g. a slice of a pinned buffer)."""
        offset, size = self._frames[index]
        self._file.seek(offset)
        if self._file.readinto(memoryview(out)) != size:  # type: ignore[attr-defined]
            raise ValueError(f"{self._path}: frame {index} lies past the end of the file")

    def read_frame_bytes(self, first: int, count: int) -> List[bytes]:
        """The JFIF files of frames [first, first + count), one `bytes` each."""
        if first < 0 or count < 0 or first + count > self.frame_count:
            raise IndexError(f"frames [{first}, {first + count}) of {self.frame_count}")
        out = []
        for offset, size in self._frames[first : first + count]:
            self._file.seek(offset)
            data = self._file.read(size)
            if len(data) != size:
                raise ValueError(f"{self._path}: a frame lies past the end of the file")
            out.append(data)
        return out

    def read_audio(self) -> Optional[Tuple[int, np.ndarray]]:
        """(sample rate, samples [n] or [n, channels]) as `read_concatenated_wavs` gave them to the writer; None without audio."""
        if self._audio_format is None:
            return None
        tag, channels, rate, bits = self._audio_format
        kinds: Dict[Tuple[int, int], str] = {(1, 8): "u1", (1, 16): "<i2", (1, 32): "<i4", (1, 64): "<i8", (3, 32): "<f4", (3, 64): "<f8"}
        if (tag, bits) not in kinds:
            raise ValueError(f"{self._path}: audio format tag {tag} with {bits} bits per sample")
        parts = []
        for offset, size in self._audio_chunks:
            self._file.seek(offset)
            parts.append(self._file.read(size))
        samples = np.frombuffer(b"".join(parts), dtype=kinds[(tag, bits)])
        return rate, (samples.reshape(-1, channels) if channels > 1 else samples)

    def close(self) -> None:
        """Release the file."""
        self._file.close()

    def __enter__(self) -> "MjpegAviReader":
        return self

    def __exit__(self, *exc) -> None:
        self.close()
