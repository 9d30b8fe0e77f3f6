"""
Helpers of the PNG tests: the numpy restatement of the encoder's filter stage, a chunk parser that checks every CRC,
and the synthetic test image `scene`.
"""

import struct
import zlib
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def scene(side: int, seed: int) -> np.ndarray:
    """Gradients plus sigma = 3 noise, uint8 [side, side, 3]: the texture of network output."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:side, 0:side]
    red = x * 256.0 / side + 20 * np.sin(y / 30.0)
    green = y * 128.0 / side + x * 64.0 / side
    blue = 128 + 60 * np.cos((x + y) / 50.0)
    return np.clip(np.stack([red, green, blue], -1) + rs.randn(side, side, 3) * 3, 0, 255).astype(np.uint8)


def filtered_rows(image: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """
    (filtered stream uint8 [H * (3 W + 1)], filter type per row) of an RGB image [H, W, 3]: per row the PNG filter
    (None, Sub, Up, Average, Paeth; bpp 3; zeros above row 0 and left of column 0) with the smallest sum of
    |int8(filtered byte)|, ties to the lowest filter number.
    """
    height, width = image.shape[:2]
    rows = image.reshape(height, 3 * width).astype(np.int32)
    out = np.zeros((height, 3 * width + 1), dtype=np.uint8)
    previous = np.zeros(3 * width, dtype=np.int32)
    for y in range(height):
        x = rows[y]
        a = np.concatenate([np.zeros(3, np.int32), x[:-3]])[: 3 * width]
        b = previous
        c = np.concatenate([np.zeros(3, np.int32), b[:-3]])[: 3 * width]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        candidates = [x, x - a, x - b, x - ((a + b) >> 1), x - paeth]
        as_bytes = [(candidate & 0xFF).astype(np.uint8) for candidate in candidates]
        sums = [int(np.abs(candidate.view(np.int8).astype(np.int32)).sum()) for candidate in as_bytes]
        best = int(np.argmin(sums))  # the first of equal minima
        out[y, 0] = best
        out[y, 1:] = as_bytes[best]
        previous = x
    return out.reshape(-1), out[:, 0].copy()


class ParsedPng(NamedTuple):
    """What `parse_png` finds in a file."""

    header: Dict[str, int]  # the IHDR fields
    chunks: List[Tuple[bytes, int]]  # (type, data length) in file order
    idat_sizes: List[int]
    payload: bytes  # the IDAT data, concatenated: one zlib stream


def parse_png(data: bytes) -> ParsedPng:
    """Walk the chunks of a PNG file; asserts the signature, every CRC, and that nothing follows the last chunk."""
    assert data[:8] == SIGNATURE, "PNG signature"
    position, chunks, idat_sizes, payload, header = 8, [], [], [], {}
    while position < len(data):
        assert position + 12 <= len(data), "chunk cut short"
        (length,) = struct.unpack(">I", data[position : position + 4])
        kind = data[position + 4 : position + 8]
        body = data[position + 8 : position + 8 + length]
        assert len(body) == length, f"{kind!r} cut short"
        (crc,) = struct.unpack(">I", data[position + 8 + length : position + 12 + length])
        assert crc == zlib.crc32(kind + body), f"CRC of {kind!r} at {position}"
        chunks.append((kind, length))
        if kind == b"IHDR":
            names = ("width", "height", "bit_depth", "colour_type", "compression", "filter", "interlace")
            header = dict(zip(names, struct.unpack(">IIBBBBB", body)))
        elif kind == b"IDAT":
            idat_sizes.append(length)
            payload.append(body)
        position += 12 + length
    assert position == len(data)
    return ParsedPng(header, chunks, idat_sizes, b"".join(payload))


def huffman_only_bytes(filtered: np.ndarray, segment_bytes: int) -> int:
    """Sum over the segments of raw-deflate Z_HUFFMAN_ONLY + Z_SYNC_FLUSH of the filtered bytes: zlib's size of the same job."""
    total = 0
    stream = filtered.tobytes()
    for start in range(0, len(stream), segment_bytes):
        compressor = zlib.compressobj(zlib.Z_DEFAULT_COMPRESSION, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        total += len(compressor.compress(stream[start : start + segment_bytes]) + compressor.flush(zlib.Z_SYNC_FLUSH))
    return total
