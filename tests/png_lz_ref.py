"""
Helpers of the tests of the PNG encoder's match search (torch.ops.gance.png_encode_lz): zlib's size of the same job, the
contents with flat and repeating areas, the per-segment payloads of a parsed file, and the contents and shapes of
tests/test_png_encode_gpu.py, re-declared.
"""

import struct
import zlib
from typing import List, Tuple

import numpy as np
from png_ref import ParsedPng, scene

SEGMENT = 32768  # hip_lib.PNG_SEGMENT_BYTES (test_png_lz.py asserts it)


def zlib_per_segment(stream: bytes, level: int, segment_bytes: int = SEGMENT) -> int:
    """Sum over the segments of a fresh raw deflate at `level`, ended with Z_SYNC_FLUSH: zlib's size of the encoder's job."""
    total = 0
    for start in range(0, len(stream), segment_bytes):
        compressor = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
        total += len(compressor.compress(stream[start : start + segment_bytes]) + compressor.flush(zlib.Z_SYNC_FLUSH))
    return total


def panel(side: int) -> np.ndarray:
    """A plot panel: white, a one-pixel black box, a two-pixel coloured sine curve."""
    image = np.full((side, side, 3), 255, dtype=np.uint8)
    margin = side // 8
    image[margin, margin : side - margin] = 0
    image[side - margin - 1, margin : side - margin] = 0
    image[margin : side - margin, margin] = 0
    image[margin : side - margin, side - margin - 1] = 0
    x = np.arange(margin + 1, side - margin - 1)
    y = (side / 2 + (side / 4) * np.sin(x * (4 * np.pi / side))).astype(np.int64)
    for offset in (0, 1):
        image[np.clip(y + offset, 0, side - 1), x] = (31, 119, 180)
    return image


def repeat_rows(height: int, width: int, period: int) -> np.ndarray:
    """`period` random rows, cycled down the image."""
    rows = np.random.RandomState(23).randint(0, 256, (period, width, 3)).astype(np.uint8)
    return np.ascontiguousarray(rows[np.arange(height) % period])


def tiles(height: int, width: int, tile: int = 16) -> np.ndarray:
    """One random tile of `tile` x `tile` pixels, repeated in both directions."""
    one = np.random.RandomState(29).randint(0, 256, (tile, tile, 3)).astype(np.uint8)
    return np.ascontiguousarray(one[np.arange(height)[:, None] % tile, np.arange(width)[None, :] % tile])


def segment_payloads(parsed: ParsedPng, file_bytes: bytes) -> List[bytes]:
    """The IDAT chunks' data in file order: the first minus its two zlib header bytes, the 4-byte Adler-32 chunk left out."""
    position, bodies = 8, []
    while position < len(file_bytes):
        (length,) = struct.unpack(">I", file_bytes[position : position + 4])
        if file_bytes[position + 4 : position + 8] == b"IDAT":
            bodies.append(file_bytes[position + 8 : position + 8 + length])
        position += 12 + length
    assert [len(body) for body in bodies] == parsed.idat_sizes and len(bodies[-1]) == 4
    return [bodies[0][2:]] + bodies[1:-1]


# ---- the contents and shapes of tests/test_png_encode_gpu.py (a test module is not imported from)


def two_segment_square() -> int:
    """The smallest square whose filtered stream is two segments, the second short, with the cut inside a row."""
    return 128  # 49 280 bytes at 32 KiB


def four_segment_shape() -> Tuple[int, int]:
    """An odd-width shape of four or more segments."""
    width = 211
    return -(-(3 * SEGMENT + 1) // (3 * width + 1)) + 1, width


SHAPES = [(1, 1), (1, 7), (5, 1), (3, 5), (16, 16), (33, 47), (64, 64), (two_segment_square(),) * 2, four_segment_shape()]
CONTENTS = ["scene", "random", "flat", "binary", "ramp", "alternating", "panel", "repeat_rows", "tiles"]


def alternating(height: int, width: int) -> np.ndarray:
    """Rows in a cycle of four: noise, a copy of the row above (Up), a smooth horizontal gradient (Sub), small values (None)."""
    rs = np.random.RandomState(11)
    image = np.zeros((height, width, 3), dtype=np.uint8)
    for y in range(height):
        kind = y % 4
        if kind == 0:
            image[y] = rs.randint(0, 256, (width, 3))
        elif kind == 1:
            image[y] = image[y - 1]
        elif kind == 2:
            image[y] = ((np.arange(width)[:, None] * 2 + np.array([0, 40, 90])[None] + rs.randint(0, 2, (width, 3))) % 256).astype(np.uint8)
        else:
            image[y] = rs.randint(0, 3, (width, 3))
    return image


def content(kind: str, height: int, width: int) -> np.ndarray:
    rs = np.random.RandomState(7)
    if kind == "scene":
        return np.ascontiguousarray(scene(max(height, width), 0)[:height, :width])
    if kind == "random":
        return rs.randint(0, 256, (height, width, 3)).astype(np.uint8)
    if kind == "flat":
        return np.full((height, width, 3), 77, dtype=np.uint8)
    if kind == "binary":
        return (rs.randint(0, 2, (height, width, 3)) * 255).astype(np.uint8)
    if kind == "ramp":
        return np.ascontiguousarray(np.broadcast_to((np.arange(width) % 256).astype(np.uint8)[None, :, None], (height, width, 3)))
    if kind == "panel":
        return np.ascontiguousarray(panel(max(height, width, 8))[:height, :width])
    if kind == "repeat_rows":
        return repeat_rows(height, width, 8)
    if kind == "tiles":
        return tiles(height, width)
    return alternating(height, width)
