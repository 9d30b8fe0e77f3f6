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


# ---- inputs that reach the limits of the three codes (tests/test_png_codes.py proves what they claim, without a GPU)


def by_magnitude(count: int) -> List[int]:
    """The byte values 0, 1, 255, 2, 254, ...: the residuals of smallest magnitude first."""
    return [0] + [value for step in range(1, 129) for value in (step, 256 - step)][: count - 1]


def image_of_residuals(residuals: np.ndarray) -> np.ndarray:
    """The image [H, W, 3] whose Sub-filtered rows are `residuals` [H, 3 W]: the sum along x of each channel, modulo 256."""
    height = residuals.shape[0]
    return (np.cumsum(residuals.reshape(height, -1, 3).astype(np.int64), axis=1) % 256).astype(np.uint8)


def residual_rows(counts: List[int], height: int, width: int, seed: int, extra_zeros: int = 0) -> np.ndarray:
    """
    uint8 [height, 3 width]: counts[k] times the k-th value of `by_magnitude`, shuffled, with `extra_zeros` zeros behind
    them. The caller has taken the rows' filter bytes out of the counts.
    """
    values = by_magnitude(len(counts))
    residuals = np.concatenate([np.full(count, value, dtype=np.uint8) for value, count in zip(values, counts)])
    np.random.RandomState(seed).shuffle(residuals)
    residuals = np.concatenate([residuals, np.zeros(extra_zeros, dtype=np.uint8)])
    assert len(residuals) == height * 3 * width, (len(residuals), height * 3 * width)
    return residuals.reshape(height, 3 * width)


FIBONACCI_SHAPE = (95, 100)  # one segment of 28 595 bytes


def fibonacci_image() -> np.ndarray:
    """
    One segment whose byte counts are twenty Fibonacci numbers, 1, 2, 3, 5 ... 10946 (sum 28 655), the most frequent on
    value 0: the 95 filter bytes (Sub: 1) come out of value 1's count, the other 60 bytes out of value 0's. With
    end-of-block 21 used symbols whose unrestricted Huffman code is 19 bits deep.
    """
    height, width = FIBONACCI_SHAPE
    series = [1, 2]
    while len(series) < 20:
        series.append(series[-1] + series[-2])
    counts = series[::-1]
    counts[1] -= height
    counts[0] -= sum(counts) - height * 3 * width
    return image_of_residuals(residual_rows(counts, height, width, seed=41))


FIBONACCI_FLAT_SHAPE = (108, 100)  # one segment of 32 508 bytes


def fibonacci_flat_image() -> np.ndarray:
    """
    For the match search: 60 rows of nineteen Fibonacci counts (1 ... 6765) above 48 rows of zeros, which the
    literal-only form pays a code each for and a match search takes as a few matches of distance 1. Few byte values with
    Fibonacci counts repeat their triples all the time, and the greedy parse's short matches then cost more than the zeros
    save; so each of the six largest counts is shared evenly among 16 byte values (the value 1, which the Sub filter bytes
    add to, is one of the first 16). The literal-only block is 17 bits deep. The block with matches is not deeper than 15
    (measured: 13): the length symbols' counts fall between the Fibonacci counts and pair with them.
    """
    height, width = FIBONACCI_FLAT_SHAPE
    rows, split, group = 60, 6, 16
    series = [1, 2]
    while len(series) < 19:
        series.append(series[-1] + series[-2])
    counts: List[int] = []
    for index, count in enumerate(series[::-1]):
        counts += [-(-count // group)] * group if index < split else [count]
    counts[1] -= rows
    counts[0] -= sum(counts) - rows * 3 * width
    return image_of_residuals(residual_rows(counts, height, width, seed=43, extra_zeros=(height - rows) * 3 * width))


DYADIC_SHAPE = (109, 100)  # 32 809 bytes: one whole segment and 41 bytes
DYADIC_PROFILE = {1: 1, 4: 3, 7: 34, 8: 8, 11: 13, 12: 21, 13: 5, 14: 2, 15: 112}  # code length: symbols; Kraft sum one


def dyadic_image() -> np.ndarray:
    """
    A first segment whose symbol counts are powers of two, 2^(15 - L) for the numbers of symbols per L of DYADIC_PROFILE
    (the last 15-bit place is end-of-block's), so that its Huffman code has exactly these lengths: 32 767 bytes, of which
    the segment's 109 filter bytes are 109 of value 1's 2048; the segment's one byte more is another 0. The 257 literal
    lengths and the one distance length then occur 58 (unused), 2, 3, 34, 8, 13, 21, 5, 2 and 112 times: a code-length
    histogram whose unrestricted code is 9 bits deep, over the limit of 7. The 41 bytes of the second segment are zeros.
    """
    height, width = DYADIC_SHAPE
    counts = [1 << (15 - length) for length, number in sorted(DYADIC_PROFILE.items()) for _ in range(number)][:-1]
    filter_bytes = -(-SEGMENT // (3 * width + 1))
    counts[1] -= filter_bytes
    counts[0] += 1
    assert sum(counts) == SEGMENT - filter_bytes
    return image_of_residuals(residual_rows(counts, height, width, seed=47, extra_zeros=height * (3 * width + 1) - SEGMENT))


def limit_inputs() -> List[Tuple[str, np.ndarray]]:
    """The inputs of tests/test_png_codes_gpu.py beyond SHAPES x CONTENTS; scene(256, 2) has a real segment of depth 16."""
    return [
        ("fibonacci", fibonacci_image()),
        ("fibonacci_flat", fibonacci_flat_image()),
        ("dyadic", dyadic_image()),
        ("scene256", scene(256, 2)),
    ]
