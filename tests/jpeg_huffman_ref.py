"""
Host restatement of libjpeg's optimize_coding for the tests of the JPEG encoder's "optimized" mode (gance_amd/csrc/mjpeg.hip):
the symbols a frame's blocks are coded with (jchuff.c htest_one_block) and the table built from their counts
(jpeg_gen_optimal_table: the merge with its chain walks, the Annex K.3 limit to 16 bits, the symbols ordered by code size),
written from the rule and not from the kernels. tests/test_jpeg_huffman.py holds it against the DHT segments of PIL's
optimize=True files. Not collected by pytest.
"""

import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from jpeg_decode_ref import ZIGZAG

# the order of the DHT segments in a file: (class 0 DC / 1 AC, table 0 luma / 1 chroma)
TABLE_ORDER = ((0, 0), (1, 0), (0, 1), (1, 1))
MAX_CODE_LENGTH = 32  # jchuff.c MAX_CLEN

Table = Tuple[List[int], List[int]]  # (codes per length 1..16, symbols in code order)


def symbol_counts(coefficients: np.ndarray, restart_interval: int) -> np.ndarray:
    """
    int64 [4][256] in TABLE_ORDER: how often each symbol codes `coefficients` [MCUs][4 (Y left, Y right, Cb, Cr)][64]
    (natural order, as jpeg_decode_ref.decode_coefficients returns them) with the DC predictors reset every
    `restart_interval` MCUs (0: never).
    """
    counts = np.zeros((4, 256), np.int64)
    zigzag = np.asarray(coefficients)[:, :, ZIGZAG]
    predictors = [0, 0, 0]
    for mcu in range(zigzag.shape[0]):
        if restart_interval and mcu % restart_interval == 0:
            predictors = [0, 0, 0]
        for kind in range(4):
            component = max(0, kind - 1)
            chroma = 1 if component else 0
            block = [int(v) for v in zigzag[mcu, kind]]
            counts[2 * chroma, abs(block[0] - predictors[component]).bit_length()] += 1
            predictors[component] = block[0]
            run = 0
            for value in block[1:]:
                if value == 0:
                    run += 1
                    continue
                while run > 15:
                    counts[2 * chroma + 1, 0xF0] += 1
                    run -= 16
                counts[2 * chroma + 1, (run << 4) | abs(value).bit_length()] += 1
                run = 0
            if run > 0:
                counts[2 * chroma + 1, 0x00] += 1
    return counts


def merged_code_sizes(counts: Sequence[int]) -> List[int]:
    """Code size of the 257 entries (256 = the reserved symbol) after jpeg_gen_optimal_table's merge, before any limit."""
    freq = [max(0, int(v)) for v in counts] + [1]
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, smallest = -1, None
        for i in range(257):  # `<=`: among equal counts the largest index wins
            if freq[i] and (smallest is None or freq[i] <= smallest):
                smallest, c1 = freq[i], i
        c2, smallest = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (smallest is None or freq[i] <= smallest):
                smallest, c2 = freq[i], i
        if c2 < 0:
            return codesize
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1


def optimal_table(counts: Sequence[int]) -> Optional[Table]:
    """
    (bits [16], values) of libjpeg's optimal table for `counts` [256]; None where the merge gives a code of more than 32
    bits (JERR_HUFF_CLEN_OVERFLOW). :raises ValueError: no symbol counted.
    """
    if not any(int(v) > 0 for v in counts):
        raise ValueError("no symbol counted")
    codesize = merged_code_sizes(counts)
    if max(codesize) > MAX_CODE_LENGTH:
        return None
    bits = [0] * (MAX_CODE_LENGTH + 1)
    for size in codesize:
        if size:
            bits[size] += 1
    for i in range(MAX_CODE_LENGTH, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    values = [symbol for size in range(1, MAX_CODE_LENGTH + 1) for symbol in range(256) if codesize[symbol] == size]
    return bits[1:17], values


def code_lengths(table: Table) -> Dict[int, int]:
    """symbol -> code length of a (bits, values) table."""
    bits, values = table
    lengths = [length for length in range(1, 17) for _ in range(bits[length - 1])]
    return dict(zip(values, lengths))


def dht_of(data: bytes) -> Dict[Tuple[int, int], Table]:
    """(class, table) -> (bits, values) of every table in the DHT segments in front of the file's first scan."""
    tables: Dict[Tuple[int, int], Table] = {}
    at = 2
    while True:
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        body = data[at + 4 : at + 2 + length]
        at += 2 + length
        if marker == 0xC4:
            while body:
                bits = list(body[1:17])
                tables[(body[0] >> 4, body[0] & 15)] = (bits, list(body[17 : 17 + sum(bits)]))
                body = body[17 + sum(bits) :]
        elif marker == 0xDA:
            return tables


def dht_range(data: bytes) -> Tuple[int, int]:
    """[begin, end) of the file's DHT segments, which must follow each other."""
    at, begin, end = 2, None, None
    while True:
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        if marker == 0xC4:
            if begin is None:
                begin = at
            elif end != at:
                raise ValueError("DHT segments apart")
            end = at + 2 + length
        elif marker == 0xDA:
            if begin is None:
                raise ValueError("no DHT")
            return begin, end
        at += 2 + length


# ---- frames and count vectors shared by the CPU and the GPU tests --------------------------------------------------------
def texture(width: int, height: int, seed: int) -> np.ndarray:
    """Two crossed waves per channel under mild noise: every run / size class gets some use."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:height, 0:width]
    waves = [128 + 70 * np.sin(x / (2.0 + c) + y / 5.0) + 40 * np.cos(y / (3.0 + c) - x / 7.0) for c in range(3)]
    return np.clip(np.stack(waves, -1) + rng.randint(-12, 13, (height, width, 3)), 0, 255).astype(np.uint8)


def flat(width: int, height: int, colour: Tuple[int, int, int] = (40, 120, 200)) -> np.ndarray:
    return np.broadcast_to(np.asarray(colour, np.uint8), (height, width, 3)).copy()


def decaying_noise(side: int, seed: int = 3) -> np.ndarray:
    """Noise of amplitude 127 exp(-10 y / side) around mid grey: at quality 100 its luma AC merge passes 16 bits (384^2: 17)."""
    rng = np.random.default_rng(seed)
    amplitude = 127 * np.exp(-10 * np.arange(side) / side)[:, None, None]
    return np.clip(128 + amplitude * rng.uniform(-1, 1, (side, side, 3)), 0, 255).astype(np.uint8)


def fibonacci_counts(depth: int) -> List[int]:
    """256 counts whose merge reaches exactly `depth` bits: `depth` symbols with the counts 1, 2, 3, 5, 8, ..."""
    series = [1, 2]
    while len(series) < depth:
        series.append(series[-1] + series[-2])
    counts = [0] * 256
    for index, value in enumerate(series[:depth]):
        counts[(3 * index + 1) % 256] = value
    return counts


def tables_of_counts(counts: np.ndarray) -> Dict[Tuple[int, int], Optional[Table]]:
    """`optimal_table` of each of the four count vectors of `symbol_counts`, keyed as `dht_of` keys them."""
    return {key: optimal_table(counts[index]) for index, key in enumerate(TABLE_ORDER)}
