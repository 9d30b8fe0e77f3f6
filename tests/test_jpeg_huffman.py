"""
CPU tests of the JPEG encoder's "optimized" Huffman mode: the host restatement of libjpeg's optimize_coding
(tests/jpeg_huffman_ref.py) against the DHT segments of PIL's optimize=True files, its length limit and overflow on counts
no small frame gives, and the refusal of an unknown `jpeg_huffman` by both products before any device is touched.
"""

from fractions import Fraction

import numpy as np
import pytest

import jpeg_huffman_ref as ref
from gance_amd import noise_blend, projection_file_blend
from jpeg_decode_ref import decode_coefficients, gradients, noise, parse_header, pil_jpeg

WIDTH, HEIGHT = 96, 112
CONTENTS = {
    "noise": lambda: noise(WIDTH, HEIGHT, 5),
    "texture": lambda: ref.texture(WIDTH, HEIGHT, 6),
    "flat": lambda: ref.flat(WIDTH, HEIGHT),
    "ramp": lambda: gradients(WIDTH, HEIGHT),
}


def pil_optimized(image: np.ndarray, quality: int) -> bytes:
    return pil_jpeg(image, quality, subsampling=1, optimize=True, restart_marker_rows=1)


def counts_of(data: bytes) -> np.ndarray:
    header = parse_header(data)
    assert header.restart_interval == header.width // 16
    return ref.symbol_counts(decode_coefficients(data, header), header.restart_interval)


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
@pytest.mark.parametrize("content", sorted(CONTENTS))
def test_restatement_gives_pils_tables(content: str, quality: int) -> None:
    data = pil_optimized(CONTENTS[content](), quality)
    assert ref.tables_of_counts(counts_of(data)) == ref.dht_of(data)


def test_restatement_gives_pils_tables_past_16_bits() -> None:
    data = pil_optimized(ref.decaying_noise(384), 100)
    counts = counts_of(data)
    assert max(ref.merged_code_sizes(counts[1])) > 16  # the luma AC merge: the Annex K.3 step does real work here
    assert ref.tables_of_counts(counts) == ref.dht_of(data)


@pytest.mark.parametrize("depth", [17, 24, 32])
def test_fibonacci_counts_are_limited_to_16_bits(depth: int) -> None:
    counts = ref.fibonacci_counts(depth)
    assert max(ref.merged_code_sizes(counts)) == depth
    bits, values = ref.optimal_table(counts)
    assert len(bits) == 16 and sum(bits) == depth == len(values)
    assert sorted(values) == sorted(symbol for symbol in range(256) if counts[symbol])
    # a prefix code that leaves room for exactly one more code of the longest length: the all-ones code stays free
    longest = max(length for length in range(1, 17) if bits[length - 1])
    kraft = sum(Fraction(bits[length - 1], 1 << length) for length in range(1, 17))
    assert kraft == 1 - Fraction(1, 1 << longest)
    # more frequent symbols never get longer codes
    lengths = ref.code_lengths((bits, values))
    used = sorted(lengths, key=lambda symbol: counts[symbol])
    assert all(lengths[a] >= lengths[b] for a, b in zip(used, used[1:]))


def test_depth_33_overflows() -> None:
    counts = ref.fibonacci_counts(33)
    assert max(ref.merged_code_sizes(counts)) == 33
    assert ref.optimal_table(counts) is None


def test_equal_counts() -> None:
    # 256 symbols of 1000 and the reserved symbol of 1: the reserved one first merges with symbol 255 (the largest index
    # among the equal counts) into 1001, 254 symbols pair into 127 nodes of 2000, the last 1000 joins the 1001, and the
    # 128 nodes left form a full tree of 7 levels: 255 symbols at 8 bits, symbol 255 and the reserved one at 9
    bits, values = ref.optimal_table([1000] * 256)
    assert bits == [0] * 7 + [255, 1] + [0] * 7
    assert values == list(range(256))


def test_single_symbol() -> None:
    # one symbol and the reserved one merge once: one bit each, and the reserved one leaves
    counts = [0] * 256
    counts[0x31] = 7
    assert ref.optimal_table(counts) == ([1] + [0] * 15, [0x31])
    with pytest.raises(ValueError):
        ref.optimal_table([0] * 256)


def test_symbol_counts_of_a_known_block() -> None:
    # MCU 0: Y left DC 5 then zeros; Y right DC 5 (difference 0), AC 17 zeros then -3 then a zero tail; Cb, Cr all zero.
    # MCU 1: Y left DC 5, 62 zeros, then 1; Y right DC 5 and zeros
    coefficients = np.zeros((2, 4, 64), np.int64)
    zigzag = ref.ZIGZAG
    coefficients[0, 0, 0] = 5
    coefficients[0, 1, 0] = 5
    coefficients[0, 1, zigzag[18]] = -3
    coefficients[1, 0, 0] = 5  # the second MCU starts a new restart interval: category 3 again, not 0
    coefficients[1, 1, 0] = 5
    coefficients[1, 0, zigzag[63]] = 1  # no end-of-block symbol after the last coefficient
    counts = ref.symbol_counts(coefficients, 1)
    dc_luma, ac_luma, dc_chroma, ac_chroma = counts
    assert dc_luma[3] == 2 and dc_luma[0] == 2 and dc_luma.sum() == 4
    assert ac_luma[0xF0] == 1 + 3 and ac_luma[0x12] == 1 and ac_luma[0xE1] == 1 and ac_luma[0x00] == 3 and ac_luma.sum() == 9
    assert dc_chroma[0] == 4 and dc_chroma.sum() == 4 and ac_chroma[0x00] == 4 and ac_chroma.sum() == 4


BLEND_ARGUMENTS = dict(
    wav=["missing.wav"], output_path="missing.avi", network_paths=[], frames_to_visualize=None, output_fps=30.0, output_side_length=64,
    debug_path=None, debug_window=None, debug_side_length=None, alpha=0.25, fft_roll_enabled=True, fft_amplitude_range=(-5, 5),
    output_format="avi",
)


def test_unknown_jpeg_huffman_is_refused_without_a_device() -> None:
    with pytest.raises(ValueError, match="jpeg_huffman"):
        projection_file_blend.projection_file_blend_api(
            **BLEND_ARGUMENTS, projection_file_path="missing.npz", blend_depth=12, complexity_change_rolling_sum_window=None,
            complexity_change_threshold=None, phash_distance=None, bbox_distance=None, track_length=None, jpeg_huffman="optimised",
        )
    with pytest.raises(ValueError, match="jpeg_huffman"):
        noise_blend.noise_blend_api(**BLEND_ARGUMENTS, jpeg_huffman="smallest")
    stream_arguments = {key: BLEND_ARGUMENTS[key] for key in ("wav", "network_paths", "frames_to_visualize", "output_fps", "output_side_length", "alpha", "fft_roll_enabled", "fft_amplitude_range")}
    with pytest.raises(ValueError, match="jpeg_huffman"):
        next(projection_file_blend.projection_file_blend_frame_chunks(
            **stream_arguments, projection_file_path="missing.npz", blend_depth=12, jpeg_quality=90, jpeg_huffman="",
        ))
    with pytest.raises(ValueError, match="jpeg_huffman"):
        next(noise_blend.noise_blend_frame_chunks(**stream_arguments, jpeg_quality=90, jpeg_huffman="Standard"))
