"""
CPU tests around the code builders of the two PNG encoders. The inputs with which tests/test_png_codes_gpu.py reaches the
limits of the three codes prove what they claim, by the restatements of tests/deflate_ref.py alone: Sub is every row's
filter, the segments' histograms are the intended ones, their unrestricted Huffman codes are deeper than the limits, and
the project's limiting rule stays within 0.1 % of the package-merge optimum on them. And the host check of the builders
themselves (tools/png_lz_codes_check.hip) is built under the address and undefined-behaviour sanitizers and run.
"""

import os
import subprocess
from pathlib import Path
from typing import List, Tuple

import deflate_ref as ref
import numpy as np
from png_lz_ref import (
    DYADIC_PROFILE, DYADIC_SHAPE, FIBONACCI_FLAT_SHAPE, FIBONACCI_SHAPE, SEGMENT, by_magnitude, dyadic_image, fibonacci_flat_image, fibonacci_image,
)
from png_ref import filtered_rows, scene

ROOT = Path(__file__).resolve().parents[1]


def segment_histograms(image: np.ndarray) -> List[List[int]]:
    """The literal histogram [257] of every segment of the image's filtered stream, end-of-block counted."""
    stream, _ = filtered_rows(image)
    histograms = []
    for start in range(0, len(stream), SEGMENT):
        histogram = np.bincount(stream[start : start + SEGMENT], minlength=257).tolist()
        histogram[256] = 1
        histograms.append(histogram)
    return histograms


def header_histogram(histogram: List[int]) -> List[int]:
    """How often each length 0 .. 18 occurs among the 257 literal lengths of the project's rule and the one distance length 1."""
    lengths = ref.limited_lengths(histogram, ref.LIT_LIMIT)
    sent = [lengths.get(symbol, 0) for symbol in range(257)] + [1]
    return [sent.count(length) for length in range(19)]


def margin(name: str, histogram: List[int], limit: int) -> Tuple[int, int, int]:
    """(unrestricted depth, the rule's cost, the package-merge optimum) at `limit`; asserts the rule within 0.1 % of the optimum."""
    depth, unrestricted = ref.huffman_depth_and_cost(histogram)
    rule, best = ref.cost(histogram, ref.limited_lengths(histogram, limit)), ref.package_merge_cost(histogram, limit)
    print(f"{name}: depth {depth} at a limit of {limit}, Huffman {unrestricted} bits, the rule {rule}, package-merge {best}: {rule - best} over")
    assert unrestricted <= best <= rule <= best * 1.001
    assert (unrestricted == best == rule) == (depth <= limit)
    return depth, rule, best


def test_fibonacci_segment_is_19_bits_deep() -> None:
    image = fibonacci_image()
    assert image.shape == FIBONACCI_SHAPE + (3,)
    stream, filters = filtered_rows(image)
    assert set(filters.tolist()) == {1} and len(stream) == 28595 < SEGMENT
    (histogram,) = segment_histograms(image)
    series = [1, 2]
    while len(series) < 20:
        series.append(series[-1] + series[-2])
    want = dict(zip(by_magnitude(20), series[::-1]))
    assert sum(series) == 28655 and want[0] == 10946
    want[0] -= 60  # the stream is 60 bytes short of the series' sum; the 95 filter bytes are 95 of value 1's 6765
    want[256] = 1
    assert {symbol: count for symbol, count in enumerate(histogram) if count} == want
    depth, rule, best = margin("fibonacci", histogram, ref.LIT_LIMIT)
    assert depth == 19 >= 17 and (rule, best) == (74911, 74885)
    assert ref.huffman_depth_and_cost(header_histogram(histogram))[0] <= ref.CL_LIMIT


def test_fibonacci_over_flat_rows_is_deep_and_has_long_runs() -> None:
    image = fibonacci_flat_image()
    assert image.shape == FIBONACCI_FLAT_SHAPE + (3,)
    stream, filters = filtered_rows(image)
    assert filters.tolist() == [1] * 60 + [0] * 48 and len(stream) == 32508 < SEGMENT
    assert not stream[60 * 301 :].any()  # 14 448 zeros: a few dozen matches at distance 1 for a match search
    (histogram,) = segment_histograms(image)
    assert sum(1 for count in histogram if count) == 6 * 16 + 13 + 1
    assert max(histogram[1:]) <= 6765 // 16 + 1  # no other byte value is one in 40 of the rows above: few chance repeats
    depth, _, _ = margin("fibonacci_flat", histogram, ref.LIT_LIMIT)
    assert depth == 17


def test_dyadic_segment_has_a_code_length_histogram_9_bits_deep() -> None:
    image = dyadic_image()
    assert image.shape == DYADIC_SHAPE + (3,)
    stream, filters = filtered_rows(image)
    assert set(filters.tolist()) == {1} and len(stream) == SEGMENT + 41
    first, second = segment_histograms(image)
    lengths = ref.huffman_depths(first)
    assert sorted(lengths.values()) == sorted(length for length, number in DYADIC_PROFILE.items() for _ in range(number))
    # every count a power of two, but for the segment's one byte more on value 0
    assert all(first[symbol] == (1 << (15 - length)) + (1 if symbol == 0 else 0) for symbol, length in lengths.items())
    assert ref.limited_lengths(first, ref.LIT_LIMIT) == lengths and margin("dyadic literals", first, ref.LIT_LIMIT)[0] == 15
    header = header_histogram(first)
    assert {length: count for length, count in enumerate(header) if count} == {0: 58, 1: 2, 4: 3, 7: 34, 8: 8, 11: 13, 12: 21, 13: 5, 14: 2, 15: 112}
    depth, rule, best = margin("dyadic code lengths", header, ref.CL_LIMIT)
    assert depth == 9 >= 8 and (rule, best) == (624, 624)
    assert [symbol for symbol, count in enumerate(second) if count] == [0, 256] and second[0] == 41


def test_scene_256_has_one_segment_of_depth_16_among_segments_of_depth_15() -> None:
    histograms = segment_histograms(scene(256, 2))
    assert len(histograms) == 7
    depths = [margin(f"scene(256, 2) segment {index}", histogram, ref.LIT_LIMIT) for index, histogram in enumerate(histograms)]
    assert [depth for depth, _, _ in depths] == [15, 16, 15, 15, 15, 15, 8]
    assert depths[1][1:] == (131045, 131041)
    for histogram in histograms:
        assert margin("its code lengths", header_histogram(histogram), ref.CL_LIMIT)[0] <= ref.CL_LIMIT
    # the contents the other GPU tests encode stay within the limit: nothing else in the suite reaches the repair
    for image in (scene(64, 0), scene(128, 1)):
        assert max(ref.huffman_depth_and_cost(histogram)[0] for histogram in segment_histograms(image)) <= ref.LIT_LIMIT


def test_host_check_of_the_code_builders_under_the_sanitizers(tmp_path: Path) -> None:
    """
    tools/png_lz_codes_check.hip, built as its header says (the host side with -fsanitize=address,undefined, errors fatal)
    and run: a stand-alone program on the CPU, no GPU touched. Measured: 6.2 s to build, 0.1 s to run.
    """
    program = tmp_path / "png_lz_codes_check"
    build = [
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
        "-Xarch_host", "-fno-sanitize-recover=all", str(ROOT / "tools" / "png_lz_codes_check.hip"), "-o", str(program),
    ]  # fmt: skip
    built = subprocess.run(build, capture_output=True, text=True, check=False)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(program)], capture_output=True, text=True, check=False)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "all checks passed" in ran.stdout and "Fibonacci byte counts" in ran.stdout and "dyadic literal profile" in ran.stdout
