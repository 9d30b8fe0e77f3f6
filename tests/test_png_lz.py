"""
CPU tests of the PNG encoder's match-search mode: the C entries gance_png_encode_lz_bounds / gance_png_encode_lz_u8 refuse
every bad argument before a device is touched and keep the stored-block capacity; the Python surface refuses an unknown
compression without a device; and the inputs of tests/test_png_lz_gpu.py prove what they claim, by zlib alone.
"""

import ctypes
from pathlib import Path

import numpy as np
import pytest
from png_lz_ref import SEGMENT, content, four_segment_shape, panel, repeat_rows, tiles, zlib_per_segment
from png_ref import filtered_rows, huffman_only_bytes, scene

from gance_amd import hip_lib

INVALID = 1  # GANCE_ERR_INVALID_ARGUMENT
FAKE = 0x10000  # a non-NULL, 16-byte aligned "device pointer": every call below must return before it is looked at


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


def stored_formula(batch: int, width: int, height: int) -> int:
    """Signature, IHDR, the zlib header, one stored block in one IDAT per segment, the Adler-32 IDAT, IEND."""
    stream = height * (3 * width + 1)
    segments = -(-stream // hip_lib.PNG_SEGMENT_BYTES)
    return batch * (63 + 17 * segments + stream)


def test_bounds_refuse_bad_arguments(library: ctypes.CDLL) -> None:
    assert SEGMENT == hip_lib.PNG_SEGMENT_BYTES
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    bounds = library.gance_png_encode_lz_bounds
    for batch, width, height in [(0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8193, 8), (1, 8, 8193), (1, -3, 8)]:
        assert bounds(batch, width, height, ctypes.byref(workspace), ctypes.byref(capacity)) == INVALID, (batch, width, height)
    assert bounds(1, 8, 8, None, ctypes.byref(capacity)) == INVALID
    assert bounds(1, 8, 8, ctypes.byref(workspace), None) == INVALID
    for width, height in [(1, 1), (8192, 8192), (7, 1), (1, 5)]:
        assert bounds(1, width, height, ctypes.byref(workspace), ctypes.byref(capacity)) == 0
    with pytest.raises(ValueError):
        hip_lib.png_encode_lz_bounds(1, 0, 8)
    assert library.gance_abi_version() == 6


def test_encode_refuses_bad_arguments_before_touching_a_device(library: ctypes.CDLL) -> None:
    workspace, capacity = hip_lib.png_encode_lz_bounds(2, 33, 47)
    encode = library.gance_png_encode_lz_u8
    good = [FAKE, 2, 33, 47, FAKE, workspace, FAKE, capacity, FAKE, None]
    for position in (0, 4, 6, 8):  # frames, workspace, out, offsets
        arguments = list(good)
        arguments[position] = None
        assert encode(*arguments) == INVALID, position
        assert b"NULL" in library.gance_last_error()
    for position, value in [(1, 0), (1, -2), (2, 0), (2, 8193), (3, 0), (3, 8193)]:
        arguments = list(good)
        arguments[position] = value
        assert encode(*arguments) == INVALID, (position, value)
    arguments = list(good)
    arguments[4] = FAKE + 8  # misaligned workspace
    assert encode(*arguments) == INVALID and b"aligned" in library.gance_last_error()
    arguments = list(good)
    arguments[5] = workspace - 1
    assert encode(*arguments) == INVALID and b"workspace" in library.gance_last_error()
    arguments = list(good)
    arguments[5] = hip_lib.png_encode_bounds(2, 33, 47)[0]  # the other encoder's workspace is too small
    assert encode(*arguments) == INVALID and b"workspace" in library.gance_last_error()
    arguments = list(good)
    arguments[7] = capacity - 1
    assert encode(*arguments) == INVALID and b"capacity" in library.gance_last_error()
    with pytest.raises(ValueError):
        hip_lib.png_encode_lz_device(FAKE, 2, 33, 47, FAKE, workspace - 1, FAKE, capacity, FAKE)


def test_bounds_grow_with_each_of_batch_width_and_height() -> None:
    base = hip_lib.png_encode_lz_bounds(2, 100, 60)
    for larger in [(3, 100, 60), (2, 101, 60), (2, 100, 61)]:
        workspace, capacity = hip_lib.png_encode_lz_bounds(*larger)
        assert workspace > base[0] and capacity > base[1], larger


@pytest.mark.parametrize("batch,width,height", [(1, 64, 64), (3, 64, 64), (1, 1, 1), (2, 47, 33), (1, 128, 128), (1, 8192, 8192)])
def test_capacity_is_the_stored_block_formula_and_the_other_entrys(batch: int, width: int, height: int) -> None:
    workspace, capacity = hip_lib.png_encode_lz_bounds(batch, width, height)
    other_workspace, other_capacity = hip_lib.png_encode_bounds(batch, width, height)
    assert capacity == stored_formula(batch, width, height) == other_capacity
    segments = -(-height * (3 * width + 1) // SEGMENT)
    assert workspace == other_workspace + batch * segments * 4 * SEGMENT  # one 4-byte token per filtered byte


def test_python_refuses_an_unknown_compression_without_a_device(tmp_path: Path) -> None:
    from gance_amd import synthesize_images  # pylint: disable=import-outside-toplevel
    from gance_amd.image_sources import still_image_common  # pylint: disable=import-outside-toplevel

    image = np.zeros((4, 4, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="compression"):
        still_image_common.write_image(image, tmp_path / "a.png", compression="zip")
    with pytest.raises(ValueError, match="compression"):
        still_image_common.write_images_device(None, [tmp_path / "a.png"], compression="zip")  # type: ignore[arg-type]
    with pytest.raises(ValueError, match="compression"):
        synthesize_images.images_from_network(str(tmp_path), str(tmp_path / "out"), 0, 0, num_images=1, png_compression="zip")
    with pytest.raises(ValueError, match="compression"):
        synthesize_images.synthesis_file_into_networks(str(tmp_path), None, str(tmp_path), None, str(tmp_path / "out"), png_compression="zip")
    assert not list(tmp_path.iterdir())  # nothing written, no directory made


def segments_of(image: np.ndarray) -> int:
    return -(-image.shape[0] * (3 * image.shape[1] + 1) // SEGMENT)


# (name, image, segments, the bar tests/test_png_lz_gpu.py sets on the file as a fraction of png_encode's file)
def cases() -> list:
    return [
        ("flat64", content("flat", 64, 64), 1, 1 / 4),
        ("ramp4seg", content("ramp", *four_segment_shape()), 4, 1 / 4),
        ("ramp4x300", content("ramp", 4, 300), 1, 1 / 4),
        ("panel256", panel(256), 7, 1 / 4),
        ("repeat_rows64", repeat_rows(64, 64, 8), 1, 1 / 2),
        ("repeat_rows128", repeat_rows(128, 128, 8), 2, 1 / 2),
        ("tiles64", tiles(64, 64), 1, 1 / 2),
        ("tiles33x47", tiles(33, 47), 1, 1 / 2),
    ]


def test_inputs_compress_under_zlib_level_1_as_the_gpu_bars_demand() -> None:
    """zlib's greedy level 1 on the same segments meets every bar the GPU test sets, with room: the bars ask nothing zlib's
    comparable design point does not reach (measured 0.07 .. 0.16 of Huffman-only on the first seven)."""
    for name, image, segments, bar in cases():
        assert segments_of(image) == segments, name
        stream, _ = filtered_rows(image)
        level_1, level_6 = zlib_per_segment(stream.tobytes(), 1), zlib_per_segment(stream.tobytes(), 6)
        literal_only = huffman_only_bytes(stream, SEGMENT)
        print(f"{name}: Huffman-only {literal_only} zlib level 1 {level_1} level 6 {level_6} ratio {level_1 / literal_only:.3f}")
        assert level_1 <= bar * literal_only, name
        if name != "tiles33x47":
            assert level_1 <= 0.16 * literal_only, name
    stream, _ = filtered_rows(content("alternating", 64, 64))
    assert zlib_per_segment(stream.tobytes(), 1) < huffman_only_bytes(stream, SEGMENT)  # 5954 < 6891


def test_repeats_lie_where_the_cases_say() -> None:
    """repeat_rows repeats at 8 rows = 1544 bytes, in both segments of 128^2; tiles repeats at 48 bytes inside one search step."""
    stream, filters = filtered_rows(repeat_rows(64, 64, 8))
    row = 3 * 64 + 1
    assert 8 * row == 1544 and np.array_equal(stream[9 * row : 64 * row], stream[row : 56 * row])
    stream, _ = filtered_rows(repeat_rows(128, 128, 8))
    row = 3 * 128 + 1
    second = stream[SEGMENT:]
    assert SEGMENT % row != 0 and np.array_equal(second[8 * row :], second[: -8 * row])  # the second segment repeats by itself
    for shape in [(64, 64), (33, 47)]:
        image = tiles(*shape)
        assert np.array_equal(image[:, 16:], image[:, :-16]) and np.array_equal(image[16:], image[:-16]) and 3 * 16 == 48 < 256


def test_matches_do_not_pay_on_noisy_texture() -> None:
    """On these two zlib level 1 is not smaller than Huffman-only: the per-segment choice must fall back there."""
    for image in (scene(64, 0), content("random", 64, 64)):
        stream, _ = filtered_rows(image)
        assert zlib_per_segment(stream.tobytes(), 1) >= huffman_only_bytes(stream, SEGMENT)
