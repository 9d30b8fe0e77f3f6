"""
CPU tests of the PNG encoder's C entries through hip_lib: every bad argument is refused before a device is touched, and
the bounds are the stored-block formula of the shape.
"""

import ctypes

import pytest

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
    return batch * (8 + 25 + 2 + segments * (12 + 5) + stream + (12 + 4) + 12)


def test_segment_size_fits_a_stored_block() -> None:
    assert 1 <= hip_lib.PNG_SEGMENT_BYTES <= 65535


def test_bounds_refuse_bad_arguments(library: ctypes.CDLL) -> None:
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    bounds = library.gance_png_encode_bounds
    for batch, width, height in [(0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8193, 8), (1, 8, 8193), (1, -3, 8)]:
        assert bounds(batch, width, height, ctypes.byref(workspace), ctypes.byref(capacity)) == INVALID, (batch, width, height)
    assert bounds(1, 8, 8, None, ctypes.byref(capacity)) == INVALID
    assert bounds(1, 8, 8, ctypes.byref(workspace), None) == INVALID
    for width, height in [(1, 1), (8192, 8192), (7, 1), (1, 5)]:
        assert bounds(1, width, height, ctypes.byref(workspace), ctypes.byref(capacity)) == 0
    with pytest.raises(ValueError):
        hip_lib.png_encode_bounds(1, 0, 8)
    assert library.gance_abi_version() == 6


def test_encode_refuses_bad_arguments_before_touching_a_device(library: ctypes.CDLL) -> None:
    workspace, capacity = hip_lib.png_encode_bounds(2, 33, 47)
    encode = library.gance_png_encode_u8
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
    arguments[5] = workspace - 1
    assert encode(*arguments) == INVALID and b"workspace" in library.gance_last_error()
    arguments = list(good)
    arguments[7] = capacity - 1
    assert encode(*arguments) == INVALID and b"capacity" in library.gance_last_error()
    with pytest.raises(ValueError):
        hip_lib.png_encode_device(FAKE, 2, 33, 47, FAKE, workspace - 1, FAKE, capacity, FAKE)


def test_bounds_grow_with_each_of_batch_width_and_height() -> None:
    base = hip_lib.png_encode_bounds(2, 100, 60)
    for larger in [(3, 100, 60), (2, 101, 60), (2, 100, 61)]:
        workspace, capacity = hip_lib.png_encode_bounds(*larger)
        assert workspace > base[0] and capacity > base[1], larger


@pytest.mark.parametrize("batch,width,height", [(1, 64, 64), (3, 64, 64), (1, 1, 1), (2, 47, 33), (1, 128, 128), (1, 8192, 8192)])
def test_capacity_is_the_stored_block_formula(batch: int, width: int, height: int) -> None:
    _, capacity = hip_lib.png_encode_bounds(batch, width, height)
    assert capacity >= stored_formula(batch, width, height)
    assert capacity == stored_formula(batch, width, height)  # and exactly that: the worst case is a formula of the shape
