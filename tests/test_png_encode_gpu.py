"""
GPU tests of the PNG encoder (torch.ops.gance.png_encode): every file is a standard PNG whose chunk CRCs, zlib stream,
filtered bytes and pixels are checked against zlib, PIL and the numpy restatement of the filter stage; a frame's bytes do
not depend on its batch; the sizes stay under the stored-block bound and close to zlib's Huffman-only coding.
"""

import io
import zlib
from typing import Dict, List, Tuple

import numpy as np
import pytest
import torch
from PIL import Image
from png_ref import filtered_rows, huffman_only_bytes, parse_png, scene

from gance_amd import hip_lib, torch_ops  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

SEGMENT = hip_lib.PNG_SEGMENT_BYTES


def two_segment_square() -> int:
    """The smallest square whose filtered stream is two segments, the second short, with the cut inside a row (128 at 32 KiB)."""
    if SEGMENT == 32768:
        return 128  # 49 280 bytes
    side = 1
    while not (SEGMENT < side * (3 * side + 1) < 2 * SEGMENT and SEGMENT % (3 * side + 1) != 0):
        side += 1
    return side


def four_segment_shape() -> Tuple[int, int]:
    """An odd-width shape of four or more segments."""
    width = 211
    return -(-(3 * SEGMENT + 1) // (3 * width + 1)) + 1, width


SHAPES = [(1, 1), (1, 7), (5, 1), (3, 5), (16, 16), (33, 47), (64, 64), (two_segment_square(),) * 2, four_segment_shape()]
CONTENTS = ["scene", "random", "flat", "binary", "ramp", "alternating"]


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
    return alternating(height, width)


def encode(frames: np.ndarray) -> List[bytes]:
    """The files of frames [B, H, W, 3], through the op."""
    data, offsets = torch.ops.gance.png_encode(torch.from_numpy(frames).cuda())
    offsets = offsets.cpu().numpy()
    assert offsets[0] == 0 and np.all(np.diff(offsets) > 0) and offsets[-1] <= data.numel()
    host = data[: int(offsets[-1])].cpu().numpy().tobytes()
    return [host[int(offsets[b]) : int(offsets[b + 1])] for b in range(len(frames))]


def check_file(file_bytes: bytes, image: np.ndarray) -> Tuple[np.ndarray, bytes]:
    """Every check of one file against its input; returns (the reference's filtered stream, the IDAT payload)."""
    height, width = image.shape[:2]
    parsed = parse_png(file_bytes)  # signature and every CRC
    assert parsed.header == dict(width=width, height=height, bit_depth=8, colour_type=2, compression=0, filter=0, interlace=0)
    kinds = [kind for kind, _ in parsed.chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"} and parsed.chunks[-1][1] == 0
    stream = zlib.decompress(parsed.payload)  # checks the Adler-32
    assert len(stream) == height * (3 * width + 1)
    want, _ = filtered_rows(image)
    assert np.array_equal(np.frombuffer(stream, dtype=np.uint8), want)
    opened = Image.open(io.BytesIO(file_bytes))
    assert opened.mode == "RGB" and np.array_equal(np.asarray(opened), image)
    assert len(file_bytes) <= hip_lib.png_encode_bounds(1, width, height)[1]
    return want, parsed.payload


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda shape: f"{shape[0]}x{shape[1]}")
def test_file_is_a_png_of_the_frame(shape: Tuple[int, int], kind: str) -> None:
    image = content(kind, *shape)
    (file_bytes,) = encode(image[None])
    check_file(file_bytes, image)


def test_shapes_and_contents_cover_what_they_claim() -> None:
    """The inputs' own properties, by the reference: segment counts, a ramp through all values, rows of several filters."""
    side = two_segment_square()
    stream = side * (3 * side + 1)
    assert SEGMENT < stream < 2 * SEGMENT and SEGMENT % (3 * side + 1) != 0
    height, width = four_segment_shape()
    assert height * (3 * width + 1) > 3 * SEGMENT and width % 2 == 1
    assert len(np.unique(content("ramp", *four_segment_shape()))) == 211 and len(np.unique(content("ramp", 4, 300))) == 256
    assert len(set(filtered_rows(content("alternating", 64, 64))[1].tolist())) >= 3
    check_file(encode(content("ramp", 4, 300)[None])[0], content("ramp", 4, 300))


def test_a_frame_has_the_same_bytes_in_any_batch() -> None:
    frames = np.stack([content(kind, 64, 64) for kind in ("scene", "random", "flat", "binary", "alternating")])
    together = encode(frames)
    assert len({len(file_bytes) for file_bytes in together}) == 5  # five different compressed sizes
    for index, file_bytes in enumerate(together):
        check_file(file_bytes, frames[index])
        assert encode(frames[index : index + 1]) == [file_bytes]
    assert encode(frames[::-1].copy()) == together[::-1]
    data, offsets = torch.ops.gance.png_encode(torch.from_numpy(frames).cuda())
    assert data.numel() == hip_lib.png_encode_bounds(5, 64, 64)[1] and int(offsets[-1]) <= data.numel()


def test_sizes_that_hold_by_construction() -> None:
    (noise,) = encode(content("random", 64, 64)[None])
    assert len(noise) <= hip_lib.png_encode_bounds(1, 64, 64)[1]  # the stored fallback
    (still,) = encode(scene(64, 0)[None])
    # zlib's Huffman-only coding of the same filtered rows is 6543 bytes and PIL's file 6608: an encoder that only stores cannot pass
    assert len(still) < 9216  # 0.75 of raw


# payload / (zlib Z_HUFFMAN_ONLY + Z_SYNC_FLUSH of the same segments), measured on an MI355X; the payload also carries
# the 2-byte zlib header and the Adler-32, and its block headers send the code lengths without repeat codes:
# scene(64, 0) 6576 / 6543, scene(128, 1) 25112 / 25067, the alternating rows 6896 / 6891 bytes
MEASURED_RATIO: Dict[str, float] = {"scene64": 1.0050, "scene128": 1.0018, "alternating": 1.0007}


def test_size_against_zlib_huffman_only() -> None:
    images = {"scene64": scene(64, 0), "scene128": scene(128, 1), "alternating": content("alternating", 64, 64)}
    for name, image in images.items():
        (file_bytes,) = encode(image[None])
        want, payload = check_file(file_bytes, image)
        ratio = len(payload) / huffman_only_bytes(want, SEGMENT)
        print(f"png size ratio {name}: payload {len(payload)} file {len(file_bytes)} ratio {ratio:.4f}")
        assert ratio <= MEASURED_RATIO[name] + 0.02, name
        if name == "scene128":
            assert len(file_bytes) <= 25979  # PIL's default file of scene(128, 1)


def test_op_checks_and_non_contiguous_input() -> None:
    frames = torch.from_numpy(np.stack([scene(48, 3), scene(48, 4)])).cuda()
    torch.library.opcheck(torch.ops.gance.png_encode.default, (frames,), test_utils=("test_schema", "test_faketensor"))
    wide = torch.from_numpy(scene(64, 5)).cuda()
    view = wide[:, 5:38][None]  # [1, 64, 33, 3], rows strided
    assert not view.is_contiguous()
    data, offsets = torch.ops.gance.png_encode(view)
    want_data, want_offsets = torch.ops.gance.png_encode(view.contiguous())
    assert torch.equal(offsets, want_offsets) and torch.equal(data[: int(offsets[-1])], want_data[: int(offsets[-1])])
    check_file(data[: int(offsets[-1])].cpu().numpy().tobytes(), view[0].cpu().numpy())
    empty_data, empty_offsets = torch.ops.gance.png_encode(frames[:0])
    assert empty_data.numel() == 0 and empty_offsets.tolist() == [0]
    with pytest.raises(ValueError):
        torch.ops.gance.png_encode(torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda"))
