"""
GPU tests of the PNG encoder's match-search mode (torch.ops.gance.png_encode_lz, gance_amd/csrc/png_lz.hip): every file is
a standard PNG of its frame and never larger than torch.ops.gance.png_encode's; every segment inflates alone; flat and
repeating content is several times smaller; a frame's bytes do not depend on its batch; the Python surface above it.
The contents and shapes (those of tests/test_png_encode_gpu.py plus panel, repeat_rows and tiles) are in png_lz_ref.py.
"""

import hashlib
import io
import json
import zlib
from functools import lru_cache
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np
import pytest
import torch
from PIL import Image
from png_lz_ref import (
    CONTENTS, SEGMENT, SHAPES, content, four_segment_shape, panel, repeat_rows, segment_payloads, tiles, two_segment_square, zlib_per_segment,
)
from png_ref import filtered_rows, parse_png, scene

from gance_amd import hip_lib, network_file, synthesize_images, torch_ops  # noqa: F401  pylint: disable=unused-import
from gance_amd.hash_file import hash_file
from gance_amd.image_sources.still_image_common import read_image, write_image, write_images_device
from gance_amd.stylegan2 import spec as sg2_spec

pytestmark = pytest.mark.gpu


def encode_with(op, frames: np.ndarray) -> List[bytes]:  # type: ignore[no-untyped-def]
    """The files of frames [B, H, W, 3], through `op`."""
    data, offsets = op(torch.from_numpy(frames).cuda())
    offsets = offsets.cpu().numpy()
    assert offsets[0] == 0 and np.all(np.diff(offsets) > 0) and offsets[-1] <= data.numel()
    host = data[: int(offsets[-1])].cpu().numpy().tobytes()
    return [host[int(offsets[b]) : int(offsets[b + 1])] for b in range(len(frames))]


def encode_lz(frames: np.ndarray) -> List[bytes]:
    return encode_with(torch.ops.gance.png_encode_lz, frames)


def encode_huffman(frames: np.ndarray) -> List[bytes]:
    return encode_with(torch.ops.gance.png_encode, frames)


@lru_cache(maxsize=None)
def both_files(kind: str, shape: Tuple[int, int]) -> Tuple[bytes, bytes]:
    """(png_encode_lz's file, png_encode's file) of content(kind, *shape), encoded once for the tests that share them."""
    image = content(kind, *shape)
    return encode_lz(image[None])[0], encode_huffman(image[None])[0]


def check_file(file_bytes: bytes, image: np.ndarray) -> Tuple[np.ndarray, bytes]:
    """Every check of one file against its input; returns (the reference's filtered stream, the IDAT payload)."""
    height, width = image.shape[:2]
    parsed = parse_png(file_bytes)  # signature and every CRC
    assert parsed.header == dict(width=width, height=height, bit_depth=8, colour_type=2, compression=0, filter=0, interlace=0)
    kinds = [kind for kind, _ in parsed.chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"} and parsed.chunks[-1][1] == 0
    assert len(parsed.idat_sizes) == -(-height * (3 * width + 1) // SEGMENT) + 1  # one IDAT per segment and the Adler-32's
    assert parsed.payload[:2] == b"\x78\x01"
    stream = zlib.decompress(parsed.payload)  # checks the Adler-32
    assert len(stream) == height * (3 * width + 1)
    want, _ = filtered_rows(image)
    assert np.array_equal(np.frombuffer(stream, dtype=np.uint8), want)
    opened = Image.open(io.BytesIO(file_bytes))
    assert opened.mode == "RGB" and np.array_equal(np.asarray(opened), image)
    assert len(file_bytes) <= hip_lib.png_encode_lz_bounds(1, width, height)[1] == hip_lib.png_encode_bounds(1, width, height)[1]
    return want, parsed.payload


def check_segments_inflate_alone(file_bytes: bytes, stream: np.ndarray) -> None:
    """Each segment's payload in a fresh raw inflate gives its slice of the stream: a distance before the segment would raise."""
    payloads = segment_payloads(parse_png(file_bytes), file_bytes)
    assert len(payloads) == -(-len(stream) // SEGMENT)
    for index, payload in enumerate(payloads):
        inflater = zlib.decompressobj(-15)
        alone = inflater.decompress(payload)
        assert alone == stream[index * SEGMENT : (index + 1) * SEGMENT].tobytes(), index
        assert inflater.unused_data == b"" and inflater.eof == (index == len(payloads) - 1)


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda shape: f"{shape[0]}x{shape[1]}")
def test_file_is_a_png_of_the_frame_and_never_larger(shape: Tuple[int, int], kind: str) -> None:
    image = content(kind, *shape)
    with_matches, literal_only = both_files(kind, shape)
    stream, _ = check_file(with_matches, image)
    check_file(literal_only, image)
    check_segments_inflate_alone(with_matches, stream)
    assert len(with_matches) <= len(literal_only)
    if kind == "random" or (kind == "scene" and shape == (64, 64)):
        assert with_matches == literal_only  # matches do not pay (test_png_lz.py): byte for byte the literal-only file


def test_ramp_of_all_byte_values() -> None:
    image = content("ramp", 4, 300)
    assert len(np.unique(image)) == 256
    with_matches, literal_only = both_files("ramp", (4, 300))
    check_file(with_matches, image)
    assert 4 * len(with_matches) <= len(literal_only)


@pytest.mark.parametrize("kind", ["flat", "ramp", "repeat_rows", "panel"])
def test_segments_are_independent(kind: str) -> None:
    shapes = [(256, 256)] if kind == "panel" else [(two_segment_square(),) * 2, four_segment_shape()]
    for shape in shapes:
        image = content(kind, *shape)
        with_matches, literal_only = both_files(kind, shape)
        stream, _ = check_file(with_matches, image)
        check_segments_inflate_alone(with_matches, stream)
        assert len(stream) > SEGMENT and len(with_matches) < len(literal_only)


# (kind, shape, the file's size as a fraction of png_encode's file of the same frame, at most); zlib level 1 meets each
# with 2x or more to spare (test_png_lz.py)
BARS = [
    ("flat", (64, 64), 1 / 4), ("flat", (128, 128), 1 / 4), ("ramp", four_segment_shape(), 1 / 4), ("ramp", (4, 300), 1 / 4),
    ("panel", (256, 256), 1 / 4), ("repeat_rows", (64, 64), 1 / 2), ("repeat_rows", (128, 128), 1 / 2), ("tiles", (64, 64), 1 / 2),
]


@pytest.mark.parametrize("kind,shape,bar", BARS, ids=[f"{kind}-{shape[0]}x{shape[1]}" for kind, shape, _ in BARS])
def test_matches_are_there_and_used_well(kind: str, shape: Tuple[int, int], bar: float) -> None:
    with_matches, literal_only = both_files(kind, shape)
    check_file(with_matches, content(kind, *shape))
    print(f"png lz {kind} {shape}: {len(with_matches)} bytes, literal-only {len(literal_only)}, ratio {len(with_matches) / len(literal_only):.4f}")
    assert len(with_matches) <= bar * len(literal_only)


def test_alternating_rows_are_strictly_smaller() -> None:
    with_matches, literal_only = both_files("alternating", (64, 64))
    print(f"png lz alternating: {len(with_matches)} bytes, literal-only {len(literal_only)}")
    assert len(with_matches) < len(literal_only)


# payload / (zlib level 1 raw deflate + Z_SYNC_FLUSH of the same segments), measured on an MI355X; the payload also
# carries the 2-byte zlib header and the 4-byte Adler-32. Bytes: flat 64^2 101 / 173, ramp 502 / 894, panel 256^2
# 2086 / 2813, alternating 6377 / 5954, repeat_rows 64^2 1710 / 1716, tiles 64^2 2708 / 1091 (the tile's 48-byte repeat
# lies inside one search step, where only the distances 1, 2, 3, 4 and 6 are tried: zlib finds it, this parser finds a
# repeat of an earlier step instead, and only from the second step of a row of tiles on)
MEASURED_LZ_RATIO: Dict[str, float] = {
    "flat64": 0.5838, "ramp": 0.5615, "panel256": 0.7416, "alternating": 1.0710, "repeat_rows64": 0.9965, "tiles64": 2.4821,
}


def test_size_against_zlib_level_1() -> None:
    images = {
        "flat64": ("flat", (64, 64)), "ramp": ("ramp", four_segment_shape()), "panel256": ("panel", (256, 256)),
        "alternating": ("alternating", (64, 64)), "repeat_rows64": ("repeat_rows", (64, 64)), "tiles64": ("tiles", (64, 64)),
    }
    for name, (kind, shape) in images.items():
        with_matches, _ = both_files(kind, shape)
        want, payload = check_file(with_matches, content(kind, *shape))
        level_1, level_6 = zlib_per_segment(want.tobytes(), 1), zlib_per_segment(want.tobytes(), 6)
        ratio = len(payload) / level_1
        print(f"png lz size ratio {name}: payload {len(payload)} file {len(with_matches)} zlib level 1 {level_1} level 6 {level_6} ratio {ratio:.4f}")
        assert ratio <= MEASURED_LZ_RATIO[name] + 0.02, name


def test_a_frame_has_the_same_bytes_in_any_batch() -> None:
    frames = np.stack([panel(64), content("flat", 64, 64), tiles(64, 64), scene(64, 0), content("alternating", 64, 64)])
    together = encode_lz(frames)
    assert len({len(file_bytes) for file_bytes in together}) == 5  # five different compressed sizes
    for index, file_bytes in enumerate(together):
        check_file(file_bytes, frames[index])
        assert encode_lz(frames[index : index + 1]) == [file_bytes]
    assert encode_lz(frames[::-1].copy()) == together[::-1]
    assert encode_lz(frames) == together  # and from call to call
    data, offsets = torch.ops.gance.png_encode_lz(torch.from_numpy(frames).cuda())
    assert data.numel() == hip_lib.png_encode_lz_bounds(5, 64, 64)[1] and int(offsets[-1]) <= data.numel()


def test_op_checks_and_non_contiguous_input() -> None:
    frames = torch.from_numpy(np.stack([panel(48), scene(48, 4)])).cuda()
    torch.library.opcheck(torch.ops.gance.png_encode_lz.default, (frames,), test_utils=("test_schema", "test_faketensor"))
    wide = torch.from_numpy(panel(64)).cuda()
    view = wide[:, 5:38][None]  # [1, 64, 33, 3], rows strided
    assert not view.is_contiguous()
    data, offsets = torch.ops.gance.png_encode_lz(view)
    want_data, want_offsets = torch.ops.gance.png_encode_lz(view.contiguous())
    assert torch.equal(offsets, want_offsets) and torch.equal(data[: int(offsets[-1])], want_data[: int(offsets[-1])])
    check_file(data[: int(offsets[-1])].cpu().numpy().tobytes(), view[0].cpu().numpy())
    empty_data, empty_offsets = torch.ops.gance.png_encode_lz(frames[:0])
    assert empty_data.numel() == 0 and empty_offsets.tolist() == [0]
    with pytest.raises(ValueError):
        torch.ops.gance.png_encode_lz(torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda"))


def test_writers_take_the_compression(tmp_path: Path) -> None:
    frames = np.stack([panel(64), tiles(64, 64), scene(64, 0)])
    paths = [tmp_path / f"{index}.png" for index in range(3)]
    hashes = write_images_device(torch.from_numpy(frames).cuda(), paths, compression="matches")
    default_paths = [tmp_path / f"default_{index}.png" for index in range(3)]
    default_hashes = write_images_device(torch.from_numpy(frames).cuda(), default_paths)
    for index, path in enumerate(paths):
        assert np.array_equal(read_image(path), frames[index])
        assert hashes[index] == hash_file(path) == hashlib.md5(path.read_bytes()).hexdigest()
        assert path.read_bytes() == encode_lz(frames[index : index + 1])[0]
        assert default_paths[index].read_bytes() == encode_huffman(frames[index : index + 1])[0]  # the default keeps its bytes
        assert default_hashes[index] == hash_file(default_paths[index])
    assert paths[0].stat().st_size < default_paths[0].stat().st_size and paths[2].read_bytes() == default_paths[2].read_bytes()
    write_image(panel(33), tmp_path / "numpy.png", compression="matches")
    write_image(torch.from_numpy(panel(33)).cuda(), tmp_path / "tensor.png", compression="matches")
    write_image(panel(33), tmp_path / "numpy_default.png")
    assert (tmp_path / "numpy.png").read_bytes() == (tmp_path / "tensor.png").read_bytes() == encode_lz(panel(33)[None])[0]
    assert (tmp_path / "numpy_default.png").read_bytes() == encode_huffman(panel(33)[None])[0]
    assert np.array_equal(read_image(tmp_path / "numpy.png"), panel(33))


def test_images_from_network_with_matches(tmp_path: Path) -> None:
    resolution = 32
    networks = tmp_path / "networks"
    networks.mkdir()
    network_file.save_network(networks / "a_plain.pkl", resolution, sg2_spec.make_random_variables(resolution, seed=1))
    runs = {}
    for compression in ("huffman", "matches"):
        output = tmp_path / compression
        keywords = {} if compression == "huffman" else {"png_compression": "matches"}
        synthesize_images.images_from_network(str(networks), str(output), 0, 0, num_images=2, noise_seed=99, **keywords)
        runs[compression] = sorted(output.rglob("*.png"))
        assert len(runs[compression]) == 2
    for default_path, path in zip(runs["huffman"], runs["matches"]):
        assert default_path.name == path.name
        assert np.array_equal(read_image(path), read_image(default_path))
        assert path.stat().st_size <= default_path.stat().st_size
        with open(path.with_suffix(".json")) as file:
            assert json.load(file)["image_hash"] == hash_file(path) == hashlib.md5(path.read_bytes()).hexdigest()
        assert default_path.read_bytes() == encode_huffman(np.array(read_image(default_path))[None])[0]
