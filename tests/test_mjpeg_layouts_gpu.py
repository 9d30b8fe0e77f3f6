"""
GPU tests of the Motion-JPEG decoder's four layouts (gance_amd/csrc/mjpeg_decode.hip: 4:2:2, 4:2:0, 4:4:4, grey) through
torch.ops.gance.jpeg_decode_layouts and the video readers that call it. The bar everywhere is libjpeg itself: every decoded
frame equals PIL's decode of the same bytes, pixel for pixel.
"""

from pathlib import Path
from typing import List, Sequence

import numpy as np
import pytest
import torch

from gance_amd import hip_lib, torch_ops  # noqa: F401
from gance_amd.video import mjpeg_avi, video_common
from jpeg_decode_ref import binary_grey_noise, gradients, noise, pil_decode, without_dht
from jpeg_layouts_ref import LAYOUT_NAMES, QUALITIES, SIZES, layout_jpeg

pytestmark = pytest.mark.gpu

RESTARTS = ({}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1})


def pack(files: Sequence[bytes]):
    """(data on the device, offsets on the host) of files back to back."""
    offsets = np.zeros((len(files) + 1,), dtype=np.int64)
    offsets[1:] = np.cumsum([len(data) for data in files])
    data = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).cuda()
    return data, torch.from_numpy(offsets)


def decode_gpu(files: Sequence[bytes]) -> np.ndarray:
    return torch.ops.gance.jpeg_decode_layouts(*pack(files)).cpu().numpy()


def assert_equals_pil(got: np.ndarray, files: Sequence[bytes], what: str) -> None:
    assert got.shape[0] == len(files) and got.dtype == np.uint8
    for index, data in enumerate(files):
        want = pil_decode(data)
        assert got[index].shape == want.shape, (what, index)
        assert np.array_equal(got[index], want), f"{what} frame {index}: {int(np.abs(got[index].astype(int) - want).max())} LSB off"


def contents(width: int, height: int, seed: int) -> List[np.ndarray]:
    return [noise(width, height, seed), gradients(width, height), binary_grey_noise(width, height, seed + 1)]


def variants(width: int, height: int, layout: str, seed: int) -> List[bytes]:
    """Every quality, content and restart form of one (layout, size): one batch."""
    return [
        layout_jpeg(image, layout, quality, **restarts)
        for image in contents(width, height, seed) for quality in QUALITIES for restarts in RESTARTS
    ]  # fmt: skip


# ---- the size list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_qualities_contents_and_restarts(size, layout) -> None:
    """Chroma widths 1, 2 (replication) and 3 (fancy), odd heights, the MCU-row boundary at row 16; widths 16 and 48 take the
    16-byte stores, the others the byte path."""
    width, height = size
    files = variants(width, height, layout, seed=width * 64 + height)
    assert len(files) == 36
    assert_equals_pil(decode_gpu(files), files, f"{layout} {width}x{height}")


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("size", [(32, 24), (2064, 16), (31, 24), (33, 24)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_aligned_and_unaligned_stores(size, layout) -> None:
    """Widths 32 and 2064 (129 groups of 16 pixels a row) go out in 16-byte stores, 31 and 33 byte by byte; 16 and 17 are in
    the size list."""
    width, height = size
    files = [layout_jpeg(image, layout, 90, **restarts) for image in contents(width, height, 5) for restarts in ({}, {"restart_marker_rows": 1})]
    assert_equals_pil(decode_gpu(files), files, f"{layout} {width}x{height}")


@pytest.mark.parametrize("layout, restarts, segments", [("4:2:0", {"restart_marker_blocks": 1}, 65), ("grey", {"restart_marker_blocks": 1}, 260)])
def test_segment_counts_past_one_workgroup(layout, restarts, segments) -> None:
    """16 x 1040 with a restart per MCU: 65 segments of 4:2:0, 260 of grey, against the entropy kernel's 64 threads."""
    files = [layout_jpeg(image, layout, quality, **restarts) for image in contents(16, 1040, 9) for quality in (1, 90)]
    info = hip_lib.jpeg_parse_header_layouts(files[0]).info
    mcus = 65 if layout == "4:2:0" else 260
    assert info.restart_interval == 1 and -(-mcus // info.restart_interval) == segments
    assert_equals_pil(decode_gpu(files), files, f"{layout} 16x1040")


# ---- batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_pixels_do_not_depend_on_the_batch(layout) -> None:
    files = [layout_jpeg(image, layout, 50 + seed, restart_marker_rows=1) for seed in range(22) for image in contents(48, 40, seed)][:64]
    assert len(files) == 64
    target = files[63]
    want = pil_decode(target)
    assert np.array_equal(decode_gpu(files)[63], want)  # last of 64
    assert np.array_equal(decode_gpu([target])[0], want)  # alone
    assert np.array_equal(decode_gpu([target] + files[:4])[0], want)  # first of 5


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_optimised_and_standard_tables_in_one_batch_and_files_without_dht(layout) -> None:
    images = contents(33, 17, 3) + [noise(33, 17, 4) // 2]
    files = [layout_jpeg(image, layout, 60 + 10 * i, optimize=True) for i, image in enumerate(images)] + [layout_jpeg(images[0], layout, 75)]
    assert len({data[: data.index(b"\xff\xda")] for data in files}) == len(files)
    assert_equals_pil(decode_gpu(files), files, "optimize")
    files = [without_dht(layout_jpeg(image, layout, 85, restart_marker_blocks=3)) for image in images]
    assert hip_lib.jpeg_parse_header_layouts(files[0]).info.has_huffman_tables == 0
    assert_equals_pil(decode_gpu(files), files, "without DHT")


# ---- the narrow-width rule, for both entries ---------------------------------------------------------------------------------
def test_narrow_422_replicates_its_chroma_through_both_ops() -> None:
    """A chroma width of 2 (widths 3 and 4): libjpeg replicates instead of the fancy upsampling, and so do both ops."""
    for width in (3, 4):
        files = [layout_jpeg(image, "4:2:2", quality, **restarts) for image in contents(width, 5, width) for quality in QUALITIES for restarts in RESTARTS]
        assert_equals_pil(decode_gpu(files), files, f"jpeg_decode_layouts {width}x5")
        assert_equals_pil(torch.ops.gance.jpeg_decode(*pack(files)).cpu().numpy(), files, f"jpeg_decode {width}x5")


@pytest.mark.parametrize("size", [(48, 32), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_422_is_the_same_through_both_ops(size) -> None:
    files = variants(*size, "4:2:2", seed=21)
    strict = torch.ops.gance.jpeg_decode(*pack(files)).cpu().numpy()
    assert np.array_equal(decode_gpu(files), strict)
    assert_equals_pil(strict, files, "jpeg_decode")


# ---- saturation ------------------------------------------------------------------------------------------------------------
def test_noise_at_q1_that_leaves_the_range_limit_table() -> None:
    """The binary grey noise of tests/test_mjpeg_decode.py (seed 2252, 48 x 64, q 1) as 4:2:0 and as grey: PIL saturates."""
    image = binary_grey_noise(48, 64, 2252)
    for layout in ("4:2:0", "grey"):
        files = [layout_jpeg(image, layout, 1, restart_marker_rows=1), layout_jpeg(image, layout, 1)]
        assert_equals_pil(decode_gpu(files), files, f"q 1 binary noise {layout}")


# ---- bad input -------------------------------------------------------------------------------------------------------------
def test_a_truncated_420_frame_is_reported_and_leaves_its_neighbours_alone() -> None:
    """The middle frame's byte range is shortened by a third inside one buffer, so any over-read would land in the next
    frame's valid bytes: this checks the reporting, it does not set out to provoke a fault."""
    files = [layout_jpeg(image, "4:2:0", 90, restart_marker_rows=1) for image in contents(64, 64, 11)]
    cut = [files[0], files[1][: len(files[1]) * 2 // 3], files[2]]
    data, offsets = pack(cut)
    with pytest.raises(ValueError, match="frame 1: truncated"):
        torch.ops.gance.jpeg_decode_layouts(data, offsets)

    infos = (hip_lib.JpegFrameInfo * 3)()
    for info, blob in zip(infos, cut):
        hip_lib.jpeg_parse_header_layouts(blob, info)
    host_offsets = offsets.numpy()
    workspace_bytes = hip_lib.jpeg_decode_layouts_bounds(3, 64, 64, LAYOUT_NAMES.index("4:2:0"), int(host_offsets[-1]))
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((3, 64, 64, 3), dtype=torch.uint8, device="cuda")
    status = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    hip_lib.jpeg_decode_layouts_device(
        data.data_ptr(), host_offsets, infos, workspace.data_ptr(), workspace_bytes, out.data_ptr(), status.data_ptr(),
        torch.cuda.current_stream().cuda_stream,
    )
    assert status.cpu().tolist() == [0, 1, 0]
    host = out.cpu().numpy()
    assert np.array_equal(host[0], pil_decode(files[0])) and np.array_equal(host[2], pil_decode(files[2]))


def test_mixed_layouts_and_sizes_are_refused_by_the_op() -> None:
    good = layout_jpeg(noise(32, 32, 1), "4:2:0", 80)
    with pytest.raises(ValueError, match="frame 1 is grey, frame 0 is 4:2:0.*one layout"):
        decode_gpu([good, layout_jpeg(noise(32, 32, 1), "grey", 80)])
    with pytest.raises(ValueError, match="one size"):
        decode_gpu([good, layout_jpeg(noise(16, 32, 1), "4:2:0", 80)])
    with pytest.raises(ValueError, match="frame 1: .*progressive"):
        decode_gpu([good, layout_jpeg(noise(32, 32, 1), "4:2:0", 80, progressive=True)])


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["4:2:0", "grey"])
def test_video_readers_take_a_foreign_avi(tmp_path: Path, layout) -> None:
    """Eight PIL-written frames of 48 x 40 in an AVI, as a camera or a re-encode would leave them (no restart markers)."""
    files = [layout_jpeg(image, layout, 85) for seed in range(3) for image in contents(48, 40, seed)][:8]
    path = tmp_path / "foreign.avi"
    with mjpeg_avi.MjpegAviWriter(path, 48, 25.0, width=48, height=40) as writer:
        for data in files:
            writer.add_frame(data)
    want = [pil_decode(data) for data in files]
    video = video_common.frames_in_video(path)
    assert (video.original_fps, video.total_frame_count, video.original_resolution) == (25.0, 8, (48, 40))
    frames = list(video.frames)
    assert len(frames) == 8 and all(np.array_equal(frame, image) for frame, image in zip(frames, want))
    chunks = list(video_common.frames_in_video_device_chunks(path, frames_per_chunk=3))
    assert [tuple(chunk.shape) for chunk in chunks] == [(3, 40, 48, 3), (3, 40, 48, 3), (2, 40, 48, 3)]
    assert np.array_equal(torch.cat(chunks).cpu().numpy(), np.stack(want))
    if layout == "grey":
        assert all(np.array_equal(frame[..., 0], frame[..., 1]) and np.array_equal(frame[..., 0], frame[..., 2]) for frame in frames)
