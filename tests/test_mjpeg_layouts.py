"""
CPU tests of the Motion-JPEG decoder's four layouts (4:2:2, 4:2:0, 4:4:4, grey): the numpy restatement
(tests/jpeg_layouts_ref.py) against PIL pixel for pixel, the header parser and the argument checks of the C entries (host
only), and the parser under the host sanitizers (tools/jpeg_header_check.hip). The kernels are tested on the GPU
(tests/test_mjpeg_layouts_gpu.py).
"""

import ctypes
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_decode_ref
import jpeg_layouts_ref as ref
from gance_amd import hip_lib
from jpeg_decode_ref import gradients, noise, pil_decode, without_dht
from jpeg_layouts_ref import LAYOUT_NAMES, QUALITIES, SIZES, layout_jpeg, with_luma_sampling

ROOT = Path(__file__).resolve().parents[1]
RESTARTS = ({}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}, {"optimize": True})


# ---- the restatement against PIL ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pil(size, layout) -> None:
    """Chroma widths 1, 2 (replication) and 3 (fancy), odd heights for the bottom edge, the MCU-row boundary at row 16."""
    width, height = size
    for name, image in (("noise", noise(width, height, width + height)), ("gradients", gradients(width, height))):
        for quality in QUALITIES:
            for restarts in RESTARTS:
                data = layout_jpeg(image, layout, quality, **restarts)
                assert ref.parse_header(data).layout == layout
                assert np.array_equal(ref.decode(data), pil_decode(data)), (name, quality, restarts)


def test_restatement_agrees_with_the_422_restatement_where_that_one_follows_pil() -> None:
    """Above a chroma width of 2 the two state the same rule; at widths 3 and 4 the older one does not give PIL's pixels."""
    for width, height in ((5, 5), (17, 33), (48, 40)):
        data = layout_jpeg(noise(width, height, 7), "4:2:2", 90)
        assert np.array_equal(ref.decode(data), jpeg_decode_ref.decode(data))
    narrow = [layout_jpeg(noise(width, 5, seed), "4:2:2", 90) for width in (3, 4) for seed in range(4)]
    assert all(np.array_equal(ref.decode(data), pil_decode(data)) for data in narrow)
    assert any(not np.array_equal(jpeg_decode_ref.decode(data), pil_decode(data)) for data in narrow)


def test_grey_decodes_the_same_whatever_its_sampling_factors() -> None:
    for width, height in ((5, 5), (17, 33), (48, 40)):
        data = layout_jpeg(noise(width, height, 3), "grey", 90, restart_marker_blocks=3)
        patched = with_luma_sampling(data, 0x22)
        assert patched != data and np.array_equal(pil_decode(patched), pil_decode(data))
        assert np.array_equal(ref.decode(patched), pil_decode(data))
        assert hip_lib.jpeg_parse_header_layouts(patched).layout == LAYOUT_NAMES.index("grey")


# ---- jpeg_parse_header_layouts -----------------------------------------------------------------------------------------
def test_layout_names_follow_the_enum() -> None:
    assert hip_lib.JPEG_LAYOUT_NAMES == LAYOUT_NAMES
    assert ctypes.sizeof(hip_lib.JpegFrameInfo) == ctypes.sizeof(hip_lib.JpegInfo) + 8
    assert hip_lib.JpegFrameInfo.info.offset == 0


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_parse_header_layouts_sizes_layout_and_restart_interval(layout) -> None:
    h, v, _ = ref.SHAPES[layout]
    for width, height, restarts, interval in (
        (64, 48, {"restart_marker_rows": 1}, -(-64 // (8 * h))), (17, 33, {"restart_marker_blocks": 3}, 3), (21, 50, {}, 0), (9, 2, {"optimize": True}, 0),
    ):
        data = layout_jpeg(noise(width, height, 1), layout, 75, **restarts)
        frame = hip_lib.jpeg_parse_header_layouts(data)
        info, want = frame.info, ref.parse_header(data)
        assert hip_lib.JPEG_LAYOUT_NAMES[frame.layout] == layout == want.layout and frame.reserved == 0
        assert (info.width, info.height, info.restart_interval, info.has_huffman_tables) == (width, height, interval, 1)
        sos = data.index(b"\xff\xda")
        assert info.scan_offset == sos + 2 + struct.unpack_from(">H", data, sos + 2)[0] == want.scan_offset
        assert info.scan_offset + info.scan_bytes == len(data)
        components = 1 if layout == "grey" else 3
        for c in range(components):
            assert list(info.quant[c]) == list(want.quant[c])
        for c in range(components, 3):  # grey: the rest are zero
            assert not any(info.quant[c]) and not any(bytes(info.huff_bits[c])) and not any(bytes(info.huff_values[c]))
    if layout == "4:2:2":  # the strict entry reads the same description
        strict = hip_lib.jpeg_parse_header(data)
        assert bytes(strict) == bytes(frame.info)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_parse_header_layouts_without_dht_fills_annex_k(layout) -> None:
    data = layout_jpeg(noise(32, 16, 2), layout, 50, restart_marker_rows=1)
    full, stripped = hip_lib.jpeg_parse_header_layouts(data), hip_lib.jpeg_parse_header_layouts(without_dht(data))
    assert (full.info.has_huffman_tables, stripped.info.has_huffman_tables) == (1, 0) and full.layout == stripped.layout
    assert bytes(stripped.info.huff_bits) == bytes(full.info.huff_bits) and bytes(stripped.info.huff_values) == bytes(full.info.huff_values)
    for c in range(1 if layout == "grey" else 3):
        for cls in range(2):
            bits, values = jpeg_decode_ref.ANNEX_K[(cls, min(c, 1))]
            assert list(stripped.info.huff_bits[c][cls]) == bits and list(stripped.info.huff_values[c][cls])[: len(values)] == values
    assert stripped.info.scan_bytes == full.info.scan_bytes and stripped.info.scan_offset < full.info.scan_offset


def over_subscribed(data: bytes) -> bytes:
    """Three codes of length 1 in the first DHT."""
    at = data.index(b"\xff\xc4")
    return data[: at + 5] + b"\x03" + data[at + 6 :]


def sixteen_bit_dqt(data: bytes) -> bytes:
    at = data.index(b"\xff\xdb")
    return data[: at + 4] + bytes([0x10 | data[at + 4]]) + data[at + 5 :]


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_parse_header_layouts_refuses_the_rest_by_name(layout) -> None:
    image = noise(32, 32, 4)
    good = layout_jpeg(image, layout, 80)
    cases = {
        "progressive": layout_jpeg(image, layout, 80, progressive=True),
        "cut short": good[: good.index(b"\xff\xda") - 20],
        "over-subscribed": over_subscribed(good),
        "16-bit DQT": sixteen_bit_dqt(good),
    }
    if layout != "grey":
        cases["4:4:0"] = with_luma_sampling(good, 0x12)
        cases["4:1:1"] = with_luma_sampling(good, 0x41)
        cases["x[12], 2x1, 1x1"] = good[: good.index(b"\xff\xc0") + 14] + b"\x21" + good[good.index(b"\xff\xc0") + 15 :]  # chroma factors
    for reason, data in cases.items():
        with pytest.raises(ValueError, match=reason):
            hip_lib.jpeg_parse_header_layouts(data)
    with pytest.raises(ValueError, match="SOI"):
        hip_lib.jpeg_parse_header_layouts(b"RIFF" + good)


def test_the_strict_parser_still_takes_422_alone() -> None:
    image = noise(32, 32, 4)
    hip_lib.jpeg_parse_header(layout_jpeg(image, "4:2:2", 80))
    for layout, words in (("4:2:0", "4:2:0; only 4:2:2"), ("4:4:4", "4:4:4; only 4:2:2"), ("grey", "grey .*only 4:2:2 colour is decoded")):
        with pytest.raises(ValueError, match=words):
            hip_lib.jpeg_parse_header(layout_jpeg(image, layout, 80))


# ---- bounds and argument checks, before a device -------------------------------------------------------------------------
def parsed(files):
    infos = (hip_lib.JpegFrameInfo * len(files))()
    for info, data in zip(infos, files):
        hip_lib.jpeg_parse_header_layouts(data, info)
    offsets = np.zeros(len(files) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(data) for data in files])
    return infos, offsets


def test_decode_layouts_entry_refuses_bad_arguments_before_a_device() -> None:
    """Host-only checks: no device is asked for (the pointers are never followed)."""
    image = noise(32, 16, 5)
    infos, offsets = parsed([layout_jpeg(image, "4:2:0", 80), layout_jpeg(image, "4:4:4", 80)])
    with pytest.raises(ValueError, match="frame 1 is 4:4:4, frame 0 is 4:2:0.*one layout"):
        hip_lib.jpeg_decode_layouts_device(16, offsets, infos, 16, 1 << 40, 16, 16)
    infos, offsets = parsed([layout_jpeg(image, "4:2:0", 80), layout_jpeg(noise(16, 16, 6), "4:2:0", 80)])
    with pytest.raises(ValueError, match="one size"):
        hip_lib.jpeg_decode_layouts_device(16, offsets, infos, 16, 1 << 40, 16, 16)
    for layout in LAYOUT_NAMES:
        infos, offsets = parsed([layout_jpeg(image, layout, 80)])
        need = hip_lib.jpeg_decode_layouts_bounds(1, 32, 16, LAYOUT_NAMES.index(layout), int(offsets[-1]))
        with pytest.raises(ValueError, match=f"workspace of {need - 1} bytes, {need} needed .*jpeg_decode_layouts_bounds"):
            hip_lib.jpeg_decode_layouts_device(16, offsets, infos, 16, need - 1, 16, 16)
        with pytest.raises(ValueError, match="scan range"):
            hip_lib.jpeg_decode_layouts_device(16, offsets + np.array([0, 7]), infos, 16, 1 << 40, 16, 16)
    for width, height, layout in ((0, 16, 0), (16, 8193, 1), (16, 16, 4), (16, 16, -1)):
        with pytest.raises(ValueError):
            hip_lib.jpeg_decode_layouts_bounds(1, width, height, layout, 1000)


def test_bounds_follow_the_layouts() -> None:
    """
    Grey < 4:4:4 at every size. 4:2:0 <= 4:2:2 where the height is a multiple of the 4:2:0 MCU's 16 rows: it has half the
    chroma and three quarters of the blocks; below that its MCU rows round the luma plane up further than 4:2:2's 8 do.
    The 4:2:2 workspace is the strict entry's.
    """
    index = {name: k for k, name in enumerate(LAYOUT_NAMES)}
    for batch, width, height in ((1, 1, 1), (1, 16, 16), (3, 17, 33), (2, 48, 32), (64, 1024, 1024), (1, 2160, 2160)):
        sizes = {name: hip_lib.jpeg_decode_layouts_bounds(batch, width, height, index[name], 1000) for name in LAYOUT_NAMES}
        assert sizes["grey"] < sizes["4:4:4"], (batch, width, height)
        assert sizes["4:2:2"] == hip_lib.jpeg_decode_bounds(batch, width, height, 1000)
        assert min(sizes.values()) > batch * width * height
        if width % 2 == 0 and height % 16 == 0:
            assert sizes["4:2:0"] <= sizes["4:2:2"], (batch, width, height)


# ---- the parser under the host sanitizers ----------------------------------------------------------------------------------
def test_colour_headers_pil_writes_differ_in_the_sampling_byte_alone() -> None:
    """What tools/jpeg_header_check.hip relies on to make its 4:2:0 and 4:4:4 headers from the 4:2:2 one."""
    image = gradients(8, 8)
    heads = {}
    for layout in LAYOUT_NAMES[:3]:
        data = layout_jpeg(image, layout, 75, restart_marker_blocks=1)
        heads[layout] = data[: ref.parse_header(data).scan_offset]
    assert with_luma_sampling(heads["4:2:2"], 0x22) == heads["4:2:0"] and with_luma_sampling(heads["4:2:2"], 0x11) == heads["4:4:4"]


def test_host_check_of_the_header_parser_under_the_sanitizers(tmp_path: Path) -> None:
    """
    tools/jpeg_header_check.hip, built as its header says (the host side with -fsanitize=address,undefined, errors fatal) and
    run: a stand-alone program on the CPU, no GPU touched. Measured: 2.0 s to build, 0.2 s to run.
    """
    program = tmp_path / "jpeg_header_check"
    build = [
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
        "-Xarch_host", "-fno-sanitize-recover=all", str(ROOT / "tools" / "jpeg_header_check.hip"), "-o", str(program),
    ]  # fmt: skip
    built = subprocess.run(build, capture_output=True, text=True, check=False)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(program)], capture_output=True, text=True, check=False)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "all checks passed" in ran.stdout
    for layout in LAYOUT_NAMES:
        assert f"{layout}: " in ran.stdout
