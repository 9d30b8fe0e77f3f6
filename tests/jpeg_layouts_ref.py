"""
Host restatement of the Motion-JPEG decoder's four layouts (gance_amd/csrc/mjpeg_decode.hip, gance_jpeg_decode_layouts_u8):
a baseline JFIF file, 4:2:2, 4:2:0, 4:4:4 or grey, to RGB with libjpeg's default arithmetic, in numpy. The Huffman, IDCT,
saturation and colour pieces are those of tests/jpeg_decode_ref.py; the layouts' block order and jdsample.c's choice of
upsampler are stated here:
  4:4:4  none
  4:2:2  h2v1_fancy_upsample over the true chroma width cw = ceil(W / 2)
  4:2:0  h2v2_fancy_upsample over the true chroma plane cw x ceil(H / 2): the further row is r - 1 for output row 2r and
         r + 1 for 2r + 1, the row itself at the plane's top and bottom; s = 3 * near + far per column, then
         out[2x] = (3 s[x] + s[x - 1] + 8) >> 4 and out[2x + 1] = (3 s[x] + s[x + 1] + 7) >> 4, s[x] itself at the two ends
  both   plain replication when cw <= 2 (jdsample.c asks for downsampled_width > 2 before it picks a fancy upsampler)
  grey   the three channels are the luma sample; the component's sampling factors do not matter (T.81 A.2.2)
tests/test_mjpeg_layouts.py holds it against PIL, pixel for pixel. Not collected by pytest.
"""

import struct
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

from jpeg_decode_ref import ANNEX_K, ZIGZAG, _Bits, _code_map, _extend, _idct_1d, saturate_limit

LAYOUT_NAMES = ("4:2:2", "4:2:0", "4:4:4", "grey")  # the order of GANCE_JPEG_LAYOUT_*
# layout: (luma H, luma V, PIL's `subsampling` for it; grey is written from a one-channel image)
SHAPES = {"4:2:2": (2, 1, 1), "4:2:0": (2, 2, 2), "4:4:4": (1, 1, 0), "grey": (1, 1, None)}
_BY_SAMPLING = {(0x21, 0x11, 0x11): "4:2:2", (0x22, 0x11, 0x11): "4:2:0", (0x11, 0x11, 0x11): "4:4:4"}


class Header(NamedTuple):
    """What the decoder needs from the segments before the entropy-coded data."""

    layout: str
    width: int
    height: int
    restart_interval: int
    scan_offset: int
    quant: List[np.ndarray]  # per component, natural order
    huffman: List[Tuple[Dict[Tuple[int, int], int], Dict[Tuple[int, int], int]]]  # per component (DC, AC): (length, code) -> symbol
    has_dht: bool


def parse_header(data: bytes) -> Header:
    """:raises ValueError: anything but baseline 8-bit 4:2:2, 4:2:0, 4:4:4 or grey in one interleaved scan."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    at, quant, huffman, restart, frame = 2, {}, {}, 0, None
    while True:
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        body = data[at + 4 : at + 2 + length]
        at += 2 + length
        if marker == 0xDB:
            while body:
                if body[0] >> 4:
                    raise ValueError("16-bit DQT")
                table = np.zeros(64, np.int64)
                table[ZIGZAG] = list(body[1:65])
                quant[body[0] & 15] = table
                body = body[65:]
        elif marker == 0xC4:
            while body:
                bits = list(body[1:17])
                huffman[(body[0] >> 4, body[0] & 15)] = _code_map(bits, list(body[17 : 17 + sum(bits)]))
                body = body[17 + sum(bits) :]
        elif marker == 0xC0:
            precision, height, width, components = struct.unpack_from(">BHHB", body)
            factors = tuple(body[6 + 3 * c + 1] for c in range(components))
            layout = "grey" if components == 1 else _BY_SAMPLING.get(factors)
            if precision != 8 or layout is None:
                raise ValueError(f"not 8-bit 4:2:2, 4:2:0, 4:4:4 or grey: {factors}")
            frame = (layout, width, height, [body[6 + 3 * c + 2] for c in range(components)])
        elif 0xC1 <= marker <= 0xCF and marker not in (0xC8, 0xCC):
            raise ValueError(f"SOF{marker - 0xC0}")
        elif marker == 0xDD:
            restart = struct.unpack(">H", body)[0]
        elif marker == 0xDA:
            if frame is None or body[0] != len(frame[3]):
                raise ValueError("not one interleaved scan")
            has_dht = bool(huffman)
            if not has_dht:
                huffman = {key: _code_map(*table) for key, table in ANNEX_K.items()}
            tables = [(huffman[(0, body[2 + 2 * c] >> 4)], huffman[(1, body[2 + 2 * c] & 15)]) for c in range(len(frame[3]))]
            return Header(frame[0], frame[1], frame[2], restart, at, [quant[q] for q in frame[3]], tables, has_dht)


def block_components(layout: str) -> List[int]:
    """The component of each block of an MCU, in the order the file has them."""
    h, v, _ = SHAPES[layout]
    return [0] if layout == "grey" else [0] * (h * v) + [1, 2]


def mcu_grid(layout: str, width: int, height: int) -> Tuple[int, int]:
    """(MCU columns, MCU rows)."""
    h, v, _ = SHAPES[layout]
    return -(-width // (8 * h)), -(-height // (8 * v))


def restart_segments(scan: bytes) -> List[bytes]:
    """The entropy-coded data split at RSTn, up to the first other marker."""
    segments, start, at = [], 0, 0
    while True:
        at = scan.find(b"\xff", at)
        if at < 0 or at + 1 >= len(scan):
            segments.append(scan[start:])
            return segments
        follower = scan[at + 1]
        if 0xD0 <= follower <= 0xD7:
            segments.append(scan[start:at])
            start = at + 2
        elif follower not in (0x00, 0xFF):
            segments.append(scan[start:at])
            return segments
        at += 2 if follower != 0xFF else 1


def decode_coefficients(data: bytes, header: Header) -> np.ndarray:
    """int64 [MCUs][blocks per MCU][64], natural order, not yet dequantised."""
    components = block_components(header.layout)
    mcu_cols, mcu_rows = mcu_grid(header.layout, header.width, header.height)
    mcus = mcu_cols * mcu_rows
    segments = restart_segments(data[header.scan_offset :])
    interval = header.restart_interval or mcus
    if len(segments) != -(-mcus // interval):
        raise ValueError("restart marker mismatch")
    out = np.zeros((mcus, len(components), 64), np.int64)
    for index, segment in enumerate(segments):
        bits, predictors = _Bits(segment), [0, 0, 0]
        for mcu in range(index * interval, min(mcus, (index + 1) * interval)):
            for kind, c in enumerate(components):
                dc_codes, ac_codes = header.huffman[c]
                size = bits.symbol(dc_codes)
                predictors[c] += _extend(bits.take(size), size)
                out[mcu, kind, 0] = predictors[c]
                k = 1
                while k < 64:
                    symbol = bits.symbol(ac_codes)
                    run, size = symbol >> 4, symbol & 15
                    if size == 0:
                        if run != 15:
                            break
                        k += 16
                        continue
                    k += run
                    out[mcu, kind, ZIGZAG[k]] = _extend(bits.take(size), size)
                    k += 1
    return out


def _along_rows(s: np.ndarray, first: int, second: int, shift: int) -> np.ndarray:
    """The triangle filter along each row of `s`: even outputs lean on the left neighbour, odd on the right, the ends on themselves."""
    left, right = np.roll(s, 1, axis=1), np.roll(s, -1, axis=1)
    left[:, 0], right[:, -1] = s[:, 0], s[:, -1]
    up = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    up[:, 0::2] = (3 * s + left + first) >> shift
    up[:, 1::2] = (3 * s + right + second) >> shift
    return up


def upsample(plane: np.ndarray, layout: str, width: int, height: int) -> np.ndarray:
    """A chroma plane of its true size to [height][width], as jdsample.c does for the layout."""
    if layout == "4:4:4":
        return plane
    if plane.shape[1] <= 2:  # too narrow for the fancy upsamplers: replication
        rows = np.repeat(plane, 2, axis=0) if layout == "4:2:0" else plane
        return np.repeat(rows, 2, axis=1)[:height, :width]
    if layout == "4:2:2":
        up = _along_rows(plane, 1, 2, 2)
        up[:, 0], up[:, -1] = plane[:, 0], plane[:, -1]
        return up[:height, :width]
    above, below = np.roll(plane, 1, axis=0), np.roll(plane, -1, axis=0)
    above[0], below[-1] = plane[0], plane[-1]
    up = np.empty((2 * plane.shape[0], 2 * plane.shape[1]), np.int64)
    up[0::2] = _along_rows(3 * plane + above, 8, 7, 4)
    up[1::2] = _along_rows(3 * plane + below, 8, 7, 4)
    return up[:height, :width]


def decode(data: bytes, limit=saturate_limit) -> np.ndarray:
    """uint8 [height][width][3] RGB of one baseline JFIF file of one of the four layouts."""
    header = parse_header(data)
    layout, width, height = header.layout, header.width, header.height
    h, v, _ = SHAPES[layout]
    components = block_components(layout)
    mcu_cols, mcu_rows = mcu_grid(layout, width, height)
    coefficients = decode_coefficients(data, header)
    quant = np.stack([header.quant[c] for c in components])
    blocks = (coefficients * quant).reshape(-1, len(components), 8, 8)
    columns = _idct_1d(blocks.swapaxes(-1, -2), 11).swapaxes(-1, -2)  # columns first, descaled by CONST_BITS - PASS1_BITS
    samples = limit(_idct_1d(columns, 18)).reshape(mcu_rows, mcu_cols, len(components), 8, 8)
    # the Y blocks of an MCU in raster order: [mcu row][mcu col][block row][block col][y][x] -> rows, columns
    luma = samples[:, :, : h * v].reshape(mcu_rows, mcu_cols, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5)
    luma = luma.reshape(mcu_rows * v * 8, mcu_cols * h * 8)[:height, :width]
    if layout == "grey":
        return np.repeat(luma[..., None], 3, axis=2).astype(np.uint8)
    chroma_width, chroma_height = -(-width // h), -(-height // v)
    cb, cr = (
        upsample(samples[:, :, kind].transpose(0, 2, 1, 3).reshape(mcu_rows * 8, mcu_cols * 8)[:chroma_height, :chroma_width], layout, width, height) - 128
        for kind in (h * v, h * v + 1)
    )

    def fix(x: float) -> int:
        return int(x * 65536 + 0.5)

    red = luma + ((fix(1.40200) * cr + 32768) >> 16)
    green = luma + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    blue = luma + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([red, green, blue], -1), 0, 255).astype(np.uint8)


# ---- test files, shared by the CPU and the GPU tests -------------------------------------------------------------------
SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (4, 3), (3, 4), (5, 5), (15, 17), (16, 16), (17, 15), (17, 33), (33, 17), (31, 32), (48, 40)]
QUALITIES = (1, 50, 90, 100)


def layout_jpeg(image: np.ndarray, layout: str, quality: int, **options) -> bytes:
    """`image` [H][W][3] as a PIL-written file of `layout`; grey takes the first channel."""
    from jpeg_decode_ref import pil_jpeg

    if layout == "grey":
        import io

        from PIL import Image

        buffer = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(image[..., 0])).save(buffer, format="JPEG", quality=quality, **options)
        return buffer.getvalue()
    return pil_jpeg(image, quality, subsampling=SHAPES[layout][2], **options)


def with_luma_sampling(data: bytes, sampling: int) -> bytes:
    """The file with the sampling byte of its first component set to `sampling` (0x22, 0x12, 0x41, ...)."""
    at = data.index(b"\xff\xc0")
    return data[: at + 11] + bytes([sampling]) + data[at + 12 :]
