"""
Host restatement of the Motion-JPEG decoder (gance_amd/csrc/mjpeg_decode.hip) for the tests: a baseline 4:2:2 JFIF file to
RGB with libjpeg's default arithmetic (Huffman decode with EXTEND and restart intervals, jidctint.c jpeg_idct_islow with
the samples saturated as libjpeg-turbo's SIMD IDCT does, h2v1 fancy upsampling over the true chroma width, jdcolor.c
colour conversion), in numpy.
tests/test_mjpeg_decode.py holds it against PIL, pixel for pixel. Not collected by pytest.
"""

import io
import struct
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
from PIL import Image

ZIGZAG = [
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
]  # fmt: skip

# Annex K.3 (ITU-T T.81) Huffman tables: (code counts per length 1..16, symbols), for files without DHT
_AC_LUMA = (
    [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa",
)
_AC_CHROMA = (
    [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa",
)
ANNEX_K = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): (_AC_LUMA[0], list(bytes.fromhex(_AC_LUMA[1]))),
    (1, 1): (_AC_CHROMA[0], list(bytes.fromhex(_AC_CHROMA[1]))),
}


class Header(NamedTuple):
    """What the decoder needs from the segments before the entropy-coded data."""

    width: int
    height: int
    restart_interval: int
    scan_offset: int
    quant: List[np.ndarray]  # per component, natural order
    huffman: List[Tuple[Dict[Tuple[int, int], int], Dict[Tuple[int, int], int]]]  # per component (DC, AC): (length, code) -> symbol
    has_dht: bool


def _code_map(bits: List[int], values: List[int]) -> Dict[Tuple[int, int], int]:
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[(length, code)] = values[k]
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def parse_header(data: bytes) -> Header:
    """:raises ValueError: anything but baseline 8-bit 4:2:2 in one interleaved scan."""
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
            layout = [(body[6 + 3 * c + 1], body[6 + 3 * c + 2]) for c in range(components)]
            if precision != 8 or [s for s, _ in layout] != [0x21, 0x11, 0x11]:
                raise ValueError("not 8-bit 4:2:2")
            frame = (width, height, [q for _, q in layout])
        elif 0xC1 <= marker <= 0xCF and marker not in (0xC8, 0xCC):
            raise ValueError(f"SOF{marker - 0xC0}")
        elif marker == 0xDD:
            restart = struct.unpack(">H", body)[0]
        elif marker == 0xDA:
            if frame is None or body[0] != 3:
                raise ValueError("not one interleaved scan")
            has_dht = bool(huffman)
            if not has_dht:
                huffman = {key: _code_map(*table) for key, table in ANNEX_K.items()}
            tables = [(huffman[(0, body[2 + 2 * c] >> 4)], huffman[(1, body[2 + 2 * c] & 15)]) for c in range(3)]
            return Header(frame[0], frame[1], restart, at, [quant[q] for q in frame[2]], tables, has_dht)


class _Bits:
    """Bits of one restart segment, stuffing removed; zeros past its end."""

    def __init__(self, data: bytes) -> None:
        self.data, self.at = data.replace(b"\xff\x00", b"\xff"), 0

    def take(self, count: int) -> int:
        value = 0
        for _ in range(count):
            byte = self.data[self.at >> 3] if self.at >> 3 < len(self.data) else 0
            value = value << 1 | (byte >> (7 - (self.at & 7)) & 1)
            self.at += 1
        return value

    def symbol(self, codes: Dict[Tuple[int, int], int]) -> int:
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.take(1)
            if (length, code) in codes:
                return codes[(length, code)]
        raise ValueError("invalid Huffman code")


def _extend(value: int, size: int) -> int:
    return value - (1 << size) + 1 if size and value < 1 << (size - 1) else value


def decode_coefficients(data: bytes, header: Header) -> np.ndarray:
    """int64 [MCUs][4 (Y left, Y right, Cb, Cr)][64], natural order, not yet dequantised."""
    mcus = -(-header.width // 16) * -(-header.height // 8)
    scan = data[header.scan_offset :]
    segments, start, at = [], 0, 0
    while True:  # split at RSTn, stop at the first other marker
        at = scan.find(b"\xff", at)
        if at < 0 or at + 1 >= len(scan):
            segments.append(scan[start:])
            break
        follower = scan[at + 1]
        if 0xD0 <= follower <= 0xD7:
            segments.append(scan[start:at])
            start = at + 2
        elif follower not in (0x00, 0xFF):
            segments.append(scan[start:at])
            break
        at += 2 if follower != 0xFF else 1
    interval = header.restart_interval or mcus
    if len(segments) != -(-mcus // interval):
        raise ValueError("restart marker mismatch")
    out = np.zeros((mcus, 4, 64), np.int64)
    for index, segment in enumerate(segments):
        bits, predictors = _Bits(segment), [0, 0, 0]
        for mcu in range(index * interval, min(mcus, (index + 1) * interval)):
            for kind in range(4):
                c = max(0, kind - 1)
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


_FIX = dict(
    f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
    f2_053=16819, f2_562=20995, f3_072=25172,
)


def _idct_1d(d: np.ndarray, shift: int) -> np.ndarray:
    """jpeg_idct_islow along the last axis of int64 [..., 8], descaled by `shift` with rounding."""
    f = _FIX
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * f["f0_541"]
    tmp2, tmp3 = z1 - z3 * f["f1_847"], z1 + z2 * f["f0_765"]
    tmp0, tmp1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * f["f1_175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * f["f0_298"], tmp1 * f["f2_053"], tmp2 * f["f3_072"], tmp3 * f["f1_501"]
    z1, z2 = -z1 * f["f0_899"], -z2 * f["f2_562"]
    z3, z4 = -z3 * f["f1_961"] + z5, -z4 * f["f0_390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)
    return (out + (1 << (shift - 1))) >> shift


def saturate_limit(values: np.ndarray) -> np.ndarray:
    """Level shift and saturation to 0..255: libjpeg-turbo's SIMD islow IDCT (saturating packs), which is what PIL runs."""
    return np.clip(values + 128, 0, 255)


def table_limit(values: np.ndarray) -> np.ndarray:
    """
    jidctint.c's C path instead: sample_range_limit[value & 0x3FF], which wraps for |value| >= 512 (only for the test
    that tells the two apart: PIL does not follow it).
    """
    v = values & 0x3FF
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896)))


def decode(data: bytes, limit=saturate_limit, header: Optional[Header] = None) -> np.ndarray:
    """uint8 [height][width][3] RGB of one baseline 4:2:2 JFIF file."""
    header = header or parse_header(data)
    width, height = header.width, header.height
    mcu_cols, mcu_rows = -(-width // 16), -(-height // 8)
    coefficients = decode_coefficients(data, header)
    quant = np.stack([header.quant[0], header.quant[0], header.quant[1], header.quant[2]])
    blocks = (coefficients * quant).reshape(-1, 4, 8, 8)
    columns = _idct_1d(blocks.swapaxes(-1, -2), 11).swapaxes(-1, -2)  # columns first, descaled by CONST_BITS - PASS1_BITS
    samples = limit(_idct_1d(columns, 18)).reshape(mcu_rows, mcu_cols, 4, 8, 8)
    luma = samples[:, :, :2].transpose(0, 3, 1, 2, 4).reshape(mcu_rows * 8, mcu_cols * 16)[:height, :width]
    chroma_width = (width + 1) // 2
    rgb_chroma = []
    for kind in (2, 3):
        plane = samples[:, :, kind].transpose(0, 2, 1, 3).reshape(mcu_rows * 8, mcu_cols * 8)[:height, :chroma_width]
        up = np.empty((height, 2 * chroma_width), np.int64)
        up[:, 0::2] = (3 * plane + np.roll(plane, 1, axis=1) + 1) >> 2
        up[:, 1::2] = (3 * plane + np.roll(plane, -1, axis=1) + 2) >> 2
        up[:, 0], up[:, -1] = plane[:, 0], plane[:, -1]
        rgb_chroma.append(up[:, :width] - 128)
    cb, cr = rgb_chroma

    def fix(x: float) -> int:
        return int(x * 65536 + 0.5)

    red = luma + ((fix(1.40200) * cr + 32768) >> 16)
    green = luma + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    blue = luma + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([red, green, blue], -1), 0, 255).astype(np.uint8)


# ---- test images and files, shared by the CPU and the GPU tests ------------------------------------------------------
def noise(width: int, height: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, (height, width, 3)).astype(np.uint8)


def binary_grey_noise(width: int, height: int, seed: int) -> np.ndarray:
    return np.repeat(np.random.RandomState(seed).randint(0, 2, (height, width, 1)) * 255, 3, 2).astype(np.uint8)


def gradients(width: int, height: int) -> np.ndarray:
    across, down = np.linspace(0, 255, width), np.linspace(0, 255, height)
    return np.stack([np.add.outer(down, across) / 2, np.add.outer(255 - down, across) / 2, np.tile(across, (height, 1))], -1).astype(np.uint8)


def pil_jpeg(image: np.ndarray, quality: int, subsampling: int = 1, **options) -> bytes:
    buffer = io.BytesIO()
    Image.fromarray(image).save(buffer, format="JPEG", quality=quality, subsampling=subsampling, **options)
    return buffer.getvalue()


def pil_decode(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def without_dht(data: bytes) -> bytes:
    """The file with its DHT segments removed (the "AVI1" Motion-JPEG form)."""
    out, at = bytearray(data[:2]), 2
    while True:
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        if marker != 0xC4:
            out += data[at : at + 2 + length]
        at += 2 + length
        if marker == 0xDA:
            return bytes(out + data[at:])
