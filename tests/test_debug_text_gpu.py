"""
GPU tests of the per-frame text kernel (gance_amd/csrc/debug_text.hip): bit-exact against font.draw_text applied in numpy
to a copy of the same random background, at sides 32 and 96 and scales 1 to 3, with every clip, in one call and split.
"""

from typing import List, Optional, Tuple

import numpy as np
import pytest
import torch

from gance_amd import hip_lib
from gance_amd.debug_video import font

pytestmark = pytest.mark.gpu

TEXT_STRIDE = 24
STRINGS: List[bytes] = [b"", b"A", b"frame: 3, step: 417", b"x" * TEXT_STRIDE, b"a\x07b\xc3c", b"~ {|} \\"]  # (the fourth has no NUL)
COLOUR = (200, 30, 90)
PANELS, PANEL = 3, 1


def encode(strings: List[bytes], stride: int) -> np.ndarray:
    out = np.zeros((len(strings), stride), dtype=np.uint8)
    for row, text in zip(out, strings):
        row[: len(text)] = np.frombuffer(text[:stride], dtype=np.uint8)
    return out


def as_drawn(text: bytes, stride: int) -> str:
    """What the kernel reads of a frame's bytes: up to the first NUL or the stride; draw_text turns the rest into '?' itself."""
    text = text[:stride].split(b"\0")[0]
    return "".join(chr(code) for code in text)


def background(side: int, batch: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, (batch, side, PANELS * side, 3)).astype(np.uint8)


def want_of(frames: np.ndarray, strings: List[bytes], stride: int, x: int, y: int, max_width: int, scale: int, side: int) -> np.ndarray:
    """font.draw_text on the panel of every frame, clipped to the panel and to the columns [x, x + max_width)."""
    want = frames.copy()
    for frame, text in zip(want, strings):
        panel = frame[:, PANEL * side : (PANEL + 1) * side]  # (a view)
        font.draw_text(panel[:, : min(side, x + max_width)], x, y, as_drawn(text, stride), COLOUR, scale)
    return want


def draw_gpu(  # pylint: disable=too-many-arguments
    frames: np.ndarray, strings: List[bytes], stride: int, x: int, y: int, max_width: int, scale: int, side: int,
    splits: Optional[Tuple[int, ...]] = None,
) -> np.ndarray:
    out = torch.from_numpy(frames).cuda()
    text = torch.from_numpy(encode(strings, stride)).cuda()
    begin = 0
    for count in splits or (len(strings),):
        rows = out[begin : begin + count]
        hip_lib.debug_draw_text_device(
            text.data_ptr() + begin * stride, stride, x, y, max_width, scale, COLOUR, side, count, rows.data_ptr() + PANEL * side * 3,
            rows.stride(0), rows.stride(1), torch.cuda.current_stream().cuda_stream,
        )
        begin += count
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("scale", [1, 2, 3])
@pytest.mark.parametrize("side", [32, 96])
def test_text_is_bit_exact_against_draw_text(side: int, scale: int) -> None:
    frames = background(side, len(STRINGS), side + scale)
    placements = [
        (3, 2, 4 * side),                  # clipped by the panel only (the long strings run off its right edge at these sides)
        (1, 5, 8 * scale + scale // 2 + 1),  # max_width cuts the second glyph, for scale > 1 in the middle of a glyph column
        (side - 7, 1, side),               # the panel's right edge cuts a glyph
        (2, side - 3, side),               # its bottom edge cuts the glyph rows
    ]
    # (at a stride of 8 the third string fills its stride without a NUL and is cut there)
    for (x, y, max_width), stride in [(placement, stride) for placement in placements for stride in (TEXT_STRIDE, 8)]:
        want = want_of(frames, STRINGS, stride, x, y, max_width, scale, side)
        got = draw_gpu(frames, STRINGS, stride, x, y, max_width, scale, side)
        changed = (want != frames).any(axis=-1)
        assert changed[1:].any() and not changed[0].any()  # the empty string draws nothing
        assert np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} pixels differ at {(x, y, max_width)}"
        # nothing outside the box [x, x + max_width) x [y, y + 7 scale) of the panel is touched, and no other panel
        box = np.zeros(frames.shape[1:3], dtype=bool)
        box[y : min(side, y + 7 * scale), PANEL * side + x : PANEL * side + min(side, x + max_width)] = True
        assert np.array_equal(got[:, ~box], frames[:, ~box])
        assert np.array_equal(draw_gpu(frames, STRINGS, stride, x, y, max_width, scale, side, splits=(2, 4)), got)


def test_a_string_that_fills_its_stride_reads_no_further() -> None:
    """text_stride = 8 with no NUL in the frame's bytes: the next frame's bytes are not part of the string."""
    side, stride = 96, 8
    strings = [b"12345678", b"abcdefgh", b"A"]
    frames = background(side, len(strings), 5)
    got = draw_gpu(frames, strings, stride, 2, 3, side, 1, side)
    want = want_of(frames, strings, stride, 2, 3, side, 1, side)
    assert np.array_equal(got, want)
    panel = (got != frames).any(axis=-1)[:, :, PANEL * side : (PANEL + 1) * side]
    assert panel[0, :, 2 + 8 * font.ADVANCE :].sum() == 0 and panel[0, :, 2 + 7 * font.ADVANCE :].sum() > 0  # eight glyphs, not sixteen
