"""
A built-in 5x7 bitmap font for printable ASCII (the classic dot-matrix display face), scaled by an integer factor:
the text of the debug video's titles, legends and limit labels. No PIL, no font files.
"""

from typing import Tuple

import numpy as np

GLYPH_WIDTH, GLYPH_HEIGHT = 5, 7
ADVANCE = GLYPH_WIDTH + 1  # one empty column between glyphs
FIRST, LAST = 32, 126

# five column bytes per glyph from ' ' to '~', bit 0 = top row
_COLUMNS = bytes.fromhex(
    "0000000000" "00005f0000" "0007000700" "147f147f14" "242a7f2a12" "2313086462" "3649552250" "0005030000"
    "001c224100" "0041221c00" "14083e0814" "08083e0808" "0050300000" "0808080808" "0060600000" "2010080402"
    "3e5149453e" "00427f4000" "4261514946" "2141454b31" "1814127f10" "2745454539" "3c4a494930" "0171090503"
    "3649494936" "064949291e" "0036360000" "0056360000" "0814224100" "1414141414" "0041221408" "0201510906"
    "324979413e" "7e1111117e" "7f49494936" "3e41414122" "7f4141221c" "7f49494941" "7f09090901" "3e4149497a"
    "7f0808087f" "00417f4100" "2040413f01" "7f08142241" "7f40404040" "7f020c027f" "7f0408107f" "3e4141413e"
    "7f09090906" "3e4151215e" "7f09192946" "4649494931" "01017f0101" "3f4040403f" "1f2040201f" "3f4038403f"
    "6314081463" "0708700807" "6151494543" "007f414100" "0204081020" "0041417f00" "0402010204" "4040404040"
    "0001020400" "2054545478" "7f48444438" "3844444420" "384444487f" "3854545418" "087e090102" "0c5252523e"
    "7f08040478" "00447d4000" "2040443d00" "7f10284400" "00417f4000" "7c04180478" "7c08040478" "3844444438"
    "7c14141408" "081414187c" "7c08040408" "4854545420" "043f444020" "3c4040207c" "1c2040201c" "3c4030403c"
    "4428102844" "0c5050503c" "4464544c44" "0008364100" "00007f0000" "0041360800" "0804081008"
)
assert len(_COLUMNS) == (LAST - FIRST + 1) * GLYPH_WIDTH


def glyph(character: str) -> np.ndarray:
    """[7, 5] bool bitmap of one character; anything outside printable ASCII is drawn as '?'."""
    code = ord(character)
    if not FIRST <= code <= LAST:
        code = ord("?")
    columns = np.frombuffer(_COLUMNS, dtype=np.uint8, count=GLYPH_WIDTH, offset=(code - FIRST) * GLYPH_WIDTH)
    return ((columns[None, :] >> np.arange(GLYPH_HEIGHT)[:, None]) & 1).astype(bool)


def scale_for_side(side: int) -> int:
    """Integer glyph scale of a panel of `side` pixels: 1 up to 383, 2 from 384, 3 from 768 ..."""
    return max(1, int(side) // 384 + 1)


def text_size(text: str, scale: int = 1) -> Tuple[int, int]:
    """(width, height) in pixels of `text` at `scale`."""
    return (max(0, len(text) * ADVANCE - 1) * scale, GLYPH_HEIGHT * scale)


def text_mask(text: str, scale: int = 1) -> np.ndarray:
    """[height, width] bool mask of `text` on one line."""
    width, height = text_size(text, scale)
    mask = np.zeros((GLYPH_HEIGHT, max(0, len(text) * ADVANCE - 1)), dtype=bool)
    for index, character in enumerate(text):
        mask[:, index * ADVANCE : index * ADVANCE + GLYPH_WIDTH] = glyph(character)
    mask = np.repeat(np.repeat(mask, scale, axis=0), scale, axis=1)
    assert mask.shape == (height, width)
    return mask


def draw_text(image: np.ndarray, x: int, y: int, text: str, colour: Tuple[int, int, int], scale: int = 1) -> None:
    """`text` with its top-left corner at (x, y) of `image` [H, W, 3] uint8, clipped to the image."""
    mask = text_mask(text, scale)
    height, width = image.shape[:2]
    x_lo, y_lo = max(0, x), max(0, y)
    x_hi, y_hi = min(width, x + mask.shape[1]), min(height, y + mask.shape[0])
    if x_hi <= x_lo or y_hi <= y_lo:
        return
    part = mask[y_lo - y : y_hi - y, x_lo - x : x_hi - x]
    image[y_lo:y_hi, x_lo:x_hi][part] = colour
