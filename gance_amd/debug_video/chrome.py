"""
The static part of a plot panel, drawn once per window with numpy: axes boxes, titles with the y limits, legends,
grid and dotted threshold lines. The per-frame marks are rasterised on top of a copy of it in HBM
(gance_amd/csrc/debug_panels.hip). Labels and limits are the reference's (network_visualization.py:95-131,
overlay_visualization.py:84-123, visualize_vector_reduction.py:139-159); the drawing is ours.
"""

from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from gance_amd.debug_video import font

Colour = Tuple[int, int, int]
BLACK: Colour = (0, 0, 0)
WHITE: Colour = (255, 255, 255)
GRID: Colour = (220, 220, 220)
PURPLE: Colour = (128, 0, 128)
# matplotlib's single-letter colours in the order of infinite_colors() (visualization_common.py:169-176)
BASE_COLOURS: Tuple[Colour, ...] = ((0, 0, 255), (0, 127, 0), (255, 0, 0), (0, 191, 191), (191, 0, 191), (191, 191, 0), (0, 0, 0))
BLUE, GREEN, RED, CYAN, MAGENTA = BASE_COLOURS[:5]


class AxisSpec(NamedTuple):
    """One axis of a panel: the pixel rectangle marks are drawn in, the limits mapped onto it, and its chrome."""

    x: int
    y: int
    width: int
    height: int
    x_limits: Tuple[float, float]
    y_limits: Tuple[float, float]
    title: str = ""
    titled: bool = False  # room for a title line above the rectangle
    legend: Tuple[Tuple[str, Colour], ...] = ()
    grid: bool = False
    hlines: Tuple[Tuple[float, Colour], ...] = ()  # dotted lines at these y values


def map_extent(value: float, low: float, high: float, extent: int) -> int:
    """Value -> pixel offset along an axis of `extent` pixels: the rule of DESIGN.md section 9, in double."""
    scaled = (np.float64(value) - np.float64(low)) / (np.float64(high) - np.float64(low)) * np.float64(extent - 1)
    return int(min(32767.0, max(-32768.0, np.floor(scaled + np.float64(0.5)))))


def span(low: float, high: float) -> Tuple[float, float]:
    """Limits an axis can map: (low, low + 1) where the data has one value only (matplotlib widens such limits too)."""
    low, high = float(low), float(high)
    return (low, high) if high > low else (low, low + 1.0)


def title_height(side: int) -> int:
    return font.GLYPH_HEIGHT * font.scale_for_side(side) + 2


def stacked_rectangles(side: int, row_spans: Sequence[Tuple[int, int]], total_rows: int) -> List[Tuple[int, int, int, int, bool]]:
    """
    (x, y, width, height, titled) of axes stacked in the rows [first, last) of a grid of `total_rows` rows over the
    panel, as fig.add_gridspec(nrows=...) splits a figure. An axis gets a title line if its cell is high enough.
    """
    margin = max(2, side // 32)
    out = []
    for first, last in row_spans:
        top, bottom = first * side // total_rows, last * side // total_rows
        titled = bottom - top >= title_height(side) + 8
        y = top + (title_height(side) if titled else 1)
        out.append((margin, y, side - 2 * margin, max(1, bottom - 2 - y), titled))
    return out


def format_limit(value: float) -> str:
    return f"{value:.3g}"


def render_chrome(side: int, axes: Sequence[AxisSpec]) -> np.ndarray:  # pylint: disable=too-many-locals
    """The template [side, side, 3] uint8 of one window of one panel."""
    image = np.full((side, side, 3), 255, dtype=np.uint8)
    scale = font.scale_for_side(side)
    for axis in axes:
        x0, y0, x1, y1 = axis.x, axis.y, axis.x + axis.width, axis.y + axis.height
        if axis.grid:
            for quarter in (1, 2, 3):
                image[y0:y1, x0 + quarter * (axis.width - 1) // 4] = GRID
                image[y0 + quarter * (axis.height - 1) // 4, x0:x1] = GRID
        for value, colour in axis.hlines:
            row = (axis.height - 1) - map_extent(value, axis.y_limits[0], axis.y_limits[1], axis.height)
            if 0 <= row < axis.height:
                columns = np.arange(axis.width)
                image[y0 + row, x0 + columns[(columns // (2 * scale)) % 2 == 0]] = colour
        # the box, one pixel outside the rectangle
        bx0, by0, bx1, by1 = max(0, x0 - 1), max(0, y0 - 1), min(side - 1, x1), min(side - 1, y1)
        image[by0, bx0 : bx1 + 1] = BLACK
        image[by1, bx0 : bx1 + 1] = BLACK
        image[by0 : by1 + 1, bx0] = BLACK
        image[by0 : by1 + 1, bx1] = BLACK
        if axis.titled:
            text_y = y0 - title_height(side)
            font.draw_text(image, x0, text_y, axis.title, BLACK, scale)
            limits = f"{format_limit(axis.y_limits[0])} .. {format_limit(axis.y_limits[1])}"
            limits_x = x1 - font.text_size(limits, scale)[0]
            if limits_x >= x0 + font.text_size(axis.title, scale)[0] + font.ADVANCE * scale:
                font.draw_text(image, limits_x, text_y, limits, BLACK, scale)
        line = font.GLYPH_HEIGHT * scale + scale
        if axis.legend and axis.height >= len(axis.legend) * line + 2:
            for index, (label, colour) in enumerate(axis.legend):
                width = font.text_size(label, scale)[0]
                font.draw_text(image[y0:y1, x0:x1], axis.width - width - 1, 1 + index * line, label, colour, scale)
    return image
