"""
CPU restatement of the debug-video rasteriser, written from the rule in DESIGN.md section 9 (not from the kernel): the
reference of tests/test_debug_panels_gpu.py. Marks and axes are plain dicts here; series are numpy arrays.

Rule: a value v on an axis of `extent` pixels with limits (lo, hi) lands at floor((v - lo) / (hi - lo) * (extent - 1) +
0.5) pixels from the left edge, or from the BOTTOM edge for y; a mark of size k stamps the k x k square whose top-left
corner is k // 2 left of and above its pixel; a line from pixel a to pixel b takes n = max(|dx|, |dy|) steps, step s at
a + floor((2 s d + n) / (2 n)) per coordinate; a dashed line draws the steps whose column c (from the axis' left edge)
has c mod (on + off) < on; every pixel a mark covers is blended once, channel = (colour * a + channel * (255 - a) +
127) // 255; marks are clipped to their axis and composited in table order; samples that are not finite, or outside
the series, are left out, and so is a line segment that touches one.
"""

from typing import Dict, List, Sequence, Tuple

import numpy as np

POINTS, POLYLINE, CURSOR, BAR = range(4)


def scaled(value: float, low: float, high: float, extent: int) -> np.float64:
    """Position in pixels before rounding, in double and in the rule's order of operations."""
    return (np.float64(value) - np.float64(low)) / (np.float64(high) - np.float64(low)) * np.float64(extent - 1)


def to_pixel(value: float, low: float, high: float, extent: int) -> int:
    return int(np.clip(np.floor(scaled(value, low, high, extent) + np.float64(0.5)), -32768, 32767))


def rounding_margin(value: float, low: float, high: float, extent: int) -> float:
    """Distance of the unrounded position from the nearest rounding boundary (k + 0.5), in pixels."""
    position = float(scaled(value, low, high, extent)) + 0.5
    return abs(position - round(position))


def _series_values(mark: dict, frame_number: int) -> List[Tuple[int, float]]:
    """(sample number, value) of the samples a mark may draw on this frame; None for those it must leave out."""
    data = np.asarray(mark["data"]).reshape(-1)
    row = frame_number // mark.get("frame_divisor", 1)
    out = []
    for i in range(mark["count"]):
        index = row * mark.get("frame_stride", 0) + i
        value = float(data[index]) if 0 <= index < data.size else float("nan")
        out.append((i, value))
    return out


def mapped_coordinates(axes: Sequence[dict], marks: Sequence[dict], frames: Sequence[dict]) -> List[Tuple[float, float, float, int]]:
    """Every (value, low, high, extent) the rule rounds for these inputs: what the margin assertion walks over."""
    found = []
    for frame in frames:
        for mark in marks:
            axis = axes[mark["axis"]]
            if (frame["flags"] & mark.get("flag_mask", 0)) != mark.get("flag_value", 0):
                continue
            if mark["kind"] == CURSOR:
                found.append((frame["cursor"], *axis["x_limits"], axis["width"]))
                continue
            values = _series_values(mark, frame["number"])
            if mark["kind"] == BAR:
                found.append((0.0, *axis["x_limits"], axis["width"]))
                if np.isfinite(values[0][1]):
                    found.append((values[0][1], *axis["x_limits"], axis["width"]))
                continue
            for i, value in values:
                if np.isfinite(value):
                    found.append((mark.get("x_start", 0.0) + i, *axis["x_limits"], axis["width"]))
                    found.append((value, *axis["y_limits"], axis["height"]))
    return found


def smallest_margin(axes: Sequence[dict], marks: Sequence[dict], frames: Sequence[dict]) -> float:
    return min(rounding_margin(*entry) for entry in mapped_coordinates(axes, marks, frames))


def _stamp(covered: np.ndarray, column: int, row: int, size: int) -> None:
    height, width = covered.shape
    left, top = column - size // 2, row - size // 2
    covered[max(0, top) : max(0, min(height, top + size)), max(0, left) : max(0, min(width, left + size))] = True


def _dash_allows(mark: dict, column: int) -> bool:
    on, off = mark.get("dash", (0, 0))
    return on == 0 or column % (on + off) < on  # (Python's % is a floor modulo)


def coverage(mark: dict, axis: dict, frame: dict) -> np.ndarray:
    """[height, width] bool: the pixels of the axis rectangle the mark covers on this frame."""
    width, height = axis["width"], axis["height"]
    covered = np.zeros((height, width), dtype=bool)
    size = mark.get("size", 1)

    def column_of(x: float) -> int:
        return to_pixel(x, *axis["x_limits"], width)

    def row_of(y: float) -> int:
        return (height - 1) - to_pixel(y, *axis["y_limits"], height)

    if mark["kind"] == CURSOR:
        if np.isfinite(frame["cursor"]):
            for row in range(height):
                _stamp(covered, column_of(frame["cursor"]), row, size)
        return covered
    values = _series_values(mark, frame["number"])
    if mark["kind"] == BAR:
        if np.isfinite(values[0][1]):
            ends = sorted((column_of(0.0), column_of(values[0][1])))
            covered[height // 4 : height - height // 4, max(0, ends[0]) : max(0, min(width, ends[1] + 1))] = True
        return covered
    x_start = mark.get("x_start", 0.0)
    if mark["kind"] == POINTS:
        for i, value in values:
            if np.isfinite(value):
                _stamp(covered, column_of(x_start + i), row_of(value), size)
        return covered
    for (i, a), (j, b) in zip(values[:-1], values[1:]):
        if not (np.isfinite(a) and np.isfinite(b)):
            continue
        xa, ya, xb, yb = column_of(x_start + i), row_of(a), column_of(x_start + j), row_of(b)
        dx, dy = xb - xa, yb - ya
        steps = max(abs(dx), abs(dy))
        for s in range(steps + 1):
            column = xa + ((2 * s * dx + steps) // (2 * steps) if steps else 0)
            row = ya + ((2 * s * dy + steps) // (2 * steps) if steps else 0)
            if _dash_allows(mark, column):
                _stamp(covered, column, row, size)
    return covered


def draw(chrome: np.ndarray, axes: Sequence[dict], marks: Sequence[dict], frames: Sequence[dict]) -> np.ndarray:
    """[len(frames), side, side, 3] uint8: the chrome with every frame's marks composited in table order."""
    out = np.repeat(chrome[None], len(frames), axis=0).astype(np.int64)
    for number, frame in enumerate(frames):
        for mark in marks:
            if (frame["flags"] & mark.get("flag_mask", 0)) != mark.get("flag_value", 0):
                continue
            axis = axes[mark["axis"]]
            covered = coverage(mark, axis, frame)
            region = out[number, axis["y"] : axis["y"] + axis["height"], axis["x"] : axis["x"] + axis["width"]]
            colour, alpha = np.array(mark["rgba"][:3], dtype=np.int64), int(mark["rgba"][3])
            region[covered] = (colour * alpha + region[covered] * (255 - alpha) + 127) // 255
    return out.astype(np.uint8)
