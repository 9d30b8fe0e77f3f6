"""
CPU restatement of the 3-D view's rasteriser, written from the rule in DESIGN.md section 9 item 8 (not from the kernel):
the reference of tests/test_scatter3d_gpu.py and tests/test_vector_synthesis_visualization_gpu.py. A view is a plain
dict here; values are numpy arrays [N, L].

Rule: point (i, n, v) -> u_k = (p_k - lo_k) / (hi_k - lo_k) - 0.5; sx = (right0 ux + right1 uy) + right2 uz, sy with
`up`, depth with `toward`; H(w) = ((|w0| + |w1|) + |w2|) / 2; column = floor((sx + H_r) / (2 H_r) (width - 1) + 0.5)
from the rectangle's left edge, row likewise from its BOTTOM edge; depth level q = floor((depth + H_t) / (2 H_t) 65535 +
0.5) clamped to 0 .. 65535; a point of size k stamps the k x k square whose top-left corner is k // 2 left of and above
its pixel, clipped to the rectangle; a pixel shows the point with the largest (q, n L + i) as LUT[floor((v - c_lo) /
(c_hi - c_lo) 255 + 0.5) clamped to 0 .. 255], or the chrome; values that are not finite are left out. The marker of a
frame is (marker_x, cursor, marker_z) projected and stamped likewise in its own colour, on top. All in double.
"""

from typing import Dict, NamedTuple, Sequence, Tuple

import numpy as np

DEPTH_LEVELS = 65535


def make_view(  # pylint: disable=too-many-arguments
    rectangle: Tuple[int, int, int, int], x_limits, y_limits, z_limits, colour_limits, right, up, toward, point_size: int = 1,
    marker_size: int = 2, marker_rgb=(255, 0, 0), marker_x: float = 0.0, marker_z: float = 0.0,
) -> dict:
    return dict(
        rectangle=tuple(rectangle), x_limits=tuple(x_limits), y_limits=tuple(y_limits), z_limits=tuple(z_limits),
        colour_limits=tuple(colour_limits), right=tuple(right), up=tuple(up), toward=tuple(toward), point_size=point_size,
        marker_size=marker_size, marker_rgb=tuple(marker_rgb), marker_x=marker_x, marker_z=marker_z,
    )


def half_extent(vector: Sequence[float]) -> np.float64:
    w = np.abs(np.asarray(vector, dtype=np.float64))
    return ((w[0] + w[1]) + w[2]) / np.float64(2.0)


def _unit(p: np.ndarray, limits: Tuple[float, float]) -> np.ndarray:
    low, high = np.float64(limits[0]), np.float64(limits[1])
    return (np.asarray(p, dtype=np.float64) - low) / (high - low) - np.float64(0.5)


def _scaled(s: np.ndarray, half: np.float64, steps: int) -> np.ndarray:
    """Position before rounding on an axis of `steps` + 1 places with limits (-half, half)."""
    return (s - (-half)) / (half - (-half)) * np.float64(steps)


def positions(view: dict, px, py, pz) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Unrounded (column, row-from-the-bottom, depth level) positions of points, in the rule's order of operations."""
    ux, uy, uz = _unit(px, view["x_limits"]), _unit(py, view["y_limits"]), _unit(pz, view["z_limits"])
    _, _, width, height = view["rectangle"]
    out = []
    for name, steps in (("right", width - 1), ("up", height - 1), ("toward", DEPTH_LEVELS)):
        w = np.asarray(view[name], dtype=np.float64)
        out.append(_scaled((w[0] * ux + w[1] * uy) + w[2] * uz, half_extent(view[name]), steps))
    return tuple(out)


def _round(position: np.ndarray, low: float, high: float) -> np.ndarray:
    return np.clip(np.floor(position + np.float64(0.5)), low, high).astype(np.int64)


def _margin(position: np.ndarray) -> float:
    shifted = np.asarray(position, dtype=np.float64) + 0.5
    return float(np.min(np.abs(shifted - np.round(shifted)))) if shifted.size else float("inf")


class Template(NamedTuple):
    image: np.ndarray  # [side, side, 3] uint8
    smallest_margin: float  # distance of any column, row or depth position from a rounding boundary
    reached: int  # pixels at least one point covers
    contested: int  # pixels more than one point covers
    most_on_a_pixel: int


def template(chrome: np.ndarray, view: dict, values: np.ndarray, lut: np.ndarray) -> Template:
    """The chrome with the cloud of `values` [N, L] on top."""
    side = chrome.shape[0]
    x0, y0, width, height = view["rectangle"]
    count, length = values.shape
    numbers = np.arange(count * length, dtype=np.int64)
    flat = np.asarray(values, dtype=np.float64).reshape(-1)
    keep = np.isfinite(flat)
    numbers, flat = numbers[keep], flat[keep]
    column_at, row_at, level_at = positions(view, numbers % length, numbers // length, flat)
    margin = min(_margin(column_at), _margin(row_at), _margin(level_at))
    columns = _round(column_at, -32768, 32767)
    rows = (height - 1) - _round(row_at, -32768, 32767)
    levels = _round(level_at, 0, DEPTH_LEVELS)
    keys = ((levels + 1) << 40) | numbers
    best = np.zeros((height, width), dtype=np.int64)
    hits = np.zeros((height, width), dtype=np.int64)
    k = view["point_size"]
    for dy in range(k):
        for dx in range(k):
            x, y = columns - k // 2 + dx, rows - k // 2 + dy
            inside = (x >= 0) & (x < width) & (y >= 0) & (y < height)
            np.maximum.at(best, (y[inside], x[inside]), keys[inside])
            np.add.at(hits, (y[inside], x[inside]), 1)
    image = chrome.copy()
    covered = best > 0
    winners = np.asarray(values, dtype=np.float64).reshape(-1)[best[covered] & ((1 << 40) - 1)]
    c_low, c_high = np.float64(view["colour_limits"][0]), np.float64(view["colour_limits"][1])
    colour = _round((winners - c_low) / (c_high - c_low) * np.float64(255.0), 0, 255)
    image[y0 : y0 + height, x0 : x0 + width][covered] = np.asarray(lut, dtype=np.uint8)[colour]
    assert image.shape == (side, side, 3)
    return Template(image, margin, int(covered.sum()), int((hits > 1).sum()), int(hits.max()))


def marker_margin(view: dict, cursors: Sequence[float]) -> float:
    column_at, row_at, _ = positions(view, np.full(len(cursors), view["marker_x"]), np.asarray(cursors, dtype=np.float64), np.full(len(cursors), view["marker_z"]))
    return min(_margin(column_at), _margin(row_at))


def frame(template_image: np.ndarray, view: dict, cursor: float) -> np.ndarray:
    """The template with the marker of the frame whose cursor is `cursor`."""
    image = template_image.copy()
    if not np.isfinite(cursor):
        return image
    x0, y0, width, height = view["rectangle"]
    column_at, row_at, _ = positions(view, np.array([view["marker_x"]]), np.array([cursor]), np.array([view["marker_z"]]))
    column = int(_round(column_at, -32768, 32767)[0])
    row = (height - 1) - int(_round(row_at, -32768, 32767)[0])
    k = view["marker_size"]
    left, top = column - k // 2, row - k // 2
    region = image[y0 : y0 + height, x0 : x0 + width]
    region[max(0, top) : max(0, min(height, top + k)), max(0, left) : max(0, min(width, left + k))] = view["marker_rgb"]
    return image


def limits_of(values: np.ndarray) -> Dict[str, Tuple[float, float]]:
    """The limits of DESIGN.md section 9 item 8 for a run's vectors [N, L]."""
    def widened(low: float, high: float) -> Tuple[float, float]:
        return (low, high) if high > low else (low, low + 1.0)

    count, length = values.shape
    finite = values[np.isfinite(values)]
    low, high = float(finite.min()), float(finite.max())
    return dict(
        x=(0.0, float(np.ceil(length + length * 0.1))), y=widened(0.0, float(count - 1)), z=widened(min(low, 0.0), max(high, 0.0)),
        colour=widened(low, high),
    )
