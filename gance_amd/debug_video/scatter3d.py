"""
The 3-D view of the synthesis inputs (plot_vectors_3d and draw_y_point of the reference's vectors_3d.py, placed by
network_visualization.py:133-142 and moved per frame by :269-285): the cloud of every input vector of a run with a
red marker moving through it. Pure host code (numpy): the view vectors, the limits, the panel's rectangle, sizes and
chrome, and the colour table. The cloud itself is rasterised once per run in HBM (gance_amd/csrc/scatter3d.hip) by the
rule of DESIGN.md section 9 item 8, which `project` restates for the chrome's cube edges.
"""

import math
from typing import Dict, List, Tuple

import numpy as np

from gance_amd import hip_lib
from gance_amd.debug_video import font
from gance_amd.debug_video.chrome import BLACK, GRID, RED, Colour, format_limit, map_extent, span, title_height

ELEVATION, AZIMUTH = 50.0, 300.0  # ax_3d.view_init(elev=50, azim=300) (vectors_3d.py:67)
X_LABEL, Y_LABEL, Z_LABEL = "Sample # In Vector (x)", "Chunk Position (y)", "Signal Amplitude (z)"  # vectors_3d.py:35-37
DEPTH_LEVELS = 65535

# matplotlib's "Greens": the nine ColorBrewer nodes and the 256 entries `greens_from_nodes` derives from them
GREENS_NODES = ((247, 252, 245), (229, 245, 224), (199, 233, 192), (161, 217, 155), (116, 196, 118), (65, 171, 93), (35, 139, 69), (0, 109, 44), (0, 68, 27))
GREENS = np.frombuffer(bytes.fromhex(
    "f7fcf5f6fbf4f5fbf3f5fbf3f4fbf2f4faf1f3faf1f3faf0f2faeff1faeff1f9eef0f9edf0f9edeff9eceff8ebeef8eb"
    "edf8eaedf8e9ecf8e9ecf7e8ebf7e7ebf7e7eaf7e6eaf6e5e9f6e5e8f6e4e8f6e3e7f6e3e7f5e2e6f5e1e6f5e1e5f5e0"
    "e4f4dfe3f4dee3f4dde2f3dce1f3dbe0f3dadff2d9def2d8ddf1d7dcf1d6dbf1d5daf0d4d9f0d3d8f0d2d7efd1d6efd0"
    "d5eecfd4eeced3eecdd3edccd2edcbd1edcad0ecc9cfecc8ceebc7cdebc6ccebc5cbeac4caeac3c9eac2c8e9c1c7e9c0"
    "c6e8bfc5e8bec4e7bdc3e7bcc1e6bbc0e6b9bfe5b8bee5b7bde4b6bbe4b5bae3b4b9e3b2b8e2b1b7e2b0b6e1afb4e1ae"
    "b3e0adb2e0abb1dfaab0dfa9aedea8addea7acdda6abdda5aadca3a8dca2a7dba1a6dba0a5da9fa4da9ea2d99ca1d99b"
    "a0d89a9fd8999dd7989cd6979ad69599d59498d49396d49295d39193d29092d28e90d18d8fd08c8ed08b8ccf8a8bce89"
    "89ce8788cd8687cc8585cc8484cb8382ca8281ca8180c97f7ec87e7dc87d7bc77c7ac67b78c67a77c57876c47774c476"
    "73c37571c27470c2746ec1736cc0726bbf7169be7068be7066bd6f64bc6e63bb6d61ba6c60ba6c5eb96b5cb86a5bb769"
    "59b76958b66856b56754b46653b36551b36550b2644eb1634cb0624bb06149af6148ae6046ad5f44ac5e43ac5e41ab5d"
    "40aa5c3fa95b3ea85b3da75a3ca6593ba5583aa45839a35738a25637a15537a055369f54359e53349d52339c51329b51"
    "319a5030994f2f984e2e974e2d964d2c954c2b944b2a934b29924a289149279048278f48268e47258d46248c45238b45"
    "228a442189431f88421e87421d86411c85401b843f1a833e19823e18813d17803c167f3b157e3a137e3a127d39117c38"
    "107b370f7a370e79360d78350c77340b76330a753308743207733106723005713004702f036f2e026f2d016e2c006d2c"
    "006b2b006a2b00692a006829006629006528006428006227006127006026005f26005d25005c25005b24005924005823"
    "005723005622005421005321005220005020004f1f004e1f004d1e004b1e004a1d00491d00471c00461c00451b00441b"
), dtype=np.uint8).reshape(256, 3).copy()


def greens_from_nodes() -> np.ndarray:
    """
    [256, 3] uint8 by matplotlib's segment rule (colors._create_lookup_table with the nodes equidistant, then
    Colormap.__call__(bytes=True)): linear between the two nodes around entry j, times 255, truncated.
    """
    nodes = np.array(GREENS_NODES, dtype=np.float64) / 255.0
    x = np.linspace(0, 1, len(GREENS_NODES)) * 255
    entries = 255 * np.linspace(0, 1, 256)
    above = np.searchsorted(x, entries)[1:-1]
    distance = (entries[1:-1] - x[above - 1]) / (x[above] - x[above - 1])
    table = np.empty((256, 3), dtype=np.float64)
    for channel in range(3):
        y = nodes[:, channel]
        table[:, channel] = np.concatenate([[y[0]], distance * (y[above] - y[above - 1]) + y[above - 1], [y[-1]]])
    return (np.clip(table, 0.0, 1.0) * 255).astype(np.uint8)


Vector = Tuple[float, float, float]


def view_vectors(elev: float = ELEVATION, azim: float = AZIMUTH) -> Tuple[Vector, Vector, Vector]:
    """(right, up, toward) of matplotlib's view_init(elev, azim), in degrees: an orthonormal frame, `toward` pointing at the viewer."""
    e, a = math.radians(elev), math.radians(azim)
    right = (-math.sin(a), math.cos(a), 0.0)
    up = (-math.sin(e) * math.cos(a), -math.sin(e) * math.sin(a), math.cos(e))
    toward = (math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e))
    return right, up, toward


def half_extent(vector: Vector) -> float:
    """What a projected coordinate reaches over the unit cube: H(w) = (|w0| + |w1| + |w2|) / 2."""
    return float(((np.float64(abs(vector[0])) + np.float64(abs(vector[1]))) + np.float64(abs(vector[2]))) / np.float64(2.0))


def marker_x(vector_length: int) -> float:
    """The marker sits a tenth of a vector to the right of the cloud (network_visualization.py:280)."""
    return float(int(np.ceil(vector_length + (vector_length * 0.1))))


def cloud_limits(values: np.ndarray) -> Dict[str, Tuple[float, float]]:
    """
    Limits of the cloud of `values` [N, L]: x reaches the marker, z includes the marker's 0, the colour is normalised over
    the data alone (as matplotlib normalises c=z_data); values that are not finite do not count.
    """
    count, length = values.shape
    finite = values[np.isfinite(values)]
    low, high = (float(finite.min()), float(finite.max())) if finite.size else (0.0, 0.0)
    return {
        "x": (0.0, marker_x(length)), "y": span(0.0, float(count - 1)), "z": span(min(low, 0.0), max(high, 0.0)), "colour": span(low, high),
    }


def marker_size(side: int) -> int:
    return 2 + side // 128


def point_size(side: int) -> int:
    """Side of a cloud point's square: `panels.line_size`."""
    return 1 + side // 512


def project(point: Vector, limits: Dict[str, Tuple[float, float]], vectors: Tuple[Vector, Vector, Vector], width: int, height: int) -> Tuple[int, int, int]:
    """(column, row, depth level) of a point, column and row relative to the axis rectangle: the rule, in double."""
    u = [(np.float64(p) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) - np.float64(0.5) for p, (lo, hi) in zip(point, (limits["x"], limits["y"], limits["z"]))]
    sx, sy, depth = ((np.float64(w[0]) * u[0] + np.float64(w[1]) * u[1]) + np.float64(w[2]) * u[2] for w in vectors)
    h_right, h_up, h_toward = (half_extent(w) for w in vectors)
    level = np.floor((depth - np.float64(-h_toward)) / (np.float64(h_toward) - np.float64(-h_toward)) * np.float64(DEPTH_LEVELS) + np.float64(0.5))
    return (
        map_extent(sx, -h_right, h_right, width), (height - 1) - map_extent(sy, -h_up, h_up, height),
        int(min(float(DEPTH_LEVELS), max(0.0, level))),
    )


def _line(region: np.ndarray, start: Tuple[int, int], stop: Tuple[int, int], colour: Colour) -> None:
    """The line stepping rule of DESIGN.md section 9 item 7 with stamps of one pixel, clipped to `region`."""
    (xa, ya), (xb, yb) = start, stop
    dx, dy = xb - xa, yb - ya
    steps = max(abs(dx), abs(dy))
    for s in range(steps + 1):
        x = xa + ((2 * s * dx + steps) // (2 * steps) if steps else 0)
        y = ya + ((2 * s * dy + steps) // (2 * steps) if steps else 0)
        if 0 <= x < region.shape[1] and 0 <= y < region.shape[0]:
            region[y, x] = colour


class Scatter3dPanel:  # pylint: disable=too-many-instance-attributes
    """
    The 3-D panel of a run: `values` [N, L] (the vector of every frame; row 0 of a latent matrix), a square of `side`.
    Holds what is the same on every frame: the axis rectangle, the sizes, the limits, the chrome and the view record.
    """

    def __init__(self, side: int, values: np.ndarray, label: str, elev: float = ELEVATION, azim: float = AZIMUTH) -> None:
        if values.ndim != 2 or values.shape[0] < 1 or values.shape[1] < 1:
            raise ValueError(f"the 3-D view needs vectors [N, L], got {values.shape}")
        self.side, self.label = int(side), label
        self.num_vectors, self.vector_length = int(values.shape[0]), int(values.shape[1])
        self.limits = cloud_limits(np.asarray(values))
        self.vectors = view_vectors(elev, azim)
        self.point_size, self.marker_size = point_size(self.side), marker_size(self.side)
        scale = font.scale_for_side(self.side)
        self._line = font.GLYPH_HEIGHT * scale + scale
        margin = max(2, self.side // 32)
        # a title line above and three label lines below, each only where the panel is large enough to keep half its height
        self.titled = self.side - title_height(self.side) - 2 >= self.side // 2
        top = title_height(self.side) if self.titled else 1
        self.labelled = self.side - top - 3 * self._line - 2 >= self.side // 2
        bottom = self.side - 1 - (3 * self._line if self.labelled else 0)
        self.rectangle = (margin, top, self.side - 2 * margin, max(1, bottom - top))  # x, y, width, height

    def cursor(self, frame: int) -> float:
        """y of the marker: the frame index (network_visualization.py:281)."""
        return float(frame)

    def chrome(self) -> np.ndarray:
        """[side, side, 3] uint8: white, the title, the projected edges of the unit cube, the axis labels with their limits."""
        side = self.side
        x0, y0, width, height = self.rectangle
        image = np.full((side, side, 3), 255, dtype=np.uint8)
        scale = font.scale_for_side(side)
        if self.titled:
            font.draw_text(image, x0, y0 - title_height(side), self.label, BLACK, scale)
        corners = {}
        for corner in range(8):
            bits = (corner & 1, corner >> 1 & 1, corner >> 2 & 1)
            point = tuple(self.limits[name][bit] for name, bit in zip("xyz", bits))
            corners[bits] = project(point, self.limits, self.vectors, width, height)[:2]
        region = image[y0 : y0 + height, x0 : x0 + width]
        for bits, start in corners.items():
            for axis in range(3):
                if bits[axis] == 0:
                    other = tuple(1 if k == axis else bit for k, bit in enumerate(bits))
                    _line(region, start, corners[other], GRID)
        if self.labelled:
            for line, (name, text) in enumerate((("x", X_LABEL), ("y", Y_LABEL), ("z", Z_LABEL))):
                low, high = self.limits[name]
                font.draw_text(image, x0, y0 + height + 1 + line * self._line, f"{text}: {format_limit(low)} .. {format_limit(high)}", BLACK, scale)
        return image

    def view(self) -> hip_lib.DebugView3d:
        """The `gance_debug_view3d` of this panel."""
        record = hip_lib.DebugView3d()
        record.x, record.y, record.width, record.height = self.rectangle
        (record.x_min, record.x_max), (record.y_min, record.y_max) = self.limits["x"], self.limits["y"]
        (record.z_min, record.z_max), (record.c_min, record.c_max) = self.limits["z"], self.limits["colour"]
        for name, vector in zip(("right", "up", "toward"), self.vectors):
            setattr(record, name, (hip_lib.ctypes.c_double * 3)(*vector))
        record.point_size, record.marker_size = self.point_size, self.marker_size
        record.marker_rgb = (hip_lib.ctypes.c_uint8 * 3)(*RED)
        record.marker_x, record.marker_z = marker_x(self.vector_length), 0.0
        return record
