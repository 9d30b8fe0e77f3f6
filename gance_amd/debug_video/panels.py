"""
Mark tables of the three plot panels of the debug video, window by window: which series, where, in which colour.
Pure host code (numpy); compose.py binds the series names to tensors in HBM and hands the tables to the rasteriser.

Semantics follow the reference: the synthesis inputs (network_visualization.py:54-157, 160-251, 254-400), the overlay
computation (overlay_visualization.py:128-234) and the overlay binary mask (visualize_vector_reduction.py:85-179).
"""

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from gance_amd.data_into_network_visualization.visualization_common import ResultLayers, VisualizationInput
from gance_amd.debug_video.chrome import (
    BASE_COLOURS, BLUE, CYAN, GREEN, MAGENTA, PURPLE, RED, AxisSpec, Colour, render_chrome, span, stacked_rectangles,
)
from gance_amd.overlay.overlay_common import OverlayContext
from gance_amd.vector_sources.vector_sources_common import pad_array

POINTS, POLYLINE, CURSOR, BAR = range(4)  # gance_debug_mark.kind
FLAG_OVERLAY_WRITTEN = 1  # bit of a frame's flags: the overlay gate passed (OverlayContext.overlay_written)
OPAQUE, HALF = 255, 128  # alpha = 1 and alpha = 0.5


def point_size(side: int) -> int:
    """Side of a scatter point's square in pixels."""
    return 1 + side // 256


def line_size(side: int) -> int:
    """Thickness of a plain line (default linewidth) and of a cursor."""
    return 1 + side // 512


def medium_line_size(side: int) -> int:
    """Thickness of the mask panel's dashed layers (linewidth=3)."""
    return 1 + side // 256


def thick_line_size(side: int) -> int:
    """Thickness of the mask panel's result line (linewidth=5)."""
    return 3 + side // 128


def dash_pattern(side: int) -> Tuple[int, int]:
    """(on, off) pixel columns of a dashed line."""
    return 4 * (1 + side // 256), 4 * (1 + side // 256)


class MarkSpec(NamedTuple):
    """A `gance_debug_mark` before its series is bound to a device pointer: `series` names it, `offset` is in elements."""

    kind: int
    axis: int
    colour: Colour
    series: Optional[str] = None
    offset: int = 0
    count: int = 0
    frame_stride: int = 0
    frame_divisor: int = 1
    size: int = 1
    alpha: int = OPAQUE
    dash: Tuple[int, int] = (0, 0)
    flag_mask: int = 0
    flag_value: int = 0
    x_start: float = 0.0


class PanelWindow(NamedTuple):
    """What is the same for every frame of one window of one panel."""

    first_frame: int
    num_frames: int
    axes: List[AxisSpec]
    marks: List[MarkSpec]

    def chrome(self, side: int) -> np.ndarray:
        return render_chrome(side, self.axes)


def window_width(num_points: int, requested: Optional[int]) -> int:
    """`debug_window`, or a fifth of the run (network_visualization.py:177-182)."""
    return int(requested) if requested is not None else int(math.ceil(num_points / 5))


def _x_limits(count: int) -> Tuple[float, float]:
    return span(0.0, float(count - 1))


class SynthesisPanel:  # pylint: disable=too-many-instance-attributes
    """
    "Synthesis inputs": six stacked axes in the 2:2:2:2:1:1 row split. Device series it reads: "a" [N][L] (stride
    `vector_length`), "b" [F][L] (one row per projected frame: frame // frame_multiplier), "combined" (row 0 of each
    frame's matrix, `combined_stride` elements apart), and the host series of `host_series()`.
    """

    ROW_SPANS = ((0, 2), (2, 4), (4, 6), (6, 8), (8, 9), (9, 10))

    def __init__(  # pylint: disable=too-many-arguments
        self, side: int, vector_length: int, limits: Dict[str, Tuple[float, float]], labels: Dict[str, str],
        network_indices: ResultLayers, window: Optional[int], frame_multiplier: int = 1, combined_stride: Optional[int] = None,
    ) -> None:
        self.side, self.vector_length, self.limits, self.labels = side, vector_length, limits, labels
        self.indices = np.asarray(network_indices.result.data)
        self.layers = list(network_indices.layers)
        self.result_label = network_indices.result.label
        self.num_frames = int(self.indices.shape[0])
        self.width = window_width(self.num_frames, window)
        if self.width < 1:
            raise ValueError(f"the debug window must be at least one frame wide, got {self.width}")
        self.frame_multiplier = int(frame_multiplier)
        self.combined_stride = int(combined_stride if combined_stride is not None else vector_length)
        self.padded = self.width * int(math.ceil(self.num_frames / self.width))

    @classmethod
    def from_visualization_input(cls, side: int, visualization_input: VisualizationInput, vector_length: int, window: Optional[int]) -> "SynthesisPanel":
        """Limits and labels as _configure_axes takes them from a VisualizationInput (network_visualization.py:95-123)."""
        members = {"a": visualization_input.a_vectors, "b": visualization_input.b_vectors, "combined": visualization_input.combined}
        return cls(
            side, vector_length,
            {name: (float(np.min(member.data)), float(np.max(member.data))) for name, member in members.items()},
            {name: member.label for name, member in members.items()},
            visualization_input.network_indices, window,
        )

    def host_series(self) -> Dict[str, np.ndarray]:
        """The network indices (int32) and their layers (float64), zero-padded to whole windows as _frame_inputs pads them."""
        series = {"indices": pad_array(self.indices.astype(np.int32), self.padded)}
        for number, layer in enumerate(self.layers):
            series[f"layer{number}"] = pad_array(np.asarray(layer.data, dtype=np.float64), self.padded)
        return series

    def window_of(self, frame: int) -> int:
        return frame // self.width

    def cursor(self, frame: int) -> float:
        """x of the red cursor: frame_index % width (network_visualization.py:339, 377)."""
        return float(frame % self.width)

    def window(self, index: int) -> PanelWindow:
        """Axes and marks of window `index` (frames [index * width, (index + 1) * width))."""
        side, length = self.side, self.vector_length
        rectangles = stacked_rectangles(side, self.ROW_SPANS, 10)
        index_limits = span(float(self.indices.min()), float(self.indices.max()))
        layer_limits = span(
            min((float(np.min(layer.data)) for layer in self.layers), default=0.0),
            max((float(np.max(layer.data)) for layer in self.layers), default=1.0),
        )
        titles = ["Input A", "Input B", "Combined Inputs", f"Composition of network index selection: {self.result_label}", "", "network Index"]
        colours = (RED, GREEN, BLUE)
        axes, marks = [], []
        for number, name in enumerate(("a", "b", "combined")):
            axes.append(AxisSpec(
                *rectangles[number][:4], (0.0, float(length)), span(*self.limits[name]), titles[number], rectangles[number][4],
                legend=((self.labels.get(name, ""), colours[number]),),
            ))
        marks.append(MarkSpec(POINTS, 0, RED, "a", count=length, frame_stride=length, size=point_size(side)))
        marks.append(MarkSpec(POINTS, 1, GREEN, "b", count=length, frame_stride=length, frame_divisor=self.frame_multiplier, size=point_size(side)))
        marks.append(MarkSpec(POINTS, 2, BLUE, "combined", count=length, frame_stride=self.combined_stride, size=point_size(side)))
        start = index * self.width
        axes.append(AxisSpec(
            *rectangles[3][:4], _x_limits(self.width), layer_limits, titles[3], rectangles[3][4],
            legend=tuple((layer.label, BASE_COLOURS[k % len(BASE_COLOURS)]) for k, layer in enumerate(self.layers)),
        ))
        for number in range(len(self.layers)):
            marks.append(MarkSpec(
                POLYLINE, 3, BASE_COLOURS[number % len(BASE_COLOURS)], f"layer{number}", offset=start, count=self.width,
                size=line_size(side), alpha=HALF,
            ))
        marks.append(MarkSpec(CURSOR, 3, RED, size=line_size(side)))
        axes.append(AxisSpec(*rectangles[4][:4], _x_limits(self.width), index_limits, titles[4], rectangles[4][4]))
        marks.append(MarkSpec(POINTS, 4, CYAN, "indices", offset=start, count=self.width, size=point_size(side)))
        marks.append(MarkSpec(CURSOR, 4, RED, size=line_size(side)))
        axes.append(AxisSpec(*rectangles[5][:4], index_limits, (0.0, 1.0), titles[5], rectangles[5][4]))
        marks.append(MarkSpec(BAR, 5, MAGENTA, "indices", count=1, frame_stride=1))
        return PanelWindow(start, min(self.width, self.num_frames - start), axes, marks)


def _values(contexts: Sequence[OverlayContext], field: str) -> np.ndarray:
    return np.array([np.nan if getattr(context, field) is None else float(getattr(context, field)) for context in contexts], dtype=np.float64)


def overlay_limits(values: Sequence[np.ndarray]) -> Tuple[float, float]:
    """min - 5 .. max + 5 of the values that filter(None, ...) keeps (not None, not 0), else -5 .. 5 (overlay_visualization.py:98-115)."""
    kept = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in values]) if values else np.zeros(0)
    kept = kept[np.isfinite(kept) & (kept != 0)]
    return (float(kept.min()) - 5.0, float(kept.max()) + 5.0) if kept.size else (-5.0, 5.0)


class OverlayPanel:
    """
    "Overlay computation": the hash axis over the box-distance axis, for windows of `window` contexts. The series of a
    window ("bbox_phash", "image_phash", "bbox_distance": float64, NaN where the context has None) come with its tables.
    """

    def __init__(self, side: int, window: Optional[int], phash_distance: float, bbox_distance: float) -> None:
        if window is None:
            raise ValueError("the overlay panel of the debug video needs debug_window (frames per context)")
        if int(window) < 1:
            raise ValueError(f"debug_window must be >= 1, got {window}")
        self.side, self.width = side, int(window)
        self.phash_distance, self.bbox_distance = float(phash_distance), float(bbox_distance)

    def window_of(self, frame: int) -> int:
        return frame // self.width

    def cursor(self, frame: int) -> float:
        return float(frame % self.width)

    def window(self, index: int, contexts: Sequence[OverlayContext]) -> Tuple[PanelWindow, Dict[str, np.ndarray]]:
        """Tables and series of window `index`, whose contexts (all of them, at most `window`) are `contexts`."""
        side, count = self.side, len(contexts)
        series = {
            "bbox_phash": _values(contexts, "bbox_perceptual_hash_distance"),
            "image_phash": _values(contexts, "image_perceptual_hash_distance"),
            "bbox_distance": _values(contexts, "bbox_distance"),
        }
        rectangles = stacked_rectangles(side, ((0, 1), (1, 2)), 2)
        axes = [
            AxisSpec(
                *rectangles[0][:4], _x_limits(count), overlay_limits([series["bbox_phash"], series["image_phash"]]),
                "Overlay Discriminator (Image Hashing)", rectangles[0][4], legend=(("Bounding Boxes", RED), ("Complete Image", BLUE)),
                grid=True, hlines=((self.phash_distance, PURPLE),),
            ),
            AxisSpec(
                *rectangles[1][:4], _x_limits(count), overlay_limits([series["bbox_distance"]]),
                "Overlay Discriminator (Face Tracking)", rectangles[1][4], legend=(("Bounding Box Distance", GREEN),),
                grid=True, hlines=((self.bbox_distance, PURPLE),),
            ),
        ]
        marks = [
            MarkSpec(POINTS, 0, RED, "bbox_phash", count=count, size=point_size(side)),
            MarkSpec(POINTS, 0, BLUE, "image_phash", count=count, size=point_size(side)),
            MarkSpec(POINTS, 1, GREEN, "bbox_distance", count=count, size=point_size(side)),
        ]
        for axis in (0, 1):  # the cursor is green where the frame's gate flag is set, red otherwise (:216-224)
            marks.append(MarkSpec(CURSOR, axis, GREEN, size=line_size(side), flag_mask=FLAG_OVERLAY_WRITTEN, flag_value=FLAG_OVERLAY_WRITTEN))
            marks.append(MarkSpec(CURSOR, axis, RED, size=line_size(side), flag_mask=FLAG_OVERLAY_WRITTEN, flag_value=0))
        return PanelWindow(index * self.width, count, axes, marks), series


class MaskPanel:
    """
    "Overlay binary mask": the music-complexity ResultLayers in windows of `window` points: the result as a thick red
    line, the layers dashed at alpha 0.5, the threshold dotted. Host series: "result", "layer<k>" (float64, NaN kept).
    """

    def __init__(self, side: int, result_layers: ResultLayers, window: Optional[int], threshold: Optional[float], title: str = "Overlay binary mask") -> None:
        if window is None:
            raise ValueError("the mask panel of the debug video needs debug_window (points per context)")
        self.side, self.width, self.threshold, self.title = side, int(window), threshold, title
        self.result_label = result_layers.result.label
        self.layer_labels = [layer.label for layer in result_layers.layers]
        self.values = [np.asarray(result_layers.result.data, dtype=np.float64)] + [
            np.asarray(layer.data, dtype=np.float64) for layer in result_layers.layers
        ]
        self.num_points = int(self.values[0].shape[0])

    def host_series(self) -> Dict[str, np.ndarray]:
        series = {"result": self.values[0]}
        for number, values in enumerate(self.values[1:]):
            series[f"layer{number}"] = values
        return series

    def window_of(self, frame: int) -> int:
        return frame // self.width

    def cursor(self, frame: int) -> float:
        return float(frame % self.width)

    def window(self, index: int) -> PanelWindow:
        side, start = self.side, index * self.width
        count = max(0, min(self.width, self.num_points - start))
        kept = np.concatenate([values[start : start + count] for values in self.values])
        kept = kept[~np.isnan(kept)]
        limits = (float(kept.min()) - 10.0, float(kept.max()) + 10.0) if kept.size else (-10.0, 10.0)
        x, y, width, height, titled = stacked_rectangles(side, ((0, 1),), 1)[0]
        legend = ((self.result_label, RED),) + tuple((label, BASE_COLOURS[k % len(BASE_COLOURS)]) for k, label in enumerate(self.layer_labels))
        axes = [AxisSpec(
            x, y, width, height, _x_limits(count), limits, self.title, titled, legend=legend, grid=True,
            hlines=((float(self.threshold), PURPLE),) if self.threshold is not None else (),
        )]
        marks = [MarkSpec(POLYLINE, 0, RED, "result", offset=start, count=count, size=thick_line_size(side))]
        for number in range(len(self.layer_labels)):
            marks.append(MarkSpec(
                POLYLINE, 0, BASE_COLOURS[number % len(BASE_COLOURS)], f"layer{number}", offset=start, count=count,
                size=medium_line_size(side), alpha=HALF, dash=dash_pattern(side),
            ))
        marks.append(MarkSpec(CURSOR, 0, RED, size=line_size(side)))
        return PanelWindow(start, count, axes, marks)
