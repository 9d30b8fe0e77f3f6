"""
The latents panel: a whole latent matrix [rows, L] as one scatter per row, each row in its own colour -- the reference's
`vector_visualizer` (gance/data_into_network_visualization/vectors_to_image.py:167-219), which
projection_visualization.py and `vectors_to_video` draw their frames with. Expressed as a `PanelWindow` of the debug
video's rasteriser (gance_debug_draw_panels_u8), so its pixels follow DESIGN.md section 9 item 7 with no new rule. A
title that changes with every frame is not part of the chrome: it is drawn on top by gance_debug_draw_text_u8
(DESIGN.md section 9 item 10).
"""

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from gance_amd import hip_lib
from gance_amd.debug_video import chrome, font, panels
from gance_amd.debug_video.chrome import AxisSpec, Colour
from gance_amd.debug_video.compose import _upload, bind_axes, bind_marks, frame_records

# infinite_colors() (visualization_common.py:169-176): matplotlib's BASE_COLORS in key order (b g r c m y k w), then its
# ten TABLEAU_COLORS, channel = floor(255 * value). Entry 7 is white, as in the reference: on the white panel row 7 of a
# matrix shows only where it covers the rows drawn before it.
ROW_COLOURS: Tuple[Colour, ...] = chrome.BASE_COLOURS + (
    (255, 255, 255),
    (0x1F, 0x77, 0xB4), (0xFF, 0x7F, 0x0E), (0x2C, 0xA0, 0x2C), (0xD6, 0x27, 0x28), (0x94, 0x67, 0xBD),
    (0x8C, 0x56, 0x4B), (0xE3, 0x77, 0xC2), (0x7F, 0x7F, 0x7F), (0xBC, 0xBD, 0x22), (0x17, 0xBE, 0xCF),
)
MAX_TEXT_STRIDE = 256  # gance_debug_draw_text_u8 takes no longer strings


class LatentsPanel:
    """
    Host tables of the panel. The series "latents" is float32 [n][num_rows][vector_length] in HBM; a frame's record number
    is its index into that array. `title` None: the title changes per frame and is drawn as text on top (`title_box`).
    """

    def __init__(self, side: int, vector_length: int, num_rows: int, y_min: float, y_max: float, title: Optional[str]) -> None:  # pylint: disable=too-many-arguments
        self.side, self.vector_length, self.num_rows = int(side), int(vector_length), int(num_rows)
        if self.vector_length < 1 or self.num_rows < 1:
            raise ValueError(f"a latents panel needs at least one row and one sample, got {num_rows} x {vector_length}")
        if self.num_rows > hip_lib.DEBUG_MAX_MARKS:
            raise ValueError(f"a latents panel draws at most {hip_lib.DEBUG_MAX_MARKS} rows, got {num_rows}")
        if not (np.isfinite(y_min) and np.isfinite(y_max)):
            raise ValueError(f"the limits of a latents panel must be finite, got {y_min} .. {y_max}")
        self.y_limits = (float(y_min) - 1.0, float(y_max) + 1.0)  # axis.set_ylim([y_min - 1, y_max + 1])
        self.title = title

    @property
    def colours(self) -> Tuple[Colour, ...]:
        """The colour of every row, in row order."""
        return tuple(ROW_COLOURS[row % len(ROW_COLOURS)] for row in range(self.num_rows))

    def window(self) -> panels.PanelWindow:
        """The one window of the panel: it is the same for every frame."""
        x, y, width, height, titled = chrome.stacked_rectangles(self.side, [(0, 1)], 1)[0]
        length = self.vector_length
        axes = [AxisSpec(x, y, width, height, (0.0, float(length)), self.y_limits, self.title or "", titled)]
        marks = [
            panels.MarkSpec(
                panels.POINTS, 0, colour, "latents", offset=row * length, count=length, frame_stride=self.num_rows * length,
                size=panels.point_size(self.side),
            )
            for row, colour in enumerate(self.colours)
        ]
        return panels.PanelWindow(0, 0, axes, marks)

    def title_box(self) -> Optional[Tuple[int, int, int, int]]:
        """
        (x, y, max_width, scale) of the per-frame title: on the axis' title line, left of the "lo .. hi" limits label
        render_chrome draws there (one glyph advance kept free), or over the whole axis width where it draws none. None:
        the panel is too small for a title line, or no column is left.
        """
        axis = self.window().axes[0]
        if not axis.titled:
            return None
        scale = font.scale_for_side(self.side)
        limits = f"{chrome.format_limit(axis.y_limits[0])} .. {chrome.format_limit(axis.y_limits[1])}"
        limits_x = axis.x + axis.width - font.text_size(limits, scale)[0]
        room = axis.width
        if limits_x >= axis.x + font.ADVANCE * scale:  # (render_chrome's condition with an empty title)
            room = limits_x - axis.x - font.ADVANCE * scale
        if room < 1:
            return None
        return axis.x, axis.y - chrome.title_height(self.side), room, scale


def title_glyphs(room: int, scale: int) -> int:
    """Whole glyphs that fit into `room` columns at `scale`: n glyphs are (6 n - 1) * scale columns wide."""
    return max(0, (room // scale + 1) // font.ADVANCE)


def fit_title(label: str, suffix: str, compact: str, glyphs: int) -> str:
    """
    A per-frame title of at most `glyphs` characters that keeps what changes from frame to frame: the first that fits of
    label + suffix; the label cut short and closed with ".." + suffix; the suffix alone, without its leading blanks;
    `compact`. Where none fits, `compact` (the text kernel clips it on the right).
    """
    if len(label) + len(suffix) <= glyphs:
        return label + suffix
    kept = glyphs - len(suffix) - 2
    if kept >= 1:
        return label[:kept] + ".." + suffix
    if len(suffix.lstrip()) <= glyphs:
        return suffix.lstrip()
    return compact


def encode_titles(titles: Sequence[str]) -> np.ndarray:
    """[n, stride] uint8, NUL padded: what gance_debug_draw_text_u8 reads (longer strings are cut at 256 bytes)."""
    encoded = [title.encode("ascii", "replace")[:MAX_TEXT_STRIDE] for title in titles]
    stride = max(1, min(MAX_TEXT_STRIDE, max(len(text) for text in encoded) + 1))
    out = np.zeros((len(encoded), stride), dtype=np.uint8)
    for row, text in zip(out, encoded):
        row[: len(text)] = np.frombuffer(text, dtype=np.uint8)
    return out


class LatentsPanelDrawer:
    """
    A LatentsPanel with its chrome in HBM. Nothing is uploaded or launched before the first `draw`. `title_box` is the
    panel's (None: no title line at this side, or no column left of the limits label; per-frame titles are then not drawn).
    """

    def __init__(self, panel: LatentsPanel, device: torch.device) -> None:
        self.panel, self.device = panel, device
        self._window = panel.window()
        self.title_box = panel.title_box()
        self._chrome: Optional[torch.Tensor] = None

    def draw(self, out: torch.Tensor, panel_index: int, latents: torch.Tensor, numbers: Sequence[int], titles: Optional[Sequence[str]] = None) -> None:
        """
        Panel `panel_index` (counted in panels from the left) of the frames out[:len(numbers)] ([n, side, P * side, 3] uint8
        in HBM): frame b shows latents[numbers[b]] (`latents` float32 [m, rows, L], contiguous, in HBM) and, for a panel
        without a static title, titles[b] (not drawn where `title_box` is None). Enqueued on the current stream of the device.
        """
        panel, side, count = self.panel, self.panel.side, len(numbers)
        if latents.dtype != torch.float32 or latents.dim() != 3 or tuple(latents.shape[1:]) != (panel.num_rows, panel.vector_length):
            raise ValueError(f"latents must be float32 [n, {panel.num_rows}, {panel.vector_length}], got {latents.dtype} {tuple(latents.shape)}")
        if count < 1 or min(numbers) < 0 or max(numbers) >= int(latents.shape[0]):
            raise ValueError("frame numbers outside the latents given")
        if (titles is not None) != (panel.title is None) or (titles is not None and len(titles) != count):
            raise ValueError("per-frame titles go with a panel without a static title, one per frame")
        stream = torch.cuda.current_stream(self.device)
        if self._chrome is None:
            self._chrome = _upload(self._window.chrome(side), self.device)
        records = _upload(frame_records(list(numbers), [0.0] * count, [0] * count).view(np.uint8), self.device)
        d_out = out.data_ptr() + panel_index * side * 3
        hip_lib.debug_draw_panels_device(
            self._chrome.data_ptr(), side, bind_axes(self._window.axes), bind_marks(self._window.marks, {"latents": latents}),
            records.data_ptr(), count, d_out, out.stride(0), out.stride(1), stream.cuda_stream,
        )
        used = [records, self._chrome, latents]
        box = self.title_box if titles is not None else None
        if box is not None:
            text = _upload(encode_titles(titles), self.device)
            x, y, room, scale = box
            hip_lib.debug_draw_text_device(
                text.data_ptr(), int(text.shape[1]), x, y, room, scale, chrome.BLACK, side, count, d_out, out.stride(0), out.stride(1),
                stream.cuda_stream,
            )
            used.append(text)
        for tensor in used:
            tensor.record_stream(stream)
