"""
Composes the debug video's frames in HBM: image panels (bicubic resize + strided placement) and plot panels (chrome
template + marks, gance_amd/csrc/debug_panels.hip) side by side, as horizontal_concat_images does in the reference
(gance/projection_file_blend.py:302-334). Everything is enqueued on the current stream; nothing waits for the GPU.
"""

import ctypes
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from gance_amd import hip_lib, torch_ops  # noqa: F401  (torch_ops registers torch.ops.gance.*)
from gance_amd.data_into_network_visualization.visualization_common import ResultLayers
from gance_amd.debug_video import panels
from gance_amd.overlay.overlay_common import OverlayContext


class DebugVideo(NamedTuple):
    """
    The keyword-only `debug` argument of projection_file_blend_frame_chunks and noise_blend_frame_chunks: what the debug stream looks like and who
    receives it. `on_encoded(first_frame, EncodedFrames)` gets every chunk of JPEG-encoded debug frames in frame
    order; `on_composed(first_frame, frames [n, side, P * side, 3] uint8 in HBM)`, if given, sees the raw frames
    first (on the reader stream: copy what is to be kept). `jpeg_huffman`: "standard" (the Annex K tables) or "optimized"
    (each frame's own tables; a debug frame is mostly flat panels, where they save the most).
    """

    side_length: int
    window: Optional[int]
    on_encoded: Callable[[int, object], None]
    on_composed: Optional[Callable[[int, torch.Tensor], None]] = None
    jpeg_quality: int = 90
    jpeg_huffman: str = "standard"


class DebugSources(NamedTuple):
    """What rank 0 keeps of the blend for the debug panels (see _prepare_blend_inputs)."""

    a_vectors: torch.Tensor  # [N, L] float64 in HBM: blend stage `final`
    b_vectors: torch.Tensor  # [F, L] float32 in HBM: row 0 of the projected latents
    limits: Dict[str, Tuple[float, float]]  # global min / max of "a", "b", "combined"
    labels: Dict[str, str]
    network_indices: ResultLayers  # host: the indices and the layer(s) they were quantised from
    final_images: Optional[np.ndarray] = None  # [F, s, s, 3] uint8: reader.final_images; None (noise-blend): no such panel


class PanelLayout(NamedTuple):
    """Where the panels of a debug frame sit, counted in panels from the left; None: the panel is not there."""

    panel_count: int
    foreground: Optional[int]
    final_images: Optional[int]
    synthesis: int
    overlay: Optional[int]
    mask: Optional[int]


def panel_layout(final_images: bool, overlay: bool, mask: bool) -> PanelLayout:
    """
    The row of panels a debug frame is (pure host arithmetic): blended output, foreground (overlay on), final images (a
    projection file's), synthesis inputs, overlay computation (overlay on), overlay binary mask (music mask on).
    projection-file-blend has 3 / 5 / 6 of them, noise-blend (no final images, no overlay) 2.
    """
    order = ["output"] + ["foreground"] * overlay + ["final_images"] * final_images + ["synthesis"] + ["overlay"] * overlay + ["mask"] * mask
    at = {name: order.index(name) if name in order else None for name in ("foreground", "final_images", "synthesis", "overlay", "mask")}
    return PanelLayout(len(order), at["foreground"], at["final_images"], at["synthesis"], at["overlay"], at["mask"])


def synthesis_panel_of(side: int, window: Optional[int], frame_multiplier: int, sources: DebugSources, combined: torch.Tensor) -> panels.SynthesisPanel:
    """
    The synthesis-inputs panel of a run (host tables only): input B advances once per `frame_multiplier` frames, and the
    combined series is read `combined.stride(0)` elements apart: 18 L for latent matrices [N, 18, L] (their row 0), L for
    z vectors [N, L].
    """
    return panels.SynthesisPanel(
        side, int(sources.a_vectors.shape[1]), sources.limits, sources.labels, sources.network_indices, window, int(frame_multiplier),
        combined_stride=int(combined.stride(0)),
    )


def validate_side_length(debug_side_length: Optional[int]) -> int:
    """:raises ValueError: no side, or one the JPEG encoder cannot take (not a multiple of 16 in [16, 4096])."""
    if debug_side_length is None:
        raise ValueError("debug_path needs debug_side_length")
    side = int(debug_side_length)
    if side < 16 or side > 4096 or side % 16 != 0:
        raise ValueError(f"debug_side_length must be a multiple of 16 in [16, 4096], got {debug_side_length}")
    return side


def bind_marks(marks: Sequence[panels.MarkSpec], series: Dict[str, torch.Tensor]) -> List[hip_lib.DebugMark]:
    """MarkSpecs -> `gance_debug_mark`s reading the tensors of `series` (contiguous, in HBM)."""
    bound = []
    for spec in marks:
        mark = hip_lib.DebugMark()
        mark.kind, mark.axis, mark.size = spec.kind, spec.axis, spec.size
        mark.frame_stride, mark.frame_divisor, mark.count = spec.frame_stride, spec.frame_divisor, spec.count
        mark.dash_on, mark.dash_off = spec.dash
        mark.flag_mask, mark.flag_value = spec.flag_mask, spec.flag_value
        mark.rgba = (ctypes.c_uint8 * 4)(*spec.colour, spec.alpha)
        mark.x_start = spec.x_start
        if spec.series is not None:
            tensor = series[spec.series]
            if not tensor.is_contiguous():
                raise ValueError(f"series {spec.series!r} must be contiguous")
            mark.dtype = hip_lib.DEBUG_DTYPES[np.dtype(str(tensor.dtype).replace("torch.", ""))]
            mark.data = tensor.data_ptr() + spec.offset * tensor.element_size()
            mark.limit = max(0, tensor.numel() - spec.offset)
        bound.append(mark)
    return bound


def bind_axes(axes: Sequence) -> List[hip_lib.DebugAxis]:
    return [hip_lib.DebugAxis(a.x, a.y, a.width, a.height, a.x_limits[0], a.x_limits[1], a.y_limits[0], a.y_limits[1]) for a in axes]


def _upload(array: np.ndarray, device: torch.device) -> torch.Tensor:
    """A host array to HBM through pinned memory, without blocking the host."""
    return torch.from_numpy(np.ascontiguousarray(array)).pin_memory().to(device, non_blocking=True)


def frame_records(numbers: Sequence[int], cursors: Sequence[float], flags: Sequence[int]) -> np.ndarray:
    """`gance_debug_frame` records of consecutive frames."""
    records = np.zeros(len(numbers), dtype=hip_lib.DEBUG_FRAME_DTYPE)
    records["number"], records["cursor"], records["flags"] = numbers, cursors, flags
    return records


class DebugVideoComposer:  # pylint: disable=too-many-instance-attributes
    """
    `push(first, frames, foreground)` takes each released chunk of the stream in frame order (tensors in HBM, on the
    current stream) and returns the composed debug chunks that are complete: [(first, [n, side, P * side, 3] uint8)].
    Panels, each a square of `side` (panel_layout): blended output, foreground (overlay on), final images (each shown
    `frame_multiplier` times; only where the sources have them), synthesis inputs, overlay computation (overlay on),
    overlay binary mask (music mask on). `combined` is what the frames were synthesised from, [N, 18, L] latent matrices
    or [N, L] z vectors: the synthesis panel reads row 0 / the vector of each frame, `combined.stride(0)` elements apart.

    Only the overlay panel can make a chunk wait: its y limits need every context of the frame's window
    (overlay_visualization.py:155-206), and the overlay stage evaluates contexts chunk by chunk (`add_contexts`). A
    composed chunk is therefore held in HBM until the contexts reach the end of the window its last frame lies in, or
    the stream ends (`flush`): at most one window plus one chunk of debug frames is held.
    """

    def __init__(  # pylint: disable=too-many-arguments
        self, side: int, window: Optional[int], num_frames: int, frame_multiplier: int, sources: DebugSources, combined: torch.Tensor,
        device: torch.device, overlay_thresholds: Optional[Tuple[float, float]] = None, mask: Optional[ResultLayers] = None,
        mask_threshold: Optional[float] = None,
    ) -> None:
        self.side, self.num_frames, self.multiplier, self.device = validate_side_length(side), num_frames, int(frame_multiplier), device
        self._sources = sources
        self._synthesis = synthesis_panel_of(self.side, window, self.multiplier, sources, combined)
        self._overlay = panels.OverlayPanel(self.side, window, *overlay_thresholds) if overlay_thresholds is not None else None
        self._mask = panels.MaskPanel(self.side, mask, window, mask_threshold) if mask is not None else None
        self.layout = panel_layout(sources.final_images is not None, self._overlay is not None, self._mask is not None)
        self.panel_count = self.layout.panel_count
        self.width = self.panel_count * self.side
        self._series = {"a": sources.a_vectors, "b": sources.b_vectors, "combined": combined}
        self._series.update({f"synthesis.{name}": _upload(values, device) for name, values in self._synthesis.host_series().items()})
        if self._mask is not None:
            self._series.update({f"mask.{name}": _upload(values, device) for name, values in self._mask.host_series().items()})
        self._chrome: Dict[Tuple[str, int], torch.Tensor] = {}  # (panel, window) of the windows in use
        self._contexts: List[OverlayContext] = []
        self._pending: List[Tuple[int, torch.Tensor]] = []
        self.frames_held_max = 0
        # once, before the stream starts: the series uploaded above are read from the stream's side stream
        torch.cuda.current_stream(device).synchronize()

    # ---- pieces -------------------------------------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _place(self, out: torch.Tensor, panel: int, images: torch.Tensor, first_number: int, divisor: int, base: int) -> None:
        if int(images.shape[1]) != self.side:
            images = torch.ops.gance.resize_bicubic(images, self.side)
        images = images.contiguous()
        hip_lib.debug_place_panels_device(
            images.data_ptr(), int(images.shape[0]), self.side, first_number, divisor, base, int(out.shape[0]),
            out.data_ptr() + panel * self.side * 3, out.stride(0), out.stride(1), self._stream(),
        )
        images.record_stream(torch.cuda.current_stream(self.device))

    def _chrome_of(self, panel: str, window_index: int, window: panels.PanelWindow) -> torch.Tensor:
        key = (panel, window_index)
        if key not in self._chrome:
            for stale in [k for k in self._chrome if k[0] == panel]:  # (frames arrive in order: one window per panel is live)
                del self._chrome[stale]
            self._chrome[key] = _upload(window.chrome(self.side), self.device)
        return self._chrome[key]

    def _draw(  # pylint: disable=too-many-arguments
        self, out: torch.Tensor, panel: int, name: str, window_index: int, window: panels.PanelWindow, series: Dict[str, torch.Tensor],
        first: int, count: int, cursor: Callable[[int], float], flags: Sequence[int],
    ) -> None:
        """Frames [first, first + count) of the stream, rows [first - chunk_first ...) of `out`, all in one window."""
        numbers = list(range(first, first + count))
        records = _upload(frame_records(numbers, [cursor(n) for n in numbers], flags).view(np.uint8), self.device)
        chrome = self._chrome_of(name, window_index, window)
        hip_lib.debug_draw_panels_device(
            chrome.data_ptr(), self.side, bind_axes(window.axes), bind_marks(window.marks, series), records.data_ptr(), count,
            out.data_ptr() + panel * self.side * 3, out.stride(0), out.stride(1), self._stream(),
        )
        for tensor in (records, chrome, *series.values()):
            tensor.record_stream(torch.cuda.current_stream(self.device))

    @staticmethod
    def _runs(first: int, count: int, width: int) -> List[Tuple[int, int, int]]:
        """[first, first + count) split at multiples of `width`: (window index, first frame, frames)."""
        runs, frame = [], first
        while frame < first + count:
            stop = min(first + count, (frame // width + 1) * width)
            runs.append((frame // width, frame, stop - frame))
            frame = stop
        return runs

    def _prefixed(self, prefix: str) -> Dict[str, torch.Tensor]:
        return {name[len(prefix):]: tensor for name, tensor in self._series.items() if name.startswith(prefix)}

    # ---- the stream -----------------------------------------------------------------------------------------------------
    def add_contexts(self, contexts: Sequence[OverlayContext]) -> None:
        """The overlay stage's contexts of the next frames, in frame order, as soon as it has evaluated them."""
        self._contexts.extend(contexts)

    def push(self, first: int, frames: torch.Tensor, foreground: Optional[torch.Tensor] = None) -> List[Tuple[int, torch.Tensor]]:
        """One released chunk in; every debug chunk that is complete out."""
        count = int(frames.shape[0])
        out = torch.empty((count, self.side, self.width, 3), dtype=torch.uint8, device=self.device)
        self._place(out, 0, frames, first, 1, first)
        if self._overlay is not None:
            if foreground is None:
                raise ValueError("the debug video of an overlay run needs the foreground frames")
            self._place(out, self.layout.foreground, foreground, first, 1, first)
        if self.layout.final_images is not None:
            low, high = first // self.multiplier, (first + count - 1) // self.multiplier + 1
            if high > len(self._sources.final_images):
                raise ValueError("the projection file holds too few final images for the frames being written")
            self._place(out, self.layout.final_images, _upload(self._sources.final_images[low:high], self.device), first, self.multiplier, low)
        panel = self.layout.synthesis
        series = {"a": self._series["a"], "b": self._series["b"], "combined": self._series["combined"], **self._prefixed("synthesis.")}
        for window_index, start, frames_in_run in self._runs(first, count, self._synthesis.width):
            self._draw(
                out[start - first :], panel, "synthesis", window_index, self._synthesis.window(window_index), series, start,
                frames_in_run, self._synthesis.cursor, [0] * frames_in_run,
            )
        if self._mask is not None:
            mask_panel = self.layout.mask
            for window_index, start, frames_in_run in self._runs(first, count, self._mask.width):
                self._draw(
                    out[start - first :], mask_panel, "mask", window_index, self._mask.window(window_index), self._prefixed("mask."),
                    start, frames_in_run, self._mask.cursor, [0] * frames_in_run,
                )
        self._pending.append((first, out))
        self.frames_held_max = max(self.frames_held_max, sum(int(chunk.shape[0]) for _, chunk in self._pending))
        return self._release(final=False)

    def _release(self, final: bool) -> List[Tuple[int, torch.Tensor]]:
        ready = []
        while self._pending:
            first, out = self._pending[0]
            count = int(out.shape[0])
            if self._overlay is not None:
                width = self._overlay.width
                needed = min(self.num_frames, ((first + count - 1) // width + 1) * width)
                if len(self._contexts) < needed and not final:
                    break
                panel = self.layout.overlay  # (output, foreground, final images if any, synthesis inputs come first)
                for window_index, start, frames_in_run in self._runs(first, count, width):
                    contexts = self._contexts[window_index * width : (window_index + 1) * width]
                    window, host_series = self._overlay.window(window_index, contexts)
                    series = {name: _upload(values, self.device) for name, values in host_series.items()}
                    flags = [
                        panels.FLAG_OVERLAY_WRITTEN if self._contexts[n].overlay_written else 0 for n in range(start, start + frames_in_run)
                    ]
                    self._draw(out[start - first :], panel, "overlay", window_index, window, series, start, frames_in_run, self._overlay.cursor, flags)
            self._pending.pop(0)
            ready.append((first, out))
        return ready

    def flush(self) -> List[Tuple[int, torch.Tensor]]:
        """End of the stream: windows that will not fill any further are drawn with the contexts they have."""
        return self._release(final=True)
