"""
Analysis videos of a projection file (gance/projection/projection_visualization.py): how did the projection converge,
and does step k already look like the target?

    visualize_final_latents              [latents panel | target | final image], one frame per projected frame
    visualize_projection_history         [latents panel | image of the step | target], every step of every projected frame
    visualize_partial_projection_history [latents panel | image of that step | target | final image], one frame per
                                         projected frame
    projection_convergence               the data half of visualize_projection_convergence (the spline figure is
                                         matplotlib's and is not built)

The reference renders one image per call through a worker process and one matplotlib canvas per frame. Here a chunk of up
to 64 frames is one engine call (the W entry with the stored noise, as `create_image_matrix`), its plot panels are
rasterised in HBM (gance_amd/debug_video/latents_panel.py) and its image panels resized and placed there
(torch.ops.gance.resize_bicubic, gance_debug_place_panels_u8). Every `visualize_*` function has a `*_frame_chunks` twin that
yields (first frame, uint8 [n, H, W, 3] in HBM); the videos are those chunks through torch.ops.gance.jpeg_encode_rect into
a Motion-JPEG AVI without audio. Panels are squares of `video_height`, which must be a multiple of 16 in [16, 4096].

All arguments are checked, and the small parts of the file read, when a function is called; nothing is loaded onto,
allocated on or launched on the GPU before the first chunk is asked for. The latent histories (GBs in a real file) are
read chunk by chunk, and the target and final images one projected frame at a time: one image of each is in HBM at once.
"""

import hashlib
import itertools
from pathlib import Path
from typing import Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from gance_amd import hip_lib, torch_ops  # noqa: F401  (torch_ops registers torch.ops.gance.*)
from gance_amd.data_into_network_visualization.vectors_to_image import CHUNK_FRAMES, write_chunks_to_avi
from gance_amd.debug_video import compose
from gance_amd.debug_video.latents_panel import LatentsPanel, LatentsPanelDrawer, fit_title, title_glyphs
from gance_amd.network_interface.network_functions import LoadedNetwork
from gance_amd.projection.projection_file_reader import ProjectionFileReader, final_latents_matrices_label, load_projection_file

PLACE_ONE_SOURCE = 1 << 30  # a divisor larger than any frame number: every frame of a call shows source 0


class Convergence(NamedTuple):
    """What `projection_convergence` returns."""

    lines: List[np.ndarray]  # per projected frame: sum |final - latents| at every projection step
    points_of_interest: List[int]  # per projected frame: the first step whose line is <= 0.2 * (max - min)
    average: int
    standard_deviation: int


def projection_convergence(projection_file_path: Path, consider_first_n_frames: Optional[int] = None) -> Convergence:
    """
    The numbers behind the reference's convergence figure (:74-106), computed on the host: how far every step of a
    frame's latent history is from the frame's final latents, the step at which a projection is "80 % complete" by the
    reference's heuristic, and the integer mean and standard deviation of those steps.
    :raises ValueError: the file holds no latent histories.
    """
    with load_projection_file(projection_file_path) as reader:
        lines = [
            np.array([np.sum(np.abs(final - latents)) for latents in history])
            for history, final in itertools.islice(zip(reader.latents_histories, reader.final_latents), consider_first_n_frames)
        ]
        if not lines or not reader.projection_attributes.latents_histories_enabled:
            raise ValueError("File doesn't contain the data to visualize.")
    points = [int(np.where(line <= (line.max() - line.min()) * 0.2)[0][0]) for line in lines]
    return Convergence(lines, points, int(np.mean(points)), int(np.std(points)))


# ---- what is read when a function is called ---------------------------------------------------------------------------
class _Setup(NamedTuple):
    side: int
    label: str
    vector_length: int
    num_rows: int
    limits: Tuple[float, float]  # min / max of the FINAL latents, also for history frames (_setup_visualization)
    final_latents: np.ndarray  # [F, W, L] float32


def _check_square_images(images: Iterator[np.ndarray], what: str) -> None:
    """One image at a time, none kept. :raises ValueError: an image that is not a square [s, s, 3]."""
    for image in images:
        shape = np.shape(image)
        if len(shape) != 3 or shape[2] != 3 or shape[0] != shape[1]:
            raise ValueError(f"the {what} images of a projection file must be squares [s, s, 3], got {shape}")


def _setup(reader: ProjectionFileReader, video_height: Optional[int]) -> _Setup:
    side = compose.validate_side_length(video_height)
    matrices_label = final_latents_matrices_label(reader)
    data = np.asarray(matrices_label.data, dtype=np.float32)
    length = int(matrices_label.vector_length)
    final_latents = np.ascontiguousarray(np.stack(np.split(data, data.shape[-1] // length, axis=-1)))
    _check_square_images(reader.target_images, "target")
    _check_square_images(reader.final_images, "final")
    return _Setup(side, matrices_label.label, length, int(data.shape[0]), (float(data.min()), float(data.max())), final_latents)


def _check_network(reader: ProjectionFileReader, projection_network_path: Path, network_not_matching_ok: bool) -> None:
    """:raises ValueError: the network file is not the one the projection was made with (before it is loaded)."""
    if network_not_matching_ok:
        return
    digest = hashlib.md5()
    with open(projection_network_path, "rb") as handle:
        for block in iter(lambda: handle.read(1 << 20), b""):
            digest.update(block)
    if digest.hexdigest() != reader.projection_attributes.network_md5_hash:
        raise ValueError("Input network was not the one used in projection.")


def _panel(setup: _Setup, static_title: bool) -> LatentsPanel:
    """The video's latents panel (host tables only). :raises ValueError: more latent rows than a panel draws."""
    return LatentsPanel(setup.side, setup.vector_length, setup.num_rows, *setup.limits, setup.label if static_title else None)


# ---- composing in HBM ----------------------------------------------------------------------------------------------------
class _ImageStream:  # pylint: disable=too-few-public-methods
    """The images of one group of the file, asked for in ascending frame order: only the current one is held."""

    def __init__(self, images: Iterator[np.ndarray]) -> None:
        self._images, self._next, self._frame, self._current = images, 0, -1, None

    def at(self, frame: int) -> Optional[np.ndarray]:
        """Image `frame` [s, s, 3] uint8, or None where the file holds fewer images."""
        if frame < self._frame:
            raise ValueError("the images of a projection file are read in ascending order")
        while self._frame < frame:
            self._current = next(self._images, None)
            self._frame += 1
        return None if self._current is None else np.ascontiguousarray(self._current, dtype=np.uint8)


class _Composer:
    """The panels of one video on one device; every method enqueues on the device's current stream."""

    def __init__(self, setup: _Setup, panel: LatentsPanel, panel_count: int, reader: ProjectionFileReader) -> None:
        self.setup, self.side, self.panel_count = setup, setup.side, panel_count
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.drawer = LatentsPanelDrawer(panel, self.device)
        self._images = {"targets": _ImageStream(iter(reader.target_images)), "finals": _ImageStream(iter(reader.final_images))}

    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def new_chunk(self, count: int) -> torch.Tensor:
        return torch.empty((count, self.side, self.panel_count * self.side, 3), dtype=torch.uint8, device=self.device)

    def fit(self, images: torch.Tensor) -> torch.Tensor:
        """[n, s, s, 3] uint8 in HBM at the panel's side."""
        if int(images.shape[1]) != self.side:
            images = torch.ops.gance.resize_bicubic(images, self.side)
        return images.contiguous()

    def place(self, out: torch.Tensor, panel: int, images: torch.Tensor) -> None:
        """Frame b of `out` shows images[b] (already at the panel's side)."""
        hip_lib.debug_place_panels_device(
            images.data_ptr(), int(images.shape[0]), self.side, 0, 1, 0, int(out.shape[0]), out.data_ptr() + panel * self.side * 3,
            out.stride(0), out.stride(1), self.stream(),
        )
        images.record_stream(torch.cuda.current_stream(self.device))

    def place_file_images(self, out: torch.Tensor, panel: int, name: str, frames: Sequence[int]) -> None:
        """
        Frame b of `out` shows image frames[b] of the file (`frames` ascending, over the whole video), or black where the
        file has no such image. An image is uploaded and resized once per run of equal frames of a chunk.
        """
        begin = 0
        for frame, run in itertools.groupby(frames):
            count = len(list(run))
            rows = out[begin : begin + count]
            host = self._images[name].at(frame)
            if host is None:
                rows[:, :, panel * self.side : (panel + 1) * self.side].zero_()
            else:
                image = self.fit(compose._upload(host[None], self.device))  # pylint: disable=protected-access
                hip_lib.debug_place_panels_device(
                    image.data_ptr(), 1, self.side, 0, PLACE_ONE_SOURCE, 0, count, rows.data_ptr() + panel * self.side * 3,
                    rows.stride(0), rows.stride(1), self.stream(),
                )
                image.record_stream(torch.cuda.current_stream(self.device))
            begin += count


def _synthesize(network: LoadedNetwork, latents: torch.Tensor) -> torch.Tensor:
    """One call of the engine's W entry with the stored noise: what create_image_matrix makes of every matrix."""
    engine = network.engine
    if int(latents.shape[2]) != engine.vector_length or int(latents.shape[1]) < engine.num_layers:
        raise ValueError(
            f"the network takes latents [{engine.num_layers}, {engine.vector_length}], the projection file holds {tuple(latents.shape[1:])}"
        )
    engine.restore_noise(stream=torch.cuda.current_stream(latents.device).cuda_stream)
    return torch.ops.gance.synthesize_w(latents[:, : engine.num_layers, :].contiguous(), engine.op_handle)


def _check_chunk_frames(chunk_frames: int) -> int:
    if int(chunk_frames) < 1:
        raise ValueError(f"chunk_frames must be >= 1, got {chunk_frames}")
    return int(chunk_frames)


# ---- the chunk generators ----------------------------------------------------------------------------------------------
def final_latents_frame_chunks(
    projection_file_path: Path, video_height: Optional[int] = 1024, chunk_frames: int = CHUNK_FRAMES
) -> Iterator[Tuple[int, torch.Tensor]]:
    """
    The frames of `visualize_final_latents` in HBM: [latents panel | target | final image] per projected frame, the
    panel titled with the file's label. Needs no network and no engine.
    :raises ValueError: (when called) a bad `video_height`, or target / final images that are not squares.
    """
    chunk_frames = _check_chunk_frames(chunk_frames)
    with load_projection_file(projection_file_path) as reader:
        setup = _setup(reader, video_height)
    panel = _panel(setup, static_title=True)

    def chunks() -> Iterator[Tuple[int, torch.Tensor]]:
        with load_projection_file(projection_file_path) as reader:
            composer = _Composer(setup, panel, 3, reader)
            total = int(setup.final_latents.shape[0])
            for first in range(0, total, chunk_frames):
                frames = list(range(first, min(total, first + chunk_frames)))
                latents = compose._upload(setup.final_latents[frames[0] : frames[-1] + 1], composer.device)  # pylint: disable=protected-access
                out = composer.new_chunk(len(frames))
                composer.drawer.draw(out, 0, latents, range(len(frames)))
                composer.place_file_images(out, 1, "targets", frames)
                composer.place_file_images(out, 2, "finals", frames)
                yield first, out

    return chunks()


def projection_history_frame_chunks(  # pylint: disable=too-many-arguments,too-many-locals
    projection_file_path: Path, projection_network_path: Path, network_not_matching_ok: bool, video_height: Optional[int] = 1024,
    start_frame_index: Optional[int] = None, end_frame_index: Optional[int] = None, chunk_frames: int = CHUNK_FRAMES,
) -> Iterator[Tuple[int, torch.Tensor]]:
    """
    The frames of `visualize_projection_history` in HBM: [latents panel | synthesized image | target] for every step of
    every projected frame of islice(start_frame_index, end_frame_index), frame-major, step-minor. The panel's title is
    f"{label} frame: {projected frame}, step: {step}", fitted to the title line by `latents_panel.fit_title`: where the line is
    too short the label is cut, not the frame and step (at small sides only "frame:step" is left). A chunk is one upload of its step latents and one engine call, and
    may span projected frames; the network is loaded with `chunk_frames` as its batch when the first chunk is asked for.
    :raises ValueError: (when called) a bad `video_height`, images that are not squares, or, unless
    `network_not_matching_ok`, a network file whose md5 is not the file's `network_md5_hash`.
    """
    chunk_frames = _check_chunk_frames(chunk_frames)
    with load_projection_file(projection_file_path) as reader:
        setup = _setup(reader, video_height)
        _check_network(reader, projection_network_path, network_not_matching_ok)
    panel = _panel(setup, static_title=False)

    def steps(reader: ProjectionFileReader) -> Iterator[Tuple[int, int, np.ndarray]]:
        for frame, history in itertools.islice(enumerate(reader.latents_histories), start_frame_index, end_frame_index):
            for step, latents in enumerate(history):
                yield frame, step, latents

    def chunks() -> Iterator[Tuple[int, torch.Tensor]]:
        network = LoadedNetwork(projection_network_path, max_batch=chunk_frames, device=torch.cuda.current_device())
        try:
            with load_projection_file(projection_file_path) as reader:
                composer = _Composer(setup, panel, 3, reader)
                glyphs = title_glyphs(*composer.drawer.title_box[2:]) if composer.drawer.title_box is not None else 0
                stream, first = steps(reader), 0
                while True:
                    taken = list(itertools.islice(stream, chunk_frames))
                    if not taken:
                        break
                    latents = compose._upload(np.stack([matrix for _, _, matrix in taken]).astype(np.float32), composer.device)  # pylint: disable=protected-access
                    out = composer.new_chunk(len(taken))
                    titles = [fit_title(setup.label, f" frame: {frame}, step: {step}", f"{frame}:{step}", glyphs) for frame, step, _ in taken]
                    composer.drawer.draw(out, 0, latents, range(len(taken)), titles)
                    composer.place(out, 1, composer.fit(_synthesize(network, latents)))
                    composer.place_file_images(out, 2, "targets", [frame for frame, _, _ in taken])
                    yield first, out
                    first += len(taken)
        finally:
            network.stop()

    return chunks()


def partial_projection_history_frame_chunks(  # pylint: disable=too-many-arguments,too-many-locals
    projection_file_path: Path, projection_network_path: Path, network_not_matching_ok: bool, projection_step_to_take: int,
    video_height: Optional[int] = 1024, chunk_frames: int = CHUNK_FRAMES,
) -> Iterator[Tuple[int, torch.Tensor]]:
    """
    The frames of `visualize_partial_projection_history` in HBM: [latents panel | image of step `projection_step_to_take`
    | target | final image] per projected frame, the panel titled with the file's label. Ends at the first projected
    frame whose history is shorter than the step, as the reference's islice does.
    :raises ValueError: (when called) as `projection_history_frame_chunks`, or a negative step.
    """
    chunk_frames = _check_chunk_frames(chunk_frames)
    step = int(projection_step_to_take)
    if step < 0:
        raise ValueError(f"projection_step_to_take must be >= 0, got {projection_step_to_take}")
    with load_projection_file(projection_file_path) as reader:
        setup = _setup(reader, video_height)
        _check_network(reader, projection_network_path, network_not_matching_ok)
    panel = _panel(setup, static_title=True)

    def matrices(reader: ProjectionFileReader) -> Iterator[np.ndarray]:
        for history in reader.latents_histories:
            taken = list(itertools.islice(history, step, step + 1))
            if not taken:
                return
            yield taken[0]

    def chunks() -> Iterator[Tuple[int, torch.Tensor]]:
        network = LoadedNetwork(projection_network_path, max_batch=chunk_frames, device=torch.cuda.current_device())
        try:
            with load_projection_file(projection_file_path) as reader:
                composer = _Composer(setup, panel, 4, reader)
                stream, first = matrices(reader), 0
                while True:
                    taken = list(itertools.islice(stream, chunk_frames))
                    if not taken:
                        break
                    frames = list(range(first, first + len(taken)))
                    latents = compose._upload(np.stack(taken).astype(np.float32), composer.device)  # pylint: disable=protected-access
                    out = composer.new_chunk(len(taken))
                    composer.drawer.draw(out, 0, latents, range(len(taken)))
                    composer.place(out, 1, composer.fit(_synthesize(network, latents)))
                    composer.place_file_images(out, 2, "targets", frames)
                    composer.place_file_images(out, 3, "finals", frames)
                    yield first, out
                    first += len(taken)
        finally:
            network.stop()

    return chunks()


# ---- the videos ------------------------------------------------------------------------------------------------------------
def _fps_of(projection_file_path: Path) -> float:
    with load_projection_file(projection_file_path) as reader:
        fps = reader.projection_attributes.projection_fps
    if not fps or float(fps) <= 0.0:
        raise ValueError(f"the projection file has no usable projection_fps ({fps})")
    return float(fps)


def _video_side(video_height: Optional[int], panel_count: int) -> int:
    """:raises ValueError: a bad `video_height`, or a row of panels wider than the JPEG encoder takes (8192)."""
    side = compose.validate_side_length(video_height)
    if panel_count * side > 8192:
        raise ValueError(f"{panel_count} panels of {side} pixels are wider than the 8192 the JPEG encoder takes")
    return side


def visualize_final_latents(  # pylint: disable=too-many-arguments
    projection_file_path: Path, output_video_path: Path, video_height: Optional[int] = 1024, jpeg_quality: int = 90,
    jpeg_huffman: str = "standard",
) -> None:
    """The target next to the final projection, with the final latents (:214-267), at the projection's fps. `jpeg_huffman`:
    "standard" or "optimized" (each frame's own Huffman tables: the same pixels, smaller files), as write_chunks_to_avi takes it."""
    side = _video_side(video_height, 3)
    chunks = final_latents_frame_chunks(projection_file_path, side)
    write_chunks_to_avi(chunks, Path(output_video_path), 3 * side, side, _fps_of(projection_file_path), jpeg_quality, jpeg_huffman)


def visualize_projection_history(  # pylint: disable=too-many-arguments
    projection_file_path: Path, output_video_path: Path, projection_network_path: Path, network_not_matching_ok: bool,
    video_height: Optional[int] = 1024, start_frame_index: Optional[int] = None, end_frame_index: Optional[int] = None,
    jpeg_quality: int = 90, jpeg_huffman: str = "standard",
) -> None:
    """Every latent of every projection history as it approaches the target (:308-381), at the projection's fps. `jpeg_huffman`:
    see visualize_final_latents."""
    side = _video_side(video_height, 3)
    chunks = projection_history_frame_chunks(
        projection_file_path, projection_network_path, network_not_matching_ok, side, start_frame_index, end_frame_index
    )
    write_chunks_to_avi(chunks, Path(output_video_path), 3 * side, side, _fps_of(projection_file_path), jpeg_quality, jpeg_huffman)


def visualize_partial_projection_history(  # pylint: disable=too-many-arguments
    projection_file_path: Path, output_video_path: Path, projection_network_path: Path, network_not_matching_ok: bool,
    projection_step_to_take: int, video_height: Optional[int] = 1024, jpeg_quality: int = 90, jpeg_huffman: str = "standard",
) -> None:
    """What taking step `projection_step_to_take` instead of the final latents does to every frame (:384-451), at 1 fps.
    `jpeg_huffman`: see visualize_final_latents."""
    side = _video_side(video_height, 4)
    chunks = partial_projection_history_frame_chunks(
        projection_file_path, projection_network_path, network_not_matching_ok, projection_step_to_take, side
    )
    write_chunks_to_avi(chunks, Path(output_video_path), 4 * side, side, 1.0, jpeg_quality, jpeg_huffman)
