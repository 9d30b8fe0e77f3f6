"""
Reading video files back into frames: frames_in_video, VideoFrames and reduce_fps_take_every of
gance/image_sources/video_common.py:198-298. Where the reference asks cv2.VideoCapture for decoded frames, this reads the
Motion-JPEG AVIs (gance_amd/video/mjpeg_avi.py) the project writes and the baseline ones a user brings (4:2:2, 4:2:0,
4:4:4 or grey frames): the compressed bytes go through a pinned staging buffer into HBM and are decoded there
(torch.ops.gance.jpeg_decode_layouts), so a 2160^2 frame costs 0.25 MB of PCIe, not 14 MB.
"""

from pathlib import Path
from typing import Iterator, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from gance_amd import divisor, torch_ops  # noqa: F401  (torch_ops registers torch.ops.gance)
from gance_amd.gance_types import RGBInt8ImageType
from gance_amd.logger_common import LOGGER
from gance_amd.video.mjpeg_avi import MjpegAviReader


class ImageResolution(NamedTuple):
    """gance/image_sources/image_sources_common.py: width, then height."""

    width: int
    height: int


class VideoFrames(NamedTuple):
    """
    Contains metadata about the video, and an iterator that produces the frames.
    """

    original_fps: float
    total_frame_count: int
    original_resolution: ImageResolution
    frames: Iterator[RGBInt8ImageType]


def reduce_fps_take_every(original_fps: float, new_fps: Optional[float]) -> Optional[int]:
    """
    Every how many frames to take to bring a video from `original_fps` down to `new_fps`; None to take them all.
    :raises ValueError: `new_fps` does not go evenly into `original_fps`.
    """
    if new_fps is not None:
        whole = divisor.divide_no_remainder(numerator=original_fps, denominator=new_fps)
        if whole != 1:
            return int(whole)
    return None


def _open_video(
    video_path: Union[str, Path], video_fps: Optional[float], reduce_fps_to: Optional[float], width_height: Optional[Tuple[int, int]]
) -> Tuple[MjpegAviReader, Optional[int]]:
    """The open reader and take_every, after every check that needs no device."""
    try:
        reader = MjpegAviReader(video_path)
    except (OSError, ValueError) as error:
        raise ValueError(f"Couldn't open video file: {video_path} ({error})") from None
    try:
        file_fps = reader.fps
        if video_fps:
            if video_fps != file_fps:
                LOGGER.warning(
                    f"Override FPS of: {video_fps} fps "
                    f"did not match the fps from the file of: {file_fps} fps. "
                    f"Projected frames will not line up exactly."
                )
            fps = video_fps
        else:
            fps = file_fps
        take_every = reduce_fps_take_every(original_fps=fps, new_fps=reduce_fps_to)
        if width_height is not None and tuple(width_height) != (reader.width, reader.height):
            raise NotImplementedError(
                f"width_height {tuple(width_height)} differs from the file's {(reader.width, reader.height)}: the only resize "
                "kernel is the square bicubic one (torch.ops.gance.resize_bicubic), which is not what cv2.resize's default "
                "(bilinear) does; read at the file's resolution"
            )
    except BaseException:
        reader.close()
        raise
    return reader, take_every


def _device_chunks(reader: MjpegAviReader, take_every: Optional[int], frames_per_chunk: int, device: torch.device) -> Iterator[torch.Tensor]:
    """Closes the reader when the frames run out or the generator is dropped. Skipped frames are neither read nor decoded."""
    try:
        wanted = list(range(0, reader.frame_count, take_every or 1))
        pinned = torch.empty((0,), dtype=torch.uint8).pin_memory()
        for at in range(0, len(wanted), frames_per_chunk):
            indices = wanted[at : at + frames_per_chunk]
            offsets = np.zeros((len(indices) + 1,), dtype=np.int64)
            offsets[1:] = np.cumsum([reader.frame_sizes(index, 1)[0] for index in indices])
            if pinned.numel() < offsets[-1]:
                pinned = torch.empty((int(offsets[-1]) * 5 // 4,), dtype=torch.uint8).pin_memory()
            staging = pinned.numpy()
            for k, index in enumerate(indices):
                reader.read_frame_into(index, staging[offsets[k] : offsets[k + 1]])
            data = pinned[: int(offsets[-1])].to(device, non_blocking=True)
            frames = torch.ops.gance.jpeg_decode_layouts(data, torch.from_numpy(offsets))  # synchronises: `pinned` is free again
            if tuple(frames.shape[1:3]) != (reader.height, reader.width):
                raise ValueError(f"frames of {frames.shape[2]} x {frames.shape[1]} in a {reader.width} x {reader.height} video")
            yield frames
    finally:
        reader.close()


def frames_in_video_device_chunks(  # pylint: disable=too-many-arguments
    video_path: Union[str, Path],
    frames_per_chunk: int = 64,
    video_fps: Optional[float] = None,
    reduce_fps_to: Optional[float] = None,
    width_height: Optional[Tuple[int, int]] = None,
    device: Union[int, str, torch.device] = "cuda",
) -> Iterator[torch.Tensor]:
    """
    The frames `frames_in_video` yields, left in HBM: uint8 RGB tensors [n, H, W, 3], n <= frames_per_chunk, in order.
    Arguments and errors as `frames_in_video`; they are checked here, before the first chunk is asked for.
    """
    if frames_per_chunk < 1:
        raise ValueError(f"frames_per_chunk must be >= 1, got {frames_per_chunk}")
    reader, take_every = _open_video(video_path, video_fps, reduce_fps_to, width_height)
    return _device_chunks(reader, take_every, frames_per_chunk, torch.device(device))


def frames_in_video(
    video_path: Union[str, Path],
    video_fps: Optional[float] = None,
    reduce_fps_to: Optional[float] = None,
    width_height: Optional[Tuple[int, int]] = None,
) -> VideoFrames:
    """
    Creates an interface to read each frame from a video into local memory for analysis + manipulation.
    :param video_path: a Motion-JPEG AVI: what this project writes, or baseline 4:2:2, 4:2:0, 4:4:4 or grey frames from elsewhere.
    :param video_fps: Can be used to override the actual FPS of the video.
    :param reduce_fps_to: Discards frames such that the frames that are returned are at this FPS; they are not decoded.
    :param width_height: if given it must be the file's own resolution.
    :return: metadata about the video, and an iterator of host uint8 RGB frames [H, W, 3] in order.
    :raises ValueError: the video can't be opened, or the given `reduce_fps_to` is impossible.
    :raises NotImplementedError: `width_height` asks for a resize.
    """
    reader, take_every = _open_video(video_path, video_fps, reduce_fps_to, width_height)
    metadata = (reader.fps, reader.frame_count, ImageResolution(reader.width, reader.height))

    def frames() -> Iterator[RGBInt8ImageType]:
        for chunk in _device_chunks(reader, take_every, 64, torch.device("cuda")):
            host: List[np.ndarray] = list(chunk.cpu().numpy())
            yield from host

    return VideoFrames(original_fps=metadata[0], total_frame_count=metadata[1], original_resolution=metadata[2], frames=frames())
