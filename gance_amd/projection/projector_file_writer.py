"""
Project a video into a projection file: project_video_to_file of gance/projection/projector_file_writer.py:617-630, with the
projector of gance_amd/stylegan2/projector.py in the place of the per-frame TF1 process.

What differs from the reference, on purpose:
* frames are projected `frames_per_batch` at a time in this process (the reference starts one process per frame);
* the container is the `.npz` one ProjectionFileReader reads (there is no HDF5 writer here, and h5py is absent);
* a frame whose side is not the network's resolution goes through torch.ops.gance.resize_bicubic, where the reference
  uses cv2.resize's default, bilinear;
* `final_images` is the image of the final latents WITH the optimised noise planes (the reference re-synthesises with the
  network's stored noise);
* noises and images histories are refused: the reader has no counterpart for them.

Write protocol: after every batch a small file (attributes with complete=False, the final latents so far) replaces the
destination through a temporary file and os.replace, so a killed run leaves something to salvage; the full file with
complete=True is written once at the end, the same way.
"""

import itertools
import json
import os
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Tuple, Union

import numpy as np
import torch

from gance_amd.hash_file import hash_file
from gance_amd.logger_common import LOGGER
from gance_amd.projection.projection_file_reader import (
    FINAL_IMAGE_GROUP_NAME,
    FINAL_LATENTS_GROUP_NAME,
    LATENTS_HISTORIES_GROUP_NAME,
    LATEST_VERSION,
    TARGET_IMAGES_GROUP_NAME,
)
from gance_amd.video.mjpeg_avi import MjpegAviReader

DEFAULT_STEPS_PER_PROJECTION = 1000  # the value baked into the stylegan2 repo (projector_file_writer.py:679-680)

Frames = Union[np.ndarray, torch.Tensor]


def write_projection_npz_with_attributes(path: Path, attributes: Dict[str, Any], arrays: Dict[str, np.ndarray]) -> None:
    """
    The `.npz` container with every attribute given by the caller (`write_projection_npz` of the reader module fills in
    synthetic ones), written to a temporary file beside `path` and moved over it: a reader never sees half a file.
    """
    path = Path(path)
    temporary = path.with_name(path.name + ".partial.npz")
    np.savez(str(temporary), attributes=np.array(json.dumps(attributes)), **arrays)
    os.replace(str(temporary), str(path))


def _refusals(projection_file_path: Path, noises_histories_enabled: bool, images_histories_enabled: bool) -> None:
    if Path(projection_file_path).suffix != ".npz":
        raise NotImplementedError(
            f"{projection_file_path}: only the .npz container is written: there is no HDF5 writer here (h5py is absent, and "
            "gance_amd/projection/hdf5_lite.py only reads); give a path that ends in .npz"
        )
    if noises_histories_enabled:
        raise NotImplementedError("noises_histories_enabled: ProjectionFileReader has no reader for noises histories (and they make the file massive)")
    if images_histories_enabled:
        raise NotImplementedError("images_histories_enabled: ProjectionFileReader has no reader for images histories (and they make the file massive)")


def project_batches_to_file(  # pylint: disable=too-many-locals,too-many-arguments
    batches: Iterable[Frames],
    projector: Any,
    projection_file_path: Path,
    attributes: Dict[str, Any],
    latents_histories_enabled: bool = True,
    final_images_of: Optional[Callable[[Any], np.ndarray]] = None,
) -> int:
    """
    The loop of project_process_intermediate (projector_file_writer.py:576-613) over batches of target frames
    [n, R, R, 3] uint8, and the file. `projector` has the surface of gance_amd.stylegan2.projector.Projector;
    `final_images_of(projector)` gives the batch's final images uint8 [n, R, R, 3] (default: projector.final_images_device()).
    `attributes` holds everything but `complete` and `noises_shapes`. Returns the number of frames projected.
    """
    _refusals(projection_file_path, False, False)
    final_latents: List[np.ndarray] = []
    target_images: List[np.ndarray] = []
    final_images: List[np.ndarray] = []
    histories: List[np.ndarray] = []
    noises_shapes: Optional[List[List[int]]] = None

    def all_attributes(complete: bool) -> Dict[str, Any]:
        return {**attributes, "complete": complete, "noises_shapes": noises_shapes, "latents_histories_enabled": bool(latents_histories_enabled)}

    for batch in batches:
        count = int(batch.shape[0])
        LOGGER.info(f"Rendering projections {len(final_latents)} ... {len(final_latents) + count - 1}")
        projector.start(batch)
        steps: List[np.ndarray] = []
        while projector.get_cur_step() < projector.num_steps:
            projector.step()
            if latents_histories_enabled:
                steps.append(np.asarray(projector.get_dlatents(), dtype=np.float32))
        # one frame's planes, as the reference records them: [1, 1, S, S] per layer
        shapes = [[1, *np.shape(noise)[1:]] for noise in projector.get_noises()]
        if noises_shapes is not None and shapes != noises_shapes:
            LOGGER.warning(f"Noises shapes have changed mid projection! Was: {noises_shapes}, now: {shapes}")
        noises_shapes = noises_shapes or shapes
        latents = np.asarray(projector.get_dlatents(), dtype=np.float32)
        images = final_images_of(projector) if final_images_of is not None else projector.final_images_device().cpu().numpy()
        targets = batch.cpu().numpy() if isinstance(batch, torch.Tensor) else np.asarray(batch)
        for index in range(count):
            final_latents.append(latents[index])
            target_images.append(np.asarray(targets[index], dtype=np.uint8))
            final_images.append(np.asarray(images[index], dtype=np.uint8))
            if latents_histories_enabled:
                histories.append(np.stack([step[index] for step in steps]) if steps else np.zeros((0, *latents[index].shape), dtype=np.float32))
        write_projection_npz_with_attributes(projection_file_path, all_attributes(False), {FINAL_LATENTS_GROUP_NAME: np.stack(final_latents)})

    arrays: Dict[str, np.ndarray] = {}
    if final_latents:
        arrays = {
            FINAL_LATENTS_GROUP_NAME: np.stack(final_latents),
            TARGET_IMAGES_GROUP_NAME: np.stack(target_images),
            FINAL_IMAGE_GROUP_NAME: np.stack(final_images),
        }
        for frame, history in enumerate(histories):
            arrays[f"{LATENTS_HISTORIES_GROUP_NAME}_{frame}"] = history
    write_projection_npz_with_attributes(projection_file_path, all_attributes(True), arrays)
    return len(final_latents)


def _square_batches(chunks: Iterator[torch.Tensor], side: int, limit: Optional[int]) -> Iterator[torch.Tensor]:
    """The video's chunks at the network's side, cut off after `limit` frames."""
    taken = 0
    for chunk in chunks:
        if limit is not None:
            if taken >= limit:
                return
            chunk = chunk[: limit - taken]
        taken += int(chunk.shape[0])
        yield chunk if chunk.shape[1] == side else torch.ops.gance.resize_bicubic(chunk, side)


def project_video_to_file(  # pylint: disable=too-many-locals,too-many-arguments
    path_to_video: Path,
    path_to_network: Path,
    projection_file_path: Path,
    video_fps: Optional[float] = None,
    projection_width_height: Optional[Tuple[int, int]] = None,
    projection_fps: Optional[float] = None,
    steps_per_projection: Optional[int] = None,
    num_frames_to_project: Optional[int] = None,
    latents_histories_enabled: bool = True,
    noises_histories_enabled: bool = False,
    images_histories_enabled: bool = False,
    batch_number: Optional[int] = None,
    frames_per_batch: int = 4,
    seed: int = 0,
    distance: Any = None,
) -> None:
    """
    Project a video (a Motion-JPEG AVI) to a projection file on disk. Parameters and defaults as the reference's; beyond them:
    :param frames_per_batch: frames projected at once, each independently.
    :param seed: of the projector's random draws; frame k's draws depend on (seed, k) only, not on frames_per_batch.
    :param distance: a callable replacing the built-in pyramid distance (gance_amd.stylegan2.projector), for instance
        gance_amd.stylegan2.lpips.VGG16Lpips(load_lpips_weights(path)): LPIPS on VGG16 from the caller's weights.
    :param projection_width_height: if given, it must be the network's (resolution, resolution): projection happens there.
    :param latents_histories_enabled: [steps, W, 512] float32 per frame, 37 MB per frame at 1000 steps, held until the end.
    :raises NotImplementedError: a destination that does not end in .npz; noises or images histories.
    :raises ValueError: the video cannot be read, is not square, or `projection_width_height` is not the network's.
    """
    from gance_amd.network_interface.network_functions import LoadedNetwork  # pylint: disable=import-outside-toplevel
    from gance_amd.stylegan2.projector import Projector  # pylint: disable=import-outside-toplevel
    from gance_amd.video.video_common import frames_in_video_device_chunks  # pylint: disable=import-outside-toplevel

    _refusals(projection_file_path, noises_histories_enabled, images_histories_enabled)
    if frames_per_batch < 1:
        raise ValueError(f"frames_per_batch must be >= 1, got {frames_per_batch}")
    try:
        with MjpegAviReader(path_to_video) as reader:
            file_fps, original_frame_count, width, height = float(reader.fps), int(reader.frame_count), int(reader.width), int(reader.height)
    except (OSError, ValueError) as error:
        raise ValueError("Couldn't read input video to do projection.") from error
    if width != height:
        raise ValueError(f"the video must be square to be projected, got {width} x {height}")
    original_fps = float(video_fps) if video_fps else file_fps
    true_projection_fps = original_fps if projection_fps is None else float(projection_fps)
    if num_frames_to_project:
        num_projection_frames = int(num_frames_to_project)
    elif projection_fps is None:
        num_projection_frames = original_frame_count
    else:
        num_projection_frames = int(original_frame_count * true_projection_fps / original_fps)
    steps = DEFAULT_STEPS_PER_PROJECTION if steps_per_projection is None else int(steps_per_projection)
    prefix = "" if batch_number is None else f"[video {batch_number}] "

    network = LoadedNetwork(Path(path_to_network), max_batch=1)
    try:
        side = network.resolution
        if projection_width_height is not None and tuple(projection_width_height) != (side, side):
            raise ValueError(f"projection_width_height {tuple(projection_width_height)} is not the network's ({side}, {side})")
        attributes = {
            "version_number": LATEST_VERSION,
            "original_target_path": str(path_to_video),
            "original_width_height": [width, height],
            "projection_width_height": [side, side],
            "target_md5_hash": hash_file(Path(path_to_video)),
            "original_network_path": str(path_to_network),
            "network_md5_hash": hash_file(Path(path_to_network)),
            "steps_in_projection": steps,
            "noises_histories_enabled": False,
            "images_histories_enabled": False,
            "original_fps": original_fps,
            "projection_fps": true_projection_fps,
            "original_frame_count": original_frame_count,
            "projection_frame_count": num_projection_frames,
        }
        projector = Projector(num_steps=steps, distance=distance, seed=seed)
        projector.set_network(network)
        chunks = frames_in_video_device_chunks(
            path_to_video, frames_per_chunk=frames_per_batch, video_fps=video_fps, reduce_fps_to=projection_fps, device=torch.device("cuda", network.engine.device)
        )
        LOGGER.info(f"{prefix}Projecting {num_projection_frames} frames of {path_to_video} at {steps} steps each")
        count = project_batches_to_file(
            _square_batches(chunks, side, num_frames_to_project or None), projector, projection_file_path, attributes, latents_histories_enabled
        )
        LOGGER.info(f"{prefix}Projected {count} frames into {projection_file_path}")
    finally:
        network.stop()
