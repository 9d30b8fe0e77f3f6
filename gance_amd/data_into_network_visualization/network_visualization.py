"""
Latents -> frames: the caller loop of the hot path.

`vector_synthesis` keeps the reference's signature and lazy-iterator contract
(gance/data_into_network_visualization/network_visualization.py:462-690). The debug visualisations
(`enable_2d` / `enable_3d`, :54-400, :542-596) come back as `visualization_images`: frames
`visualization_height` high and `visualization_height * (enable_2d + enable_3d)` wide, the 2-D
"synthesis inputs" panel on the left and the 3-D view of every input vector on the right, composed in
HBM without matplotlib (gance_amd/debug_video/synthesis_visualization.py) and without a network: with
`networks=None` the visualisation alone is produced. `vector_synthesis_visualization_chunks` is the
same frames as chunks that stay in HBM.

Differences by design: frames are synthesised in batches, and because `MultiNetwork` keeps every
network resident the reference's "sort frames by network, spill each to a gzip-HDF5 temp file, reload
in order" detour (:653-674) disappears -- frames of a batch are grouped by network index in memory
and emitted in frame order.
"""

from typing import Iterator, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from gance_amd.data_into_network_visualization.visualization_common import VisualizationInput
from gance_amd.debug_video import synthesis_visualization
from gance_amd.gance_types import ImageSourceType, RGBInt8ImageType
from gance_amd.logger_common import LOGGER
from gance_amd.network_interface.network_functions import MultiNetwork
from gance_amd.vector_sources.vector_sources_common import sub_vectors


class SynthesisOutput(NamedTuple):
    """The two image sources of a synthesis run (network_visualization.py:403-409)."""

    synthesized_images: Optional[ImageSourceType]
    visualization_images: Optional[ImageSourceType]


def _batched_frames(
    samples: np.ndarray, indices: List[int], networks: MultiNetwork, batch: int
) -> Iterator[RGBInt8ImageType]:
    """Synthesize `samples[f]` on network `indices[f]`, `batch` frames at a time, in frame order."""
    total = len(samples)
    for start in range(0, total, batch):
        stop = min(total, start + batch)
        chunk_indices = np.asarray(indices[start:stop])
        frames: List[Optional[np.ndarray]] = [None] * (stop - start)
        for network_index in np.unique(chunk_indices):
            members = np.nonzero(chunk_indices == network_index)[0]
            images = networks.indexed_create_images_generic(int(network_index), samples[start:stop][members])
            for slot, image in zip(members, images):
                frames[slot] = image
        for offset, frame in enumerate(frames):
            LOGGER.info(f"Rendered frame #{start + offset}")
            yield RGBInt8ImageType(frame)


def _visualization_side(visualization_height: Optional[int], networks: Optional[MultiNetwork]) -> int:
    """`visualization_height`, or the networks' resolution (network_visualization.py:531-540)."""
    if visualization_height is None:
        if networks is None:
            raise ValueError("visualization_height is needed where there are no networks to take the resolution from")
        visualization_height = networks.resolution
    return synthesis_visualization.validate_height(visualization_height)


def vector_synthesis_visualization_chunks(  # pylint: disable=too-many-arguments
    data: VisualizationInput,
    vector_length: int,
    visualization_height: int,
    enable_3d: bool = False,
    enable_2d: bool = True,
    frames_to_visualize: Optional[int] = None,
    network_index_window_width: Optional[int] = None,
    chunk_frames: int = synthesis_visualization.CHUNK_FRAMES,
) -> Iterator[Tuple[int, torch.Tensor]]:
    """
    The visualisation of `vector_synthesis` without the trip to the host: a lazy generator of (first frame, uint8
    [n, height, height * (enable_2d + enable_3d), 3] in HBM) chunks of at most `chunk_frames` frames, ready for
    `torch.ops.gance.jpeg_encode_rect` / `MjpegAviWriter`. The frames do not depend on `chunk_frames`.
    :raises ValueError: nothing to render, or a height that is not a multiple of 16 in [16, 4096] (both when called).
    """
    if not enable_3d and not enable_2d:
        raise ValueError("Nothing to render!")
    side = synthesis_visualization.validate_height(visualization_height)
    return synthesis_visualization.visualization_chunks(
        data, int(vector_length), side, enable_2d, enable_3d, frames_to_visualize, network_index_window_width, chunk_frames
    )


def vector_synthesis(  # pylint: disable=too-many-arguments,unused-argument
    data: VisualizationInput,
    networks: Optional[MultiNetwork],
    default_vector_length: Optional[int] = 1024,
    visualization_height: Optional[int] = None,
    enable_3d: bool = False,
    enable_2d: bool = True,
    frames_to_visualize: Optional[int] = None,
    network_index_window_width: Optional[int] = None,
    force_optimize_synthesis_order: bool = True,
    unload_networks_when_complete: bool = False,
) -> SynthesisOutput:
    """
    For every vector (1-D `combined`) or matrix (2-D `combined`) in `data.combined`, synthesize
    the frame on the network `data.network_indices` selects. Frames come back lazily, at the
    network's native size, as uint8 (H, W, 3) RGB. With `enable_2d` / `enable_3d` the visualisation
    frames come back lazily too, `visualization_height` (default: the networks' resolution) high;
    each iterator owns its work, so they can be drained in any order. Without networks only the
    visualisation is produced, for vectors of `default_vector_length`.
    :raises ValueError: nothing to render (no networks and no visualisation requested), as in the
    reference (:513-514); a visualisation with neither a height nor networks, or with a height that
    is not a multiple of 16 in [16, 4096].
    """
    if not enable_3d and not enable_2d and networks is None:
        raise ValueError("Nothing to render!")
    visualization = None
    if enable_2d or enable_3d:
        side = _visualization_side(visualization_height, networks)
        vector_length = int(networks.expected_vector_length if networks is not None else default_vector_length)
        visualization = synthesis_visualization.visualization_frames(
            synthesis_visualization.visualization_chunks(
                data, vector_length, side, enable_2d, enable_3d, frames_to_visualize, network_index_window_width
            )
        )
    if networks is None:
        return SynthesisOutput(synthesized_images=None, visualization_images=visualization)

    vector_length = networks.expected_vector_length
    samples = sub_vectors(data=data.combined.data, vector_length=vector_length)  # (N, L) or (N, W, L)
    indices = [int(index) for index in data.network_indices.result.data]
    if frames_to_visualize is not None:
        samples = samples[:frames_to_visualize]
    indices = indices[: len(samples)]

    def frames() -> Iterator[RGBInt8ImageType]:
        yield from _batched_frames(samples, indices, networks, networks.max_batch)  # full engine calls: the capacity the networks were loaded with
        if unload_networks_when_complete:
            networks.unload()

    return SynthesisOutput(synthesized_images=frames(), visualization_images=visualization)
