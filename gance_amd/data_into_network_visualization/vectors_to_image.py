"""
`vectors_to_video` of gance/data_into_network_visualization/vectors_to_image.py:222-259: one latents panel
(gance_amd/debug_video/latents_panel.py, the reference's `vector_visualizer`) per vector or matrix of a VectorsLabel /
MatricesLabel, composed in HBM and written as a Motion-JPEG AVI. Needs no network and no engine. `multi_plot_vectors`
and the spectrogram figure of that module are matplotlib figures and are not built.
"""

from pathlib import Path
from typing import Iterator, Tuple, Union

import numpy as np
import torch

from gance_amd import torch_ops  # (registers torch.ops.gance.*)
from gance_amd.debug_video import compose
from gance_amd.debug_video.latents_panel import LatentsPanel, LatentsPanelDrawer
from gance_amd.vector_sources.vector_sources_common import sub_vectors
from gance_amd.vector_sources.vector_types import MatricesLabel, VectorsLabel
from gance_amd.video import mjpeg_avi

CHUNK_FRAMES = 64


def write_chunks_to_avi(  # pylint: disable=too-many-arguments
    chunks: Iterator[Tuple[int, torch.Tensor]], output_path: Path, width: int, height: int, video_fps: float, jpeg_quality: int,
    jpeg_huffman: str = "standard",
) -> int:
    """
    Composed chunks (first frame, [n, height, width, 3] uint8 in HBM) -> a Motion-JPEG AVI without audio: every chunk goes
    through torch.ops.gance.jpeg_encode_rect (`jpeg_huffman` "optimized": jpeg_encode_optimized, each frame's own Huffman
    tables) and its frames to the writer in order. Returns the frames written.
    :raises ValueError: an unknown `jpeg_huffman`, before the file is opened.
    """
    encode = torch_ops.jpeg_encode_op(jpeg_huffman, square=False)
    with mjpeg_avi.MjpegAviWriter(output_path, height, video_fps, width=width, height=height) as writer:
        for _first, chunk in chunks:
            data, offsets = encode(chunk, int(jpeg_quality))
            offsets_host = offsets.cpu().numpy()  # (waits for the encode)
            data_host = data[: int(offsets_host[-1])].cpu().numpy()
            for index in range(int(chunk.shape[0])):
                writer.add_frame(data_host[int(offsets_host[index]) : int(offsets_host[index + 1])])
        return writer.frames_written


def vectors_frame_chunks(
    labeled_data: Union[VectorsLabel, MatricesLabel], video_height: int, chunk_frames: int = CHUNK_FRAMES
) -> Iterator[Tuple[int, torch.Tensor]]:
    """
    (first frame, [n, video_height, video_height, 3] uint8 in HBM) chunks of `vectors_to_video`: frame k is the latents
    panel of vector / matrix k, limits = the data's min / max, title = the label. The arguments are checked when this is
    called; nothing is uploaded or launched before the first chunk is asked for.
    :raises ValueError: a height that is not a multiple of 16 in [16, 4096], more matrix rows than a panel draws.
    """
    side = compose.validate_side_length(video_height)
    if chunk_frames < 1:
        raise ValueError(f"chunk_frames must be >= 1, got {chunk_frames}")
    data = np.asarray(labeled_data.data)
    divided = np.asarray(sub_vectors(data=data, vector_length=labeled_data.vector_length), dtype=np.float32)
    if divided.ndim == 2:  # a single vector is one row
        divided = divided[:, None, :]
    panel = LatentsPanel(side, int(divided.shape[2]), int(divided.shape[1]), float(data.min()), float(data.max()), labeled_data.label)

    def chunks() -> Iterator[Tuple[int, torch.Tensor]]:
        device = torch.device("cuda", torch.cuda.current_device())
        drawer = LatentsPanelDrawer(panel, device)
        for first in range(0, int(divided.shape[0]), chunk_frames):
            rows = compose._upload(divided[first : first + chunk_frames], device)  # pylint: disable=protected-access
            out = torch.empty((int(rows.shape[0]), side, side, 3), dtype=torch.uint8, device=device)
            drawer.draw(out, 0, rows, range(int(rows.shape[0])))
            yield first, out

    return chunks()


def vectors_to_video(
    labeled_data: Union[VectorsLabel, MatricesLabel], output_path: Path, video_height: int, video_fps: float, jpeg_quality: int = 90,
    jpeg_huffman: str = "standard",
) -> Path:
    """
    The canonical video of some vectors / matrices (vectors_to_image.py:222-259) as a Motion-JPEG AVI, `video_height`
    square. Returns `output_path` once the video has been written. `jpeg_huffman`: see write_chunks_to_avi.
    """
    side = compose.validate_side_length(video_height)
    write_chunks_to_avi(vectors_frame_chunks(labeled_data, side), Path(output_path), side, side, video_fps, jpeg_quality, jpeg_huffman)
    return output_path
