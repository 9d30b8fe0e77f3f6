"""
Still images (gance/image_sources/still_image_common.py): written as PNG by the HIP encoder in HBM
(torch.ops.gance.png_encode, or torch.ops.gance.png_encode_lz with compression="matches"), read back through PIL.

`write_image` / `read_image` keep the reference's signatures. `write_images_device` is the batched form the still
products use: one encode call per batch, only the compressed bytes cross to the host.
"""

import hashlib
from pathlib import Path
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from PIL import Image

from gance_amd import torch_ops  # noqa: F401  pylint: disable=unused-import  (registers torch.ops.gance.*)
from gance_amd.gance_types import RGBInt8ImageType

PNG = "png"  # still_image_common.py:16

# `compression`: "huffman" codes literals only (the default, right for network texture); "matches" adds the LZ77 match
# search: never a larger file, several times smaller on flat or repeating content, a slower encode
COMPRESSIONS = ("huffman", "matches")


def check_compression(compression: str) -> None:
    """:raises ValueError: `compression` is none of COMPRESSIONS. Touches no device."""
    if compression not in COMPRESSIONS:
        raise ValueError(f"compression must be one of {COMPRESSIONS}, got {compression!r}")


def write_images_device(frames: torch.Tensor, paths: Sequence[Path], compression: str = "huffman") -> List[str]:
    """
    Encode `frames` [B, H, W, 3] uint8 (CUDA) as PNG in one call, copy the files' bytes (not the worst-case buffer) to the
    host and write frame b to paths[b].
    :param compression: one of COMPRESSIONS.
    :return: the md5 hex digest of each file, from the bytes in memory: what `hash_file` of the written file gives.
    """
    check_compression(compression)
    if frames.dim() != 4 or frames.shape[0] != len(paths):
        raise ValueError(f"frames must be [B, H, W, 3] with one path per frame, got {tuple(frames.shape)} and {len(paths)} paths")
    if not paths:
        return []
    encode = torch.ops.gance.png_encode_lz if compression == "matches" else torch.ops.gance.png_encode
    data, offsets = encode(frames)
    host_offsets = offsets.cpu().numpy()  # synchronises with the encode
    host_data = data[: int(host_offsets[-1])].cpu().numpy()
    hashes = []
    for index, path in enumerate(paths):
        file_bytes = host_data[int(host_offsets[index]) : int(host_offsets[index + 1])].tobytes()
        with open(str(path), "wb") as file:
            file.write(file_bytes)
        hashes.append(hashlib.md5(file_bytes).hexdigest())
    return hashes


def write_image(image: Union[RGBInt8ImageType, torch.Tensor], path: Path, compression: str = "huffman") -> None:
    """
    Write one image [H, W, 3] uint8 to `path` as PNG (still_image_common.py:19-28). A numpy image is uploaded to the
    current GPU first; a CUDA tensor is encoded where it is. There is no CPU encoder. `compression` is one of COMPRESSIONS.
    """
    check_compression(compression)
    if isinstance(image, torch.Tensor):
        frames = image
    else:
        array = np.ascontiguousarray(image)
        if array.dtype != np.uint8:
            raise TypeError(f"image must be uint8, got {array.dtype}")
        frames = torch.from_numpy(array).cuda()
    if frames.dim() != 3 or frames.shape[2] != 3:
        raise ValueError(f"image must be [H, W, 3], got {tuple(frames.shape)}")
    write_images_device(frames[None], [path], compression=compression)


def read_image(image_path: Path, mode: Optional[str] = None) -> RGBInt8ImageType:
    """
    Read an image from disk into the canonical in-memory format (still_image_common.py:31-45); `mode`, if given, is the
    PIL mode the image is converted to. Reading one still is not a hot path: PIL.
    """
    image = Image.open(str(image_path))
    if mode is not None:
        image = image.convert(mode)
    return RGBInt8ImageType(np.asarray(image))
