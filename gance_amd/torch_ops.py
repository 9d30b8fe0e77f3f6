"""
The C ABI of libgance_hip.so surfaced as PyTorch-ROCm custom ops (namespace `gance`).

    torch.ops.gance.synthesize_w(dlatents, engine)         [B, W, 512] f32  -> [B, R, R, 3] u8
    torch.ops.gance.synthesize_z(z, engine, psi)           [B, 512]    f32  -> [B, R, R, 3] u8
    torch.ops.gance.synthesize_w_image(dlatents, engine)   ... -> ([B, R, R, 3] u8, [B, 3, R, R] f32)
    torch.ops.gance.resize_bicubic(frames, side)           [B, S, S, 3] u8  -> [B, side, side, 3] u8
    torch.ops.gance.synthesize_w_out / synthesize_z_out / resize_bicubic_out   the same, into a caller-owned `out`
    torch.ops.gance.blend(audio, latent_row0, blend)       [samples] f32, [F, L] f32 -> ([N, depth, L] f32, [N] i32)
    torch.ops.gance.jpeg_encode_rect(frames, quality)      [B, H, W, 3] u8  -> the same for frames that are not square
    torch.ops.gance.jpeg_encode(frames, quality)           [B, S, S, 3] u8  -> ([capacity] u8, [B + 1] i64): B JFIF files
    torch.ops.gance.jpeg_encode_optimized(frames, quality) [B, H, W, 3] u8  -> the same with each frame's own optimised Huffman tables: smaller files
    torch.ops.gance.jpeg_optimal_huffman(counts)           [N, 256] i32     -> ([N, 16] u8, [N, 256] u8, [N] i32): bits, values, status of that table build
    torch.ops.gance.png_encode(frames)              [B, H, W, 3] u8  -> ([capacity] u8, [B + 1] i64): B PNG files, any H and W
    torch.ops.gance.png_encode_lz(frames)                  [B, H, W, 3] u8  -> the same with an LZ77 match search: no file larger, flat areas far smaller
    torch.ops.gance.jpeg_decode(data, offsets)             [bytes] u8, [B + 1] i64 -> [B, H, W, 3] u8: what the two above return, decoded
    torch.ops.gance.jpeg_decode_layouts(data, offsets)     the same for baseline 4:2:2, 4:2:0, 4:4:4 and grey files: videos from elsewhere
    torch.ops.gance.modconv3x3(x, style, demod, weight, up)        [B, Cin, S, S] f32 -> [B, Cout, S or 2S, ...] f32   differentiable
    torch.ops.gance.noise_bias_lrelu(x, noise, strength, bias)     [B, C, S, S] f32 -> the same                          differentiable
    torch.ops.gance.torgb_skip(x, style, weight, bias, y_prev)     [B, Cin, S, S] f32 -> [B, 3, S, S] f32                differentiable
    (each with a `_backward` op; gradients reach x, style, demod, y_prev and the noise planes: gance_amd/stylegan2/differentiable.py is the user)
    torch.ops.gance.conv3x3(x, weight, weight_transposed)          [B, Cin, S, S] f32 -> [B, Cout, S, S] f32             differentiable in x
    (the plain 3x3 convolution, csrc/conv3x3.hip; `conv3x3_transposed_weight` builds the third argument)
    torch.ops.gance.noise_regularizer(noise)                       [B, 1, S, S] f32 -> [B] f32                           differentiable
    torch.ops.gance.pyramid_distance(image, target)                [B, 3, R, R], [B, 3, min(R, 256), ...] f32 -> [B]     differentiable
    (projection's losses: gance_amd/stylegan2/projector.py is the user)

Tensors are CUDA (HIP) tensors; every op launches on torch's CURRENT stream of the tensor's device and returns
without synchronising, so the ops compose with torch code and with `torch.distributed` collectives in stream
order. `engine` / `blend` are integer handles of objects created through `register_engine` /
`register_blend` (the ops cannot take Python objects); status codes of the C ABI become Python exceptions
(`hip_lib.GanceHipError`, or ValueError for argument errors the reference reports as ValueError).

The ops are thin: they validate shapes, allocate the outputs with torch and pass raw pointers + the stream to the
ctypes binding (gance_amd/hip_lib.py). There is no CPU implementation: on a CPU tensor an op raises.
"""

import ctypes
import weakref
from typing import Optional, Tuple

import numpy as np
import torch

from gance_amd import hip_lib

# weak: a handle must not keep an engine's HBM (weights + its share of the workspace) alive after its owner let go
_ENGINES: "weakref.WeakValueDictionary[int, hip_lib.Engine]" = weakref.WeakValueDictionary()
_BLENDS: "weakref.WeakValueDictionary[int, hip_lib.Blend]" = weakref.WeakValueDictionary()
_NEXT_HANDLE = [1]


def register_engine(engine: hip_lib.Engine) -> int:
    """Make an Engine addressable from the ops; returns its integer handle."""
    handle = _NEXT_HANDLE[0]
    _NEXT_HANDLE[0] += 1
    _ENGINES[handle] = engine
    return handle


def register_blend(blend: hip_lib.Blend) -> int:
    """Make a Blend addressable from the ops; returns its integer handle."""
    handle = _NEXT_HANDLE[0]
    _NEXT_HANDLE[0] += 1
    _BLENDS[handle] = blend
    return handle


def unregister(handle: int) -> None:
    """Forget a handle (the object itself is closed by its owner)."""
    _ENGINES.pop(handle, None)
    _BLENDS.pop(handle, None)


def _engine(handle: int) -> hip_lib.Engine:
    try:
        return _ENGINES[handle]
    except KeyError:
        raise ValueError(f"unknown engine handle {handle} (never registered, closed or garbage-collected)") from None


def _require_cuda(tensor: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    if not tensor.is_cuda:
        raise RuntimeError(f"gance ops run on an MI355X only: `{name}` is on {tensor.device} (there is no CPU fallback)")
    if tensor.dtype != dtype:
        raise TypeError(f"`{name}` must be {dtype}, got {tensor.dtype}")


def _stream(tensor: torch.Tensor) -> int:
    return torch.cuda.current_stream(tensor.device).cuda_stream


@torch.library.custom_op("gance::synthesize_w", mutates_args=(), device_types="cuda")
def synthesize_w(dlatents: torch.Tensor, engine: int) -> torch.Tensor:
    """create_image_matrix for a batch (network_functions.py:160-169): synthesis with the stored noise."""
    eng = _engine(engine)
    _require_cuda(dlatents, torch.float32, "dlatents")
    if dlatents.dim() != 3 or dlatents.shape[1] != eng.num_layers or dlatents.shape[2] != eng.vector_length:
        raise ValueError(f"dlatents must be [B, {eng.num_layers}, {eng.vector_length}], got {tuple(dlatents.shape)}")
    dlatents = dlatents.contiguous()
    frames = torch.empty((dlatents.shape[0], eng.resolution, eng.resolution, 3), dtype=torch.uint8, device=dlatents.device)
    eng.synthesize_w_device(dlatents.data_ptr(), dlatents.shape[0], frames.data_ptr(), 0, _stream(dlatents))
    return frames


@synthesize_w.register_fake
def _(dlatents: torch.Tensor, engine: int) -> torch.Tensor:
    side = _engine(engine).resolution
    return dlatents.new_empty((dlatents.shape[0], side, side, 3), dtype=torch.uint8)


@torch.library.custom_op("gance::synthesize_w_image", mutates_args=(), device_types="cuda")
def synthesize_w_image(dlatents: torch.Tensor, engine: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """As synthesize_w, also returning the float image [B, 3, R, R] before the uint8 conversion."""
    eng = _engine(engine)
    _require_cuda(dlatents, torch.float32, "dlatents")
    if dlatents.dim() != 3 or dlatents.shape[1] != eng.num_layers or dlatents.shape[2] != eng.vector_length:
        raise ValueError(f"dlatents must be [B, {eng.num_layers}, {eng.vector_length}], got {tuple(dlatents.shape)}")
    dlatents = dlatents.contiguous()
    batch, side = dlatents.shape[0], eng.resolution
    frames = torch.empty((batch, side, side, 3), dtype=torch.uint8, device=dlatents.device)
    image = torch.empty((batch, 3, side, side), dtype=torch.float32, device=dlatents.device)
    eng.synthesize_w_device(dlatents.data_ptr(), batch, frames.data_ptr(), image.data_ptr(), _stream(dlatents))
    return frames, image


@synthesize_w_image.register_fake
def _(dlatents: torch.Tensor, engine: int) -> Tuple[torch.Tensor, torch.Tensor]:
    side = _engine(engine).resolution
    batch = dlatents.shape[0]
    return dlatents.new_empty((batch, side, side, 3), dtype=torch.uint8), dlatents.new_empty((batch, 3, side, side))


@torch.library.custom_op("gance::synthesize_z", mutates_args=(), device_types="cuda")
def synthesize_z(z: torch.Tensor, engine: int, truncation_psi: float) -> torch.Tensor:
    """create_image_vector for a batch (network_functions.py:144-158): mapping, truncation, synthesis."""
    eng = _engine(engine)
    _require_cuda(z, torch.float32, "z")
    if z.dim() != 2 or z.shape[1] != eng.vector_length:
        raise ValueError(f"z must be [B, {eng.vector_length}], got {tuple(z.shape)}")
    z = z.contiguous()
    frames = torch.empty((z.shape[0], eng.resolution, eng.resolution, 3), dtype=torch.uint8, device=z.device)
    eng.synthesize_z_device(z.data_ptr(), z.shape[0], float(truncation_psi), frames.data_ptr(), 0, _stream(z))
    return frames


@synthesize_z.register_fake
def _(z: torch.Tensor, engine: int, truncation_psi: float) -> torch.Tensor:
    side = _engine(engine).resolution
    return z.new_empty((z.shape[0], side, side, 3), dtype=torch.uint8)


@torch.library.custom_op("gance::synthesize_w_out", mutates_args=("out",), device_types="cuda")
def synthesize_w_out(dlatents: torch.Tensor, engine: int, out: torch.Tensor) -> None:
    """synthesize_w writing into caller-owned frames `out` [B, R, R, 3] u8 (a contiguous slice of a larger buffer)."""
    eng = _engine(engine)
    _require_cuda(dlatents, torch.float32, "dlatents")
    _require_cuda(out, torch.uint8, "out")
    batch = dlatents.shape[0]
    if dlatents.dim() != 3 or dlatents.shape[1] != eng.num_layers or dlatents.shape[2] != eng.vector_length:
        raise ValueError(f"dlatents must be [B, {eng.num_layers}, {eng.vector_length}], got {tuple(dlatents.shape)}")
    if tuple(out.shape) != (batch, eng.resolution, eng.resolution, 3) or not out.is_contiguous() or out.device != dlatents.device:
        raise ValueError(f"out must be a contiguous [{batch}, {eng.resolution}, {eng.resolution}, 3] uint8 tensor on {dlatents.device}")
    dlatents = dlatents.contiguous()
    eng.synthesize_w_device(dlatents.data_ptr(), batch, out.data_ptr(), 0, _stream(dlatents))


@torch.library.custom_op("gance::synthesize_z_out", mutates_args=("out",), device_types="cuda")
def synthesize_z_out(z: torch.Tensor, engine: int, truncation_psi: float, out: torch.Tensor) -> None:
    """synthesize_z writing into caller-owned frames `out` [B, R, R, 3] u8."""
    eng = _engine(engine)
    _require_cuda(z, torch.float32, "z")
    _require_cuda(out, torch.uint8, "out")
    batch = z.shape[0]
    if z.dim() != 2 or z.shape[1] != eng.vector_length:
        raise ValueError(f"z must be [B, {eng.vector_length}], got {tuple(z.shape)}")
    if tuple(out.shape) != (batch, eng.resolution, eng.resolution, 3) or not out.is_contiguous() or out.device != z.device:
        raise ValueError(f"out must be a contiguous [{batch}, {eng.resolution}, {eng.resolution}, 3] uint8 tensor on {z.device}")
    z = z.contiguous()
    eng.synthesize_z_device(z.data_ptr(), batch, float(truncation_psi), out.data_ptr(), 0, _stream(z))


@torch.library.custom_op("gance::resize_bicubic_out", mutates_args=("out",), device_types="cuda")
def resize_bicubic_out(frames: torch.Tensor, out: torch.Tensor) -> None:
    """resize_bicubic writing into caller-owned `out` [B, side, side, 3] u8."""
    _require_cuda(frames, torch.uint8, "frames")
    _require_cuda(out, torch.uint8, "out")
    if frames.dim() != 4 or frames.shape[1] != frames.shape[2] or frames.shape[3] != 3 or out.dim() != 4 or out.shape[0] != frames.shape[0]:
        raise ValueError("frames must be [B, S, S, 3] and out [B, side, side, 3]")
    if out.shape[1] != out.shape[2] or out.shape[3] != 3 or not out.is_contiguous() or out.device != frames.device:
        raise ValueError("out must be a contiguous [B, side, side, 3] uint8 tensor on the frames' device")
    frames = frames.contiguous()
    if frames.shape[0]:
        hip_lib.resize_bicubic_u8_device(frames.data_ptr(), frames.shape[0], frames.shape[1], out.data_ptr(), out.shape[1], _stream(frames))


@torch.library.custom_op("gance::resize_bicubic", mutates_args=(), device_types="cuda")
def resize_bicubic(frames: torch.Tensor, side: int) -> torch.Tensor:
    """cv2.resize(..., INTER_CUBIC) of video_common.py:416-418 on uint8 NHWC frames in HBM."""
    _require_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[1] != frames.shape[2] or frames.shape[3] != 3:
        raise ValueError(f"frames must be [B, S, S, 3], got {tuple(frames.shape)}")
    frames = frames.contiguous()
    out = torch.empty((frames.shape[0], side, side, 3), dtype=torch.uint8, device=frames.device)
    if frames.shape[0]:
        hip_lib.resize_bicubic_u8_device(frames.data_ptr(), frames.shape[0], frames.shape[1], out.data_ptr(), side, _stream(frames))
    return out


@resize_bicubic.register_fake
def _(frames: torch.Tensor, side: int) -> torch.Tensor:
    return frames.new_empty((frames.shape[0], side, side, 3))


@torch.library.custom_op("gance::blend", mutates_args=(), device_types="cuda")
def blend(audio: torch.Tensor, latent_row0: torch.Tensor, blend_handle: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """alpha_blend_projection_file (visualization_inputs.py:169-270): audio + projected latents -> per-frame latent matrices and network indices."""
    try:
        owner = _BLENDS[blend_handle]
    except KeyError:
        raise ValueError(f"unknown blend handle {blend_handle}") from None
    _require_cuda(audio, torch.float32, "audio")
    _require_cuda(latent_row0, torch.float32, "latent_row0")
    config = owner.config
    audio, latent_row0 = audio.contiguous(), latent_row0.contiguous()
    if latent_row0.numel() != config.num_projection_frames * config.vector_length:
        raise ValueError("latent_row0 must hold num_projection_frames * vector_length values")
    dlatents = torch.empty((config.num_frames, config.latent_depth, config.vector_length), dtype=torch.float32, device=audio.device)
    indices = torch.empty((config.num_frames,), dtype=torch.int32, device=audio.device)
    owner.run_device(audio.data_ptr(), audio.numel(), latent_row0.data_ptr(), dlatents.data_ptr(), indices.data_ptr(), stream=_stream(audio))
    return dlatents, indices


@blend.register_fake
def _(audio: torch.Tensor, latent_row0: torch.Tensor, blend_handle: int) -> Tuple[torch.Tensor, torch.Tensor]:
    config = _BLENDS[blend_handle].config
    return (
        audio.new_empty((config.num_frames, config.latent_depth, config.vector_length)),
        audio.new_empty((config.num_frames,), dtype=torch.int32),
    )


@torch.library.custom_op("gance::jpeg_encode", mutates_args=(), device_types="cuda")
def jpeg_encode(frames: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    Baseline JPEG of each frame (the video encode of write_source_to_disk_forward, video_common.py:301-376, as Motion-JPEG):
    `data` [capacity] u8 holds the files back to back, frame b at data[offsets[b]:offsets[b + 1]]; `capacity` is the
    worst case of the shape (hip_lib.jpeg_encode_bounds), only offsets[-1] bytes are written.
    """
    _require_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[1] != frames.shape[2] or frames.shape[3] != 3:
        raise ValueError(f"frames must be [B, S, S, 3], got {tuple(frames.shape)}")
    batch, side = int(frames.shape[0]), int(frames.shape[1])
    workspace_bytes, capacity = hip_lib.jpeg_encode_bounds(batch, side)
    frames = frames.contiguous()
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=frames.device)
    data = torch.empty((capacity,), dtype=torch.uint8, device=frames.device)
    offsets = torch.empty((batch + 1,), dtype=torch.int64, device=frames.device)
    hip_lib.jpeg_encode_device(
        frames.data_ptr(), batch, side, int(quality), workspace.data_ptr(), workspace_bytes, data.data_ptr(), capacity,
        offsets.data_ptr(), _stream(frames),
    )
    return data, offsets


@jpeg_encode.register_fake
def _(frames: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    batch, side = int(frames.shape[0]), int(frames.shape[1])
    _, capacity = hip_lib.jpeg_encode_bounds(batch, side)
    return frames.new_empty((capacity,), dtype=torch.uint8), frames.new_empty((batch + 1,), dtype=torch.int64)


@torch.library.custom_op("gance::jpeg_encode_rect", mutates_args=(), device_types="cuda")
def jpeg_encode_rect(frames: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    `jpeg_encode` for frames [B, H, W, 3] with H and W multiples of 16 (the debug video's row of panels, written by the
    reference through write_source_to_disk_consume, gance/projection_file_blend.py:302-341): the same (data, offsets);
    square frames give the bytes `jpeg_encode` gives.
    """
    _require_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be [B, H, W, 3], got {tuple(frames.shape)}")
    batch, height, width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    workspace_bytes, capacity = hip_lib.jpeg_encode_rect_bounds(batch, width, height)
    frames = frames.contiguous()
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=frames.device)
    data = torch.empty((capacity,), dtype=torch.uint8, device=frames.device)
    offsets = torch.empty((batch + 1,), dtype=torch.int64, device=frames.device)
    hip_lib.jpeg_encode_rect_device(
        frames.data_ptr(), batch, width, height, int(quality), workspace.data_ptr(), workspace_bytes, data.data_ptr(), capacity,
        offsets.data_ptr(), _stream(frames),
    )
    return data, offsets


@jpeg_encode_rect.register_fake
def _(frames: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    batch, height, width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    _, capacity = hip_lib.jpeg_encode_rect_bounds(batch, width, height)
    return frames.new_empty((capacity,), dtype=torch.uint8), frames.new_empty((batch + 1,), dtype=torch.int64)


@torch.library.custom_op("gance::jpeg_encode_optimized", mutates_args=(), device_types="cuda")
def jpeg_encode_optimized(frames: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    `jpeg_encode_rect` with per-frame optimised Huffman tables (libjpeg's optimize_coding, PIL's optimize=True): the same
    (data, offsets) and capacity, the same decoded pixels, smaller files; each file carries its own four DHT segments, so
    header lengths differ between frames.
    """
    _require_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be [B, H, W, 3], got {tuple(frames.shape)}")
    batch, height, width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    workspace_bytes, capacity = hip_lib.jpeg_encode_rect_optimized_bounds(batch, width, height)
    frames = frames.contiguous()
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=frames.device)
    data = torch.empty((capacity,), dtype=torch.uint8, device=frames.device)
    offsets = torch.empty((batch + 1,), dtype=torch.int64, device=frames.device)
    hip_lib.jpeg_encode_rect_optimized_device(
        frames.data_ptr(), batch, width, height, int(quality), workspace.data_ptr(), workspace_bytes, data.data_ptr(), capacity,
        offsets.data_ptr(), _stream(frames),
    )
    return data, offsets


@jpeg_encode_optimized.register_fake
def _(frames: torch.Tensor, quality: int) -> Tuple[torch.Tensor, torch.Tensor]:
    batch, height, width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    _, capacity = hip_lib.jpeg_encode_rect_optimized_bounds(batch, width, height)
    return frames.new_empty((capacity,), dtype=torch.uint8), frames.new_empty((batch + 1,), dtype=torch.int64)


@torch.library.custom_op("gance::jpeg_optimal_huffman", mutates_args=(), device_types="cuda")
def jpeg_optimal_huffman(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """
    The table build of `jpeg_encode_optimized` on given symbol counts [N, 256] i32 (jchuff.c jpeg_gen_optimal_table):
    (bits [N, 16] u8: codes per length 1..16, values [N, 256] u8: the symbols in code order, status [N] i32: 0 a table,
    1 a code of more than 32 bits before the limiting, 2 no symbol counted). Bits and values are 0 unless the status is 0.
    """
    _require_cuda(counts, torch.int32, "counts")
    if counts.dim() != 2 or counts.shape[0] < 1 or counts.shape[1] != 256:
        raise ValueError(f"counts must be [N, 256] with N >= 1, got {tuple(counts.shape)}")
    counts = counts.contiguous()
    count = int(counts.shape[0])
    bits = torch.empty((count, 16), dtype=torch.uint8, device=counts.device)
    values = torch.empty((count, 256), dtype=torch.uint8, device=counts.device)
    status = torch.empty((count,), dtype=torch.int32, device=counts.device)
    hip_lib.jpeg_optimal_tables_device(counts.data_ptr(), count, bits.data_ptr(), values.data_ptr(), status.data_ptr(), _stream(counts))
    return bits, values, status


@jpeg_optimal_huffman.register_fake
def _(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    count = int(counts.shape[0])
    return (
        counts.new_empty((count, 16), dtype=torch.uint8),
        counts.new_empty((count, 256), dtype=torch.uint8),
        counts.new_empty((count,), dtype=torch.int32),
    )


def jpeg_encode_op(jpeg_huffman: str, square: bool):  # type: ignore[no-untyped-def]
    """The encode op of a table mode ("standard" / "optimized", hip_lib.check_jpeg_huffman): `square` picks
    torch.ops.gance.jpeg_encode over jpeg_encode_rect in the standard mode; the optimised op takes any frames."""
    if hip_lib.check_jpeg_huffman(jpeg_huffman) == "optimized":
        return torch.ops.gance.jpeg_encode_optimized
    return torch.ops.gance.jpeg_encode if square else torch.ops.gance.jpeg_encode_rect


def _png_encode(frames: torch.Tensor, bounds, encode_device) -> Tuple[torch.Tensor, torch.Tensor]:  # type: ignore[no-untyped-def]
    """The body of the two PNG ops: `bounds` / `encode_device` are hip_lib's pair of one encoder."""
    _require_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be [B, H, W, 3], got {tuple(frames.shape)}")
    batch, height, width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    if batch == 0:
        return frames.new_empty((0,), dtype=torch.uint8), frames.new_zeros((1,), dtype=torch.int64)
    workspace_bytes, capacity = bounds(batch, width, height)
    frames = frames.contiguous()
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=frames.device)
    data = torch.empty((capacity,), dtype=torch.uint8, device=frames.device)
    offsets = torch.empty((batch + 1,), dtype=torch.int64, device=frames.device)
    encode_device(
        frames.data_ptr(), batch, width, height, workspace.data_ptr(), workspace_bytes, data.data_ptr(), capacity, offsets.data_ptr(),
        _stream(frames),
    )
    return data, offsets


@torch.library.custom_op("gance::png_encode", mutates_args=(), device_types="cuda")
def png_encode(frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    Lossless PNG of each frame (write_image, still_image_common.py:19-28): `data` [capacity] u8 holds the files back to
    back, frame b at data[offsets[b]:offsets[b + 1]]; `capacity` is the worst case of the shape (hip_lib.png_encode_bounds),
    only offsets[-1] bytes are written. H and W are any sizes in [1, 8192]; B == 0 gives empty data and offsets [0].
    """
    return _png_encode(frames, hip_lib.png_encode_bounds, hip_lib.png_encode_device)


@png_encode.register_fake
def _(frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    batch, height, width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    capacity = hip_lib.png_encode_bounds(batch, width, height)[1] if batch else 0
    return frames.new_empty((capacity,), dtype=torch.uint8), frames.new_empty((batch + 1,), dtype=torch.int64)


@torch.library.custom_op("gance::png_encode_lz", mutates_args=(), device_types="cuda")
def png_encode_lz(frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    `png_encode` with an LZ77 match search (hip_lib.png_encode_lz_device): the same pixels, the same capacity, and per
    frame a file that is never larger; frames with flat or repeating areas come out several times smaller, noisy texture
    byte for byte as `png_encode` writes it.
    """
    return _png_encode(frames, hip_lib.png_encode_lz_bounds, hip_lib.png_encode_lz_device)


@png_encode_lz.register_fake
def _(frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    batch, height, width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    capacity = hip_lib.png_encode_lz_bounds(batch, width, height)[1] if batch else 0
    return frames.new_empty((capacity,), dtype=torch.uint8), frames.new_empty((batch + 1,), dtype=torch.int64)


def _jpeg_headers(data: torch.Tensor, offsets: torch.Tensor, layouts: bool = False) -> Tuple[np.ndarray, "ctypes.Array"]:
    """
    (host offsets, descriptions) of the files of a `jpeg_decode` call (`JpegInfo`), or with `layouts` of a
    `jpeg_decode_layouts` call (`JpegFrameInfo`). Only each file's first bytes cross to the host: the header is a few
    hundred bytes, and a parse that runs out of them is repeated with more.
    """
    info_type, parse = (hip_lib.JpegFrameInfo, hip_lib.jpeg_parse_header_layouts) if layouts else (hip_lib.JpegInfo, hip_lib.jpeg_parse_header)
    host_offsets = offsets.detach().cpu().numpy().astype(np.int64)
    batch = host_offsets.shape[0] - 1
    if batch < 1 or host_offsets[0] < 0 or np.any(np.diff(host_offsets) < 0) or host_offsets[-1] > data.numel():
        raise ValueError(f"offsets must be [B + 1] non-decreasing positions inside the {data.numel()} bytes of data, B >= 1")
    infos = (info_type * batch)()
    head_bytes = 1024
    while True:
        spans = [(int(host_offsets[b]), int(min(host_offsets[b] + head_bytes, host_offsets[b + 1]))) for b in range(batch)]
        index = torch.cat([torch.arange(first, last, device=data.device) for first, last in spans])
        heads = data[index].cpu().numpy()
        at, retry = 0, False
        for b, (first, last) in enumerate(spans):
            head = heads[at : at + last - first]
            at += last - first
            try:
                parse(head, infos[b])
            except ValueError as error:
                if "cut short" in str(error) and last < host_offsets[b + 1]:
                    retry = True
                    break
                raise ValueError(f"frame {b}: {error}") from None
            info = infos[b].info if layouts else infos[b]
            info.scan_bytes = int(host_offsets[b + 1]) - first - info.scan_offset
        if not retry:
            return host_offsets, infos
        head_bytes *= 16


@torch.library.custom_op("gance::jpeg_decode", mutates_args=(), device_types="cuda")
def jpeg_decode(data: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """
    The reverse of `jpeg_encode` / `jpeg_encode_rect`, and the frame decode of frames_in_video (video_common.py:229-298):
    file b at data[offsets[b]:offsets[b + 1]] (baseline 4:2:2 JFIF of one size, any tables and restart interval; `offsets`
    on either device) to RGB [B, H, W, 3] u8, pixel for pixel what libjpeg decodes. The headers and the per-frame status
    cross to the host once per call, so the op synchronises.
    :raises ValueError: a file the decoder does not take, or a frame whose data is bad: the first such frame and the reason.
    """
    _require_cuda(data, torch.uint8, "data")
    if data.dim() != 1 or offsets.dim() != 1 or offsets.dtype != torch.int64:
        raise ValueError("data must be [bytes] uint8 and offsets [B + 1] int64")
    data = data.contiguous()
    host_offsets, infos = _jpeg_headers(data, offsets)
    batch, width, height = len(infos), infos[0].width, infos[0].height
    workspace_bytes = hip_lib.jpeg_decode_bounds(batch, width, height, int(host_offsets[-1] - host_offsets[0]))
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=data.device)
    frames = torch.empty((batch, height, width, 3), dtype=torch.uint8, device=data.device)
    status = torch.empty((batch,), dtype=torch.int32, device=data.device)
    hip_lib.jpeg_decode_device(
        data.data_ptr(), host_offsets, infos, workspace.data_ptr(), workspace_bytes, frames.data_ptr(), status.data_ptr(), _stream(data)
    )
    host_status = status.cpu().numpy()
    bad = np.flatnonzero(host_status)
    if bad.size:
        reason = hip_lib.JPEG_STATUS_REASONS.get(int(host_status[bad[0]]), f"status {int(host_status[bad[0]])}")
        raise ValueError(f"frame {int(bad[0])}: {reason}")
    return frames


@jpeg_decode.register_fake
def _(data: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    # the frame size is in the bytes: a data-dependent shape
    context = torch.library.get_ctx()
    height, width = context.new_dynamic_size(), context.new_dynamic_size()
    return data.new_empty((offsets.shape[0] - 1, height, width, 3))


@torch.library.custom_op("gance::jpeg_decode_layouts", mutates_args=(), device_types="cuda")
def jpeg_decode_layouts(data: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """
    `jpeg_decode` for the videos a user brings: baseline JFIF files of one size and one layout, 4:2:2, 4:2:0, 4:4:4 or grey
    (three equal channels), to RGB [B, H, W, 3] u8, pixel for pixel what libjpeg decodes. Contract and errors as `jpeg_decode`.
    :raises ValueError: a file the decoder does not take, files of more than one size or layout, or a frame whose data is
    bad: the first such frame and the reason.
    """
    _require_cuda(data, torch.uint8, "data")
    if data.dim() != 1 or offsets.dim() != 1 or offsets.dtype != torch.int64:
        raise ValueError("data must be [bytes] uint8 and offsets [B + 1] int64")
    data = data.contiguous()
    host_offsets, infos = _jpeg_headers(data, offsets, layouts=True)
    batch, width, height, layout = len(infos), infos[0].info.width, infos[0].info.height, infos[0].layout
    workspace_bytes = hip_lib.jpeg_decode_layouts_bounds(batch, width, height, layout, int(host_offsets[-1] - host_offsets[0]))
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=data.device)
    frames = torch.empty((batch, height, width, 3), dtype=torch.uint8, device=data.device)
    status = torch.empty((batch,), dtype=torch.int32, device=data.device)
    hip_lib.jpeg_decode_layouts_device(
        data.data_ptr(), host_offsets, infos, workspace.data_ptr(), workspace_bytes, frames.data_ptr(), status.data_ptr(), _stream(data)
    )
    host_status = status.cpu().numpy()
    bad = np.flatnonzero(host_status)
    if bad.size:
        reason = hip_lib.JPEG_STATUS_REASONS.get(int(host_status[bad[0]]), f"status {int(host_status[bad[0]])}")
        raise ValueError(f"frame {int(bad[0])}: {reason}")
    return frames


@jpeg_decode_layouts.register_fake
def _(data: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    context = torch.library.get_ctx()
    height, width = context.new_dynamic_size(), context.new_dynamic_size()
    return data.new_empty((offsets.shape[0] - 1, height, width, 3))


# ---- differentiable synthesis (csrc/synthesis_grad.hip): forward and backward ops of the generator's three layer operations ----


def _f32_cuda(tensor: torch.Tensor, shape: Tuple[int, ...], name: str) -> torch.Tensor:
    _require_cuda(tensor, torch.float32, name)
    if tuple(tensor.shape) != tuple(shape):
        raise ValueError(f"`{name}` must be {list(shape)}, got {list(tensor.shape)}")
    return tensor.contiguous()


def _activation_shape(x: torch.Tensor) -> Tuple[int, int, int, int]:
    if x.dim() != 4:
        raise ValueError(f"`x` must be [B, C, S, S], got {list(x.shape)}")
    return int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), int(x.shape[3])


def _modconv_weight_shape(weight: torch.Tensor) -> Tuple[int, int]:
    if weight.dim() != 4 or weight.shape[0] != 3 or weight.shape[1] != 3:
        raise ValueError(f"`weight` must be [3, 3, Cin, Cout], got {list(weight.shape)}")
    return int(weight.shape[2]), int(weight.shape[3])


@torch.library.custom_op("gance::modconv3x3", mutates_args=(), device_types="cuda")
def modconv3x3(x: torch.Tensor, style: torch.Tensor, demod: torch.Tensor, weight: torch.Tensor, up: bool) -> torch.Tensor:
    """
    The modulated 3x3 conv of the published generator with its style [B, Cin] and demodulation [B, Cout] as inputs:
    demod * conv(style * x, weight), weight [3, 3, Cin, Cout] runtime-scaled; `up`: the stride-2 transposed conv + FIR.
    """
    batch, cin, height, width = _activation_shape(x)
    cout = _modconv_weight_shape(weight)[1]
    x = _f32_cuda(x, (batch, cin, height, width), "x")
    style, demod = _f32_cuda(style, (batch, cin), "style"), _f32_cuda(demod, (batch, cout), "demod")
    weight = _f32_cuda(weight, (3, 3, cin, cout), "weight")
    workspace_bytes = hip_lib.modconv3x3_workspace_bytes(batch, cin, cout, height, up)
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=x.device)
    factor = 2 if up else 1
    y = torch.empty((batch, cout, height * factor, width * factor), dtype=torch.float32, device=x.device)
    hip_lib.modconv3x3_forward_device(
        x.data_ptr(), style.data_ptr(), demod.data_ptr(), weight.data_ptr(), batch, cin, cout, height, width, up, y.data_ptr(),
        workspace.data_ptr(), workspace_bytes, _stream(x),
    )
    return y


@modconv3x3.register_fake
def _(x: torch.Tensor, style: torch.Tensor, demod: torch.Tensor, weight: torch.Tensor, up: bool) -> torch.Tensor:
    factor = 2 if up else 1
    return x.new_empty((x.shape[0], weight.shape[3], x.shape[2] * factor, x.shape[3] * factor))


@torch.library.custom_op("gance::modconv3x3_backward", mutates_args=(), device_types="cuda")
def modconv3x3_backward(  # pylint: disable=too-many-arguments
    grad_y: torch.Tensor, x: torch.Tensor, y: torch.Tensor, style: torch.Tensor, demod: torch.Tensor, weight: torch.Tensor, up: bool
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(grad_x, grad_style, grad_demod) of `modconv3x3` from its inputs and its output `y`; no weight gradient."""
    batch, cin, height, width = _activation_shape(x)
    cout = _modconv_weight_shape(weight)[1]
    factor = 2 if up else 1
    x = _f32_cuda(x, (batch, cin, height, width), "x")
    y = _f32_cuda(y, (batch, cout, height * factor, width * factor), "y")
    grad_y = _f32_cuda(grad_y, tuple(y.shape), "grad_y")
    style, demod = _f32_cuda(style, (batch, cin), "style"), _f32_cuda(demod, (batch, cout), "demod")
    weight = _f32_cuda(weight, (3, 3, cin, cout), "weight")
    workspace_bytes = hip_lib.modconv3x3_workspace_bytes(batch, cin, cout, height, up)
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=x.device)
    grad_x, grad_style, grad_demod = torch.empty_like(x), torch.empty_like(style), torch.empty_like(demod)
    hip_lib.modconv3x3_backward_device(
        grad_y.data_ptr(), x.data_ptr(), y.data_ptr(), style.data_ptr(), demod.data_ptr(), weight.data_ptr(), batch, cin, cout, height, width,
        up, grad_x.data_ptr(), grad_style.data_ptr(), grad_demod.data_ptr(), workspace.data_ptr(), workspace_bytes, _stream(x),
    )
    return grad_x, grad_style, grad_demod


@modconv3x3_backward.register_fake
def _(  # pylint: disable=too-many-arguments
    grad_y: torch.Tensor, x: torch.Tensor, y: torch.Tensor, style: torch.Tensor, demod: torch.Tensor, weight: torch.Tensor, up: bool
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return x.new_empty(x.shape), style.new_empty(style.shape), demod.new_empty(demod.shape)


def _modconv3x3_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    x, style, demod, weight, up = inputs
    ctx.save_for_backward(x, output, style, demod, weight)
    ctx.up = up


def _modconv3x3_grad(ctx, grad_y: torch.Tensor):  # type: ignore[no-untyped-def]
    x, y, style, demod, weight = ctx.saved_tensors
    grad_x, grad_style, grad_demod = modconv3x3_backward(grad_y, x, y, style, demod, weight, ctx.up)
    return grad_x, grad_style, grad_demod, None, None


torch.library.register_autograd("gance::modconv3x3", _modconv3x3_grad, setup_context=_modconv3x3_setup)


@torch.library.custom_op("gance::noise_bias_lrelu", mutates_args=(), device_types="cuda")
def noise_bias_lrelu(x: torch.Tensor, noise: torch.Tensor, strength: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """lrelu_0.2(x + noise * strength + bias[c]) * sqrt(2): noise [1 or B, 1, S, S], strength one value, bias [C]."""
    batch, channels, height, width = _activation_shape(x)
    x = _f32_cuda(x, (batch, channels, height, width), "x")
    if noise.dim() != 4 or noise.shape[0] not in (1, batch):
        raise ValueError(f"`noise` must be [1 or {batch}, 1, {height}, {width}], got {list(noise.shape)}")
    noise = _f32_cuda(noise, (int(noise.shape[0]), 1, height, width), "noise")
    if strength.numel() != 1:
        raise ValueError(f"`strength` must hold one value, got {list(strength.shape)}")
    strength = _f32_cuda(strength, tuple(strength.shape), "strength")
    bias = _f32_cuda(bias, (channels,), "bias")
    out = torch.empty_like(x)
    hip_lib.noise_bias_lrelu_forward_device(
        x.data_ptr(), noise.data_ptr(), int(noise.shape[0]), strength.data_ptr(), bias.data_ptr(), batch, channels, height, width,
        out.data_ptr(), _stream(x),
    )
    return out


@noise_bias_lrelu.register_fake
def _(x: torch.Tensor, noise: torch.Tensor, strength: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return x.new_empty(x.shape)


@torch.library.custom_op("gance::noise_bias_lrelu_backward", mutates_args=(), device_types="cuda")
def noise_bias_lrelu_backward(grad_out: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """grad_x of `noise_bias_lrelu`: the slope of every position is read off the sign of the saved output."""
    batch, channels, height, width = _activation_shape(out)
    out = _f32_cuda(out, (batch, channels, height, width), "out")
    grad_out = _f32_cuda(grad_out, tuple(out.shape), "grad_out")
    grad_x = torch.empty_like(out)
    hip_lib.noise_bias_lrelu_backward_device(grad_out.data_ptr(), out.data_ptr(), batch, channels, height, width, grad_x.data_ptr(), _stream(out))
    return grad_x


@noise_bias_lrelu_backward.register_fake
def _(grad_out: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    return out.new_empty(out.shape)


@torch.library.custom_op("gance::noise_bias_lrelu_backward_noise", mutates_args=(), device_types="cuda")
def noise_bias_lrelu_backward_noise(
    grad_out: torch.Tensor, out: torch.Tensor, strength: torch.Tensor, noise_batch: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    (grad_x, grad_noise) of `noise_bias_lrelu` in one pass over grad_out and out: grad_x is bit for bit what
    `noise_bias_lrelu_backward` gives, grad_noise [noise_batch, 1, S, S] = strength * the sum of grad_x over the channels
    (and, for a shared plane, over the batch), in a fixed order.
    """
    batch, channels, height, width = _activation_shape(out)
    out = _f32_cuda(out, (batch, channels, height, width), "out")
    grad_out = _f32_cuda(grad_out, tuple(out.shape), "grad_out")
    if strength.numel() != 1:
        raise ValueError(f"`strength` must hold one value, got {list(strength.shape)}")
    strength = _f32_cuda(strength, tuple(strength.shape), "strength")
    if noise_batch not in (1, batch):
        raise ValueError(f"`noise_batch` must be 1 or {batch}, got {noise_batch}")
    grad_x = torch.empty_like(out)
    grad_noise = torch.empty((noise_batch, 1, height, width), dtype=torch.float32, device=out.device)
    hip_lib.noise_bias_lrelu_backward_noise_device(
        grad_out.data_ptr(), out.data_ptr(), strength.data_ptr(), noise_batch, batch, channels, height, width, grad_x.data_ptr(),
        grad_noise.data_ptr(), _stream(out),
    )
    return grad_x, grad_noise


@noise_bias_lrelu_backward_noise.register_fake
def _(grad_out: torch.Tensor, out: torch.Tensor, strength: torch.Tensor, noise_batch: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return out.new_empty(out.shape), out.new_empty((noise_batch, 1, out.shape[2], out.shape[3]))


def _noise_bias_lrelu_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    _, noise, strength, _ = inputs
    ctx.save_for_backward(output, strength)
    ctx.noise_batch = int(noise.shape[0])


def _noise_bias_lrelu_grad(ctx, grad_out: torch.Tensor):  # type: ignore[no-untyped-def]
    out, strength = ctx.saved_tensors
    if ctx.needs_input_grad[1]:
        grad_x, grad_noise = noise_bias_lrelu_backward_noise(grad_out, out, strength, ctx.noise_batch)
        return grad_x, grad_noise, None, None
    return noise_bias_lrelu_backward(grad_out, out), None, None, None  # (strength and bias have no gradient)


torch.library.register_autograd("gance::noise_bias_lrelu", _noise_bias_lrelu_grad, setup_context=_noise_bias_lrelu_setup)


@torch.library.custom_op("gance::torgb_skip", mutates_args=(), device_types="cuda")
def torgb_skip(x: torch.Tensor, style: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, y_prev: Optional[torch.Tensor]) -> torch.Tensor:
    """
    The image step of the skip generator: upsample_2d(y_prev) + sum_i weight[i, c] * style[b, i] * x[b, i] + bias[c], no
    demodulation; weight [Cin, 3] runtime-scaled, y_prev [B, 3, S / 2, S / 2] or None (the 4x4 layer).
    """
    batch, cin, height, width = _activation_shape(x)
    x = _f32_cuda(x, (batch, cin, height, width), "x")
    style, weight, bias = _f32_cuda(style, (batch, cin), "style"), _f32_cuda(weight, (cin, 3), "weight"), _f32_cuda(bias, (3,), "bias")
    if y_prev is not None:
        y_prev = _f32_cuda(y_prev, (batch, 3, height // 2, width // 2), "y_prev")
    y = torch.empty((batch, 3, height, width), dtype=torch.float32, device=x.device)
    hip_lib.torgb_skip_forward_device(
        x.data_ptr(), style.data_ptr(), weight.data_ptr(), bias.data_ptr(), 0 if y_prev is None else y_prev.data_ptr(), batch, cin, height,
        width, y.data_ptr(), _stream(x),
    )
    return y


@torgb_skip.register_fake
def _(x: torch.Tensor, style: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, y_prev: Optional[torch.Tensor]) -> torch.Tensor:
    return x.new_empty((x.shape[0], 3, x.shape[2], x.shape[3]))


@torch.library.custom_op("gance::torgb_skip_backward", mutates_args=(), device_types="cuda")
def torgb_skip_backward(
    grad_y: torch.Tensor, x: torch.Tensor, style: torch.Tensor, weight: torch.Tensor, has_y_prev: bool
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(grad_x, grad_style, grad_y_prev) of `torgb_skip`; grad_y_prev is empty ([0]) without a skip image."""
    batch, cin, height, width = _activation_shape(x)
    x = _f32_cuda(x, (batch, cin, height, width), "x")
    grad_y = _f32_cuda(grad_y, (batch, 3, height, width), "grad_y")
    style, weight = _f32_cuda(style, (batch, cin), "style"), _f32_cuda(weight, (cin, 3), "weight")
    workspace_bytes = hip_lib.torgb_skip_workspace_bytes(batch, cin, height)
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=x.device)
    grad_x, grad_style = torch.empty_like(x), torch.empty_like(style)
    grad_y_prev = torch.empty((batch, 3, height // 2, width // 2) if has_y_prev else (0,), dtype=torch.float32, device=x.device)
    hip_lib.torgb_skip_backward_device(
        grad_y.data_ptr(), x.data_ptr(), style.data_ptr(), weight.data_ptr(), batch, cin, height, width, grad_x.data_ptr(),
        grad_style.data_ptr(), grad_y_prev.data_ptr() if has_y_prev else 0, workspace.data_ptr(), workspace_bytes, _stream(x),
    )
    return grad_x, grad_style, grad_y_prev


@torgb_skip_backward.register_fake
def _(
    grad_y: torch.Tensor, x: torch.Tensor, style: torch.Tensor, weight: torch.Tensor, has_y_prev: bool
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    prev_shape = (x.shape[0], 3, x.shape[2] // 2, x.shape[3] // 2) if has_y_prev else (0,)
    return x.new_empty(x.shape), style.new_empty(style.shape), x.new_empty(prev_shape)


def _torgb_skip_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    x, style, weight, _, y_prev = inputs
    ctx.save_for_backward(x, style, weight)
    ctx.has_y_prev = y_prev is not None


def _torgb_skip_grad(ctx, grad_y: torch.Tensor):  # type: ignore[no-untyped-def]
    x, style, weight = ctx.saved_tensors
    grad_x, grad_style, grad_y_prev = torgb_skip_backward(grad_y, x, style, weight, ctx.has_y_prev)
    return grad_x, grad_style, None, None, grad_y_prev if ctx.has_y_prev else None


torch.library.register_autograd("gance::torgb_skip", _torgb_skip_grad, setup_context=_torgb_skip_setup)


# ---- projection's losses (csrc/projection.hip) ----


def _regularizer_planes(noise: torch.Tensor) -> Tuple[int, int]:
    if noise.dim() != 4 or noise.shape[1] != 1 or noise.shape[2] != noise.shape[3]:
        raise ValueError(f"`noise` must be [B, 1, S, S], got {list(noise.shape)}")
    return int(noise.shape[0]), int(noise.shape[2])


def _regularizer_forward(noise: torch.Tensor, batch: int, side: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(reg, means, workspace) of one forward call; the workspace holds the pyramid the backward reads."""
    workspace_bytes = hip_lib.noise_regularizer_workspace_bytes(batch, side)
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=noise.device)
    reg = torch.empty((batch,), dtype=torch.float32, device=noise.device)
    means = torch.empty((batch, hip_lib.noise_regularizer_levels(side), 2), dtype=torch.float32, device=noise.device)
    hip_lib.noise_regularizer_forward_device(
        noise.data_ptr(), batch, side, reg.data_ptr(), means.data_ptr(), workspace.data_ptr(), workspace_bytes, _stream(noise)
    )
    return reg, means, workspace


@torch.library.custom_op("gance::noise_regularizer", mutates_args=(), device_types="cuda")
def noise_regularizer(noise: torch.Tensor) -> torch.Tensor:
    """
    The noise regulariser of StyleGAN2's projector per sample: over the pyramid of 2x2 means of each plane [B, 1, S, S] (S a
    power of two in [4, 1024], down to 8 x 8), the sum of mean(v * roll(v, 1, W))^2 + mean(v * roll(v, 1, H))^2 -> [B].
    """
    batch, side = _regularizer_planes(noise)
    noise = _f32_cuda(noise, (batch, 1, side, side), "noise")
    return _regularizer_forward(noise, batch, side)[0]


@noise_regularizer.register_fake
def _(noise: torch.Tensor) -> torch.Tensor:
    return noise.new_empty((noise.shape[0],))


@torch.library.custom_op("gance::noise_regularizer_backward", mutates_args=(), device_types="cuda")
def noise_regularizer_backward(grad_reg: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """
    grad_noise of `noise_regularizer`. The pyramid and the means are rebuilt here (three small launches over 4/3 of the plane)
    instead of being carried from the forward op: the op stays a function of its inputs alone.
    """
    batch, side = _regularizer_planes(noise)
    noise = _f32_cuda(noise, (batch, 1, side, side), "noise")
    grad_reg = _f32_cuda(grad_reg, (batch,), "grad_reg")
    _, means, workspace = _regularizer_forward(noise, batch, side)
    grad_noise = torch.empty_like(noise)
    hip_lib.noise_regularizer_backward_device(
        grad_reg.data_ptr(), noise.data_ptr(), means.data_ptr(), workspace.data_ptr(), workspace.numel(), batch, side, grad_noise.data_ptr(),
        _stream(noise),
    )
    return grad_noise


@noise_regularizer_backward.register_fake
def _(grad_reg: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    return noise.new_empty(noise.shape)


def _noise_regularizer_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    ctx.save_for_backward(inputs[0])


def _noise_regularizer_grad(ctx, grad_reg: torch.Tensor):  # type: ignore[no-untyped-def]
    (noise,) = ctx.saved_tensors
    return noise_regularizer_backward(grad_reg, noise)


torch.library.register_autograd("gance::noise_regularizer", _noise_regularizer_grad, setup_context=_noise_regularizer_setup)


def _distance_shapes(image: torch.Tensor, target: torch.Tensor) -> Tuple[int, int]:
    if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != image.shape[3]:
        raise ValueError(f"`image` must be [B, 3, R, R], got {list(image.shape)}")
    return int(image.shape[0]), int(image.shape[2])


def _distance_forward(image: torch.Tensor, target: torch.Tensor, batch: int, resolution: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dist, workspace) of one forward call; the workspace holds the pyramid of differences the backward reads."""
    workspace_bytes = hip_lib.pyramid_distance_workspace_bytes(batch, resolution)
    side = min(resolution, 256)
    image = _f32_cuda(image, (batch, 3, resolution, resolution), "image")
    target = _f32_cuda(target, (batch, 3, side, side), "target")
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=image.device)
    dist = torch.empty((batch,), dtype=torch.float32, device=image.device)
    hip_lib.pyramid_distance_forward_device(
        image.data_ptr(), target.data_ptr(), batch, resolution, dist.data_ptr(), workspace.data_ptr(), workspace_bytes, _stream(image)
    )
    return dist, workspace


@torch.library.custom_op("gance::pyramid_distance", mutates_args=(), device_types="cuda")
def pyramid_distance(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """
    A weight-free multi-scale squared distance (not LPIPS): image [B, 3, R, R] in -1 ... 1 (R a power of two in [8, 1024]) is
    area-averaged to T = min(R, 256) on the 0 ... 255 scale, d_0 = (that - target [B, 3, T, T]) / 255, d_l the 2x2 means down to
    8 x 8; the sum over the levels of mean(d_l^2) -> [B].
    """
    batch, resolution = _distance_shapes(image, target)
    return _distance_forward(image, target, batch, resolution)[0]


@pyramid_distance.register_fake
def _(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return image.new_empty((image.shape[0],))


@torch.library.custom_op("gance::pyramid_distance_backward", mutates_args=(), device_types="cuda")
def pyramid_distance_backward(grad_dist: torch.Tensor, image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """grad_image of `pyramid_distance`; the pyramid of differences is rebuilt here, as in `noise_regularizer_backward`."""
    batch, resolution = _distance_shapes(image, target)
    grad_dist = _f32_cuda(grad_dist, (batch,), "grad_dist")
    _, workspace = _distance_forward(image, target, batch, resolution)
    grad_image = torch.empty((batch, 3, resolution, resolution), dtype=torch.float32, device=image.device)
    hip_lib.pyramid_distance_backward_device(
        grad_dist.data_ptr(), workspace.data_ptr(), workspace.numel(), batch, resolution, grad_image.data_ptr(), _stream(image)
    )
    return grad_image


@pyramid_distance_backward.register_fake
def _(grad_dist: torch.Tensor, image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return image.new_empty(image.shape)


def _pyramid_distance_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    ctx.save_for_backward(*inputs)


def _pyramid_distance_grad(ctx, grad_dist: torch.Tensor):  # type: ignore[no-untyped-def]
    image, target = ctx.saved_tensors
    return pyramid_distance_backward(grad_dist, image, target), None  # (the target has no gradient)


torch.library.register_autograd("gance::pyramid_distance", _pyramid_distance_grad, setup_context=_pyramid_distance_setup)


# ---- the plain 3x3 convolution (csrc/conv3x3.hip): no style, no demodulation, no weight gradient ----


def conv3x3_transposed_weight(weight: torch.Tensor) -> torch.Tensor:
    """wt[ty, tx, o, i] = w[2 - ty, 2 - tx, i, o] of a weight [3, 3, Cin, Cout]: the image under which `conv3x3` is its own
    input gradient (and the weight's own image again: an involution)."""
    _modconv_weight_shape(weight)
    return weight.flip(0, 1).transpose(2, 3).contiguous()


def _conv3x3_f32_cuda(tensor: torch.Tensor, shape: Tuple[int, ...], name: str) -> None:
    """:raises ValueError: a tensor the kernel does not take as it is (nothing is copied or converted on the way in)."""
    if not tensor.is_cuda:
        raise ValueError(f"gance::conv3x3 runs on an MI355X only: `{name}` is on {tensor.device} (there is no CPU fallback)")
    if tensor.dtype != torch.float32:
        raise ValueError(f"`{name}` must be torch.float32, got {tensor.dtype}")
    if tuple(tensor.shape) != tuple(shape):
        raise ValueError(f"`{name}` must be {list(shape)}, got {list(tensor.shape)}")
    if not tensor.is_contiguous():
        raise ValueError(f"`{name}` must be contiguous")


# (registered for every device, so that a CPU tensor reaches the ValueError below instead of the dispatcher's NotImplementedError)
@torch.library.custom_op("gance::conv3x3", mutates_args=())
def conv3x3(x: torch.Tensor, weight: torch.Tensor, weight_transposed: torch.Tensor) -> torch.Tensor:
    """
    The 3x3 convolution with zero padding 1 and stride 1 (cross-correlation) of x [B, Cin, S, S] with weight [3, 3, Cin, Cout];
    `weight_transposed` [3, 3, Cout, Cin] = `conv3x3_transposed_weight(weight)` is read by the backward only: grad_x =
    conv3x3(grad_y, weight_transposed, weight). The weights receive no gradient.
    """
    batch, cin, height, width = _activation_shape(x)
    cout = _modconv_weight_shape(weight)[1]
    if height != width:
        raise ValueError(f"`x` must be square, got {list(x.shape)}")
    _conv3x3_f32_cuda(x, (batch, cin, height, width), "x")
    _conv3x3_f32_cuda(weight, (3, 3, cin, cout), "weight")
    _conv3x3_f32_cuda(weight_transposed, (3, 3, cout, cin), "weight_transposed")
    workspace_bytes = hip_lib.conv3x3_workspace_bytes(batch, cin, cout, height)
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=x.device)
    y = torch.empty((batch, cout, height, width), dtype=torch.float32, device=x.device)
    hip_lib.conv3x3_forward_device(
        x.data_ptr(), weight.data_ptr(), batch, cin, cout, height, width, y.data_ptr(), workspace.data_ptr(), workspace_bytes, _stream(x)
    )
    return y


@conv3x3.register_fake
def _(x: torch.Tensor, weight: torch.Tensor, weight_transposed: torch.Tensor) -> torch.Tensor:
    return x.new_empty((x.shape[0], weight.shape[3], x.shape[2], x.shape[3]))


def _conv3x3_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    _, weight, weight_transposed = inputs
    ctx.save_for_backward(weight, weight_transposed)


def _conv3x3_grad(ctx, grad_y: torch.Tensor):  # type: ignore[no-untyped-def]
    weight, weight_transposed = ctx.saved_tensors
    return conv3x3(grad_y.contiguous(), weight_transposed, weight), None, None


torch.library.register_autograd("gance::conv3x3", _conv3x3_grad, setup_context=_conv3x3_setup)


# ---- LPIPS on VGG16 (csrc/lpips.hip; the convolutions are gance::modconv3x3 with unit style and demodulation) ----


def _square_activation(x: torch.Tensor, name: str) -> Tuple[int, int, int]:
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f"`{name}` must be [B, C, S, S], got {list(x.shape)}")
    return int(x.shape[0]), int(x.shape[1]), int(x.shape[2])


def _lpips_image_shape(image: torch.Tensor) -> Tuple[int, int]:
    if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != image.shape[3]:
        raise ValueError(f"`image` must be [B, 3, R, R], got {list(image.shape)}")
    return int(image.shape[0]), int(image.shape[2])


LPIPS_INPUT_CHANNELS = 16  # RGB and 13 zero channels: conv1_1 runs through modconv3x3, whose channel counts are multiples of 16


@torch.library.custom_op("gance::lpips_input", mutates_args=(), device_types="cuda")
def lpips_input(image: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, side: int) -> torch.Tensor:
    """
    The input of the VGG16 of LPIPS: image [B, 3, R, R] (R a multiple of `side`) is area-averaged by R / side, then
    (x - shift[c]) / scale[c] -> [B, 16, side, side] with channels 3 ... 15 zero.
    """
    batch, resolution = _lpips_image_shape(image)
    image = _f32_cuda(image, (batch, 3, resolution, resolution), "image")
    shift, scale = _f32_cuda(shift, (3,), "shift"), _f32_cuda(scale, (3,), "scale")
    out = torch.empty((batch, LPIPS_INPUT_CHANNELS, side, side), dtype=torch.float32, device=image.device)
    hip_lib.lpips_input_forward_device(image.data_ptr(), shift.data_ptr(), scale.data_ptr(), batch, resolution, side, out.data_ptr(), _stream(image))
    return out


@lpips_input.register_fake
def _(image: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, side: int) -> torch.Tensor:
    return image.new_empty((image.shape[0], LPIPS_INPUT_CHANNELS, side, side))


@torch.library.custom_op("gance::lpips_input_backward", mutates_args=(), device_types="cuda")
def lpips_input_backward(grad: torch.Tensor, scale: torch.Tensor, resolution: int) -> torch.Tensor:
    """grad_image [B, 3, R, R] of `lpips_input`: grad[:, :3] / (scale[c] * (R / side)^2) over each cell."""
    batch, _, side = _square_activation(grad, "grad")
    grad = _f32_cuda(grad, (batch, LPIPS_INPUT_CHANNELS, side, side), "grad")
    scale = _f32_cuda(scale, (3,), "scale")
    grad_image = torch.empty((batch, 3, resolution, resolution), dtype=torch.float32, device=grad.device)
    hip_lib.lpips_input_backward_device(grad.data_ptr(), scale.data_ptr(), batch, resolution, side, grad_image.data_ptr(), _stream(grad))
    return grad_image


@lpips_input_backward.register_fake
def _(grad: torch.Tensor, scale: torch.Tensor, resolution: int) -> torch.Tensor:
    return grad.new_empty((grad.shape[0], 3, resolution, resolution))


def _lpips_input_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    image, _, scale, _ = inputs
    ctx.save_for_backward(scale)
    ctx.resolution = int(image.shape[2])


def _lpips_input_grad(ctx, grad: torch.Tensor):  # type: ignore[no-untyped-def]
    (scale,) = ctx.saved_tensors
    return lpips_input_backward(grad, scale, ctx.resolution), None, None, None  # (shift and scale have no gradient)


torch.library.register_autograd("gance::lpips_input", _lpips_input_grad, setup_context=_lpips_input_setup)


@torch.library.custom_op("gance::bias_relu", mutates_args=(), device_types="cuda")
def bias_relu(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """max(x + bias[c], 0) over x [B, C, S, S]."""
    batch, channels, side = _square_activation(x, "x")
    x, bias = _f32_cuda(x, (batch, channels, side, side), "x"), _f32_cuda(bias, (channels,), "bias")
    y = torch.empty_like(x)
    hip_lib.bias_relu_forward_device(x.data_ptr(), bias.data_ptr(), batch, channels, side, False, y.data_ptr(), 0, _stream(x))
    return y


@bias_relu.register_fake
def _(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return x.new_empty(x.shape)


@torch.library.custom_op("gance::bias_relu_backward", mutates_args=(), device_types="cuda")
def bias_relu_backward(grad_y: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """grad_x of `bias_relu` from the saved output: (y > 0) * grad_y."""
    batch, channels, side = _square_activation(y, "y")
    y = _f32_cuda(y, (batch, channels, side, side), "y")
    grad_y = _f32_cuda(grad_y, tuple(y.shape), "grad_y")
    grad_x = torch.empty_like(y)
    hip_lib.bias_relu_backward_device(grad_y.data_ptr(), 0, y.data_ptr(), batch, channels, side, False, grad_x.data_ptr(), _stream(y))
    return grad_x


@bias_relu_backward.register_fake
def _(grad_y: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return y.new_empty(y.shape)


def _bias_relu_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    ctx.save_for_backward(output)


def _bias_relu_grad(ctx, grad_y: torch.Tensor):  # type: ignore[no-untyped-def]
    (y,) = ctx.saved_tensors
    return bias_relu_backward(grad_y, y), None  # (the bias has no gradient)


torch.library.register_autograd("gance::bias_relu", _bias_relu_grad, setup_context=_bias_relu_setup)


@torch.library.custom_op("gance::bias_relu_pool", mutates_args=(), device_types="cuda")
def bias_relu_pool(x: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, p): y = max(x + bias[c], 0) over x [B, C, S, S], S even, and p [B, C, S / 2, S / 2] its 2x2 max pool, in one pass over x."""
    batch, channels, side = _square_activation(x, "x")
    x, bias = _f32_cuda(x, (batch, channels, side, side), "x"), _f32_cuda(bias, (channels,), "bias")
    y = torch.empty_like(x)
    p = torch.empty((batch, channels, side // 2, side // 2), dtype=torch.float32, device=x.device)
    hip_lib.bias_relu_forward_device(x.data_ptr(), bias.data_ptr(), batch, channels, side, True, y.data_ptr(), p.data_ptr(), _stream(x))
    return y, p


@bias_relu_pool.register_fake
def _(x: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return x.new_empty(x.shape), x.new_empty((x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2))


@torch.library.custom_op("gance::bias_relu_pool_backward", mutates_args=(), device_types="cuda")
def bias_relu_pool_backward(grad_y: torch.Tensor, grad_p: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """
    grad_x of `bias_relu_pool`: (y > 0) * (grad_y + grad_p routed to the selected element of its window), the largest y of the
    window and the first in row-major order among equals.
    """
    batch, channels, side = _square_activation(y, "y")
    y = _f32_cuda(y, (batch, channels, side, side), "y")
    grad_y = _f32_cuda(grad_y, tuple(y.shape), "grad_y")
    grad_p = _f32_cuda(grad_p, (batch, channels, side // 2, side // 2), "grad_p")
    grad_x = torch.empty_like(y)
    hip_lib.bias_relu_backward_device(
        grad_y.data_ptr(), grad_p.data_ptr(), y.data_ptr(), batch, channels, side, True, grad_x.data_ptr(), _stream(y)
    )
    return grad_x


@bias_relu_pool_backward.register_fake
def _(grad_y: torch.Tensor, grad_p: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return y.new_empty(y.shape)


def _bias_relu_pool_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    ctx.save_for_backward(output[0])


def _bias_relu_pool_grad(ctx, grad_y: torch.Tensor, grad_p: torch.Tensor):  # type: ignore[no-untyped-def]
    (y,) = ctx.saved_tensors
    return bias_relu_pool_backward(grad_y, grad_p, y), None  # (the bias has no gradient)


torch.library.register_autograd("gance::bias_relu_pool", _bias_relu_pool_grad, setup_context=_bias_relu_pool_setup)


def _lpips_layer_arguments(f: torch.Tensor, target: torch.Tensor, lin: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int, int, int]:
    batch, channels, side = _square_activation(f, "f")
    f = _f32_cuda(f, (batch, channels, side, side), "f")
    return f, _f32_cuda(target, tuple(f.shape), "target"), _f32_cuda(lin, (channels,), "lin"), batch, channels, side


@torch.library.custom_op("gance::lpips_layer", mutates_args=(), device_types="cuda")
def lpips_layer(f: torch.Tensor, target: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """
    The LPIPS head of one tap: with u = f / (|f|_2 over the channels + 1e-10) per pixel and `target` [B, C, S, S] normalised
    already (`lpips_normalize`), the mean over the pixels of sum_c lin[c] * (u_c - target_c)^2 -> [B].
    """
    f, target, lin, batch, channels, side = _lpips_layer_arguments(f, target, lin)
    workspace_bytes = hip_lib.lpips_layer_workspace_bytes(batch, side)
    workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=f.device)
    dist = torch.empty((batch,), dtype=torch.float32, device=f.device)
    hip_lib.lpips_layer_forward_device(
        f.data_ptr(), target.data_ptr(), lin.data_ptr(), batch, channels, side, dist.data_ptr(), workspace.data_ptr(), workspace_bytes, _stream(f)
    )
    return dist


@lpips_layer.register_fake
def _(f: torch.Tensor, target: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    return f.new_empty((f.shape[0],))


@torch.library.custom_op("gance::lpips_layer_backward", mutates_args=(), device_types="cuda")
def lpips_layer_backward(grad_dist: torch.Tensor, f: torch.Tensor, target: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """grad_f of `lpips_layer`; the norm and the per-pixel dot product are recomputed. At an all-zero pixel d|f| / df is taken as 0."""
    f, target, lin, batch, channels, side = _lpips_layer_arguments(f, target, lin)
    grad_dist = _f32_cuda(grad_dist, (batch,), "grad_dist")
    grad_f = torch.empty_like(f)
    hip_lib.lpips_layer_backward_device(
        grad_dist.data_ptr(), f.data_ptr(), target.data_ptr(), lin.data_ptr(), batch, channels, side, grad_f.data_ptr(), _stream(f)
    )
    return grad_f


@lpips_layer_backward.register_fake
def _(grad_dist: torch.Tensor, f: torch.Tensor, target: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    return f.new_empty(f.shape)


def _lpips_layer_setup(ctx, inputs, output) -> None:  # type: ignore[no-untyped-def]
    ctx.save_for_backward(*inputs)


def _lpips_layer_grad(ctx, grad_dist: torch.Tensor):  # type: ignore[no-untyped-def]
    f, target, lin = ctx.saved_tensors
    return lpips_layer_backward(grad_dist, f, target, lin), None, None  # (the target and lin have no gradient)


torch.library.register_autograd("gance::lpips_layer", _lpips_layer_grad, setup_context=_lpips_layer_setup)


@torch.library.custom_op("gance::lpips_normalize", mutates_args=(), device_types="cuda")
def lpips_normalize(f: torch.Tensor) -> torch.Tensor:
    """f / (|f|_2 over the channels + 1e-10) per pixel of f [B, C, S, S]: the target's side of `lpips_layer`. No gradient."""
    batch, channels, side = _square_activation(f, "f")
    f = _f32_cuda(f, (batch, channels, side, side), "f")
    out = torch.empty_like(f)
    hip_lib.lpips_normalize_device(f.data_ptr(), batch, channels, side, out.data_ptr(), _stream(f))
    return out


@lpips_normalize.register_fake
def _(f: torch.Tensor) -> torch.Tensor:
    return f.new_empty(f.shape)
