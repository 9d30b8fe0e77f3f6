"""
ctypes binding of libgance_hip.so (C ABI in include/gance_hip.h).

This is the ONLY route from Python to the synthesis / audio kernels. If the shared library has not
been built (`python -c "import __graft_entry__ as g; g.build()"` or `make -C gance_amd/csrc`) or no
MI355X is visible, calls raise: there is no CPU fallback in the product path.
"""

import ctypes
import os
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch  # noqa: F401  pylint: disable=unused-import
# torch is imported BEFORE the dlopen below on purpose: the PyTorch-ROCm wheel carries its own HIP /
# HSA runtime, and a process must end up with exactly one. Loading libgance_hip.so first would pull
# in /opt/rocm's copy and the two runtimes then fight over the device (observed: hipGetDeviceCount
# fails). With torch loaded first the library binds to the runtime torch already mapped.

from gance_amd.stylegan2 import spec as sg2_spec

LIBRARY_NAME = "libgance_hip.so"
# GANCE_HIP_LIBRARY: another build of the same ABI (A/B timing of kernel variants); default in-tree
LIBRARY_PATH = Path(os.environ.get("GANCE_HIP_LIBRARY") or Path(__file__).resolve().parent / LIBRARY_NAME)

GANCE_OK = 0
GANCE_FLAG_PROFILE_STEPS = 1
GANCE_FLAG_DIRECT_CONV = 2
GANCE_FLAG_FORCE_WINOGRAD = 4
GANCE_FLAG_SPLIT_UPFIR = 8
GANCE_FLAG_FORCE_FUSED_UPFIR = 16
GANCE_FLAG_PRIVATE_WORKSPACE = 32
GANCE_FLAG_WINOGRAD43 = 64
GANCE_FLAG_FMAP_BASE_8K = 128  # the network is config-e (fmap_base = 8 << 10)

STATUS_NAMES = {
    1: "GANCE_ERR_INVALID_ARGUMENT",
    2: "GANCE_ERR_BAD_WEIGHTS",
    3: "GANCE_ERR_HIP",
    4: "GANCE_ERR_OUT_OF_MEMORY",
    5: "GANCE_ERR_NO_DEVICE",
}


class GanceHipError(RuntimeError):
    """A libgance_hip call returned a non-zero status."""

    def __init__(self, status: int, message: str) -> None:
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class EngineConfig(ctypes.Structure):
    """`gance_engine_config` of include/gance_hip.h."""

    _fields_ = [
        ("resolution", ctypes.c_int32),
        ("max_batch", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("flags", ctypes.c_int32),
    ]


class BlendConfig(ctypes.Structure):
    """`gance_blend_config` of include/gance_hip.h."""

    _fields_ = [
        ("num_frames", ctypes.c_int32),
        ("vector_length", ctypes.c_int32),
        ("num_projection_frames", ctypes.c_int32),
        ("latent_depth", ctypes.c_int32),
        ("blend_depth", ctypes.c_int32),
        ("fft_roll_enabled", ctypes.c_int32),
        ("num_networks", ctypes.c_int32),
        ("has_amplitude_range", ctypes.c_int32),
        ("alpha", ctypes.c_double),
        ("amplitude_lo", ctypes.c_double),
        ("amplitude_hi", ctypes.c_double),
        ("index_savgol_window_length", ctypes.c_int32),
        ("index_savgol_polyorder", ctypes.c_int32),
    ]


_F32P = ctypes.POINTER(ctypes.c_float)
_U8P = ctypes.POINTER(ctypes.c_uint8)

# name -> (restype, argtypes); every symbol include/gance_hip.h declares.
SIGNATURES = {
    "gance_last_error": (ctypes.c_char_p, []),
    "gance_abi_version": (ctypes.c_int, []),
    "gance_engine_create": (
        ctypes.c_int,
        [ctypes.POINTER(EngineConfig), _F32P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)],
    ),
    "gance_engine_destroy": (None, [ctypes.c_void_p]),
    "gance_engine_set_profiling": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p]),
    "gance_engine_vector_length": (ctypes.c_int32, [ctypes.c_void_p]),
    "gance_engine_num_layers": (ctypes.c_int32, [ctypes.c_void_p]),
    "gance_engine_resolution": (ctypes.c_int32, [ctypes.c_void_p]),
    "gance_engine_max_batch": (ctypes.c_int32, [ctypes.c_void_p]),
    "gance_weight_blob_floats": (ctypes.c_uint64, [ctypes.c_int32]),
    "gance_weight_blob_floats_flags": (ctypes.c_uint64, [ctypes.c_int32, ctypes.c_int32]),
    "gance_synthesize_w": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_synthesize_z": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_synthesize_w_host": (ctypes.c_int, [ctypes.c_void_p, _F32P, ctypes.c_int32, _U8P, _F32P]),
    "gance_synthesize_z_host": (
        ctypes.c_int,
        [ctypes.c_void_p, _F32P, ctypes.c_int32, ctypes.c_float, _U8P, _F32P],
    ),
    "gance_engine_randomize_noise": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    ),
    "gance_engine_restore_noise": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "gance_engine_debug_read_noise": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _F32P, ctypes.c_uint64]),
    "gance_engine_step_count": (ctypes.c_int32, [ctypes.c_void_p]),
    "gance_engine_step_info": (
        ctypes.c_int,
        [
            ctypes.c_void_p,
            ctypes.c_int32,
            ctypes.c_char_p,
            ctypes.POINTER(ctypes.c_float),
            ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(ctypes.c_double),
        ],
    ),
    "gance_engine_describe_plan": (
        ctypes.c_int, [ctypes.POINTER(EngineConfig), ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_uint64]
    ),
    "gance_engine_debug_stop_after": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "gance_engine_debug_read_activation": (
        ctypes.c_int,
        [
            ctypes.c_void_p,
            ctypes.c_int32,
            _F32P,
            ctypes.c_uint64,
            ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32),
        ],
    ),
    "gance_engine_debug_read_skip_image": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _F32P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int32)]
    ),
    "gance_engine_debug_mapping": (ctypes.c_int, [ctypes.c_void_p, _F32P, ctypes.c_int32, ctypes.c_int32, _F32P, ctypes.c_uint64]),
    "gance_engine_debug_dlatents": (ctypes.c_int, [ctypes.c_void_p, _F32P, ctypes.c_int32, ctypes.c_float, _F32P, ctypes.c_uint64]),
    "gance_engine_debug_read_style": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _F32P, ctypes.c_uint64]),
    "gance_engine_debug_read_demod": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _F32P, ctypes.c_uint64]),
    "gance_engine_debug_border_residue": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64]),
    "gance_engine_debug_poison_scratch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float, ctypes.c_int32]),
    "gance_blend_create": (
        ctypes.c_int,
        [ctypes.POINTER(BlendConfig), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)],
    ),
    "gance_blend_destroy": (None, [ctypes.c_void_p]),
    "gance_blend_run": (
        ctypes.c_int,
        [
            ctypes.c_void_p,
            ctypes.c_void_p,
            ctypes.c_uint64,
            ctypes.c_void_p,
            ctypes.c_void_p,
            ctypes.c_void_p,
            ctypes.c_int32,
            ctypes.c_void_p,
        ],
    ),
    "gance_blend_read_stage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64]),
    "gance_vec_savgol_f64": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_vec_fourier_resample_f64": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    ),
    "gance_vec_spectrogram_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gance_vec_spectrogram2_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gance_vec_minmax_scale_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    "gance_vec_remap_f64": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_vec_rms_rolling_average": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p],
    ),
    "gance_vec_quantize_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "gance_debug_fourier_resample_matrix": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]),
    "gance_debug_savgol_table": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_uint64]),
    "gance_resize_bicubic_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p],
    ),
    "gance_phash_crops_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
         ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p],
    ),
    "gance_overlay_boxes_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
         ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_void_p],
    ),
    "gance_resample_audio_f32": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_resample_audio_f64": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_debug_resample_filter": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_uint64]),
    "gance_jpeg_encode_bounds": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_jpeg_encode_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_jpeg_encode_rect_bounds": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_jpeg_encode_rect_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_jpeg_encode_rect_optimized_bounds": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_jpeg_encode_rect_optimized_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_jpeg_optimal_tables": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_jpeg_parse_header": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "gance_png_encode_bounds": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_png_encode_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_png_encode_lz_bounds": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_png_encode_lz_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_jpeg_decode_bounds": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_jpeg_decode_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_jpeg_parse_header_layouts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "gance_jpeg_decode_layouts_bounds": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_jpeg_decode_layouts_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_debug_place_panels_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
         ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p],
    ),
    "gance_debug_draw_panels_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p],
    ),
    "gance_debug_scatter3d_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_debug_draw_scatter3d_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
         ctypes.c_void_p],
    ),
    "gance_debug_draw_text_u8": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p],
    ),
    "gance_debug_font_columns": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    "gance_vec_rms_rolling_max": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p],
    ),
    "gance_gaussian_noise": (
        ctypes.c_int,
        [
            ctypes.c_void_p,
            ctypes.c_int32,
            ctypes.c_int32,
            ctypes.c_double,
            ctypes.c_double,
            ctypes.POINTER(ctypes.c_double),
            ctypes.c_void_p,
            ctypes.c_void_p,
        ],
    ),
    "gance_modconv3x3_workspace_bytes": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_modconv3x3_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_modconv3x3_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_noise_bias_lrelu_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_noise_bias_lrelu_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_torgb_skip_workspace_bytes": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_torgb_skip_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_torgb_skip_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_noise_bias_lrelu_backward_noise": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_noise_regularizer_workspace_bytes": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]),
    "gance_noise_regularizer_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_noise_regularizer_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_void_p],
    ),
    "gance_pyramid_distance_workspace_bytes": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]),
    "gance_pyramid_distance_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_pyramid_distance_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_lpips_input_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_lpips_input_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_bias_relu_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p],
    ),
    "gance_bias_relu_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_void_p],
    ),
    "gance_lpips_layer_workspace_bytes": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]),
    "gance_lpips_layer_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p],
    ),
    "gance_lpips_layer_backward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_void_p],
    ),
    "gance_lpips_normalize": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "gance_conv3x3_form": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    "gance_conv3x3_workspace_bytes": (
        ctypes.c_int,
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)],
    ),
    "gance_conv3x3_forward": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
}

# entries added without an ABI bump: an older build of the same ABI (GANCE_HIP_LIBRARY, e.g. the A/B tools'
# libgance_hip_prev.so) may lack them, and only a call of the missing entry fails there
ADDED_WITHIN_ABI = {
    "gance_engine_describe_plan", "gance_jpeg_encode_rect_bounds", "gance_jpeg_encode_rect_u8", "gance_debug_place_panels_u8",
    "gance_debug_draw_panels_u8", "gance_debug_scatter3d_u8", "gance_debug_draw_scatter3d_u8", "gance_jpeg_parse_header",
    "gance_jpeg_decode_bounds", "gance_jpeg_decode_u8", "gance_debug_draw_text_u8", "gance_debug_font_columns",
    "gance_engine_debug_read_skip_image", "gance_png_encode_bounds", "gance_png_encode_u8", "gance_modconv3x3_workspace_bytes",
    "gance_modconv3x3_forward", "gance_modconv3x3_backward", "gance_noise_bias_lrelu_forward", "gance_noise_bias_lrelu_backward",
    "gance_torgb_skip_workspace_bytes", "gance_torgb_skip_forward", "gance_torgb_skip_backward",
    "gance_noise_bias_lrelu_backward_noise", "gance_noise_regularizer_workspace_bytes", "gance_noise_regularizer_forward",
    "gance_noise_regularizer_backward", "gance_pyramid_distance_workspace_bytes", "gance_pyramid_distance_forward",
    "gance_pyramid_distance_backward", "gance_png_encode_lz_bounds", "gance_png_encode_lz_u8", "gance_lpips_input_forward",
    "gance_lpips_input_backward", "gance_bias_relu_forward", "gance_bias_relu_backward", "gance_lpips_layer_workspace_bytes",
    "gance_lpips_layer_forward", "gance_lpips_layer_backward", "gance_lpips_normalize", "gance_conv3x3_form",
    "gance_conv3x3_workspace_bytes", "gance_conv3x3_forward", "gance_jpeg_encode_rect_optimized_bounds",
    "gance_jpeg_encode_rect_optimized_u8", "gance_jpeg_optimal_tables", "gance_engine_debug_mapping", "gance_engine_debug_dlatents",
    "gance_engine_debug_read_style", "gance_engine_debug_read_demod", "gance_jpeg_parse_header_layouts",
    "gance_jpeg_decode_layouts_bounds", "gance_jpeg_decode_layouts_u8", "gance_debug_savgol_table",
    "gance_engine_debug_border_residue", "gance_engine_debug_poison_scratch",
}

_LIB: Optional[ctypes.CDLL] = None


def load_library() -> ctypes.CDLL:
    """
    dlopen the in-tree library and declare every prototype.
    :raises RuntimeError: if the library has not been built. Never falls back to another backend.
    """
    global _LIB  # pylint: disable=global-statement
    if _LIB is not None:
        return _LIB
    if not LIBRARY_PATH.exists():
        raise RuntimeError(
            f"{LIBRARY_PATH} is missing: build the HIP extension first "
            "(`make -C gance_amd/csrc` or `__graft_entry__.build()`). "
            "gance_amd has no CPU fallback."
        )
    lib = ctypes.CDLL(str(LIBRARY_PATH))
    for name, (restype, argtypes) in SIGNATURES.items():
        if name in ADDED_WITHIN_ABI and not hasattr(lib, name):
            continue
        function = getattr(lib, name)  # AttributeError if the .so does not export it
        function.restype = restype
        function.argtypes = argtypes
    _LIB = lib
    return lib


def _check(lib: ctypes.CDLL, status: int) -> None:
    if status != GANCE_OK:
        raise GanceHipError(status, lib.gance_last_error().decode("utf-8", "replace"))


def _f32(array: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(array, dtype=np.float32)


class StepInfo(NamedTuple):
    """One kernel launch of the last synthesize call (GANCE_FLAG_PROFILE_STEPS)."""

    name: str
    ms: float
    flops: float
    bytes: float


class Engine:
    """
    One StyleGAN2 generator resident in HBM. Thin owner of a `gance_engine*`.
    Replaces the TF session + unpickled `Network` the reference keeps per worker process
    (gance/network_interface/network_functions.py:93-111).
    """

    def __init__(
        self,
        variables: Dict[str, np.ndarray],
        resolution: int,
        max_batch: int = 1,
        device: int = 0,
        profile: bool = False,
        conv_form: str = "auto",
        up_form: str = "auto",
        private_workspace: bool = False,
    ) -> None:
        """
        :param private_workspace: give this engine its own activation scratch instead of the one every engine of
        the same (device, resolution, max_batch) shares (only needed to overlap calls of different engines on
        different streams; costs ~0.8 GB per frame of max_batch at 1024^2).
        :param up_form: Conv0_up layers with an input >= 64 wide: "auto" = one fused kernel (transposed conv +
        FIR + noise + bias + leaky ReLU) when the launch fills the chip, else two passes; "split" = always two
        passes; "fused" = the fused kernel whatever the batch.
        :param conv_form: "auto" = every Conv1 from 32x32 up in Winograd F(4x4,3x3) form when its launch has a tile per
        CU, else F(2x2,3x3) when that launch has a block per CU, else the direct form; "direct" = never Winograd;
        "winograd" = the F(2x2,3x3) kernels on every layer that supports them, whatever the batch; "winograd43" = the
        F(4x4,3x3) kernel on every Conv1 from 32x32 up (F(2x2,3x3) on what is left), whatever the batch. With either of
        the two a 32-channel last layer (config-f at 1024^2, config-e at 512^2) runs in that Winograd form with the ToRGB
        channel sum in its epilogue (convW<N>+rgb / convV<N>+rgb, then torgb), as "auto" does once the launch fills the chip.
        """
        self._lib = load_library()
        self._handle = ctypes.c_void_p()
        # (the config is read off the variables: a config-e network, fmap_base = 8 << 10, carries GANCE_FLAG_FMAP_BASE_8K)
        self.fmap_base = sg2_spec.fmap_base_of(variables, resolution)
        spec = sg2_spec.make_spec(resolution, self.fmap_base)
        blob = sg2_spec.pack_variables(variables, spec)
        form_flags = {
            "auto": 0, "direct": GANCE_FLAG_DIRECT_CONV, "winograd": GANCE_FLAG_FORCE_WINOGRAD,
            "winograd43": GANCE_FLAG_FORCE_WINOGRAD | GANCE_FLAG_WINOGRAD43,
        }[conv_form]
        form_flags |= {"auto": 0, "split": GANCE_FLAG_SPLIT_UPFIR, "fused": GANCE_FLAG_FORCE_FUSED_UPFIR}[up_form]
        if private_workspace:
            form_flags |= GANCE_FLAG_PRIVATE_WORKSPACE
        if self.fmap_base == sg2_spec.FMAP_BASE_CONFIG_E:
            form_flags |= GANCE_FLAG_FMAP_BASE_8K
        config = EngineConfig(resolution, max_batch, device, (GANCE_FLAG_PROFILE_STEPS if profile else 0) | form_flags)
        _check(
            self._lib,
            self._lib.gance_engine_create(
                ctypes.byref(config),
                blob.ctypes.data_as(_F32P),
                ctypes.c_uint64(blob.size),
                ctypes.byref(self._handle),
            ),
        )
        self.resolution = resolution
        self.max_batch = max_batch
        self.device = device
        self.noise_randomized = False
        self.vector_length = int(self._lib.gance_engine_vector_length(self._handle))
        self.num_layers = int(self._lib.gance_engine_num_layers(self._handle))

    def close(self) -> None:
        """Free the engine's HBM. Idempotent."""
        if self._handle:
            if getattr(self, "_op_handle", None) is not None:
                from gance_amd import torch_ops  # pylint: disable=import-outside-toplevel

                torch_ops.unregister(self._op_handle)
                self._op_handle = None
            self._lib.gance_engine_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    @property
    def op_handle(self) -> int:
        """Integer handle of this engine for the `torch.ops.gance.*` custom ops (gance_amd/torch_ops.py)."""
        self._require_open()
        if getattr(self, "_op_handle", None) is None:
            from gance_amd import torch_ops  # pylint: disable=import-outside-toplevel

            self._op_handle = torch_ops.register_engine(self)
        return self._op_handle

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass

    def _require_open(self) -> None:
        if not self._handle:
            raise ValueError("Engine has been closed")

    # ---- host-buffer calls (numpy in, numpy out) ----

    def synthesize_w(self, dlatents: np.ndarray, want_float: bool = False):
        """dlatents [B, W, 512] -> uint8 [B, R, R, 3] (and float32 [B, 3, R, R] if want_float)."""
        self._require_open()
        dl = _f32(dlatents)
        if dl.ndim != 3 or dl.shape[1] != self.num_layers or dl.shape[2] != self.vector_length:
            raise ValueError(f"dlatents must be [B, {self.num_layers}, {self.vector_length}], got {dl.shape}")
        batch = dl.shape[0]
        out = np.empty((batch, self.resolution, self.resolution, 3), dtype=np.uint8)
        fout = np.empty((batch, 3, self.resolution, self.resolution), dtype=np.float32) if want_float else None
        _check(
            self._lib,
            self._lib.gance_synthesize_w_host(
                self._handle,
                dl.ctypes.data_as(_F32P),
                batch,
                out.ctypes.data_as(_U8P),
                fout.ctypes.data_as(_F32P) if fout is not None else None,
            ),
        )
        return (out, fout) if want_float else out

    def synthesize_z(self, z: np.ndarray, truncation_psi: float = 1.2, want_float: bool = False):
        """z [B, 512] -> uint8 [B, R, R, 3] (and float32 [B, 3, R, R] if want_float)."""
        self._require_open()
        zz = _f32(z)
        if zz.ndim != 2 or zz.shape[1] != self.vector_length:
            raise ValueError(f"z must be [B, {self.vector_length}], got {zz.shape}")
        batch = zz.shape[0]
        out = np.empty((batch, self.resolution, self.resolution, 3), dtype=np.uint8)
        fout = np.empty((batch, 3, self.resolution, self.resolution), dtype=np.float32) if want_float else None
        _check(
            self._lib,
            self._lib.gance_synthesize_z_host(
                self._handle,
                zz.ctypes.data_as(_F32P),
                batch,
                ctypes.c_float(truncation_psi),
                out.ctypes.data_as(_U8P),
                fout.ctypes.data_as(_F32P) if fout is not None else None,
            ),
        )
        return (out, fout) if want_float else out

    # ---- device-pointer calls (torch tensors or raw pointers; asynchronous on `stream`) ----

    def synthesize_w_device(self, d_dlatents: int, batch: int, d_out_u8: int, d_out_f32: int = 0, stream: int = 0) -> None:
        """Raw device pointers (ints). Asynchronous on `stream`."""
        self._require_open()
        _check(
            self._lib,
            self._lib.gance_synthesize_w(self._handle, d_dlatents, batch, d_out_u8 or None, d_out_f32 or None, stream or None),
        )

    def synthesize_z_device(
        self, d_z: int, batch: int, truncation_psi: float, d_out_u8: int, d_out_f32: int = 0, stream: int = 0
    ) -> None:
        """Raw device pointers (ints). Asynchronous on `stream`."""
        self._require_open()
        _check(
            self._lib,
            self._lib.gance_synthesize_z(
                self._handle, d_z, batch, ctypes.c_float(truncation_psi), d_out_u8 or None, d_out_f32 or None, stream or None
            ),
        )

    # ---- randomize_noise (the reference's vector path draws fresh noise per call) ----

    def randomize_noise(
        self, seed: Optional[int] = None, count: Optional[int] = None, first_sample: int = 0, d_sample_ids: int = 0, stream: int = 0
    ) -> None:
        """
        Draw fresh standard-normal noise planes, one per layer and PER SAMPLE (upstream: tf.random_normal([N, 1, H, W])),
        for `count` samples (default: max_batch), asynchronously on `stream`; the following calls read them until
        `restore_noise`. Sample b reads the plane of id `first_sample + b` (or of the int64 id at `d_sample_ids[b]`, a raw
        device pointer); a plane is a function of (seed, layer, id) only. `seed` None: a new seed from the OS, as
        `tf.random_normal` would give. Layers whose noise strength is zero (all of them at random init) are skipped.
        """
        self._require_open()
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        _check(
            self._lib,
            self._lib.gance_engine_randomize_noise(
                self._handle, ctypes.c_uint64(seed & (2**64 - 1)), int(count or 0), ctypes.c_uint64(int(first_sample)), d_sample_ids or None,
                stream or None,
            ),
        )
        self.noise_randomized = True

    def restore_noise(self, stream: int = 0) -> None:
        """Go back to the stored noise buffers (no-op if they are in use)."""
        self._require_open()
        if getattr(self, "noise_randomized", False):
            _check(self._lib, self._lib.gance_engine_restore_noise(self._handle, stream or None))
            self.noise_randomized = False

    def debug_noise(self, conv_layer: int, sample: int = 0) -> np.ndarray:
        """The noise plane sample `sample` of conv layer `conv_layer` currently reads, [res, res] float32 (synchronises)."""
        self._require_open()
        side = 2 ** sg2_spec.make_spec(self.resolution, self.fmap_base).convs[conv_layer].res_log2
        out = np.empty((side, side), dtype=np.float32)
        _check(
            self._lib,
            self._lib.gance_engine_debug_read_noise(self._handle, conv_layer, sample, out.ctypes.data_as(_F32P), ctypes.c_uint64(out.size)),
        )
        return out

    # ---- profiling / debugging ----

    def set_profiling(self, enabled: bool, only_step: Optional[str] = None) -> None:
        """Per-launch HIP events on / off; `only_step` restricts them to launches whose name contains it."""
        self._require_open()
        _check(
            self._lib,
            self._lib.gance_engine_set_profiling(
                self._handle, GANCE_FLAG_PROFILE_STEPS if enabled else 0, only_step.encode() if only_step else None
            ),
        )

    def steps(self) -> List[StepInfo]:
        """Per-launch timings of the last call (engine created with profile=True)."""
        self._require_open()
        count = int(self._lib.gance_engine_step_count(self._handle))
        result = []
        name = ctypes.create_string_buffer(64)
        ms = ctypes.c_float()
        flops = ctypes.c_double()
        nbytes = ctypes.c_double()
        for index in range(count):
            _check(
                self._lib,
                self._lib.gance_engine_step_info(
                    self._handle, index, name, ctypes.byref(ms), ctypes.byref(flops), ctypes.byref(nbytes)
                ),
            )
            result.append(StepInfo(name.value.decode(), float(ms.value), float(flops.value), float(nbytes.value)))
        return result

    def debug_activation_after(self, dlatents: np.ndarray, num_conv_layers: int) -> np.ndarray:
        """Run only the first `num_conv_layers` conv layers and return x [B, C, res, res]."""
        self._require_open()
        dl = _f32(dlatents)
        batch = dl.shape[0]
        _check(self._lib, self._lib.gance_engine_debug_stop_after(self._handle, num_conv_layers))
        try:
            _check(
                self._lib,
                self._lib.gance_synthesize_w_host(self._handle, dl.ctypes.data_as(_F32P), batch, None, None),
            )
            capacity = batch * 512 * self.resolution * self.resolution
            channels = ctypes.c_int32()
            side = ctypes.c_int32()
            spec = sg2_spec.make_spec(self.resolution, self.fmap_base)
            conv = spec.convs[num_conv_layers - 1]
            count = batch * conv.cout * (2 ** conv.res_log2) ** 2
            out = np.empty(count, dtype=np.float32)
            _check(
                self._lib,
                self._lib.gance_engine_debug_read_activation(
                    self._handle, batch, out.ctypes.data_as(_F32P), ctypes.c_uint64(min(capacity, count)),
                    ctypes.byref(channels), ctypes.byref(side),
                ),
            )
            return out.reshape(batch, channels.value, side.value, side.value)
        finally:
            self._lib.gance_engine_debug_stop_after(self._handle, 0)

    def debug_image_after(self, dlatents: np.ndarray, num_conv_layers: int) -> np.ndarray:
        """
        Run only the first `num_conv_layers` conv layers and return the fp32 skip image [B, 3, res, res] the last ToRGB of that
        call left. Stopped after an up layer this is the image of the resolution before it, whose Conv1 ran as it does in a whole
        call (with the up layer's style on its stores where the plan has that); stopped after a Conv1, the same layer without it.
        """
        self._require_open()
        dl = _f32(dlatents)
        batch = dl.shape[0]
        convs = sg2_spec.make_spec(self.resolution, self.fmap_base).convs
        if not 1 <= num_conv_layers <= len(convs):
            raise ValueError(f"num_conv_layers must be in [1, {len(convs)}], got {num_conv_layers}")
        _check(self._lib, self._lib.gance_engine_debug_stop_after(self._handle, num_conv_layers))
        try:
            _check(
                self._lib,
                self._lib.gance_synthesize_w_host(self._handle, dl.ctypes.data_as(_F32P), batch, None, None),
            )
            last = convs[num_conv_layers - 1]
            res = 2 ** (last.res_log2 - 1 if last.up else last.res_log2)
            side = ctypes.c_int32()
            out = np.empty((batch, 3, res, res), dtype=np.float32)
            _check(
                self._lib,
                self._lib.gance_engine_debug_read_skip_image(
                    self._handle, batch, out.ctypes.data_as(_F32P), ctypes.c_uint64(out.size), ctypes.byref(side)
                ),
            )
            if side.value != res:
                raise RuntimeError(f"the skip image is {side.value} wide, expected {res}")
            return out
        finally:
            self._lib.gance_engine_debug_stop_after(self._handle, 0)

    # ---- the part of a call in front of the first convolution, stage by stage ----

    def _z_of(self, z: np.ndarray) -> np.ndarray:
        zz = _f32(z)
        if zz.ndim != 2 or zz.shape[1] != self.vector_length:
            raise ValueError(f"z must be [B, {self.vector_length}], got {zz.shape}")
        return zz

    def debug_mapping_after(self, z: np.ndarray, num_dense_layers: int) -> np.ndarray:
        """The output [B, 512] of the first `num_dense_layers` (1 ... 8) dense layers of the mapping network for z [B, 512]."""
        self._require_open()
        zz = self._z_of(z)
        out = np.empty((zz.shape[0], self.vector_length), dtype=np.float32)
        _check(
            self._lib,
            self._lib.gance_engine_debug_mapping(
                self._handle, zz.ctypes.data_as(_F32P), zz.shape[0], num_dense_layers, out.ctypes.data_as(_F32P), ctypes.c_uint64(out.size)
            ),
        )
        return out

    def debug_dlatents(self, z: np.ndarray, truncation_psi: float) -> np.ndarray:
        """The dlatents [B, num_layers, 512] a z call hands to synthesis: mapping network, then truncation with `truncation_psi`."""
        self._require_open()
        zz = self._z_of(z)
        out = np.empty((zz.shape[0], self.num_layers, self.vector_length), dtype=np.float32)
        _check(
            self._lib,
            self._lib.gance_engine_debug_dlatents(
                self._handle, zz.ctypes.data_as(_F32P), zz.shape[0], ctypes.c_float(truncation_psi), out.ctypes.data_as(_F32P),
                ctypes.c_uint64(out.size),
            ),
        )
        return out

    def debug_run_front_end(self, dlatents: np.ndarray) -> int:
        """
        A w-call stopped after the first conv layer: styles and demodulation of EVERY layer are computed in front of it and
        stay in the workspace for `debug_read_style` / `debug_read_demod`. Returns the batch.
        """
        self._require_open()
        dl = _f32(dlatents)
        if dl.ndim != 3 or dl.shape[1] != self.num_layers or dl.shape[2] != self.vector_length:
            raise ValueError(f"dlatents must be [B, {self.num_layers}, {self.vector_length}], got {dl.shape}")
        _check(self._lib, self._lib.gance_engine_debug_stop_after(self._handle, 1))
        try:
            _check(self._lib, self._lib.gance_synthesize_w_host(self._handle, dl.ctypes.data_as(_F32P), dl.shape[0], None, None))
        finally:
            self._lib.gance_engine_debug_stop_after(self._handle, 0)
        return dl.shape[0]

    def debug_read_style(self, batch: int, kind: str, index: int) -> np.ndarray:
        """The style [batch, cin] of conv layer `index` (kind "conv") or ToRGB `index` (kind "torgb", 0 = 4x4) of the engine's last call."""
        self._require_open()
        spec = sg2_spec.make_spec(self.resolution, self.fmap_base)
        layers = {"conv": spec.convs, "torgb": spec.torgbs}[kind]
        if not 0 <= index < len(layers):
            raise ValueError(f"{kind} index must be in [0, {len(layers)}), got {index}")
        out = np.empty((batch, layers[index].cin), dtype=np.float32)
        _check(
            self._lib,
            self._lib.gance_engine_debug_read_style(
                self._handle, 0 if kind == "conv" else 1, index, batch, out.ctypes.data_as(_F32P), ctypes.c_uint64(out.size)
            ),
        )
        return out

    def debug_read_demod(self, batch: int, conv_index: int) -> np.ndarray:
        """The demodulation coefficients [batch, cout] of conv layer `conv_index` of the engine's last call."""
        self._require_open()
        convs = sg2_spec.make_spec(self.resolution, self.fmap_base).convs
        if not 0 <= conv_index < len(convs):
            raise ValueError(f"conv_index must be in [0, {len(convs)}), got {conv_index}")
        out = np.empty((batch, convs[conv_index].cout), dtype=np.float32)
        _check(
            self._lib,
            self._lib.gance_engine_debug_read_demod(self._handle, conv_index, batch, out.ctypes.data_as(_F32P), ctypes.c_uint64(out.size)),
        )
        return out

    def debug_style(self, dlatents: np.ndarray, kind: str, index: int) -> np.ndarray:
        """Style [B, cin] of one conv or ToRGB layer for dlatents [B, W, 512] (a stopped w-call, then the read)."""
        return self.debug_read_style(self.debug_run_front_end(dlatents), kind, index)

    def debug_demod(self, dlatents: np.ndarray, conv_index: int) -> np.ndarray:
        """Demodulation coefficients [B, cout] of one conv layer for dlatents [B, W, 512] (a stopped w-call, then the read)."""
        return self.debug_read_demod(self.debug_run_front_end(dlatents), conv_index)

    # ---- what the workspace keeps between calls: its zero borders, and nothing else ----

    def debug_border_residue(self) -> np.ndarray:
        """
        uint64 [conv layers, 6]: border words that are not zero, border words scanned and planes scanned of each layer's
        activation buffer, then the same three of its parity planes (zeros for a stride-1 layer), over the buffers' whole
        capacity. Waits for the workspace's last call, whichever engine made it.
        """
        self._require_open()
        convs = sg2_spec.make_spec(self.resolution, self.fmap_base).convs
        out = np.zeros((len(convs), 6), dtype=np.uint64)
        _check(
            self._lib,
            self._lib.gance_engine_debug_border_residue(self._handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.c_uint64(out.size)),
        )
        return out

    def debug_poison_scratch(self, value: float, include_borders: bool = False) -> None:
        """
        Fill every scratch cell of the workspace that is not a zero border with `value`: a call after it must return what it
        returned before. `include_borders` fills the borders too, which breaks the workspace for good (private workspaces only).
        """
        self._require_open()
        _check(self._lib, self._lib.gance_engine_debug_poison_scratch(self._handle, ctypes.c_float(value), 1 if include_borders else 0))


# stage ids of `enum gance_blend_stage`: name -> (id, dtype, per-frame width or None for [N])
BLEND_STAGES = {
    "db": (0, np.float64, "bins"),
    "scaled": (1, np.float64, "L"),
    "smoothed_time": (2, np.float64, "L"),
    "smoothed": (3, np.float64, "L"),
    "rolled": (4, np.float64, "L"),
    "final": (5, np.float64, "L"),
    "blend_row": (6, np.float64, "L"),
    "raw_rms": (7, np.float32, None),
    "roll_values": (8, np.int32, None),
    "roll_cumulative": (9, np.int32, None),
    "network_indices": (10, np.int32, None),
    "rolling_average": (11, np.float64, None),
    "rolling_smoothed": (12, np.float64, None),
    "index_smoothed": (13, np.float64, None),
}


class Blend:
    """
    Audio -> blended latents on the GPU. Thin owner of a `gance_blend*` (operator tables and
    workspace for one (N, F, depth, alpha, ...) configuration).
    """

    def __init__(
        self,
        num_frames: int,
        num_projection_frames: int,
        alpha: float,
        fft_roll_enabled: bool,
        fft_amplitude_range,
        blend_depth: int,
        num_networks: int,
        vector_length: int = 512,
        latent_depth: int = 18,
        device: int = 0,
        index_savgol: Tuple[int, int] = (3, 2),
    ) -> None:
        """
        :param index_savgol: (window_length, polyorder) of the savgol_filter in front of the
        network-index quantisation: (3, 2) for projection-file-blend, (7, 3) for noise-blend.
        """
        self._lib = load_library()
        self._handle = ctypes.c_void_p()
        has_range = fft_amplitude_range is not None
        lo, hi = (fft_amplitude_range if has_range else (0.0, 0.0))
        self.config = BlendConfig(
            num_frames, vector_length, num_projection_frames, latent_depth, blend_depth,
            int(bool(fft_roll_enabled)), num_networks, int(has_range), float(alpha), float(lo), float(hi),
            int(index_savgol[0]), int(index_savgol[1]),
        )
        status = self._lib.gance_blend_create(ctypes.byref(self.config), device, ctypes.byref(self._handle))
        if status == 1 and (
            b"Cannot duplicate" in self._lib.gance_last_error() or b"num_frames must be >= 7" in self._lib.gance_last_error()
        ):
            # the reference raises ValueError in both cases (vector_sources_common.py:318-331;
            # scipy.signal.savgol_filter: window_length must not exceed the number of frames)
            raise ValueError(self._lib.gance_last_error().decode())
        _check(self._lib, status)
        self.device = device

    def close(self) -> None:
        """Free the tables and workspace. Idempotent."""
        if self._handle:
            self._lib.gance_blend_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass

    def run_device(
        self, d_audio: int, num_samples: int, d_latent_row0: int, d_dlatents: int = 0, d_network_indices: int = 0,
        debug_stages: bool = False, stream: int = 0,
    ) -> None:
        """Raw device pointers (ints). Asynchronous on `stream`."""
        if not self._handle:
            raise ValueError("Blend has been closed")
        _check(
            self._lib,
            self._lib.gance_blend_run(
                self._handle, d_audio, ctypes.c_uint64(num_samples), d_latent_row0, d_dlatents or None,
                d_network_indices or None, int(debug_stages), stream or None,
            ),
        )

    def check_finite(self) -> None:
        """
        The reference fails on audio with a silent 510-sample window: log10(0) = -inf reaches
        sklearn's minmax_scale, which raises ValueError (apply_spectrogram.py:43,81). Same here:
        inspect the global extrema of the last run (one 24-byte read-back).
        :raises ValueError: if the spectrogram holds a non-finite value.
        """
        extrema = np.empty(3, dtype=np.float64)
        _check(self._lib, self._lib.gance_blend_read_stage(self._handle, 14, extrema.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(24)))
        if not np.all(np.isfinite(extrema)) or extrema[0] == 0.0:
            raise ValueError("Input contains infinity or a value too large for dtype('float64').")

    def read_stage(self, name: str) -> np.ndarray:
        """Copy one stage of the last run to the host (synchronises)."""
        stage_id, dtype, width = BLEND_STAGES[name]
        frames = self.config.num_frames
        if width == "L":
            shape = (frames, self.config.vector_length)
        elif width == "bins":
            shape = (frames, (self.config.vector_length - 2) // 2)
        else:
            shape = (frames,)
        out = np.empty(shape, dtype=dtype)
        _check(
            self._lib,
            self._lib.gance_blend_read_stage(self._handle, stage_id, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.nbytes)),
        )
        return out


def resize_bicubic_u8_device(d_in: int, batch: int, src_side: int, d_out: int, dst_side: int, stream: int = 0) -> None:
    """Bicubic (a = -0.75) resize of uint8 NHWC frames in HBM; raw device pointers; asynchronous."""
    lib = load_library()
    _check(lib, lib.gance_resize_bicubic_u8(d_in, batch, src_side, d_out, dst_side, stream or None))


def gaussian_noise_device(  # pylint: disable=too-many-arguments
    d_randn: int,
    num_vectors: int,
    vector_length: int,
    sigma_across: float,
    sigma_within: float,
    feature_range: Optional[Tuple[float, float]],
    d_out: int,
    stream: int = 0,
) -> None:
    """
    Gaussian-filtered ("wrap"), RMS-normalised and optionally min-max scaled noise field from
    float32 standard-normal draws already in HBM (raw device pointers, [N][L]); returns once
    `stream` has drained.
    :raises ValueError: for a feature range sklearn's minmax_scale rejects.
    """
    lib = load_library()
    bounds = None
    if feature_range is not None:
        if not feature_range[0] < feature_range[1]:
            raise ValueError(f"Minimum of desired feature range must be smaller than maximum. Got {feature_range}.")
        bounds = (ctypes.c_double * 2)(float(feature_range[0]), float(feature_range[1]))
    _check(
        lib,
        lib.gance_gaussian_noise(
            d_randn, num_vectors, vector_length, float(sigma_across), float(sigma_within), bounds, d_out, stream or None
        ),
    )


def phash_crops_device(d_frames: int, num_frames: int, side: int, crops: np.ndarray, stream: int = 0) -> np.ndarray:
    """
    Perceptual hashes of crops of uint8 NHWC frames in HBM. `crops` is (n, 5) int32: frame index,
    x, y, width, height. Returns (n,) uint64 (bit 63 = DCT coefficient (0, 0)).
    """
    lib = load_library()
    crops = np.ascontiguousarray(crops, dtype=np.int32).reshape(-1, 5)
    hashes = np.zeros((crops.shape[0],), dtype=np.uint64)
    _check(
        lib,
        lib.gance_phash_crops_u8(
            d_frames, num_frames, side, crops.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), crops.shape[0],
            hashes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), stream or None,
        ),
    )
    return hashes


def overlay_boxes_device(  # pylint: disable=too-many-arguments
    d_foreground: int, d_background: int, d_out: int, num_frames: int, side: int, boxes: np.ndarray, stream: int = 0
) -> None:
    """Foreground regions around `boxes` ((n, 5) int32: frame, x, y, width, height) written over the background."""
    lib = load_library()
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5)
    _check(
        lib,
        lib.gance_overlay_boxes_u8(
            d_foreground, d_background, d_out, num_frames, side, boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            boxes.shape[0], stream or None,
        ),
    )


def jpeg_encode_bounds(batch: int, side: int) -> Tuple[int, int]:
    """(workspace bytes, output capacity) of one `jpeg_encode_device` call of `batch` frames of side `side`.
    :raises ValueError: side not a multiple of 16 in [16, 8192], or batch < 1."""
    lib = load_library()
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_jpeg_encode_bounds(batch, side, ctypes.byref(workspace), ctypes.byref(capacity)))
    return int(workspace.value), int(capacity.value)


def jpeg_encode_device(  # pylint: disable=too-many-arguments
    d_frames: int, batch: int, side: int, quality: int, d_workspace: int, workspace_bytes: int, d_out: int, out_capacity: int,
    d_offsets: int, stream: int = 0,
) -> None:
    """
    Baseline JPEG (4:2:2, standard tables, one restart interval per MCU row) of uint8 frames [batch][side][side][3] in HBM:
    frame b's file lands at d_out[offsets[b]:offsets[b + 1]], offsets int64 [batch + 1] on the device. Asynchronous on `stream`.
    :raises ValueError: bad side, quality outside 1..100, workspace or capacity below `jpeg_encode_bounds`.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_jpeg_encode_u8(
            d_frames, batch, side, quality, d_workspace, workspace_bytes, d_out, out_capacity, d_offsets, stream or None
        ),
    )


def jpeg_encode_rect_bounds(batch: int, width: int, height: int) -> Tuple[int, int]:
    """(workspace bytes, output capacity) of one `jpeg_encode_rect_device` call of `batch` frames [height][width][3].
    :raises ValueError: width or height not a multiple of 16 in [16, 8192], or batch < 1."""
    lib = load_library()
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    _value_error_on_invalid_argument(
        lib, lib.gance_jpeg_encode_rect_bounds(batch, width, height, ctypes.byref(workspace), ctypes.byref(capacity))
    )
    return int(workspace.value), int(capacity.value)


def jpeg_encode_rect_device(  # pylint: disable=too-many-arguments
    d_frames: int, batch: int, width: int, height: int, quality: int, d_workspace: int, workspace_bytes: int, d_out: int,
    out_capacity: int, d_offsets: int, stream: int = 0,
) -> None:
    """
    `jpeg_encode_device` for frames [batch][height][width][3] (DRI = width / 16): the debug video's row of panels.
    :raises ValueError: bad width or height, quality outside 1..100, workspace or capacity below `jpeg_encode_rect_bounds`.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_jpeg_encode_rect_u8(
            d_frames, batch, width, height, quality, d_workspace, workspace_bytes, d_out, out_capacity, d_offsets, stream or None
        ),
    )


JPEG_HUFFMAN_MODES = ("standard", "optimized")


def check_jpeg_huffman(jpeg_huffman: str) -> str:
    """`jpeg_huffman` if it names a table mode of the JPEG encoder. Host only.
    :raises ValueError: anything but "standard" (the Annex K tables) or "optimized" (each frame's own tables)."""
    if jpeg_huffman not in JPEG_HUFFMAN_MODES:
        raise ValueError(f"jpeg_huffman must be one of {JPEG_HUFFMAN_MODES}, got {jpeg_huffman!r}")
    return jpeg_huffman


def jpeg_encode_rect_optimized_bounds(batch: int, width: int, height: int) -> Tuple[int, int]:
    """(workspace bytes, output capacity) of one `jpeg_encode_rect_optimized_device` call: the capacity of
    `jpeg_encode_rect_bounds`, a workspace larger by the frames' symbol counts and tables.
    :raises ValueError: width or height not a multiple of 16 in [16, 8192], or batch < 1."""
    lib = load_library()
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    _value_error_on_invalid_argument(
        lib, lib.gance_jpeg_encode_rect_optimized_bounds(batch, width, height, ctypes.byref(workspace), ctypes.byref(capacity))
    )
    return int(workspace.value), int(capacity.value)


def jpeg_encode_rect_optimized_device(  # pylint: disable=too-many-arguments
    d_frames: int, batch: int, width: int, height: int, quality: int, d_workspace: int, workspace_bytes: int, d_out: int,
    out_capacity: int, d_offsets: int, stream: int = 0,
) -> None:
    """
    `jpeg_encode_rect_device` with each frame's four Huffman tables built from the frame's own symbol counts as libjpeg's
    optimize_coding builds them: the same coefficients and decoded pixels, smaller files, a header length per frame.
    :raises ValueError: bad width or height, quality outside 1..100, workspace or capacity below `jpeg_encode_rect_optimized_bounds`.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_jpeg_encode_rect_optimized_u8(
            d_frames, batch, width, height, quality, d_workspace, workspace_bytes, d_out, out_capacity, d_offsets, stream or None
        ),
    )


def jpeg_optimal_tables_device(d_counts: int, count: int, d_bits: int, d_values: int, d_status: int, stream: int = 0) -> None:  # pylint: disable=too-many-arguments
    """
    The table build of the optimised mode on `count` given count vectors: d_counts [count][256] int32 -> d_bits [count][16] u8,
    d_values [count][256] u8, d_status [count] int32 (0 a table, 1 a code past 32 bits before the limiting, 2 nothing counted).
    :raises ValueError: count < 1.
    """
    lib = load_library()
    _value_error_on_invalid_argument(lib, lib.gance_jpeg_optimal_tables(d_counts, count, d_bits, d_values, d_status, stream or None))


# filtered bytes per independently deflated segment of a PNG (kSegmentBytes of csrc/png.hip): one IDAT chunk each
PNG_SEGMENT_BYTES = 32768


def png_encode_bounds(batch: int, width: int, height: int) -> Tuple[int, int]:
    """(workspace bytes, output capacity) of one `png_encode_device` call of `batch` frames [height][width][3]. The capacity
    is the size of the batch with every segment stored: batch * (63 + 17 * segments + height * (3 * width + 1)).
    :raises ValueError: width or height outside [1, 8192], or batch < 1."""
    lib = load_library()
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_png_encode_bounds(batch, width, height, ctypes.byref(workspace), ctypes.byref(capacity)))
    return int(workspace.value), int(capacity.value)


def png_encode_device(  # pylint: disable=too-many-arguments
    d_frames: int, batch: int, width: int, height: int, d_workspace: int, workspace_bytes: int, d_out: int, out_capacity: int,
    d_offsets: int, stream: int = 0,
) -> None:
    """
    PNG (8-bit RGB, libpng's minimum-sum filter choice per row, Huffman-only deflate in segments of PNG_SEGMENT_BYTES) of
    uint8 frames [batch][height][width][3] in HBM: frame b's file lands at d_out[offsets[b]:offsets[b + 1]], offsets int64
    [batch + 1] on the device. Asynchronous on `stream`.
    :raises ValueError: bad width or height, workspace or capacity below `png_encode_bounds`.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_png_encode_u8(d_frames, batch, width, height, d_workspace, workspace_bytes, d_out, out_capacity, d_offsets, stream or None),
    )


def png_encode_lz_bounds(batch: int, width: int, height: int) -> Tuple[int, int]:
    """(workspace bytes, output capacity) of one `png_encode_lz_device` call. The capacity is `png_encode_bounds`'s (the
    stored form stays the worst case); the workspace is larger by the match search's tokens, 4 * PNG_SEGMENT_BYTES per segment.
    :raises ValueError: width or height outside [1, 8192], or batch < 1."""
    lib = load_library()
    workspace, capacity = ctypes.c_uint64(), ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_png_encode_lz_bounds(batch, width, height, ctypes.byref(workspace), ctypes.byref(capacity)))
    return int(workspace.value), int(capacity.value)


def png_encode_lz_device(  # pylint: disable=too-many-arguments
    d_frames: int, batch: int, width: int, height: int, d_workspace: int, workspace_bytes: int, d_out: int, out_capacity: int,
    d_offsets: int, stream: int = 0,
) -> None:
    """
    `png_encode_device` with an LZ77 match search (csrc/png_lz.hip): the same filter, container and segments; each segment
    takes the smallest of the stored block, the literal-only block and a block with length / distance pairs that never
    reach before the segment, so no file is larger than `png_encode_device`'s. Asynchronous on `stream`.
    :raises ValueError: bad width or height, workspace or capacity below `png_encode_lz_bounds`.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_png_encode_lz_u8(d_frames, batch, width, height, d_workspace, workspace_bytes, d_out, out_capacity, d_offsets, stream or None),
    )


# ---- differentiable synthesis (csrc/synthesis_grad.hip): raw device pointers, asynchronous on `stream` ----


def modconv3x3_workspace_bytes(batch: int, cin: int, cout: int, side: int, up: bool) -> int:
    """Workspace of one `modconv3x3_forward_device` / `modconv3x3_backward_device` call (`side` is the input's).
    :raises ValueError: a shape the kernels refuse (include/gance_hip.h)."""
    lib = load_library()
    size = ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_modconv3x3_workspace_bytes(batch, cin, cout, side, int(up), ctypes.byref(size)))
    return int(size.value)


def modconv3x3_forward_device(  # pylint: disable=too-many-arguments
    d_x: int, d_style: int, d_demod: int, d_weight: int, batch: int, cin: int, cout: int, height: int, width: int, up: bool, d_y: int,
    d_workspace: int, workspace_bytes: int, stream: int = 0,
) -> None:
    """y = demod * conv3x3(style * x, weight), with `up` the transposed conv + FIR to twice the side (gance_modconv3x3_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_modconv3x3_forward(d_x, d_style, d_demod, d_weight, batch, cin, cout, height, width, int(up), d_y, d_workspace, workspace_bytes,
                                     stream or None),
    )


def modconv3x3_backward_device(  # pylint: disable=too-many-arguments
    d_grad_y: int, d_x: int, d_y: int, d_style: int, d_demod: int, d_weight: int, batch: int, cin: int, cout: int, height: int, width: int,
    up: bool, d_grad_x: int, d_grad_style: int, d_grad_demod: int, d_workspace: int, workspace_bytes: int, stream: int = 0,
) -> None:
    """grad_x, grad_style and grad_demod of `modconv3x3_forward_device` (gance_modconv3x3_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_modconv3x3_backward(d_grad_y, d_x, d_y, d_style, d_demod, d_weight, batch, cin, cout, height, width, int(up), d_grad_x,
                                      d_grad_style, d_grad_demod, d_workspace, workspace_bytes, stream or None),
    )


def noise_bias_lrelu_forward_device(  # pylint: disable=too-many-arguments
    d_x: int, d_noise: int, noise_batch: int, d_strength: int, d_bias: int, batch: int, channels: int, height: int, width: int, d_out: int,
    stream: int = 0,
) -> None:
    """out = lrelu_0.2(x + noise * strength + bias) * sqrt(2) (gance_noise_bias_lrelu_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_noise_bias_lrelu_forward(d_x, d_noise, noise_batch, d_strength, d_bias, batch, channels, height, width, d_out, stream or None),
    )


def noise_bias_lrelu_backward_device(  # pylint: disable=too-many-arguments
    d_grad_out: int, d_out: int, batch: int, channels: int, height: int, width: int, d_grad_x: int, stream: int = 0
) -> None:
    """grad_x of `noise_bias_lrelu_forward_device` from the saved output (gance_noise_bias_lrelu_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_noise_bias_lrelu_backward(d_grad_out, d_out, batch, channels, height, width, d_grad_x, None, None, None, stream or None)
    )


def noise_bias_lrelu_backward_noise_device(  # pylint: disable=too-many-arguments
    d_grad_out: int, d_out: int, d_strength: int, noise_batch: int, batch: int, channels: int, height: int, width: int, d_grad_x: int,
    d_grad_noise: int, stream: int = 0,
) -> None:
    """grad_x and grad_noise [noise_batch, 1, S, S] of `noise_bias_lrelu_forward_device` in one pass (gance_noise_bias_lrelu_backward_noise)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_noise_bias_lrelu_backward_noise(d_grad_out, d_out, d_strength, noise_batch, batch, channels, height, width, d_grad_x,
                                                  d_grad_noise, stream or None),
    )



def torgb_skip_workspace_bytes(batch: int, cin: int, side: int) -> int:
    """Workspace of one `torgb_skip_backward_device` call."""
    lib = load_library()
    size = ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_torgb_skip_workspace_bytes(batch, cin, side, ctypes.byref(size)))
    return int(size.value)


def torgb_skip_forward_device(  # pylint: disable=too-many-arguments
    d_x: int, d_style: int, d_weight: int, d_bias: int, d_y_prev: int, batch: int, cin: int, height: int, width: int, d_y: int, stream: int = 0
) -> None:
    """y = upsample_2d(y_prev) + ToRGB(x) + bias; `d_y_prev` 0: no skip image (gance_torgb_skip_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_torgb_skip_forward(d_x, d_style, d_weight, d_bias, d_y_prev or None, batch, cin, height, width, d_y, stream or None)
    )


def torgb_skip_backward_device(  # pylint: disable=too-many-arguments
    d_grad_y: int, d_x: int, d_style: int, d_weight: int, batch: int, cin: int, height: int, width: int, d_grad_x: int, d_grad_style: int,
    d_grad_y_prev: int, d_workspace: int, workspace_bytes: int, stream: int = 0,
) -> None:
    """grad_x, grad_style and (unless `d_grad_y_prev` is 0) grad_y_prev of `torgb_skip_forward_device` (gance_torgb_skip_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_torgb_skip_backward(d_grad_y, d_x, d_style, d_weight, batch, cin, height, width, d_grad_x, d_grad_style, d_grad_y_prev or None,
                                      d_workspace, workspace_bytes, stream or None),
    )


# ---- projection's losses (csrc/projection.hip): raw device pointers, asynchronous on `stream` ----


def noise_regularizer_levels(side: int) -> int:
    """Pyramid levels of the noise regulariser: sides side, side / 2, ... 8 (one level for 4 and 8)."""
    return max(1, int(side).bit_length() - 3)


def noise_regularizer_workspace_bytes(batch: int, side: int) -> int:
    """Workspace shared by `noise_regularizer_forward_device` and `noise_regularizer_backward_device`.
    :raises ValueError: a side that is not a power of two in [4, 1024], a batch outside [1, 65535]."""
    lib = load_library()
    size = ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_noise_regularizer_workspace_bytes(batch, side, ctypes.byref(size)))
    return int(size.value)


def noise_regularizer_forward_device(  # pylint: disable=too-many-arguments
    d_noise: int, batch: int, side: int, d_reg: int, d_means: int, d_workspace: int, workspace_bytes: int, stream: int = 0
) -> None:
    """reg [batch] and means [batch, levels, 2] of planes [batch, 1, side, side] (gance_noise_regularizer_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_noise_regularizer_forward(d_noise, batch, side, d_reg, d_means, d_workspace, workspace_bytes, stream or None)
    )


def noise_regularizer_backward_device(  # pylint: disable=too-many-arguments
    d_grad_reg: int, d_noise: int, d_means: int, d_workspace: int, workspace_bytes: int, batch: int, side: int, d_grad_noise: int, stream: int = 0
) -> None:
    """grad_noise from grad_reg, the forward's means and its workspace (gance_noise_regularizer_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_noise_regularizer_backward(d_grad_reg, d_noise, d_means, d_workspace, workspace_bytes, batch, side, d_grad_noise, stream or None),
    )


def pyramid_distance_workspace_bytes(batch: int, resolution: int) -> int:
    """Workspace shared by `pyramid_distance_forward_device` and `pyramid_distance_backward_device`.
    :raises ValueError: a resolution that is not a power of two in [8, 1024], a batch outside [1, 65535]."""
    lib = load_library()
    size = ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_pyramid_distance_workspace_bytes(batch, resolution, ctypes.byref(size)))
    return int(size.value)


def pyramid_distance_forward_device(  # pylint: disable=too-many-arguments
    d_image: int, d_target: int, batch: int, resolution: int, d_dist: int, d_workspace: int, workspace_bytes: int, stream: int = 0
) -> None:
    """dist [batch] of image [batch, 3, R, R] in -1 ... 1 against target [batch, 3, min(R, 256), ...] in 0 ... 255 (gance_pyramid_distance_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_pyramid_distance_forward(d_image, d_target, batch, resolution, d_dist, d_workspace, workspace_bytes, stream or None)
    )


def pyramid_distance_backward_device(  # pylint: disable=too-many-arguments
    d_grad_dist: int, d_workspace: int, workspace_bytes: int, batch: int, resolution: int, d_grad_image: int, stream: int = 0
) -> None:
    """grad_image from grad_dist and the forward's workspace (gance_pyramid_distance_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_pyramid_distance_backward(d_grad_dist, d_workspace, workspace_bytes, batch, resolution, d_grad_image, stream or None)
    )


# ---- LPIPS on VGG16 (csrc/lpips.hip): raw device pointers, asynchronous on `stream` ----


def lpips_input_forward_device(  # pylint: disable=too-many-arguments
    d_image: int, d_shift: int, d_scale: int, batch: int, resolution: int, side: int, d_out: int, stream: int = 0
) -> None:
    """image [batch, 3, R, R] -> [batch, 16, side, side]: area mean, (x - shift) / scale, zero channels 3 ... 15 (gance_lpips_input_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(lib, lib.gance_lpips_input_forward(d_image, d_shift, d_scale, batch, resolution, side, d_out, stream or None))


def lpips_input_backward_device(d_grad: int, d_scale: int, batch: int, resolution: int, side: int, d_grad_image: int, stream: int = 0) -> None:
    """grad_image [batch, 3, R, R] from grad [batch, 16, side, side] (gance_lpips_input_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(lib, lib.gance_lpips_input_backward(d_grad, d_scale, batch, resolution, side, d_grad_image, stream or None))


def bias_relu_forward_device(  # pylint: disable=too-many-arguments
    d_x: int, d_bias: int, batch: int, channels: int, side: int, pool: bool, d_y: int, d_p: int, stream: int = 0
) -> None:
    """y = max(x + bias, 0) and, with `pool`, p = the 2x2 max pool of y; `d_p` 0 without it (gance_bias_relu_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_bias_relu_forward(d_x, d_bias, batch, channels, side, int(pool), d_y, d_p or None, stream or None)
    )


def bias_relu_backward_device(  # pylint: disable=too-many-arguments
    d_grad_y: int, d_grad_p: int, d_y: int, batch: int, channels: int, side: int, pool: bool, d_grad_x: int, stream: int = 0
) -> None:
    """grad_x of `bias_relu_forward_device` from grad_y, grad_p (0 without `pool`) and the saved y (gance_bias_relu_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_bias_relu_backward(d_grad_y, d_grad_p or None, d_y, batch, channels, side, int(pool), d_grad_x, stream or None)
    )


def lpips_layer_workspace_bytes(batch: int, side: int) -> int:
    """Workspace of one `lpips_layer_forward_device` call.
    :raises ValueError: a side outside [4, 1024], a batch outside [1, 65535]."""
    lib = load_library()
    size = ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_lpips_layer_workspace_bytes(batch, side, ctypes.byref(size)))
    return int(size.value)


def lpips_layer_forward_device(  # pylint: disable=too-many-arguments
    d_f: int, d_target: int, d_lin: int, batch: int, channels: int, side: int, d_dist: int, d_workspace: int, workspace_bytes: int, stream: int = 0
) -> None:
    """dist [batch] of features f against normalised target features, weights lin [channels] (gance_lpips_layer_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_lpips_layer_forward(d_f, d_target, d_lin, batch, channels, side, d_dist, d_workspace, workspace_bytes, stream or None)
    )


def lpips_layer_backward_device(  # pylint: disable=too-many-arguments
    d_grad_dist: int, d_f: int, d_target: int, d_lin: int, batch: int, channels: int, side: int, d_grad_f: int, stream: int = 0
) -> None:
    """grad_f of `lpips_layer_forward_device` from grad_dist [batch] (gance_lpips_layer_backward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_lpips_layer_backward(d_grad_dist, d_f, d_target, d_lin, batch, channels, side, d_grad_f, stream or None)
    )


def lpips_normalize_device(d_f: int, batch: int, channels: int, side: int, d_out: int, stream: int = 0) -> None:
    """out = f / (|f|_2 over the channels + 1e-10) per pixel (gance_lpips_normalize)."""
    lib = load_library()
    _value_error_on_invalid_argument(lib, lib.gance_lpips_normalize(d_f, batch, channels, side, d_out, stream or None))


# ---- the plain 3x3 convolution (csrc/conv3x3.hip): raw device pointers, asynchronous on `stream` ----


def conv3x3_form(cin: int, cout: int, side: int) -> int:
    """The kernel form `conv3x3_forward_device` launches for a shape (include/gance_hip.h); a host-side function of the
    shape alone, never of the batch.
    :raises ValueError: a shape the kernels refuse."""
    lib = load_library()
    form = ctypes.c_int32()
    _value_error_on_invalid_argument(lib, lib.gance_conv3x3_form(cin, cout, side, ctypes.byref(form)))
    return int(form.value)


def conv3x3_workspace_bytes(batch: int, cin: int, cout: int, side: int) -> int:
    """Workspace of one `conv3x3_forward_device` call (never 0).
    :raises ValueError: a shape the kernels refuse (include/gance_hip.h)."""
    lib = load_library()
    size = ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_conv3x3_workspace_bytes(batch, cin, cout, side, ctypes.byref(size)))
    return int(size.value)


def conv3x3_forward_device(  # pylint: disable=too-many-arguments
    d_x: int, d_weight: int, batch: int, cin: int, cout: int, height: int, width: int, d_y: int, d_workspace: int, workspace_bytes: int,
    stream: int = 0,
) -> None:
    """y = conv3x3(x, weight), zero padding 1, stride 1, weight [3, 3, cin, cout] (gance_conv3x3_forward)."""
    lib = load_library()
    _value_error_on_invalid_argument(
        lib, lib.gance_conv3x3_forward(d_x, d_weight, batch, cin, cout, height, width, d_y, d_workspace, workspace_bytes, stream or None)
    )


JPEG_STATUS_REASONS = {0: "ok", 1: "truncated data", 2: "invalid Huffman code", 3: "restart marker mismatch"}


class JpegInfo(ctypes.Structure):
    """`gance_jpeg_info` of include/gance_hip.h: what `jpeg_parse_header` reads from one JFIF file."""

    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
        ("has_huffman_tables", ctypes.c_int32), ("scan_offset", ctypes.c_uint64), ("scan_bytes", ctypes.c_uint64),
        ("quant", ctypes.c_uint8 * 64 * 3), ("huff_bits", ctypes.c_uint8 * 16 * 2 * 3), ("huff_values", ctypes.c_uint8 * 256 * 2 * 3),
    ]


def jpeg_parse_header(data: Union[bytes, bytearray, memoryview, np.ndarray], info: Optional[JpegInfo] = None) -> JpegInfo:
    """
    The description of one JFIF file (host bytes), read on the host: sizes, restart interval, where the entropy-coded data
    lies, and the tables. `info`: an element of a `JpegInfo` array to fill instead of a new one.
    :raises ValueError: a header cut short, a file the decoder does not take (progressive, 4:2:0, 4:4:4, grey, 12-bit
    samples, a 16-bit DQT, more than one scan) or an invalid Huffman table; the message names the reason.
    """
    lib = load_library()
    buffer = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    info = JpegInfo() if info is None else info
    _value_error_on_invalid_argument(lib, lib.gance_jpeg_parse_header(buffer.ctypes.data, buffer.size, ctypes.byref(info)))
    return info


def jpeg_decode_bounds(batch: int, width: int, height: int, total_bytes: int) -> int:
    """Workspace bytes of one `jpeg_decode_device` call of `batch` files of width x height that total `total_bytes`.
    :raises ValueError: batch < 1, or width or height outside [1, 8192]."""
    lib = load_library()
    workspace = ctypes.c_uint64()
    _value_error_on_invalid_argument(lib, lib.gance_jpeg_decode_bounds(batch, width, height, total_bytes, ctypes.byref(workspace)))
    return int(workspace.value)


def jpeg_decode_device(  # pylint: disable=too-many-arguments
    d_data: int, offsets: np.ndarray, infos: "ctypes.Array[JpegInfo]", d_workspace: int, workspace_bytes: int, d_out: int,
    d_status: int, stream: int = 0,
) -> None:
    """
    Baseline 4:2:2 JFIF files in HBM (file b at d_data[offsets[b]:offsets[b + 1]], `offsets` int64 [batch + 1] and `infos`
    [batch] on the host) to uint8 [batch][height][width][3] RGB at d_out, equal to libjpeg's default decode; d_status
    [batch] int32 receives a key of `JPEG_STATUS_REASONS` per frame. Asynchronous on `stream`.
    :raises ValueError: frames of different sizes, descriptions that do not fit the offsets, a workspace below `jpeg_decode_bounds`.
    """
    lib = load_library()
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    batch = len(infos)
    if offsets.shape != (batch + 1,):
        raise ValueError(f"offsets must be [{batch + 1}] for {batch} descriptions, got {offsets.shape}")
    _value_error_on_invalid_argument(
        lib,
        lib.gance_jpeg_decode_u8(
            d_data, offsets.ctypes.data, ctypes.addressof(infos), batch, d_workspace, workspace_bytes, d_out, d_status, stream or None
        ),
    )


JPEG_LAYOUT_NAMES = ("4:2:2", "4:2:0", "4:4:4", "grey")  # by GANCE_JPEG_LAYOUT_*


class JpegFrameInfo(ctypes.Structure):
    """`gance_jpeg_frame_info` of include/gance_hip.h: a `JpegInfo` and the file's layout, an index of `JPEG_LAYOUT_NAMES`."""

    _fields_ = [("info", JpegInfo), ("layout", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def jpeg_parse_header_layouts(
    data: Union[bytes, bytearray, memoryview, np.ndarray], info: Optional[JpegFrameInfo] = None
) -> JpegFrameInfo:
    """
    `jpeg_parse_header` for baseline 4:2:2, 4:2:0, 4:4:4 and grey files: `.info` as there, `.layout` which of the four. For
    grey only component 0's tables are filled.
    :raises ValueError: a header cut short, a file the decoder does not take (progressive, other sampling factors such as
    4:4:0 and 4:1:1, two or four components, 12-bit samples, a 16-bit DQT, more than one scan) or an invalid Huffman table.
    """
    lib = load_library()
    buffer = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    info = JpegFrameInfo() if info is None else info
    _value_error_on_invalid_argument(lib, lib.gance_jpeg_parse_header_layouts(buffer.ctypes.data, buffer.size, ctypes.byref(info)))
    return info


def jpeg_decode_layouts_bounds(batch: int, width: int, height: int, layout: int, total_bytes: int) -> int:
    """Workspace bytes of one `jpeg_decode_layouts_device` call of `batch` files of width x height in `layout`.
    :raises ValueError: batch < 1, width or height outside [1, 8192], or a layout that is none of the four."""
    lib = load_library()
    workspace = ctypes.c_uint64()
    _value_error_on_invalid_argument(
        lib, lib.gance_jpeg_decode_layouts_bounds(batch, width, height, layout, total_bytes, ctypes.byref(workspace))
    )
    return int(workspace.value)


def jpeg_decode_layouts_device(  # pylint: disable=too-many-arguments
    d_data: int, offsets: np.ndarray, infos: "ctypes.Array[JpegFrameInfo]", d_workspace: int, workspace_bytes: int, d_out: int,
    d_status: int, stream: int = 0,
) -> None:
    """
    `jpeg_decode_device` for files of any one of the four layouts: `infos` [batch] as `jpeg_parse_header_layouts` fills them.
    :raises ValueError: frames of different sizes ("one size") or layouts ("one layout"), descriptions that do not fit the
    offsets, a workspace below `jpeg_decode_layouts_bounds`; all before a device is touched.
    """
    lib = load_library()
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    batch = len(infos)
    if offsets.shape != (batch + 1,):
        raise ValueError(f"offsets must be [{batch + 1}] for {batch} descriptions, got {offsets.shape}")
    _value_error_on_invalid_argument(
        lib,
        lib.gance_jpeg_decode_layouts_u8(
            d_data, offsets.ctypes.data, ctypes.addressof(infos), batch, d_workspace, workspace_bytes, d_out, d_status, stream or None
        ),
    )


class DebugAxis(ctypes.Structure):
    """`gance_debug_axis` of include/gance_hip.h: a pixel rectangle of a panel and the data limits mapped onto it."""

    _fields_ = [
        ("x", ctypes.c_int32), ("y", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("x_min", ctypes.c_double), ("x_max", ctypes.c_double), ("y_min", ctypes.c_double), ("y_max", ctypes.c_double),
    ]


class DebugMark(ctypes.Structure):
    """`gance_debug_mark` of include/gance_hip.h."""

    _fields_ = [
        ("kind", ctypes.c_int32), ("axis", ctypes.c_int32), ("dtype", ctypes.c_int32), ("count", ctypes.c_int32),
        ("data", ctypes.c_void_p), ("limit", ctypes.c_int64), ("frame_stride", ctypes.c_int64),
        ("frame_divisor", ctypes.c_int32), ("size", ctypes.c_int32), ("dash_on", ctypes.c_int32), ("dash_off", ctypes.c_int32),
        ("flag_mask", ctypes.c_int32), ("flag_value", ctypes.c_int32), ("rgba", ctypes.c_uint8 * 4), ("reserved", ctypes.c_int32),
        ("x_start", ctypes.c_double),
    ]


DEBUG_MARK_POINTS, DEBUG_MARK_POLYLINE, DEBUG_MARK_CURSOR, DEBUG_MARK_BAR = range(4)
DEBUG_DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2}
DEBUG_MAX_AXES, DEBUG_MAX_MARKS = 8, 24
# `gance_debug_frame`: what changes from frame to frame
DEBUG_FRAME_DTYPE = np.dtype([("number", np.int64), ("cursor", np.float64), ("flags", np.int32), ("reserved", np.int32)])


def debug_place_panels_device(  # pylint: disable=too-many-arguments
    d_src: int, src_count: int, side: int, first_number: int, divisor: int, src_base: int, batch: int, d_out: int,
    out_frame_stride: int, out_row_stride: int, stream: int = 0,
) -> None:
    """
    One image panel of `batch` consecutive debug frames: frame b shows src[(first_number + b) // divisor - src_base]
    ([src_count][side][side][3] uint8 in HBM); the panel's row r of frame b starts at d_out + b * out_frame_stride +
    r * out_row_stride. Asynchronous on `stream`.
    :raises ValueError: bad side, strides or alignment, or frames that would read outside `src_count`.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_debug_place_panels_u8(
            d_src or None, src_count, side, first_number, divisor, src_base, batch, d_out or None, out_frame_stride, out_row_stride,
            stream or None,
        ),
    )


def debug_draw_panels_device(  # pylint: disable=too-many-arguments
    d_chrome: int, side: int, axes, marks, d_frames: int, batch: int, d_out: int, out_frame_stride: int, out_row_stride: int,
    stream: int = 0,
) -> None:
    """
    One plot panel of `batch` debug frames: the chrome template [side][side][3] (HBM) copied to every frame, then `marks`
    (a sequence of DebugMark, or None) composited in order on `axes` (a sequence of DebugAxis, or None) with the per-frame
    records at d_frames (DEBUG_FRAME_DTYPE [batch] in HBM). Asynchronous on `stream`; see include/gance_hip.h.
    :raises ValueError: a missing table, bad sizes or strides, axes that overlap or leave the panel, a bad mark.
    """
    lib = load_library()
    # (None stands for a NULL table with a count of one: the library refuses it, like every other bad argument)
    axes_array = (DebugAxis * len(axes))(*axes) if axes is not None else None
    marks_array = (DebugMark * max(1, len(marks)))(*marks) if marks is not None else None
    _value_error_on_invalid_argument(
        lib,
        lib.gance_debug_draw_panels_u8(
            d_chrome or None, side, axes_array, len(axes) if axes is not None else 1, marks_array,
            len(marks) if marks is not None else 1, d_frames or None, batch, d_out or None, out_frame_stride, out_row_stride,
            stream or None,
        ),
    )


def debug_draw_text_device(  # pylint: disable=too-many-arguments
    d_text: int, text_stride: int, x: int, y: int, max_width: int, scale: int, colour: Tuple[int, int, int], side: int, batch: int,
    d_out: int, out_frame_stride: int, out_row_stride: int, stream: int = 0,
) -> None:
    """
    One line of text per frame on one panel of `batch` debug frames, on top of what is there (draw it after
    `debug_draw_panels_device`): frame b shows the bytes at d_text + b * text_stride (HBM) up to the first NUL or
    `text_stride`, in the 5 x 7 font at `scale`, with its top-left corner at (x, y), in `colour` (r, g, b), clipped to the
    panel and to `max_width` columns. Output addressing as `debug_draw_panels_device`. Asynchronous on `stream`.
    :raises ValueError: a missing pointer, bad side, strides, alignment, text_stride, scale, max_width, position or batch.
    """
    lib = load_library()
    red, green, blue = (int(channel) & 0xFF for channel in colour)
    _value_error_on_invalid_argument(
        lib,
        lib.gance_debug_draw_text_u8(
            d_text or None, text_stride, x, y, max_width, scale, red | (green << 8) | (blue << 16), side, batch, d_out or None,
            out_frame_stride, out_row_stride, stream or None,
        ),
    )


def debug_font_columns() -> bytes:
    """The 475 column bytes of the library's 5 x 7 font, ' ' to '~' (host only, no GPU needed)."""
    lib = load_library()
    table = (ctypes.c_uint8 * 475)()
    _check(lib, lib.gance_debug_font_columns(table, ctypes.c_uint64(475)))
    return bytes(table)


class DebugView3d(ctypes.Structure):
    """`gance_debug_view3d` of include/gance_hip.h: the rectangle, limits, view vectors, sizes and marker of the 3-D view."""

    _fields_ = [
        ("x", ctypes.c_int32), ("y", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("x_min", ctypes.c_double), ("x_max", ctypes.c_double), ("y_min", ctypes.c_double), ("y_max", ctypes.c_double),
        ("z_min", ctypes.c_double), ("z_max", ctypes.c_double), ("c_min", ctypes.c_double), ("c_max", ctypes.c_double),
        ("right", ctypes.c_double * 3), ("up", ctypes.c_double * 3), ("toward", ctypes.c_double * 3),
        ("point_size", ctypes.c_int32), ("marker_size", ctypes.c_int32), ("marker_rgb", ctypes.c_uint8 * 3), ("reserved0", ctypes.c_uint8),
        ("reserved1", ctypes.c_int32), ("marker_x", ctypes.c_double), ("marker_z", ctypes.c_double),
    ]


def debug_scatter3d_device(  # pylint: disable=too-many-arguments
    d_chrome: int, side: int, view: Optional[DebugView3d], d_values: int, dtype: int, num_vectors: int, vector_length: int,
    vector_stride: int, d_lut: int, d_keys: int, d_template: int, stream: int = 0,
) -> None:
    """
    The template of a run's 3-D view: the chrome [side][side][3] (HBM) with the cloud of the values on top ([num_vectors]
    vectors of `vector_length`, `vector_stride` elements apart, DEBUG_DTYPES float32 or float64), coloured through the
    LUT [256][3], into d_template; d_keys is a workspace of side * side int64. Asynchronous on `stream`; see
    include/gance_hip.h.
    :raises ValueError: a missing pointer, a bad side, alignment, rectangle, limits, view vector, size, dtype or count.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_debug_scatter3d_u8(
            d_chrome or None, side, ctypes.byref(view) if view is not None else None, d_values or None, dtype, num_vectors, vector_length,
            vector_stride, d_lut or None, d_keys or None, d_template or None, stream or None,
        ),
    )


def debug_draw_scatter3d_device(  # pylint: disable=too-many-arguments
    d_template: int, side: int, view: Optional[DebugView3d], d_frames: int, batch: int, d_out: int, out_frame_stride: int,
    out_row_stride: int, stream: int = 0,
) -> None:
    """
    The 3-D panel of `batch` debug frames: the template copied to every frame, the marker stamped at y = the cursor of the
    frame's record (DEBUG_FRAME_DTYPE [batch] in HBM). Output addressing as `debug_draw_panels_device`. Asynchronous.
    :raises ValueError: a missing pointer, bad sizes, strides or alignment, or a view the library refuses.
    """
    lib = load_library()
    _value_error_on_invalid_argument(
        lib,
        lib.gance_debug_draw_scatter3d_u8(
            d_template or None, side, ctypes.byref(view) if view is not None else None, d_frames or None, batch, d_out or None,
            out_frame_stride, out_row_stride, stream or None,
        ),
    )


def resample_audio_device(
    d_in: int, num_in: int, sr_orig: float, sr_new: float, d_out: int, num_out: int, stream: int = 0, double_precision: bool = False
) -> None:
    """
    resampy's kaiser_best resampling of a mono float32 (or float64) signal in HBM (raw device pointers);
    num_out = int(num_in * sr_new / sr_orig). Returns once `stream` has drained.
    :raises ValueError: for the arguments resampy rejects (non-positive rates, an output shorter than one sample).
    """
    lib = load_library()
    entry = lib.gance_resample_audio_f64 if double_precision else lib.gance_resample_audio_f32
    _value_error_on_invalid_argument(lib, entry(d_in, num_in, float(sr_orig), float(sr_new), d_out, num_out, stream or None))


def resample_filter_table() -> np.ndarray:
    """The 32 769-entry kaiser_best half window the resampler interpolates (host only, no GPU needed)."""
    lib = load_library()
    table = np.empty(32769, dtype=np.float64)
    _check(lib, lib.gance_debug_resample_filter(table.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_uint64(table.size)))
    return table


# ---- stand-alone stages of the audio -> latent chain (gance_vec_*): numpy in, numpy out ------------
# The arrays involved are a few MB; every call uploads, runs one stage on the GPU and downloads. The
# fused pipeline (`Blend`) is what the hot path uses; these exist so that a caller of the reference's
# stand-alone functions finds each of them (gance_amd/apply_spectrogram.py, gance_amd/vector_sources/*).


def _value_error_on_invalid_argument(lib: ctypes.CDLL, status: int) -> None:
    """The argument checks restate scipy / sklearn ValueErrors; everything else stays a GanceHipError."""
    if status == 1:
        raise ValueError(lib.gance_last_error().decode("utf-8", "replace"))
    _check(lib, status)


def _cuda(device: int) -> "torch.device":
    if not torch.cuda.is_available():
        raise RuntimeError("gance_amd needs an MI355X: there is no CPU fallback for the audio stages")
    return torch.device("cuda", device)


def vec_savgol(data: np.ndarray, axis: int, window_length: int, polyorder: int, device: int = 0) -> np.ndarray:
    """scipy.signal.savgol_filter (mode "interp") along `axis` of a 2-D float64 array, on the GPU."""
    lib = load_library()
    host = np.ascontiguousarray(data, dtype=np.float64)
    d_in = torch.from_numpy(host).to(_cuda(device))
    d_out = torch.empty_like(d_in)
    stream = torch.cuda.current_stream(d_in.device).cuda_stream
    _value_error_on_invalid_argument(
        lib,
        lib.gance_vec_savgol_f64(d_in.data_ptr(), host.shape[0], host.shape[1], axis, int(window_length), int(polyorder), d_out.data_ptr(), stream or None),
    )
    return d_out.cpu().numpy()


def savgol_table(window_length: int, polyorder: int) -> np.ndarray:
    """
    The Savitzky-Golay operator every stage applies, as the host builds it (no device involved): `window_length` interior
    taps, then `window_length // 2` edge rows of `window_length` weights each (row i: the fitted value at position i of
    the first `window_length` samples; the trailing edge uses the same rows mirrored).
    """
    lib = load_library()
    window = int(window_length)
    table = np.empty(max(window + (window // 2) * window, 1), dtype=np.float64)
    _value_error_on_invalid_argument(
        lib, lib.gance_debug_savgol_table(window, int(polyorder), table.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_uint64(table.size))
    )
    return table


def fourier_resample_matrix(in_length: int, out_length: int) -> np.ndarray:
    """The [in_length][out_length] operator of `vec_fourier_resample` (y = x M), as the host builds it (no device involved)."""
    lib = load_library()
    if int(in_length) < 1 or int(out_length) < 1:
        raise ValueError("lengths must be positive")
    matrix = np.empty((int(in_length), int(out_length)), dtype=np.float64)
    _value_error_on_invalid_argument(
        lib, lib.gance_debug_fourier_resample_matrix(int(in_length), int(out_length), matrix.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    )
    return matrix


def vec_fourier_resample(data: np.ndarray, out_length: int, device: int = 0) -> np.ndarray:
    """scipy.signal.resample of every row of a 2-D float64 array to `out_length` points, on the GPU."""
    lib = load_library()
    host = np.ascontiguousarray(data, dtype=np.float64)
    d_in = torch.from_numpy(host).to(_cuda(device))
    d_out = torch.empty((host.shape[0], int(out_length)), dtype=torch.float64, device=d_in.device)
    stream = torch.cuda.current_stream(d_in.device).cuda_stream
    _value_error_on_invalid_argument(
        lib, lib.gance_vec_fourier_resample_f64(d_in.data_ptr(), host.shape[0], host.shape[1], int(out_length), d_out.data_ptr(), stream or None)
    )
    return d_out.cpu().numpy()


def vec_spectrogram(audio: np.ndarray, num_frequency_bins: int, device: int = 0, truncate: bool = True) -> np.ndarray:
    """compute_spectrogram: float32 mono samples -> float64 [(bins - 2) // 2][frames] dB magnitudes ([bins - 2][frames] with `truncate=False`)."""
    lib = load_library()
    host = np.ascontiguousarray(audio, dtype=np.float32)
    window = num_frequency_bins - 2
    if host.shape[0] < window:
        raise ValueError("fewer samples than one window")
    frames = (host.shape[0] - window) // num_frequency_bins + 1
    d_audio = torch.from_numpy(host).to(_cuda(device))
    d_out = torch.empty((window // 2 if truncate else window, frames), dtype=torch.float64, device=d_audio.device)
    stream = torch.cuda.current_stream(d_audio.device).cuda_stream
    _value_error_on_invalid_argument(
        lib,
        lib.gance_vec_spectrogram2_f64(
            d_audio.data_ptr(), ctypes.c_uint64(host.shape[0]), int(num_frequency_bins), 1 if truncate else 0, d_out.data_ptr(), stream or None
        ),
    )
    return d_out.cpu().numpy()


def vec_minmax_scale(data: np.ndarray, feature_range: Tuple[float, float], device: int = 0) -> np.ndarray:
    """sklearn.preprocessing.minmax_scale of a whole array (any shape), on the GPU."""
    lib = load_library()
    host = np.ascontiguousarray(data, dtype=np.float64)
    d_data = torch.from_numpy(host).to(_cuda(device))
    stream = torch.cuda.current_stream(d_data.device).cuda_stream
    _value_error_on_invalid_argument(
        lib, lib.gance_vec_minmax_scale_f64(d_data.data_ptr(), ctypes.c_uint64(host.size), float(feature_range[0]), float(feature_range[1]), stream or None)
    )
    return d_data.cpu().numpy()


def vec_remap(data: np.ndarray, input_range: Tuple[float, float], output_range: Tuple[float, float], device: int = 0) -> np.ndarray:
    """scipy.interpolate.interp1d(input_range, output_range) applied to every value, on the GPU."""
    lib = load_library()
    host = np.ascontiguousarray(data, dtype=np.float64)
    d_in = torch.from_numpy(host).to(_cuda(device))
    d_out = torch.empty_like(d_in)
    stream = torch.cuda.current_stream(d_in.device).cuda_stream
    _value_error_on_invalid_argument(
        lib,
        lib.gance_vec_remap_f64(
            d_in.data_ptr(), ctypes.c_uint64(host.size), float(input_range[0]), float(input_range[1]), float(output_range[0]),
            float(output_range[1]), d_out.data_ptr(), stream or None,
        ),
    )
    return d_out.cpu().numpy()


def vec_rms_rolling_average(
    audio: np.ndarray, vector_length: int, rolling_window: int, savgol_window_length: int, savgol_polyorder: int, device: int = 0
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(raw RMS float32, rolling mean float64, Savitzky-Golay smoothed float64), one value per hop of 512 samples."""
    lib = load_library()
    host = np.ascontiguousarray(audio, dtype=np.float32)
    if host.shape[0] < vector_length:
        raise ValueError("fewer samples than one frame")
    count = 1 + (host.shape[0] - vector_length) // 512
    d_audio = torch.from_numpy(host).to(_cuda(device))
    d_rms = torch.empty((count,), dtype=torch.float32, device=d_audio.device)
    d_rolling = torch.empty((count,), dtype=torch.float64, device=d_audio.device)
    d_smoothed = torch.empty((count,), dtype=torch.float64, device=d_audio.device)
    stream = torch.cuda.current_stream(d_audio.device).cuda_stream
    _value_error_on_invalid_argument(
        lib,
        lib.gance_vec_rms_rolling_average(
            d_audio.data_ptr(), ctypes.c_uint64(host.shape[0]), int(vector_length), int(rolling_window), int(savgol_window_length),
            int(savgol_polyorder), d_rms.data_ptr(), d_rolling.data_ptr(), d_smoothed.data_ptr(), count, stream or None,
        ),
    )
    return d_rms.cpu().numpy(), d_rolling.cpu().numpy(), d_smoothed.cpu().numpy()


def vec_rms_rolling_max(audio: np.ndarray, vector_length: int, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(raw RMS float32, its rolling maximum over len // 80 values), one value per hop of 512 samples."""
    lib = load_library()
    host = np.ascontiguousarray(audio, dtype=np.float32)
    if host.shape[0] < vector_length:
        raise ValueError("fewer samples than one frame")
    count = 1 + (host.shape[0] - vector_length) // 512
    d_audio = torch.from_numpy(host).to(_cuda(device))
    d_rms = torch.empty((count,), dtype=torch.float32, device=d_audio.device)
    d_out = torch.empty((count,), dtype=torch.float32, device=d_audio.device)
    stream = torch.cuda.current_stream(d_audio.device).cuda_stream
    _value_error_on_invalid_argument(
        lib,
        lib.gance_vec_rms_rolling_max(
            d_audio.data_ptr(), ctypes.c_uint64(host.shape[0]), int(vector_length), d_rms.data_ptr(), d_out.data_ptr(), count, stream or None
        ),
    )
    return d_rms.cpu().numpy(), d_out.cpu().numpy()


def vec_quantize(data: np.ndarray, num_indices: int, device: int = 0) -> np.ndarray:
    """Remap [min, max] of a series onto [0, num_indices - 1] and round half to even -> int64."""
    lib = load_library()
    host = np.ascontiguousarray(data, dtype=np.float64)
    d_in = torch.from_numpy(host).to(_cuda(device))
    d_out = torch.empty((host.size,), dtype=torch.int64, device=d_in.device)
    stream = torch.cuda.current_stream(d_in.device).cuda_stream
    _value_error_on_invalid_argument(lib, lib.gance_vec_quantize_f64(d_in.data_ptr(), host.size, int(num_indices), d_out.data_ptr(), stream or None))
    return d_out.cpu().numpy()
