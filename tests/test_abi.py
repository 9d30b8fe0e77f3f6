"""
CPU tests of the drop-in boundary: libgance_hip.so builds, loads, exports every symbol that
include/gance_hip.h declares, and refuses to run without a GPU (no silent CPU fallback).
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec

REPO_ROOT = Path(__file__).resolve().parent.parent
HEADER = REPO_ROOT / "include" / "gance_hip.h"


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    """The in-tree shared library, built on demand (hipcc cross-compiles without a GPU)."""
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


def declared_functions() -> list:
    """Names of every function prototype in the public header."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gance_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_boundary() -> None:
    names = declared_functions()
    for required in ("gance_engine_create", "gance_engine_destroy", "gance_synthesize_w", "gance_synthesize_z"):
        assert required in names


def test_library_exports_every_declared_symbol(library: ctypes.CDLL) -> None:
    for name in declared_functions():
        assert hasattr(library, name), f"{name} declared in gance_hip.h but not exported"
        assert name in hip_lib.SIGNATURES, f"{name} has no ctypes prototype in hip_lib.SIGNATURES"
    assert library.gance_abi_version() == 6


def test_blob_size_agrees_between_python_and_c(library: ctypes.CDLL) -> None:
    for resolution in (8, 32, 256, 1024):
        spec = sg2_spec.make_spec(resolution)
        assert library.gance_weight_blob_floats(resolution) == sg2_spec.blob_size(spec)
    assert library.gance_weight_blob_floats(1000) == 0
    assert library.gance_weight_blob_floats(2048) == 0


def test_bad_arguments_are_rejected_before_touching_a_device(library: ctypes.CDLL) -> None:
    handle = ctypes.c_void_p()
    config = hip_lib.EngineConfig(32, 1, 0, 0)
    blob = np.zeros(10, dtype=np.float32)
    status = library.gance_engine_create(
        ctypes.byref(config), blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 10, ctypes.byref(handle)
    )
    assert status == 2  # GANCE_ERR_BAD_WEIGHTS
    assert b"expected" in library.gance_last_error()
    config = hip_lib.EngineConfig(33, 1, 0, 0)
    status = library.gance_engine_create(
        ctypes.byref(config), blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 10, ctypes.byref(handle)
    )
    assert status == 1  # GANCE_ERR_INVALID_ARGUMENT
    library.gance_engine_destroy(None)  # NULL is a no-op


FRONT_END_TAPS = ("gance_engine_debug_mapping", "gance_engine_debug_dlatents", "gance_engine_debug_read_style", "gance_engine_debug_read_demod")


def test_the_front_end_taps_came_within_abi_6_and_refuse_a_null_engine(library: ctypes.CDLL) -> None:
    names = declared_functions()
    for name in FRONT_END_TAPS:
        assert name in names and name in hip_lib.ADDED_WITHIN_ABI and hasattr(library, name), name
    assert hip_lib.ADDED_WITHIN_ABI <= set(hip_lib.SIGNATURES)
    out = np.full(8, 7.0, dtype=np.float32)
    z = np.zeros(512, dtype=np.float32)
    pointer, z_pointer = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), z.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    # GANCE_ERR_INVALID_ARGUMENT before a device is touched, and nothing written
    assert library.gance_engine_debug_mapping(None, z_pointer, 1, 8, pointer, ctypes.c_uint64(8)) == 1
    assert library.gance_engine_debug_dlatents(None, z_pointer, 1, ctypes.c_float(0.7), pointer, ctypes.c_uint64(8)) == 1
    assert library.gance_engine_debug_read_style(None, 0, 0, 1, pointer, ctypes.c_uint64(8)) == 1
    assert library.gance_engine_debug_read_demod(None, 0, 1, pointer, ctypes.c_uint64(8)) == 1
    assert b"NULL" in library.gance_last_error() and np.all(out == 7.0)


WORKSPACE_TAPS = ("gance_engine_debug_border_residue", "gance_engine_debug_poison_scratch")


def test_the_workspace_taps_came_within_abi_6_and_refuse_a_null_engine(library: ctypes.CDLL) -> None:
    names = declared_functions()
    for name in WORKSPACE_TAPS:
        assert name in names and name in hip_lib.ADDED_WITHIN_ABI and hasattr(library, name), name
    assert hip_lib.ADDED_WITHIN_ABI <= set(hip_lib.SIGNATURES) and library.gance_abi_version() == 6
    out = np.full(6, 7, dtype=np.uint64)
    pointer = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    # GANCE_ERR_INVALID_ARGUMENT before a device is touched, and nothing written
    assert library.gance_engine_debug_border_residue(None, pointer, ctypes.c_uint64(6)) == 1
    assert b"NULL" in library.gance_last_error() and np.all(out == 7)
    for include_borders in (0, 1):
        assert library.gance_engine_debug_poison_scratch(None, ctypes.c_float(2.0 ** 20), include_borders) == 1
        assert b"NULL" in library.gance_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_gpu_means_loud_failure_not_cpu_fallback(library: ctypes.CDLL) -> None:
    variables = sg2_spec.make_random_variables(8, seed=0)
    with pytest.raises(hip_lib.GanceHipError) as error:
        hip_lib.Engine(variables, 8)
    assert error.value.status == 5  # GANCE_ERR_NO_DEVICE
