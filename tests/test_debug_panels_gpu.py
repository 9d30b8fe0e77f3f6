"""
GPU tests of the debug-video rasteriser and panel placement (gance_amd/csrc/debug_panels.hip) against the numpy
restatement of the rule in tests/debug_video_ref.py: bit-exact, for every mark kind and series dtype, at sides 64 and 96,
in one call and frame by frame.
"""

import ctypes
from typing import Dict, List, Tuple

import numpy as np
import pytest
import torch

import debug_video_ref as ref
from gance_amd import hip_lib

pytestmark = pytest.mark.gpu

DTYPES = {"float32": np.float32, "float64": np.float64, "int32": np.int32}
BATCH = 5


def case(side: int, dtype_name: str) -> Tuple[np.ndarray, List[dict], List[dict], List[dict]]:
    """
    A chrome, three axes, marks of every kind on series of `dtype_name`, and BATCH frames. Limits are irrational-looking
    on purpose: no mapped coordinate may sit on a rounding boundary (asserted by the test). The polylines hold three
    samples per pixel column and swing over the axis height, so their stamps overlap themselves many times; "wide" has
    a NaN in it for the float types.
    """
    dtype = DTYPES[dtype_name]
    rs = np.random.RandomState(side + len(dtype_name))
    chrome = rs.randint(0, 256, (side, side, 3)).astype(np.uint8)
    third = side // 3
    axes = [
        dict(x=3, y=2, width=side - 7, height=third - 4, x_limits=(-0.313, 40.217), y_limits=(-9.137, 9.291)),
        dict(x=1, y=third + 1, width=side - 2, height=third - 3, x_limits=(-0.731, 3 * side - 0.377), y_limits=(-11.213, 10.871)),
        dict(x=5, y=2 * third + 2, width=side - 11, height=side - 2 * third - 5, x_limits=(-0.419, 6.283), y_limits=(0.0, 1.0)),
    ]
    integer = dtype is np.int32

    def values(shape, scale):
        drawn = rs.uniform(-scale, scale, shape)
        return np.round(drawn).astype(dtype) if integer else drawn.astype(dtype)

    per_frame = values((BATCH + 3, 40), 8.5)          # a row per frame: stride 40
    per_pair = values((BATCH // 2 + 3, 40), 8.5)      # a row per two frames: divisor 2
    wide = values((3 * side,), 10.0)                  # shared by every frame: stride 0
    if not integer:
        wide[17] = np.nan
    zigzag = values((3 * side,), 10.0)
    bar = (rs.randint(0, 7, (BATCH + 8,))).astype(dtype)
    marks = [
        dict(kind=ref.POINTS, axis=0, data=per_frame, count=40, frame_stride=40, size=1, rgba=(255, 0, 0, 255)),
        dict(kind=ref.POINTS, axis=0, data=per_pair, count=40, frame_stride=40, frame_divisor=2, size=3, rgba=(0, 127, 0, 200)),
        dict(kind=ref.POLYLINE, axis=0, data=per_frame, count=40, frame_stride=40, size=2, rgba=(0, 0, 255, 128)),
        dict(kind=ref.CURSOR, axis=0, size=2, rgba=(0, 127, 0, 255), flag_mask=1, flag_value=1),
        dict(kind=ref.CURSOR, axis=0, size=1, rgba=(255, 0, 0, 255), flag_mask=1, flag_value=0),
        dict(kind=ref.POLYLINE, axis=1, data=wide, count=3 * side, size=3, rgba=(255, 0, 0, 128)),
        dict(kind=ref.POLYLINE, axis=1, data=zigzag, count=3 * side, size=2, rgba=(0, 191, 191, 128), dash=(4, 3)),
        dict(kind=ref.POLYLINE, axis=1, data=zigzag[5:], count=3 * side - 5, size=1, rgba=(0, 0, 0, 77), x_start=2.0),
        dict(kind=ref.CURSOR, axis=1, size=3, rgba=(255, 0, 0, 128)),
        dict(kind=ref.BAR, axis=2, data=bar, count=1, frame_stride=1, rgba=(191, 0, 191, 255)),
        dict(kind=ref.POINTS, axis=2, data=bar, count=4, frame_stride=1, size=5, rgba=(0, 0, 0, 64), x_start=1.0),
    ]
    frames = [dict(number=3 + b, cursor=7.3 + 5.9 * b, flags=b % 2) for b in range(BATCH)]
    return chrome, axes, marks, frames


def draw_gpu(chrome: np.ndarray, axes: List[dict], marks: List[dict], frames: List[dict], panels: int = 3, panel: int = 1) -> np.ndarray:
    """The frames' panel `panel` of a row of `panels` panels through gance_debug_draw_panels_u8."""
    side = chrome.shape[0]
    keep: Dict[int, torch.Tensor] = {}
    bound = []
    for mark in marks:
        entry = hip_lib.DebugMark()
        entry.kind, entry.axis, entry.size = mark["kind"], mark["axis"], mark.get("size", 1)
        entry.count, entry.frame_stride, entry.frame_divisor = mark.get("count", 0), mark.get("frame_stride", 0), mark.get("frame_divisor", 1)
        entry.dash_on, entry.dash_off = mark.get("dash", (0, 0))
        entry.flag_mask, entry.flag_value = mark.get("flag_mask", 0), mark.get("flag_value", 0)
        entry.rgba = (ctypes.c_uint8 * 4)(*mark["rgba"])
        entry.x_start = mark.get("x_start", 0.0)
        if "data" in mark:
            data = np.ascontiguousarray(mark["data"]).reshape(-1)
            tensor = keep.setdefault(id(mark["data"]), torch.from_numpy(data.copy()).cuda())
            entry.dtype, entry.data, entry.limit = hip_lib.DEBUG_DTYPES[data.dtype], tensor.data_ptr(), data.size
        bound.append(entry)
    bound_axes = [hip_lib.DebugAxis(a["x"], a["y"], a["width"], a["height"], *a["x_limits"], *a["y_limits"]) for a in axes]
    records = np.zeros(len(frames), dtype=hip_lib.DEBUG_FRAME_DTYPE)
    for index, frame in enumerate(frames):
        records[index] = (frame["number"], frame["cursor"], frame["flags"], 0)
    d_records = torch.from_numpy(records.view(np.uint8)).cuda()
    d_chrome = torch.from_numpy(chrome).cuda()
    out = torch.full((len(frames), side, panels * side, 3), 7, dtype=torch.uint8, device="cuda")
    hip_lib.debug_draw_panels_device(
        d_chrome.data_ptr(), side, bound_axes, bound, d_records.data_ptr(), len(frames), out.data_ptr() + panel * side * 3,
        out.stride(0), out.stride(1), torch.cuda.current_stream().cuda_stream,
    )
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    untouched = np.delete(host, np.s_[panel * side : (panel + 1) * side], axis=2)
    assert (untouched == 7).all(), "the rasteriser wrote outside its panel"
    return host[:, :, panel * side : (panel + 1) * side]


@pytest.mark.parametrize("dtype_name", sorted(DTYPES))
@pytest.mark.parametrize("side", [64, 96])
def test_marks_are_bit_exact_against_the_restated_rule(side: int, dtype_name: str) -> None:
    chrome, axes, marks, frames = case(side, dtype_name)
    margin = ref.smallest_margin(axes, marks, frames)
    print(f"side {side} {dtype_name}: smallest distance to a rounding boundary {margin:.3e} px")
    assert margin > 1e-6, "the test data sits on a rounding boundary: choose other limits"
    want = ref.draw(chrome, axes, marks, frames)
    assert (want != chrome[None]).any(axis=-1).mean() > 0.05  # (the marks cover a good part of the panel)
    got = draw_gpu(chrome, axes, marks, frames)
    wrong = int((got != want).any(axis=-1).sum())
    print(f"side {side} {dtype_name}: {wrong} pixels differ")
    assert np.array_equal(got, want)
    # the same frames one call each, and again: a pure function of the inputs
    singly = np.concatenate([draw_gpu(chrome, axes, marks, [frame]) for frame in frames])
    assert np.array_equal(singly, got)
    assert np.array_equal(draw_gpu(chrome, axes, marks, frames), got)


def test_self_overlap_of_an_alpha_polyline_blends_once() -> None:
    """A half-transparent polyline three samples per column over white: every covered pixel holds exactly one blend."""
    side = 64
    chrome = np.full((side, side, 3), 255, dtype=np.uint8)
    axes = [dict(x=0, y=0, width=side, height=side, x_limits=(-0.731, 3 * side - 0.377), y_limits=(-11.213, 10.871))]
    data = np.random.RandomState(3).uniform(-10, 10, 3 * side)
    marks = [dict(kind=ref.POLYLINE, axis=0, data=data, count=3 * side, size=3, rgba=(0, 0, 0, 128))]
    got = draw_gpu(chrome, axes, marks, [dict(number=0, cursor=0.0, flags=0)])
    once = (0 * 128 + 255 * 127 + 127) // 255
    assert set(np.unique(got)) == {once, 255}


def test_place_panels_repeats_sources_like_frame_multiplier() -> None:
    side, sources, batch = 32, 4, 7
    images = np.random.RandomState(1).randint(0, 256, (sources, side, side, 3)).astype(np.uint8)
    d_images = torch.from_numpy(images).cuda()
    out = torch.zeros((batch, side, 2 * side, 3), dtype=torch.uint8, device="cuda")
    # frames 5 .. 11 of a stream that shows every source 3 times; the sources on hand start at source 1
    hip_lib.debug_place_panels_device(
        d_images.data_ptr(), sources, side, 5, 3, 1, batch, out.data_ptr() + side * 3, out.stride(0), out.stride(1),
        torch.cuda.current_stream().cuda_stream,
    )
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, :, :side] == 0).all()
    for b in range(batch):
        assert np.array_equal(host[b, :, side:], images[(5 + b) // 3 - 1])
    with pytest.raises(ValueError):  # frame 14 would read source 4 of 4
        hip_lib.debug_place_panels_device(
            d_images.data_ptr(), sources, side, 5, 3, 0, 10, out.data_ptr(), out.stride(0), out.stride(1), 0
        )
