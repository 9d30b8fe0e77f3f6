"""
GPU tests of the 3-D view's rasteriser (gance_amd/csrc/scatter3d.hip) against the numpy restatement of the rule in
tests/scatter3d_ref.py: the template bit-exact for sparse, dense and overlapping clouds in float32 and float64, with a
strided layout, at equal depth, twice over; and the per-frame panels with their marker, in one call and in two.
"""

import ctypes
from typing import Dict, Tuple

import numpy as np
import pytest
import torch

import scatter3d_ref as ref
from gance_amd import hip_lib
from gance_amd.debug_video import scatter3d

pytestmark = pytest.mark.gpu

# (N, L), side, rectangle, point size: sparse with odd lengths; dense; stamps that overlap and clip at the rectangle
CASES = {
    "sparse": ((7, 33), 64, (8, 12, 48, 44), 1),
    "dense": ((300, 64), 32, (2, 4, 28, 26), 1),
    "stamps": ((40, 48), 128, (16, 16, 96, 100), 2),
}
REFERENCE_VIEW = scatter3d.view_vectors(50, 300)
TOP_VIEW = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
LUT = scatter3d.GREENS


def case_values() -> Dict[str, np.ndarray]:
    """The draws of every case from one RandomState(7), in the order of CASES, with a NaN and an infinity in each."""
    rs = np.random.RandomState(7)
    out = {}
    for name, ((count, length), _side, _rectangle, _size) in CASES.items():
        values = rs.standard_normal((count, length))
        values[count // 2, 3] = np.nan
        values[0, 0] = np.inf
        out[name] = values
    return out


def case_chrome(side: int) -> np.ndarray:
    return np.random.RandomState(side).randint(0, 256, (side, side, 3)).astype(np.uint8)


def view_of(values: np.ndarray, rectangle, vectors=REFERENCE_VIEW, point_size: int = 1, marker_size: int = 2, **limits) -> dict:
    """The view of a run's vectors: the limits of DESIGN.md section 9 item 8 unless given."""
    found = ref.limits_of(values)
    found.update(limits)
    return ref.make_view(
        rectangle, found["x"], found["y"], found["z"], found["colour"], *vectors, point_size=point_size, marker_size=marker_size,
        marker_x=found["x"][1], marker_z=0.0,
    )


def bind(view: dict) -> hip_lib.DebugView3d:
    record = hip_lib.DebugView3d()
    record.x, record.y, record.width, record.height = view["rectangle"]
    (record.x_min, record.x_max), (record.y_min, record.y_max) = view["x_limits"], view["y_limits"]
    (record.z_min, record.z_max), (record.c_min, record.c_max) = view["z_limits"], view["colour_limits"]
    for name in ("right", "up", "toward"):
        setattr(record, name, (ctypes.c_double * 3)(*view[name]))
    record.point_size, record.marker_size = view["point_size"], view["marker_size"]
    record.marker_rgb = (ctypes.c_uint8 * 3)(*view["marker_rgb"])
    record.marker_x, record.marker_z = view["marker_x"], view["marker_z"]
    return record


def template_gpu(chrome: np.ndarray, view: dict, values: np.ndarray, lut: np.ndarray = LUT, rows: int = 1) -> torch.Tensor:
    """
    The template [side, side, 3] in HBM through gance_debug_scatter3d_u8. `values` [N, L] of float32 or float64; with
    `rows` > 1 they are laid out as row 0 of [N][rows][L] (the other rows hold a value that would show) and read with
    vector_stride = rows * L. The workspace comes dirty: the entry zeroes it itself.
    """
    side = chrome.shape[0]
    count, length = values.shape
    laid_out = values
    if rows > 1:
        laid_out = np.full((count, rows, length), 1e3, dtype=values.dtype)
        laid_out[:, 0, :] = values
    d_values = torch.from_numpy(np.ascontiguousarray(laid_out)).cuda()
    d_chrome, d_lut = torch.from_numpy(chrome).cuda(), torch.from_numpy(np.ascontiguousarray(lut)).cuda()
    d_keys = torch.full((side * side,), -1, dtype=torch.int64, device="cuda")
    d_template = torch.full((side, side, 3), 9, dtype=torch.uint8, device="cuda")
    hip_lib.debug_scatter3d_device(
        d_chrome.data_ptr(), side, bind(view), d_values.data_ptr(), hip_lib.DEBUG_DTYPES[values.dtype], count, length, rows * length,
        d_lut.data_ptr(), d_keys.data_ptr(), d_template.data_ptr(), torch.cuda.current_stream().cuda_stream,
    )
    torch.cuda.synchronize()
    return d_template


@pytest.fixture(scope="module")
def wanted() -> Dict[Tuple[str, str], Tuple[dict, np.ndarray, ref.Template]]:
    """(case, dtype) -> (view, values in that dtype, the restatement's template): computed once, never changed."""
    out = {}
    for name, values in case_values().items():
        _shape, side, rectangle, size = CASES[name]
        for dtype in ("float32", "float64"):
            typed = values.astype(dtype)
            view = view_of(typed.astype(np.float64), rectangle, point_size=size)
            out[name, dtype] = (view, typed, ref.template(case_chrome(side), view, typed.astype(np.float64), LUT))
    return out


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_template_is_bit_exact_against_the_restated_rule(wanted, name: str, dtype: str) -> None:
    view, values, want = wanted[name, dtype]
    side = CASES[name][1]
    print(
        f"{name} {dtype}: smallest distance to a rounding boundary {want.smallest_margin:.3e}; {want.contested} of {want.reached} "
        f"reached pixels contested, up to {want.most_on_a_pixel} points on one"
    )
    assert want.smallest_margin > 1e-6, "the test data sits on a rounding boundary: choose another seed"
    assert want.reached > 0 and want.contested > 0
    if name == "dense":
        assert 2 * want.contested >= want.reached and want.most_on_a_pixel >= 50
    if dtype == "float64":  # the figures of the cases as they were chosen
        assert (want.reached, want.contested) == {"sparse": (211, 17), "dense": (372, 343), "stamps": (3339, 2150)}[name]
    got = template_gpu(case_chrome(side), view, values).cpu().numpy()
    wrong = int((got != want.image).any(axis=-1).sum())
    print(f"{name} {dtype}: {wrong} pixels differ")
    assert np.array_equal(got, want.image)
    x, y, width, height = view["rectangle"]
    outside = np.ones((side, side), dtype=bool)
    outside[y : y + height, x : x + width] = False
    assert np.array_equal(got[outside], case_chrome(side)[outside])  # clipped to the rectangle


@pytest.mark.parametrize("name", ["sparse", "stamps"])
def test_strided_input_reads_row_zero(wanted, name: str) -> None:
    """The same points as row 0 of [N][18][L], vector_stride = 18 L: the same bytes as the dense layout."""
    for dtype in ("float32", "float64"):
        view, values, want = wanted[name, dtype]
        got = template_gpu(case_chrome(CASES[name][1]), view, values, rows=18).cpu().numpy()
        assert np.array_equal(got, want.image)


def test_dense_case_twice_gives_identical_bytes(wanted) -> None:
    view, values, want = wanted["dense", "float64"]
    first = template_gpu(case_chrome(32), view, values).cpu().numpy()
    second = template_gpu(case_chrome(32), view, values).cpu().numpy()
    assert np.array_equal(first, second) and np.array_equal(first, want.image)


def test_equal_depth_shows_the_largest_point_number() -> None:
    """
    A top view of N = 60 rows on a rectangle 26 pixels high: every depth level is equal, rows of points share pixel rows,
    and every contested pixel must show the point with the largest number. Once with constant data (against the
    restatement); once with values that differ too little to change the depth level but colour every row of points
    differently, so the winner of a pixel can be read off its colour.
    """
    count, length, side, rectangle = 60, 19, 32, (2, 4, 28, 26)
    chrome = np.full((side, side, 3), 255, dtype=np.uint8)  # (no chrome pixel can be taken for a point's colour)
    constant = np.full((count, length), 1.5)
    view = view_of(constant, rectangle, vectors=TOP_VIEW)
    want = ref.template(chrome, view, constant, LUT)
    assert want.smallest_margin > 1e-6 and want.contested == want.reached > 0
    assert np.array_equal(template_gpu(chrome, view, constant).cpu().numpy(), want.image)

    by_row = np.repeat(np.arange(count, dtype=np.float64)[:, None], length, axis=1)  # v = n
    lut = np.zeros((256, 3), dtype=np.uint8)
    lut[:, 0], lut[:, 1] = np.arange(256), 255 - np.arange(256)
    view = view_of(by_row, rectangle, vectors=TOP_VIEW, z=(-1e9, 3e9), colour=(0.0, 255.0))  # colour index = n
    want = ref.template(chrome, view, by_row, lut)
    _, row_at, level_at = ref.positions(view, np.zeros(count), np.arange(count), np.arange(count))
    assert len(set(np.floor(level_at + 0.5))) == 1 and want.smallest_margin > 1e-6  # one depth level for all
    for reverse in (False, True):
        values = by_row[::-1].copy() if reverse else by_row
        got = template_gpu(chrome, view, values, lut).cpu().numpy()
        x, y, width, height = rectangle
        pixel_rows = (height - 1) - np.floor(row_at + 0.5).astype(int)
        for pixel_row in np.unique(pixel_rows):
            last = int(np.nonzero(pixel_rows == pixel_row)[0].max())  # the largest vector number on this pixel row
            shown = int(values[last, 0])
            assert (got[y + pixel_row, x : x + width][:, 0] == shown).sum() == length, (reverse, pixel_row)
        assert np.array_equal(got, ref.template(chrome, view, values, lut).image)


def test_constant_data_and_data_that_excludes_zero() -> None:
    """Limits widened by span (one value only), and z limits stretched to take in the marker's 0."""
    chrome = case_chrome(64)
    rectangle = (8, 12, 48, 44)
    rs = np.random.RandomState(11)
    for values in (np.full((6, 13), -2.25), rs.uniform(3.0, 9.0, (6, 14)), rs.uniform(-7.0, -2.0, (6, 14)).astype(np.float32)):
        as_double = values.astype(np.float64)
        view = view_of(as_double, rectangle)
        assert view["z_limits"][0] == min(as_double.min(), 0.0) and view["z_limits"][1] == max(as_double.max(), 0.0)
        assert view["colour_limits"][1] > view["colour_limits"][0] >= as_double.min()
        want = ref.template(chrome, view, as_double, LUT)
        assert want.smallest_margin > 1e-6 and want.reached > 0
        assert np.array_equal(template_gpu(chrome, view, values).cpu().numpy(), want.image)


def test_frames_are_the_template_with_the_marker() -> None:
    """N = 9 frames into the right half of frames two panels wide; the left half must come back untouched."""
    count, length, side, rectangle = 9, 16, 64, (8, 12, 48, 44)
    values = np.random.RandomState(13).standard_normal((count, length))
    chrome = case_chrome(side)
    view = view_of(values, rectangle, marker_size=3)
    cursors = [float(n) for n in range(count)]
    assert ref.marker_margin(view, cursors) > 1e-6
    d_template = template_gpu(chrome, view, values)
    template = ref.template(chrome, view, values, LUT).image
    assert np.array_equal(d_template.cpu().numpy(), template)
    pattern = np.random.RandomState(17).randint(0, 256, (count, side, 2 * side, 3)).astype(np.uint8)

    def draw(batches) -> np.ndarray:
        out = torch.from_numpy(pattern).cuda()
        for first, frames_in_batch in batches:
            records = np.zeros(frames_in_batch, dtype=hip_lib.DEBUG_FRAME_DTYPE)
            records["number"], records["cursor"] = np.arange(first, first + frames_in_batch), cursors[first : first + frames_in_batch]
            d_records = torch.from_numpy(records.view(np.uint8)).cuda()
            rows = out[first:]
            hip_lib.debug_draw_scatter3d_device(
                d_template.data_ptr(), side, bind(view), d_records.data_ptr(), frames_in_batch, rows.data_ptr() + side * 3, rows.stride(0),
                rows.stride(1), torch.cuda.current_stream().cuda_stream,
            )
        torch.cuda.synchronize()
        return out.cpu().numpy()

    whole = draw([(0, count)])
    assert np.array_equal(whole[:, :, :side], pattern[:, :, :side]), "the left panel was written to"
    shown = set()
    for number in (0, 4, 8):
        want = ref.frame(template, view, cursors[number])
        marked = (want != template).any(axis=-1)
        assert 0 < marked.sum() <= 9 and (want[marked] == (255, 0, 0)).all()
        shown.add(tuple(np.argwhere(marked)[0]))
        assert np.array_equal(whole[number, :, side:], want), number
    assert len(shown) == 3  # the marker moves
    assert np.array_equal(draw([(0, 5), (5, 4)]), whole)
    # a cursor that is not finite: the template alone
    records = np.zeros(1, dtype=hip_lib.DEBUG_FRAME_DTYPE)
    records["cursor"] = np.nan
    out = torch.zeros((1, side, side, 3), dtype=torch.uint8, device="cuda")
    d_records = torch.from_numpy(records.view(np.uint8)).cuda()
    hip_lib.debug_draw_scatter3d_device(
        d_template.data_ptr(), side, bind(view), d_records.data_ptr(), 1, out.data_ptr(), out.stride(0), out.stride(1),
        torch.cuda.current_stream().cuda_stream,
    )
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], template)
