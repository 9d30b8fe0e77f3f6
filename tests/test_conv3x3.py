"""
Tests of the plain 3x3 convolution that need no GPU (gance_amd/csrc/conv3x3.hip, gance::conv3x3, `VGG16Lpips(convolution=)`):
the refusals of the C entries before a device is touched, the form and the workspace as pure functions of the shape, the
fake kernel, the transposed weight, and the coverage of tests/conv3x3_cases.CASES: every kernel form the dispatcher picks
for a VGG16 layer, forward or backward, at a side from 4 to 256 has a case that the GPU test runs.
"""

import ctypes

import pytest
import torch

from conv3x3_cases import CASES, VGG_LAYERS
from gance_amd import hip_lib, torch_ops
from gance_amd.stylegan2 import lpips

INVALID = 1  # GANCE_ERR_INVALID_ARGUMENT
FAKE = 0x10000  # a non-NULL, aligned "device pointer": every call below must return before it is looked at


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


def expected_form(cin: int, cout: int, side: int) -> int:
    """include/gance_hip.h, restated: 8 * (channel tile class) + log2(splits)."""
    tile_class = 2 if cout >= 64 else 1 if cout >= 32 else 0
    wanted = 16 if side <= 16 else 4 if side <= 32 else 2 if side <= 64 else 1
    log2_splits = 0
    while 2 << log2_splits <= wanted and 2 * (2 << log2_splits) <= cin // 16:
        log2_splits += 1
    return 8 * tile_class + log2_splits


def test_forward_refuses_bad_arguments_before_touching_a_device(library: ctypes.CDLL) -> None:
    entry = library.gance_conv3x3_forward
    good = [FAKE, FAKE, 2, 64, 128, 10, 10, FAKE, FAKE, 1 << 30, None]
    for position in (0, 1, 7, 8):
        arguments = list(good)
        arguments[position] = None
        assert entry(*arguments) == INVALID and b"NULL" in library.gance_last_error(), position
        assert b"gance_conv3x3_forward" in library.gance_last_error()
        arguments[position] = FAKE + 2
        assert entry(*arguments) == INVALID and b"misaligned" in library.gance_last_error(), position
    bad = (
        [(2, batch, b"batch") for batch in (0, -1, 65536)]
        + [(position, channels, b"multiples of 16") for position in (3, 4) for channels in (0, 8, 24, 528, -16)]
        + [(5, 12, b"square"), (6, 12, b"square")]
        + [(9, 0, b"workspace"), (9, 2 * 2 * 128 * 100 * 4 - 1, b"workspace")]  # cin 64 at side 10: two splits
    )
    for position, value, word in bad:
        arguments = list(good)
        arguments[position] = value
        assert entry(*arguments) == INVALID, (position, value)
        assert word in library.gance_last_error(), (position, value, library.gance_last_error())
    for side in (3, 0, 1025, -4):
        arguments = list(good)
        arguments[5] = arguments[6] = side
        assert entry(*arguments) == INVALID and b"[4, 1024]" in library.gance_last_error(), side
    with pytest.raises(ValueError):
        hip_lib.conv3x3_forward_device(FAKE, FAKE, 1, 20, 16, 8, 8, FAKE, FAKE, 1 << 20)


def test_form_and_workspace_are_pure_functions_of_the_shape(library: ctypes.CDLL) -> None:
    form, size = ctypes.c_int32(), ctypes.c_uint64()
    former, sizer = library.gance_conv3x3_form, library.gance_conv3x3_workspace_bytes
    assert len(former.argtypes) == 4  # (cin, cout, side, form): the batch is no argument at all
    assert former(64, 64, 8, None) == INVALID and b"NULL" in library.gance_last_error()
    assert sizer(1, 64, 64, 8, None) == INVALID and b"NULL" in library.gance_last_error()
    for cin, cout, side in [(8, 64, 8), (64, 528, 8), (64, 64, 3), (64, 64, 1025), (24, 64, 8)]:
        assert former(cin, cout, side, ctypes.byref(form)) == INVALID, (cin, cout, side)
        assert sizer(1, cin, cout, side, ctypes.byref(size)) == INVALID, (cin, cout, side)
    assert sizer(0, 64, 64, 8, ctypes.byref(size)) == INVALID and sizer(65536, 64, 64, 8, ctypes.byref(size)) == INVALID
    for cin in (16, 32, 48, 64, 128, 256, 512):
        for cout in (16, 32, 48, 64, 80, 512):
            for side in (4, 5, 16, 17, 32, 33, 64, 65, 130, 256, 1024):
                assert former(cin, cout, side, ctypes.byref(form)) == 0
                assert form.value == expected_form(cin, cout, side) == hip_lib.conv3x3_form(cin, cout, side), (cin, cout, side)
                assert former(cin, cout, side, ctypes.byref(form)) == 0 and form.value == expected_form(cin, cout, side)  # the same again
                splits = 1 << (form.value % 8)
                for batch in (1, 3):
                    assert sizer(batch, cin, cout, side, ctypes.byref(size)) == 0
                    assert size.value == (16 if splits == 1 else splits * batch * cout * side * side * 4), (batch, cin, cout, side)
                    assert hip_lib.conv3x3_workspace_bytes(batch, cin, cout, side) == size.value
    with pytest.raises(ValueError):
        hip_lib.conv3x3_form(64, 64, 2)
    with pytest.raises(ValueError):
        hip_lib.conv3x3_workspace_bytes(1, 64, 20, 8)


def test_cases_cover_every_form_vgg16_reaches() -> None:
    """Tied to the dispatcher: gance_conv3x3_form over VGG16's layers, both directions, every side from 4 to 256."""
    reached = {}
    for cin, cout in VGG_LAYERS:
        for pair in ((cin, cout), (cout, cin)):  # the backward runs the pair swapped
            for side in range(4, 257):
                reached.setdefault(hip_lib.conv3x3_form(pair[0], pair[1], side), (pair[0], pair[1], side))
    covered = {hip_lib.conv3x3_form(cin, cout, side) for _, cin, cout, side in CASES}
    print(f"forms reached by VGG16: {sorted(reached)}; forms of CASES: {sorted(covered)}")
    missing = {form: shape for form, shape in reached.items() if form not in covered}
    assert not missing, f"forms without a GPU case (form: first (cin, cout, side) that takes it): {missing}"
    assert len(set(CASES)) == len(CASES)


def test_callable_refuses_an_unknown_convolution_without_a_device() -> None:
    weights = lpips.random_lpips_weights(0)
    for convolution in ("nonsense", "", "CONV3X3", None):
        with pytest.raises(ValueError, match="convolution"):
            lpips.VGG16Lpips(weights, side=64, convolution=convolution)  # type: ignore[arg-type]


def test_fake_kernel() -> None:
    from torch._subclasses.fake_tensor import FakeTensorMode  # pylint: disable=import-outside-toplevel

    with FakeTensorMode():
        empty = lambda *shape: torch.empty(shape, device="cuda")  # noqa: E731
        y = torch.ops.gance.conv3x3(empty(2, 32, 9, 9), empty(3, 3, 32, 80), empty(3, 3, 80, 32))
        assert y.shape == (2, 80, 9, 9) and y.dtype == torch.float32 and y.device.type == "cuda"


def test_transposed_weight_is_an_involution() -> None:
    weight = torch.randn(3, 3, 32, 48, generator=torch.Generator().manual_seed(0))
    image = torch_ops.conv3x3_transposed_weight(weight)
    assert image.shape == (3, 3, 48, 32) and image.is_contiguous()
    assert torch.equal(image, weight.flip(0, 1).transpose(2, 3))
    assert float(image[0, 2, 5, 7]) == float(weight[2, 0, 7, 5])
    assert torch.equal(torch_ops.conv3x3_transposed_weight(image), weight)
    with pytest.raises(ValueError):
        torch_ops.conv3x3_transposed_weight(torch.zeros(3, 3, 16))
