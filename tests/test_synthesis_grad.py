"""
CPU tests of differentiable synthesis (gance_amd/csrc/synthesis_grad.hip, the gance::modconv3x3 / noise_bias_lrelu /
torgb_skip ops, gance_amd/stylegan2/differentiable.py): the reference helper of the GPU tests (tests/grad_ref.py) equals the
oracle, the yardstick of the gradient bars is sound, every new entry point refuses bad arguments before a device is
touched, and the ops have fake-tensor registrations.
"""

import ctypes
from typing import List

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import grad_ref
from gance_amd import hip_lib, torch_ops  # noqa: F401  pylint: disable=unused-import
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref


@pytest.mark.parametrize("name", grad_ref.CASE_NAMES)
def test_helper_with_default_signs_is_g_synthesis(name: str) -> None:
    """With sign = pre > 0 the helper is the oracle's g_synthesis bit for bit, image and every activation, in float64."""
    case = grad_ref.case(name)
    activations: List[torch.Tensor] = []
    with torch.no_grad():
        image = grad_ref.g_synthesis_with_signs(
            torch.from_numpy(case.dlatents).double(), case.variables, case.resolution, case.fmap_base, collect=activations
        )
    assert torch.equal(image, case.image64)
    assert len(activations) == len(case.activations64)
    for got, want in zip(activations, case.activations64):
        assert torch.equal(got, want)


@pytest.mark.parametrize("name", grad_ref.CASE_NAMES)
def test_yardstick_is_finite_and_small(name: str) -> None:
    """The float32 oracle against the float64 helper with its slope masks: 0.9e-6 ... 1.5e-6 measured, far below 1e-5."""
    value = grad_ref.yardstick(name)
    print(f"{name}: float32 oracle gradient error {value:.3e}")
    assert 0.0 < value < 1e-5


def test_injected_signs_change_the_function() -> None:
    """Flipping one slope mask entry changes the helper's image: the masks are used, not recomputed."""
    case = grad_ref.case("perturb-16-f")
    signs = [activation > 0 for activation in case.activations64]
    signs[1] = ~signs[1]
    with torch.no_grad():
        image = grad_ref.g_synthesis_with_signs(torch.from_numpy(case.dlatents).double(), case.variables, case.resolution, signs=signs)
    assert not torch.equal(image, case.image64)


# ---- the C ABI's argument checks ----

P = 0x1000  # a non-NULL, aligned address: never dereferenced, the checks come first


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    return hip_lib.load_library()


def _modconv_forward(lib, pointers=None, batch=1, cin=16, cout=16, height=4, width=4, up=0, workspace_bytes=1 << 20):  # type: ignore[no-untyped-def]
    x, style, demod, weight, y, workspace = pointers or (P,) * 6
    return lib.gance_modconv3x3_forward(x, style, demod, weight, batch, cin, cout, height, width, up, y, workspace, workspace_bytes, None)


def _modconv_backward(lib, pointers=None, batch=1, cin=16, cout=16, height=4, width=4, up=0, workspace_bytes=1 << 20):  # type: ignore[no-untyped-def]
    a = pointers or (P,) * 10
    return lib.gance_modconv3x3_backward(*a[:6], batch, cin, cout, height, width, up, *a[6:9], a[9], workspace_bytes, None)


def _lrelu_forward(lib, pointers=None, noise_batch=1, batch=1, channels=16, height=4, width=4):  # type: ignore[no-untyped-def]
    x, noise, strength, bias, out = pointers or (P,) * 5
    return lib.gance_noise_bias_lrelu_forward(x, noise, noise_batch, strength, bias, batch, channels, height, width, out, None)


def _lrelu_backward(lib, pointers=None, batch=1, channels=16, height=4, width=4, reserved=(None, None, None)):  # type: ignore[no-untyped-def]
    grad_out, out, grad_x = pointers or (P,) * 3
    return lib.gance_noise_bias_lrelu_backward(grad_out, out, batch, channels, height, width, grad_x, *reserved, None)


def _torgb_forward(lib, pointers=None, y_prev=None, batch=1, cin=16, height=4, width=4):  # type: ignore[no-untyped-def]
    x, style, weight, bias, y = pointers or (P,) * 5
    return lib.gance_torgb_skip_forward(x, style, weight, bias, y_prev, batch, cin, height, width, y, None)


def _torgb_backward(lib, pointers=None, grad_y_prev=None, batch=1, cin=16, height=4, width=4, workspace_bytes=1 << 20):  # type: ignore[no-untyped-def]
    grad_y, x, style, weight, grad_x, grad_style, workspace = pointers or (P,) * 7
    return lib.gance_torgb_skip_backward(grad_y, x, style, weight, batch, cin, height, width, grad_x, grad_style, grad_y_prev, workspace,
                                         workspace_bytes, None)


ENTRY_POINTS = [
    (_modconv_forward, 6, "gance_modconv3x3_forward", "cin"),
    (_modconv_backward, 10, "gance_modconv3x3_backward", "cout"),
    (_lrelu_forward, 5, "gance_noise_bias_lrelu_forward", "channels"),
    (_lrelu_backward, 3, "gance_noise_bias_lrelu_backward", "channels"),
    (_torgb_forward, 5, "gance_torgb_skip_forward", "cin"),
    (_torgb_backward, 7, "gance_torgb_skip_backward", "cin"),
]


@pytest.mark.parametrize("call, pointer_count, name, channel_argument", ENTRY_POINTS, ids=[entry[2] for entry in ENTRY_POINTS])
def test_entry_points_refuse_bad_arguments(library: ctypes.CDLL, call, pointer_count: int, name: str, channel_argument: str) -> None:
    def refused(status: int, *words: str) -> None:
        message = library.gance_last_error().decode()
        assert status == 1, message  # GANCE_ERR_INVALID_ARGUMENT
        assert message.startswith(name + ":") and all(word in message for word in words), message

    for position in range(pointer_count):  # every required pointer: NULL, then misaligned
        pointers = [P] * pointer_count
        pointers[position] = None
        refused(call(library, tuple(pointers)), "NULL pointer")
        pointers[position] = P + 2
        refused(call(library, tuple(pointers)), "misaligned pointer")
    for count in (0, 8, 24, 528):
        refused(call(library, **{channel_argument: count}), "multiples of 16", str(count))
    refused(call(library, height=8, width=4), "square", "8 x 4")
    for side in (2, 3, 1025, 2048):
        refused(call(library, height=side, width=side), "side must be in [4, 1024]", str(side))
    refused(call(library, batch=0), "batch")
    refused(call(library, batch=4096, height=1024, width=1024), "one call's grid")


def test_entry_point_specific_refusals(library: ctypes.CDLL) -> None:
    def message() -> str:
        return library.gance_last_error().decode()

    for call in (_modconv_forward, _modconv_backward):
        assert call(library, height=1024, width=1024, up=1) == 1 and "up layer's input side" in message()
        assert call(library, workspace_bytes=16) == 1 and "workspace of 16 bytes" in message()
    assert _torgb_backward(library, workspace_bytes=16) == 1 and "workspace of 16 bytes" in message()
    assert _lrelu_forward(library, noise_batch=2, batch=3) == 1 and "1 or 3 planes" in message()
    assert _lrelu_backward(library, reserved=(P, None, None)) == 1 and "not implemented" in message()
    assert _torgb_forward(library, y_prev=P + 1) == 1 and "misaligned" in message()
    assert _torgb_forward(library, y_prev=P, height=5, width=5) == 1 and "even" in message()
    assert _torgb_backward(library, grad_y_prev=P, height=5, width=5) == 1 and "even" in message()
    size = ctypes.c_uint64()
    assert library.gance_modconv3x3_workspace_bytes(1, 16, 16, 4, 0, None) == 1 and "NULL" in message()
    assert library.gance_modconv3x3_workspace_bytes(1, 16, 20, 4, 0, ctypes.byref(size)) == 1 and "multiples of 16" in message()
    assert library.gance_torgb_skip_workspace_bytes(1, 16, 3, ctypes.byref(size)) == 1 and "side must be" in message()
    # the bound covers the partial sums of both position sums and, for an up layer, the (2 side + 1)^2 intermediate
    assert library.gance_modconv3x3_workspace_bytes(2, 32, 16, 8, 0, ctypes.byref(size)) == 0 and size.value == 2 * 32 * 64 * 4
    assert library.gance_modconv3x3_workspace_bytes(2, 32, 16, 8, 1, ctypes.byref(size)) == 0
    assert size.value == 2 * 32 * 64 * 4 + (2 * 16 * 17 * 17 * 4 + 15) // 16 * 16
    with pytest.raises(ValueError, match="multiples of 16"):
        hip_lib.modconv3x3_workspace_bytes(1, 16, 20, 4, False)


# ---- the ops ----


def test_ops_have_fake_tensor_registrations_and_the_right_shapes() -> None:
    with FakeTensorMode():
        def empty(*shape: int) -> torch.Tensor:
            return torch.empty(shape, dtype=torch.float32, device="cuda")

        x, style, demod, weight = empty(3, 32, 8, 8), empty(3, 32), empty(3, 48), empty(3, 3, 32, 48)
        for up, side in ((False, 8), (True, 16)):
            y = torch.ops.gance.modconv3x3(x, style, demod, weight, up)
            assert y.shape == (3, 48, side, side) and y.dtype == torch.float32 and y.device.type == "cuda"
            grads = torch.ops.gance.modconv3x3_backward(y, x, y, style, demod, weight, up)
            assert [tuple(grad.shape) for grad in grads] == [(3, 32, 8, 8), (3, 32), (3, 48)]
        out = torch.ops.gance.noise_bias_lrelu(x, empty(1, 1, 8, 8), empty(1), empty(32))
        assert out.shape == x.shape
        assert torch.ops.gance.noise_bias_lrelu_backward(out, out).shape == x.shape
        rgb_weight, rgb_bias = empty(32, 3), empty(3)
        for y_prev in (None, empty(3, 3, 4, 4)):
            y = torch.ops.gance.torgb_skip(x, style, rgb_weight, rgb_bias, y_prev)
            assert y.shape == (3, 3, 8, 8)
            grads = torch.ops.gance.torgb_skip_backward(y, x, style, rgb_weight, y_prev is not None)
            assert [tuple(grad.shape) for grad in grads] == [(3, 32, 8, 8), (3, 32), (3, 3, 4, 4) if y_prev is not None else (0,)]


def test_existing_ops_stay_without_autograd() -> None:
    """synthesize_w_image is the engine's forward-only path: nothing registers a backward on it."""
    assert torch_ops.synthesize_w_image._backward_fn is None  # pylint: disable=protected-access
    for op in (torch_ops.modconv3x3, torch_ops.noise_bias_lrelu, torch_ops.torgb_skip):
        assert op._backward_fn is not None  # pylint: disable=protected-access


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_gpu_means_loud_failure() -> None:
    from gance_amd.stylegan2.differentiable import DifferentiableSynthesis  # pylint: disable=import-outside-toplevel

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DifferentiableSynthesis(sg2_spec.make_random_variables(8, seed=0), 8)


def test_oracle_functions_take_the_style_as_a_leaf() -> None:
    """The isolated oracles' trick (identity mod_weight, mod_bias -1) reproduces the style exactly enough: compare with a direct conv."""
    inputs = grad_ref.modconv_inputs(1, 16, 16, 4, False, seed=0)
    y = grad_ref.modconv_oracle(inputs, False, torch.float64)[0]
    weight = torch.from_numpy(grad_ref.scaled_weight(inputs["weight"]).astype("float64")).permute(3, 2, 0, 1)
    x = torch.from_numpy(inputs["x"]).double() * torch.from_numpy(inputs["style"]).double()[:, :, None, None]
    want = torch.nn.functional.conv2d(x, weight, padding=1) * torch.from_numpy(inputs["demod"]).double()[:, :, None, None]
    assert grad_ref.relative_error(y, want) < 1e-6  # (the float32 rounding of the scaled weight)
    assert ref.upsample_2d(torch.ones(1, 1, 2, 2, dtype=torch.float64)).shape == (1, 1, 4, 4)


def test_torgb_oracle_takes_any_even_side() -> None:
    """Side 66 is no power of two: the scope the helper builds is the one ref.torgb_layer reads, and the result is the ToRGB step."""
    inputs = grad_ref.torgb_inputs(2, 16, 66, True, seed=0)
    y, grad_x, grad_style, grad_y_prev = grad_ref.torgb_oracle(inputs, torch.float64)
    assert grad_x.shape == (2, 16, 66, 66) and grad_style.shape == (2, 16) and grad_y_prev.shape == (2, 3, 33, 33)
    coefficients = torch.from_numpy(grad_ref.scaled_weight(inputs["weight"]).astype("float64")).reshape(16, 3)
    rgb = torch.einsum("bi,ic,bihw->bchw", torch.from_numpy(inputs["style"]).double(), coefficients, torch.from_numpy(inputs["x"]).double())
    want = ref.upsample_2d(torch.from_numpy(inputs["y_prev"]).double()) + rgb + torch.from_numpy(inputs["bias"]).double().reshape(1, 3, 1, 1)
    assert grad_ref.relative_error(y, want) < 1e-6  # (the float32 rounding of the scaled weight)


def test_sign_flip_cap_keeps_the_density_of_the_small_cases() -> None:
    assert grad_ref.activations_per_sample(64, sg2_spec.FMAP_BASE) == grad_ref.SIGN_FLIP_ACTIVATIONS
    assert all(grad_ref.sign_flip_cap(name) == grad_ref.MAX_SIGN_FLIPS == 8 for name in grad_ref.CASE_NAMES)
    assert [grad_ref.sign_flip_cap(name) for name in grad_ref.LARGE_CASE_NAMES] == [11, 11, 23]
    assert not set(grad_ref.LARGE_CASE_NAMES) & set(grad_ref.CASE_NAMES)
