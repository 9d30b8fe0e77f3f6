"""
CPU tests of LPIPS on VGG16 (gance_amd/stylegan2/lpips.py, gance_amd/csrc/lpips.hip): the restatement of tests/lpips_ref.py
against an independent composition, the weights' file format and converter, every refusal that comes before a device, and the
flip condition of the GPU file's whole-chain inputs on the reference alone.
"""

import ctypes
from pathlib import Path
from typing import Dict, List

import numpy as np
import pytest
import torch

import grad_ref
import lpips_ref
from gance_amd import hip_lib
from gance_amd.stylegan2 import lpips

INVALID = 1  # GANCE_ERR_INVALID_ARGUMENT
FAKE = 0x10000  # a non-NULL, aligned "device pointer": every call below must return before it is looked at


def plain_distance(image: torch.Tensor, other: torch.Tensor, weights: lpips.LpipsWeights, side: int) -> torch.Tensor:
    """LPIPS written a second time, straight from conv2d / relu / max_pool2d, sharing nothing with lpips_ref but the weights."""

    def features(x: torch.Tensor) -> List[torch.Tensor]:
        if x.shape[2] > side:
            x = torch.nn.functional.avg_pool2d(x, x.shape[2] // side)
        x = (x - torch.tensor(weights.shift, dtype=x.dtype).reshape(1, 3, 1, 1)) / torch.tensor(weights.scale, dtype=x.dtype).reshape(1, 3, 1, 1)
        out = []
        for index, (weight, bias) in enumerate(weights.convs):
            kernel = torch.from_numpy(weight.transpose(3, 2, 0, 1).copy()).to(x.dtype)
            x = torch.relu(torch.nn.functional.conv2d(x, kernel, torch.from_numpy(bias).to(x.dtype), padding=1))
            if index in (1, 3, 6, 9, 12):
                out.append(x)
            if index in (1, 3, 6, 9):
                x = torch.nn.functional.max_pool2d(x, 2)
        return out

    total = torch.zeros(image.shape[0], dtype=image.dtype)
    for mine, theirs, lin in zip(features(image), features(other), weights.lins):
        mine = mine / (torch.linalg.vector_norm(mine, dim=1, keepdim=True) + 1e-10)
        theirs = theirs / (torch.linalg.vector_norm(theirs, dim=1, keepdim=True) + 1e-10)
        total = total + (torch.from_numpy(lin).to(image.dtype).reshape(1, -1, 1, 1) * (mine - theirs) ** 2).sum(dim=1).mean(dim=(1, 2))
    return total


def two_images(seed: int, resolution: int, dtype: torch.dtype, batch: int = 1) -> List[torch.Tensor]:
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(np.stack([lpips_ref.smooth_image(rng, resolution) for _ in range(batch)])).to(dtype) for _ in range(2)]


# ---- the restatement ----


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_without_masks_is_the_plain_composition(dtype: torch.dtype) -> None:
    weights = lpips_ref.chain_weights(0)
    image, other = two_images(5, 64, dtype, batch=2)
    leaf, plain_leaf = image.clone().requires_grad_(True), image.clone().requires_grad_(True)
    collected: List[torch.Tensor] = []
    mine = lpips_ref.image_distance(leaf, other, weights, 64, collect=collected)
    plain = plain_distance(plain_leaf, other, weights, 64)
    assert len(collected) == 13 and torch.equal(mine, plain)
    (gradient,) = torch.autograd.grad(mine.sum(), leaf)
    (plain_gradient,) = torch.autograd.grad(plain.sum(), plain_leaf)
    assert torch.equal(gradient, plain_gradient)
    # ... and handing a run its own activations back changes nothing
    again = lpips_ref.image_distance(leaf, other, weights, 64, activations=[activation.detach() for activation in collected])
    assert torch.equal(again, mine)
    (masked_gradient,) = torch.autograd.grad(again.sum(), leaf)
    assert torch.equal(masked_gradient, gradient)


def test_restatement_area_mean_is_the_plain_one() -> None:
    weights = lpips_ref.chain_weights(1)
    image, other = two_images(6, 128, torch.float64)
    # (avg_pool2d adds the four pixels in another order than reshape-mean: equal to rounding, not to the bit)
    mine, plain = float(lpips_ref.image_distance(image, other, weights, 64)), float(plain_distance(image, other, weights, 64))
    assert plain > 0 and abs(mine - plain) <= 1e-12 * plain


def test_distance_of_an_image_to_itself_is_zero() -> None:
    weights = lpips_ref.chain_weights(0)
    for dtype in (torch.float32, torch.float64):
        image, _ = two_images(7, 64, dtype)
        assert float(lpips_ref.image_distance(image, image.clone(), weights, 64)) == 0.0


def test_distance_is_symmetric() -> None:
    weights = lpips_ref.chain_weights(2)
    image, other = two_images(8, 64, torch.float64)
    forth, back = float(lpips_ref.image_distance(image, other, weights, 64)), float(lpips_ref.image_distance(other, image, weights, 64))
    assert forth > 0 and abs(forth - back) <= 1e-12 * forth


def test_gradient_is_finite_at_an_all_zero_feature_pixel() -> None:
    weights = lpips_ref.chain_weights(0)
    convs = list(weights.convs)
    convs[1] = (convs[1][0], np.full_like(convs[1][1], -1e3))  # relu1_2, the first tap, is zero everywhere
    weights = weights._replace(convs=tuple(convs))
    image, other = two_images(9, 64, torch.float64)
    leaf = image.requires_grad_(True)
    collected: List[torch.Tensor] = []
    total = lpips_ref.image_distance(leaf, other, weights, 64, collect=collected)
    assert float(collected[1].detach().abs().max()) == 0.0
    (gradient,) = torch.autograd.grad(total.sum(), leaf)
    assert bool(torch.isfinite(total).all()) and bool(torch.isfinite(gradient).all())
    # the head alone, with a non-zero target at the zero pixels: the gradient is lin * -2 t / 1e-10 / pixels, finite
    f = torch.zeros((1, 16, 4, 4), dtype=torch.float64, requires_grad=True)
    target = lpips_ref.normalize(torch.ones((1, 16, 4, 4), dtype=torch.float64))
    (head_gradient,) = torch.autograd.grad(lpips_ref.layer_distance(f, target, torch.ones(16, dtype=torch.float64)).sum(), f)
    assert bool(torch.isfinite(head_gradient).all())
    assert torch.allclose(head_gradient, torch.full_like(head_gradient, -2.0 * 0.25 / 1e-10 / 16.0), rtol=1e-9)


# ---- the weights ----


def assert_same_weights(got: lpips.LpipsWeights, want: lpips.LpipsWeights) -> None:
    for (weight, bias), (want_weight, want_bias) in zip(got.convs, want.convs):
        assert weight.dtype == np.float32 and np.array_equal(weight, want_weight) and np.array_equal(bias, want_bias)
    assert len(got.convs) == 13 and len(got.lins) == 5
    assert all(np.array_equal(lin, want_lin) for lin, want_lin in zip(got.lins, want.lins))
    assert np.array_equal(got.shift, want.shift) and np.array_equal(got.scale, want.scale)


def test_random_weights_follow_the_recipe() -> None:
    weights = lpips.random_lpips_weights(3)
    assert [tuple(weight.shape) for weight, _ in weights.convs] == [(3, 3, cin, cout) for _, cin, cout in lpips.CONV_LAYERS]
    assert [tuple(lin.shape) for lin in weights.lins] == [(64,), (128,), (256,), (512,), (512,)]
    assert all(float(lin.min()) >= 0 for lin in weights.lins)
    assert np.allclose(weights.shift, (-0.030, -0.088, -0.188)) and np.allclose(weights.scale, (0.458, 0.448, 0.450))
    weight = weights.convs[8][0]
    assert abs(float(weight.std()) / np.sqrt(2.0 / (9 * 512)) - 1.0) < 0.01 and abs(float(weights.convs[8][1].std()) / 0.1 - 1.0) < 0.15
    assert_same_weights(lpips.random_lpips_weights(3), weights)


def test_npz_round_trip(tmp_path: Path) -> None:
    weights = lpips.random_lpips_weights(4)
    path = tmp_path / "weights.npz"
    lpips.save_lpips_weights(path, weights)
    with np.load(path, allow_pickle=False) as file:
        assert set(file.files) == {f"{name}/{part}" for name, _, _ in lpips.CONV_LAYERS for part in ("weight", "bias")} | {
            "lin0", "lin1", "lin2", "lin3", "lin4", "shift", "scale"}  # fmt: skip
    assert_same_weights(lpips.load_lpips_weights(path), weights)


def _arrays(weights: lpips.LpipsWeights) -> Dict[str, np.ndarray]:
    arrays = {}
    for (name, _, _), (weight, bias) in zip(lpips.CONV_LAYERS, weights.convs):
        arrays[f"{name}/weight"], arrays[f"{name}/bias"] = weight.copy(), bias.copy()
    for index, lin in enumerate(weights.lins):
        arrays[f"lin{index}"] = lin.copy()
    arrays["shift"], arrays["scale"] = weights.shift.copy(), weights.scale.copy()
    return arrays


@pytest.mark.parametrize(
    "key, change, word",
    [
        ("conv3_2/weight", None, "missing"),
        ("lin2", None, "missing"),
        ("scale", None, "missing"),
        ("conv1_1/weight", lambda a: a.transpose(3, 2, 0, 1), "must be [3, 3, 3, 64]"),
        ("conv4_1/bias", lambda a: a[:-1], "must be [512]"),
        ("lin0", lambda a: a.reshape(1, 64, 1, 1), "must be [64]"),
        ("shift", lambda a: a[:2], "must be [3]"),
        ("conv2_1/weight", lambda a: np.where(np.arange(a.size).reshape(a.shape) == 7, np.nan, a), "not finite"),
        ("conv5_3/bias", lambda a: np.where(np.arange(a.size) == 1, np.inf, a), "not finite"),
        ("lin4", lambda a: np.where(np.arange(a.size) == 3, -1e-3, a), "negative"),
    ],
)
def test_load_refuses_bad_files(tmp_path: Path, key: str, change, word: str) -> None:  # type: ignore[no-untyped-def]
    arrays = _arrays(lpips.random_lpips_weights(5))
    if change is None:
        del arrays[key]
    else:
        arrays[key] = change(arrays[key]).astype(np.float32)
    path = tmp_path / "bad.npz"
    np.savez(path, **arrays)
    with pytest.raises(ValueError) as raised:
        lpips.load_lpips_weights(path)
    assert f"`{key}`" in str(raised.value) and word in str(raised.value)


@pytest.mark.parametrize("prefix", ["", "features."])
@pytest.mark.parametrize("tensors", [False, True])
def test_converter_on_random_dictionaries(prefix: str, tensors: bool) -> None:
    rng = np.random.RandomState(6)
    wrap = torch.from_numpy if tensors else (lambda array: array)
    vgg, linear, convs, lins = {}, {}, [], []
    for index, (_, cin, cout) in zip(lpips.TORCHVISION_CONV_INDICES, lpips.CONV_LAYERS):
        oihw = (rng.randn(cout, cin, 3, 3) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        bias = (0.1 * rng.randn(cout)).astype(np.float32)
        vgg[f"{prefix}{index}.weight"], vgg[f"{prefix}{index}.bias"] = wrap(oihw), wrap(bias)
        convs.append((oihw, bias))
    for index, channels in enumerate(lpips.TAP_CHANNELS):
        lin = (0.1 * np.abs(rng.randn(1, channels, 1, 1))).astype(np.float32)
        linear[f"lin{index}.model.1.weight"] = wrap(lin)
        lins.append(lin)
    if prefix:
        vgg["classifier.0.weight"] = wrap(np.zeros((4, 4), dtype=np.float32))  # the whole model's state dict has more
    weights = lpips.lpips_weights_from_state_dicts(vgg, linear)
    assert all(weight.shape == (3, 3, cin, cout) and weight.flags.c_contiguous for (weight, _), (_, cin, cout) in zip(weights.convs, lpips.CONV_LAYERS))
    assert weights.convs[2][0][0, 2, 5, 7] == convs[2][0][7, 5, 0, 2]  # [ky, kx, i, o] = OIHW [o, i, ky, kx]

    # the restatement on the converted weights against conv2d on the dictionary's own OIHW arrays
    image, other = two_images(10, 64, torch.float64)

    def features(x: torch.Tensor) -> List[torch.Tensor]:
        shift, scale = (torch.tensor(np.float32(values)).to(x.dtype).reshape(1, 3, 1, 1) for values in (lpips.DEFAULT_SHIFT, lpips.DEFAULT_SCALE))  # stored as float32
        x = (x - shift) / scale
        out = []
        for index, (oihw, bias) in enumerate(convs):
            x = torch.relu(torch.nn.functional.conv2d(x, torch.from_numpy(oihw).double(), torch.from_numpy(bias).double(), padding=1))
            if index in (1, 3, 6, 9, 12):
                out.append(x)
            if index in (1, 3, 6, 9):
                x = torch.nn.functional.max_pool2d(x, 2)
        return out

    want = torch.zeros(1, dtype=torch.float64)
    for mine, theirs, lin in zip(features(image), features(other), lins):
        difference = lpips_ref.normalize(mine) - lpips_ref.normalize(theirs)
        want = want + (torch.from_numpy(lin).double() * difference ** 2).sum(dim=1).mean(dim=(1, 2))
    assert torch.equal(lpips_ref.image_distance(image, other, weights, 64), want)

    del vgg[f"{prefix}10.bias"]
    with pytest.raises(ValueError, match="10.bias"):
        lpips.lpips_weights_from_state_dicts(vgg, linear)


# ---- refusals before a device ----


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


# (entry, good arguments, positions of the pointers that must not be NULL, [(position, bad value, word of the message)])
BAD_CHANNELS = [(0, "multiple of 16"), (8, "multiple of 16"), (24, "multiple of 16"), (528, "multiple of 16")]
BAD_SIDES = [(3, "[4, 1024]"), (0, "[4, 1024]"), (1025, "[4, 1024]"), (-4, "[4, 1024]")]
BAD_BATCHES = [(0, "batch"), (-1, "batch"), (65536, "batch")]


def _bad(position: int, values):  # type: ignore[no-untyped-def]
    return [(position, value, word) for value, word in values]


ENTRIES = [
    ("gance_lpips_input_forward", [FAKE, FAKE, FAKE, 2, 128, 64, FAKE, None], (0, 1, 2, 6),
     _bad(3, BAD_BATCHES) + _bad(4, [(2, "[4, 1024]"), (2048, "[4, 1024]"), (96, "multiple of side"), (32, "multiple of side")]) + _bad(5, BAD_SIDES) + _bad(5, [(48, "multiple of side")])),
    ("gance_lpips_input_backward", [FAKE, FAKE, 2, 128, 64, FAKE, None], (0, 1, 5),
     _bad(2, BAD_BATCHES) + _bad(3, [(2, "[4, 1024]"), (2048, "[4, 1024]"), (96, "multiple of side")]) + _bad(4, BAD_SIDES) + _bad(4, [(48, "multiple of side")])),
    ("gance_bias_relu_forward", [FAKE, FAKE, 2, 64, 10, 1, FAKE, FAKE, None], (0, 1, 6, 7),
     _bad(2, BAD_BATCHES) + _bad(3, BAD_CHANNELS) + _bad(4, BAD_SIDES) + _bad(4, [(5, "even"), (33, "even")])),
    ("gance_bias_relu_forward", [FAKE, FAKE, 2, 64, 5, 0, FAKE, None, None], (0, 1, 6), _bad(2, BAD_BATCHES) + _bad(3, BAD_CHANNELS) + _bad(4, BAD_SIDES)),
    ("gance_bias_relu_backward", [FAKE, FAKE, FAKE, 2, 64, 10, 1, FAKE, None], (0, 1, 2, 7),
     _bad(3, BAD_BATCHES) + _bad(4, BAD_CHANNELS) + _bad(5, BAD_SIDES) + _bad(5, [(5, "even"), (33, "even")])),
    ("gance_bias_relu_backward", [FAKE, None, FAKE, 2, 64, 5, 0, FAKE, None], (0, 2, 7), _bad(3, BAD_BATCHES) + _bad(4, BAD_CHANNELS) + _bad(5, BAD_SIDES)),
    ("gance_lpips_layer_forward", [FAKE, FAKE, FAKE, 2, 64, 9, FAKE, FAKE, 1 << 20, None], (0, 1, 2, 6, 7),
     _bad(3, BAD_BATCHES) + _bad(4, BAD_CHANNELS) + _bad(5, BAD_SIDES) + _bad(8, [(0, "workspace"), (7, "workspace")])),
    ("gance_lpips_layer_backward", [FAKE, FAKE, FAKE, FAKE, 2, 64, 9, FAKE, None], (0, 1, 2, 3, 7),
     _bad(4, BAD_BATCHES) + _bad(5, BAD_CHANNELS) + _bad(6, BAD_SIDES)),
    ("gance_lpips_normalize", [FAKE, 2, 64, 9, FAKE, None], (0, 4), _bad(1, BAD_BATCHES) + _bad(2, BAD_CHANNELS) + _bad(3, BAD_SIDES)),
]  # fmt: skip


@pytest.mark.parametrize("name, good, pointers, bad", ENTRIES, ids=[f"{entry[0]}-{index}" for index, entry in enumerate(ENTRIES)])
def test_entries_refuse_bad_arguments_before_touching_a_device(library: ctypes.CDLL, name: str, good, pointers, bad) -> None:  # type: ignore[no-untyped-def]
    entry = getattr(library, name)
    for position in pointers:
        arguments = list(good)
        arguments[position] = None
        assert entry(*arguments) == INVALID, position
        assert b"NULL" in library.gance_last_error() and name.encode() in library.gance_last_error()
        arguments[position] = FAKE + 2
        assert entry(*arguments) == INVALID and b"misaligned" in library.gance_last_error(), position
    for position, value, word in bad:
        arguments = list(good)
        arguments[position] = value
        assert entry(*arguments) == INVALID, (position, value)
        assert word.encode() in library.gance_last_error(), (position, value, library.gance_last_error())


def test_workspace_entry_and_wrappers(library: ctypes.CDLL) -> None:
    size = ctypes.c_uint64()
    sizer = library.gance_lpips_layer_workspace_bytes
    assert sizer(1, 64, None) == INVALID and b"NULL" in library.gance_last_error()
    assert sizer(0, 64, ctypes.byref(size)) == INVALID and sizer(1, 3, ctypes.byref(size)) == INVALID and sizer(1, 1025, ctypes.byref(size)) == INVALID
    # one fp64 partial per block: 16 positions per block below 4096 positions, 64 from there
    for batch, side, blocks in [(1, 4, 1), (3, 9, 6), (2, 33, 69), (1, 63, 249), (1, 64, 64), (2, 256, 1024), (1, 1024, 16384)]:
        assert sizer(batch, side, ctypes.byref(size)) == 0 and size.value == batch * blocks * 8, (batch, side)
        assert hip_lib.lpips_layer_workspace_bytes(batch, side) == size.value
    with pytest.raises(ValueError):
        hip_lib.lpips_layer_workspace_bytes(1, 2)
    with pytest.raises(ValueError):
        hip_lib.bias_relu_forward_device(FAKE, FAKE, 1, 64, 7, True, FAKE, FAKE)
    with pytest.raises(ValueError):
        hip_lib.lpips_input_forward_device(FAKE, FAKE, FAKE, 1, 100, 64, FAKE)
    with pytest.raises(ValueError):
        hip_lib.lpips_layer_forward_device(FAKE, FAKE, FAKE, 1, 20, 8, FAKE, FAKE, 1 << 20)
    with pytest.raises(ValueError):
        hip_lib.lpips_normalize_device(FAKE, 1, 16, 2000, FAKE)
    assert library.gance_abi_version() == 6


def test_ops_have_fake_kernels_and_refuse_the_cpu() -> None:
    from torch._subclasses.fake_tensor import FakeTensorMode  # pylint: disable=import-outside-toplevel

    with FakeTensorMode():
        empty = lambda *shape: torch.empty(shape, device="cuda")  # noqa: E731
        x = torch.ops.gance.lpips_input(empty(2, 3, 128, 128), empty(3), empty(3), 64)
        assert x.shape == (2, 16, 64, 64) and torch.ops.gance.lpips_input_backward(x, empty(3), 128).shape == (2, 3, 128, 128)
        y = torch.ops.gance.bias_relu(empty(2, 32, 5, 5), empty(32))
        assert y.shape == (2, 32, 5, 5) and torch.ops.gance.bias_relu_backward(y, y).shape == y.shape
        y, p = torch.ops.gance.bias_relu_pool(empty(2, 32, 10, 10), empty(32))
        assert y.shape == (2, 32, 10, 10) and p.shape == (2, 32, 5, 5) and torch.ops.gance.bias_relu_pool_backward(y, p, y).shape == y.shape
        d = torch.ops.gance.lpips_layer(y, y, empty(32))
        assert d.shape == (2,) and torch.ops.gance.lpips_layer_backward(d, y, y, empty(32)).shape == y.shape
        assert torch.ops.gance.lpips_normalize(y).shape == y.shape
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.gance.bias_relu(torch.zeros(1, 16, 4, 4), torch.zeros(16))  # no CPU implementation


def test_callable_refuses_bad_sides_and_a_missing_gpu() -> None:
    weights = lpips.random_lpips_weights(0)
    for side in (100, 48, 0, 2048):
        with pytest.raises(ValueError, match="side"):
            lpips.VGG16Lpips(weights, side=side)
    bad = weights._replace(lins=(weights.lins[0][:-1],) + weights.lins[1:])
    with pytest.raises(ValueError, match="lin0"):
        lpips.VGG16Lpips(bad, side=64)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lpips.VGG16Lpips(weights, side=64)


# ---- the flip condition of the GPU file's whole-chain inputs, on the reference alone ----


@pytest.mark.parametrize("seed, resolution", [(seed, resolution) for seed in lpips_ref.CHAIN_SEEDS for resolution in lpips_ref.CHAIN_RESOLUTIONS])
def test_float32_restatement_meets_the_flip_condition(seed: int, resolution: int) -> None:
    for sample in range(max(lpips_ref.CHAIN_BATCHES)):
        figures = lpips_ref.sample_yardstick(seed, resolution, sample)  # asserts the count and the magnitudes, prints the count
        own_distance = grad_ref.relative_error(figures["distance32"], figures["distance64"])
        own_gradient = grad_ref.relative_error(figures["gradient32"], figures["gradient64"])
        print(f"seed {seed} R {resolution} sample {sample}: float32 own error {own_distance:.3e} on the distance, {own_gradient:.3e} on the image gradient")
        assert 0 < own_gradient < 1e-4 and own_distance < 1e-5 and float(figures["distance64"]) > 0
    # the cap is on the whole input: the B = 2 case holds both samples (and the B = 1 case is its first)
    for batch in lpips_ref.CHAIN_BATCHES:
        lpips_ref.gradient_yardstick(seed, resolution, batch)
