"""
CPU tests of projection (gance_amd/csrc/projection.hip, the noise gradient of synthesis_grad.hip, the gance::noise_regularizer /
pyramid_distance / noise_bias_lrelu_backward_noise ops, gance_amd/stylegan2/projector.py and
gance_amd/projection/projector_file_writer.py): every new entry point refuses bad arguments before a device is touched,
the schedules are the published formulas, the mapping network equals the oracle's, a frame's random draws do not depend on
the batching, and the writer's file round-trips through ProjectionFileReader.
"""

import ctypes
import json
import math
from pathlib import Path
from typing import List

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import projection_ref
from gance_amd import hip_lib, torch_ops  # noqa: F401  pylint: disable=unused-import
from gance_amd.hash_file import hash_file
from gance_amd.projection import projection_file_reader as reader_module
from gance_amd.projection import projector_file_writer as writer_module
from gance_amd.stylegan2 import projector as projector_module
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.video.mjpeg_avi import MjpegAviWriter
from oracle import stylegan2_ref as ref

P = 0x1000  # a non-NULL, aligned address: never dereferenced, the checks come first


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    return hip_lib.load_library()


def _noise_backward(lib, pointers=None, noise_batch=1, batch=1, channels=16, height=4, width=4):  # type: ignore[no-untyped-def]
    grad_out, out, strength, grad_x, grad_noise = pointers or (P,) * 5
    return lib.gance_noise_bias_lrelu_backward_noise(grad_out, out, strength, noise_batch, batch, channels, height, width, grad_x, grad_noise, None)


def _regularizer_forward(lib, pointers=None, batch=1, side=16, workspace_bytes=1 << 24):  # type: ignore[no-untyped-def]
    noise, reg, means, workspace = pointers or (P,) * 4
    return lib.gance_noise_regularizer_forward(noise, batch, side, reg, means, workspace, workspace_bytes, None)


def _regularizer_backward(lib, pointers=None, batch=1, side=16, workspace_bytes=1 << 24):  # type: ignore[no-untyped-def]
    grad_reg, noise, means, workspace, grad_noise = pointers or (P,) * 5
    return lib.gance_noise_regularizer_backward(grad_reg, noise, means, workspace, workspace_bytes, batch, side, grad_noise, None)


def _distance_forward(lib, pointers=None, batch=1, side=16, workspace_bytes=1 << 24):  # type: ignore[no-untyped-def]
    image, target, dist, workspace = pointers or (P,) * 4
    return lib.gance_pyramid_distance_forward(image, target, batch, side, dist, workspace, workspace_bytes, None)


def _distance_backward(lib, pointers=None, batch=1, side=16, workspace_bytes=1 << 24):  # type: ignore[no-untyped-def]
    grad_dist, workspace, grad_image = pointers or (P,) * 3
    return lib.gance_pyramid_distance_backward(grad_dist, workspace, workspace_bytes, batch, side, grad_image, None)


# (call, required pointers, name, sides refused, the words of that refusal)
POWER_OF_TWO_ENTRY_POINTS = [
    (_regularizer_forward, 4, "gance_noise_regularizer_forward", (2, 3, 12, 24, 1000, 2048), "side must be a power of two in [4, 1024]"),
    (_regularizer_backward, 5, "gance_noise_regularizer_backward", (2, 3, 12, 24, 1000, 2048), "side must be a power of two in [4, 1024]"),
    (_distance_forward, 4, "gance_pyramid_distance_forward", (4, 12, 48, 1000, 2048), "resolution must be a power of two in [8, 1024]"),
    (_distance_backward, 3, "gance_pyramid_distance_backward", (4, 12, 48, 1000, 2048), "resolution must be a power of two in [8, 1024]"),
]


def _refused(library: ctypes.CDLL, name: str, status: int, *words: str) -> None:
    message = library.gance_last_error().decode()
    assert status == 1, message  # GANCE_ERR_INVALID_ARGUMENT
    assert message.startswith(name + ":") and all(word in message for word in words), message


def _refuses_pointers(library: ctypes.CDLL, call, pointer_count: int, name: str) -> None:  # type: ignore[no-untyped-def]
    for position in range(pointer_count):  # every required pointer: NULL, then misaligned
        pointers: List = [P] * pointer_count
        pointers[position] = None
        _refused(library, name, call(library, tuple(pointers)), "NULL pointer")
        pointers[position] = P + 2
        _refused(library, name, call(library, tuple(pointers)), "misaligned pointer")


@pytest.mark.parametrize("call, pointer_count, name, bad_sides, words", POWER_OF_TWO_ENTRY_POINTS, ids=[entry[2] for entry in POWER_OF_TWO_ENTRY_POINTS])
def test_loss_entry_points_refuse_bad_arguments(library: ctypes.CDLL, call, pointer_count: int, name: str, bad_sides, words: str) -> None:
    _refuses_pointers(library, call, pointer_count, name)
    for side in bad_sides:
        _refused(library, name, call(library, side=side), words, str(side))
    for batch in (0, -1, 65536):
        _refused(library, name, call(library, batch=batch), "batch must be in [1, 65535]", str(batch))
    _refused(library, name, call(library, workspace_bytes=16), "workspace of 16 bytes")


def test_noise_gradient_entry_point_refuses_bad_arguments(library: ctypes.CDLL) -> None:
    name = "gance_noise_bias_lrelu_backward_noise"
    _refuses_pointers(library, _noise_backward, 5, name)
    for count in (0, 8, 24, 528):
        _refused(library, name, _noise_backward(library, channels=count), "multiples of 16", str(count))
    _refused(library, name, _noise_backward(library, height=8, width=4), "square", "8 x 4")
    for side in (2, 3, 1025, 2048):
        _refused(library, name, _noise_backward(library, height=side, width=side), "side must be in [4, 1024]", str(side))
    _refused(library, name, _noise_backward(library, batch=0), "batch")
    _refused(library, name, _noise_backward(library, noise_batch=2, batch=3), "1 or 3 planes", "got 2")
    _refused(library, name, _noise_backward(library, noise_batch=0, batch=3), "1 or 3 planes")


def test_workspace_sizes(library: ctypes.CDLL) -> None:
    size = ctypes.c_uint64()

    def message() -> str:
        return library.gance_last_error().decode()

    assert library.gance_noise_regularizer_workspace_bytes(1, 16, None) == 1 and "NULL" in message()
    assert library.gance_noise_regularizer_workspace_bytes(1, 24, ctypes.byref(size)) == 1 and "power of two" in message()
    assert library.gance_noise_regularizer_workspace_bytes(0, 16, ctypes.byref(size)) == 1 and "batch" in message()
    assert library.gance_pyramid_distance_workspace_bytes(1, 4, ctypes.byref(size)) == 1 and "power of two in [8, 1024]" in message()
    assert library.gance_pyramid_distance_workspace_bytes(1, 2048, ctypes.byref(size)) == 1
    # regulariser: [B][levels][2][256] partial sums, then the pyramid's levels below the plane itself
    assert library.gance_noise_regularizer_workspace_bytes(3, 8, ctypes.byref(size)) == 0 and size.value == 3 * 1 * 2 * 256 * 4
    assert library.gance_noise_regularizer_workspace_bytes(2, 32, ctypes.byref(size)) == 0
    assert size.value == 2 * 3 * 2 * 256 * 4 + 2 * (16 * 16 + 8 * 8) * 4
    # distance: [B][3][64] tile partials, then every level of the differences: at most 4/3 * 3 * 256^2 floats per sample
    assert library.gance_pyramid_distance_workspace_bytes(2, 32, ctypes.byref(size)) == 0
    assert size.value == 2 * 3 * 64 * 4 + 2 * 3 * (32 * 32 + 16 * 16 + 8 * 8) * 4
    small = library.gance_pyramid_distance_workspace_bytes(1, 256, ctypes.byref(size)) == 0 and size.value
    assert library.gance_pyramid_distance_workspace_bytes(1, 1024, ctypes.byref(size)) == 0 and size.value == small
    assert small - 3 * 64 * 4 <= 4 * 3 * 256 * 256 * 4 // 3
    assert [hip_lib.noise_regularizer_levels(side) for side in (4, 8, 16, 64, 1024)] == [1, 1, 2, 4, 8]
    with pytest.raises(ValueError, match="power of two"):
        hip_lib.noise_regularizer_workspace_bytes(1, 48)


# ---- the schedules ----


@pytest.mark.parametrize("num_steps", [1000, 40])
def test_learning_rate_and_noise_ramps(num_steps: int) -> None:
    projector = projector_module.Projector(num_steps=num_steps)
    projector.dlatent_std = 2.5
    for t in (0.0, 0.025, 0.05, 0.5, 0.75, 0.9, (num_steps - 1) / num_steps):
        step = int(round(t * num_steps))
        t = step / num_steps
        ramp = min(1.0, (1.0 - t) / 0.25)
        ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
        ramp *= min(1.0, t / 0.05)
        assert projector.learning_rate(step) == pytest.approx(0.1 * ramp, rel=1e-12, abs=1e-18)
        assert projector.noise_strength(step) == pytest.approx(2.5 * 0.05 * max(0.0, 1.0 - t / 0.75) ** 2, rel=1e-12, abs=1e-18)
    assert projector.learning_rate(0) == 0.0 and projector.noise_strength(0) == pytest.approx(0.125)
    assert projector.learning_rate(num_steps // 2) == pytest.approx(0.1)
    assert projector.noise_strength(num_steps * 3 // 4) == 0.0 and projector.noise_strength(num_steps - 1) == 0.0
    assert 0.0 < projector.learning_rate(num_steps - 1) < 0.1 * 0.05
    assert (projector.dlatent_avg_samples, projector.regularize_noise_weight) == (10000, 1e5)
    assert (projector.adam_beta1, projector.adam_beta2, projector.adam_epsilon) == (0.9, 0.999, 1e-8)


def test_mapping_dlatents_is_g_mapping() -> None:
    variables = sg2_spec.make_random_variables(8, seed=4, perturb=True)
    z = torch.from_numpy(np.random.RandomState(5).randn(7, 512).astype(np.float32))
    got = projector_module.mapping_dlatents(variables, z)
    assert got.shape == (7, 512) and got.dtype == torch.float32
    assert torch.allclose(got, ref.g_mapping(z, variables, 3)[:, 0], rtol=0.0, atol=0.0)  # the same operations in the same order
    want = ref.g_mapping(z.double(), variables, 1)[:, 0]
    assert float((got.double() - want).abs().max() / want.abs().max()) < 1e-5
    assert projector_module.mapping_dlatents(variables, z.double()).dtype == torch.float64


def test_frame_draws_do_not_depend_on_the_batching() -> None:
    sides = (4, 8, 8, 16, 16)

    def frames(first: int, count: int) -> List[projector_module.FrameDraws]:
        return [projector_module.frame_draws(9, first + index, 12, sides) for index in range(count)]

    whole, cut = frames(0, 3), frames(0, 1) + frames(1, 2)
    for one, other in zip(whole, cut):
        assert np.array_equal(one.w_noise, other.w_noise) and one.w_noise.shape == (12, 512) and one.w_noise.dtype == np.float32
        assert [plane.shape for plane in one.planes] == [(1, side, side) for side in sides]
        assert all(np.array_equal(a, b) for a, b in zip(one.planes, other.planes))
    assert not np.array_equal(whole[0].w_noise, whole[1].w_noise)
    assert not np.array_equal(whole[0].w_noise, projector_module.frame_draws(10, 0, 12, sides).w_noise)


# ---- the writer ----


class StubProjector:
    """The projector's surface without a network: frame k of the run ends at latents full of k + 1."""

    def __init__(self, num_steps: int) -> None:
        self.num_steps = num_steps
        self.started: List[int] = []
        self._step, self._frames, self._first = 0, 0, 0

    def start(self, targets) -> None:  # type: ignore[no-untyped-def]
        self._first += self._frames
        self._frames, self._step = int(targets.shape[0]), 0
        self.started.append(self._frames)

    def step(self) -> None:
        self._step += 1

    def get_cur_step(self) -> int:
        return self._step

    def get_dlatents(self) -> np.ndarray:
        rows = np.arange(self._first, self._first + self._frames, dtype=np.float32) + 1.0
        return np.broadcast_to((rows * self._step / self.num_steps)[:, None, None], (self._frames, 18, 512)).copy()

    def get_noises(self) -> List[np.ndarray]:
        return [np.zeros((self._frames, 1, side, side), dtype=np.float32) for side in (4, 8, 8)]


def _attributes(tmp_path: Path) -> dict:
    video, network = tmp_path / "video.avi", tmp_path / "network.pkl"
    video.write_bytes(b"video bytes")
    network.write_bytes(b"network bytes")
    return {
        "version_number": 2, "original_target_path": str(video), "original_width_height": [48, 48], "projection_width_height": [32, 32],
        "target_md5_hash": hash_file(video), "original_network_path": str(network), "network_md5_hash": hash_file(network),
        "steps_in_projection": 5, "noises_histories_enabled": False, "images_histories_enabled": False, "original_fps": 30.0,
        "projection_fps": 15.0, "original_frame_count": 6, "projection_frame_count": 3,
    }


def test_writer_reader_round_trip_with_a_stub_projector(tmp_path: Path) -> None:
    path = tmp_path / "projection.npz"
    attributes = _attributes(tmp_path)
    targets = np.random.RandomState(0).randint(0, 256, size=(3, 32, 32, 3)).astype(np.uint8)
    seen_incomplete = []

    def batches():  # type: ignore[no-untyped-def]
        yield targets[:2]
        with reader_module.ProjectionFileReader(path) as partial:  # the file after the first batch
            seen_incomplete.append((partial.projection_attributes.complete, len(list(partial.final_latents)), list(partial.target_images)))
        yield targets[2:]

    projector = StubProjector(5)
    count = writer_module.project_batches_to_file(batches(), projector, path, attributes, True, final_images_of=lambda p: 255 - targets[p._first : p._first + p._frames])
    assert count == 3 and projector.started == [2, 1]
    assert seen_incomplete == [(False, 2, [])]
    assert not list(tmp_path.glob("*.partial*"))

    with reader_module.ProjectionFileReader(path) as reader:
        got = reader.projection_attributes
        assert got.complete is True
        for key, value in attributes.items():
            stored = getattr(got, key)
            assert (list(stored) if isinstance(value, list) else stored) == value, key
        assert got.target_md5_hash == hash_file(tmp_path / "video.avi") and got.network_md5_hash == hash_file(tmp_path / "network.pkl")
        assert got.latents_histories_enabled is True
        assert [list(shape) for shape in got.noises_shapes] == [[1, 1, 4, 4], [1, 1, 8, 8], [1, 1, 8, 8]]
        latents = list(reader.final_latents)
        assert [matrix.shape for matrix in latents] == [(18, 512)] * 3
        assert [float(matrix[0, 0]) for matrix in latents] == [1.0, 2.0, 3.0]
        assert np.array_equal(np.stack(list(reader.target_images)), targets) and np.stack(list(reader.final_images)).dtype == np.uint8
        assert np.array_equal(np.stack(list(reader.final_images)), 255 - targets)
        histories = [np.stack(list(history)) for history in reader.latents_histories]
        assert [history.shape for history in histories] == [(5, 18, 512)] * 3
        assert np.allclose(histories[2][:, 0, 0], 3.0 * np.arange(1, 6) / 5)
        label = reader_module.final_latents_matrices_label(reader)
        assert label.data.shape == (18, 3 * 512) and "video.avi" in label.label
    reader_module.verify_projection_file_assumptions(path)
    assert json.loads(str(np.load(str(path))["attributes"]))["complete"] is True

    # histories are ragged-safe: frames with different step counts, and none at all
    ragged = tmp_path / "ragged.npz"
    writer_module.write_projection_npz_with_attributes(
        ragged, {**attributes, "complete": True, "latents_histories_enabled": True},
        {"final_latents": np.zeros((2, 18, 512), np.float32), "latents_histories_0": np.zeros((3, 18, 512), np.float32), "latents_histories_1": np.zeros((5, 18, 512), np.float32)},
    )
    with reader_module.ProjectionFileReader(ragged) as reader:
        assert [len(list(history)) for history in reader.latents_histories] == [3, 5]
    without = tmp_path / "without.npz"
    writer_module.project_batches_to_file([targets[:1]], StubProjector(2), without, attributes, False, final_images_of=lambda p: targets[:1])
    with reader_module.ProjectionFileReader(without) as reader:
        assert not list(reader.latents_histories) and reader.projection_attributes.latents_histories_enabled is False


def test_writer_refusals(tmp_path: Path) -> None:
    video, network = tmp_path / "wide.avi", tmp_path / "network.pkl"
    with MjpegAviWriter(video, 32, 30.0, width=48, height=32) as writer:
        writer.add_frame(b"\xff\xd8\xff\xd9")  # never decoded: the headers say 48 x 32
    network.write_bytes(b"")
    with pytest.raises(NotImplementedError, match="no HDF5 writer.*h5py is absent"):
        writer_module.project_video_to_file(video, network, tmp_path / "projection.hdf5")
    with pytest.raises(NotImplementedError, match="noises_histories_enabled"):
        writer_module.project_video_to_file(video, network, tmp_path / "projection.npz", noises_histories_enabled=True)
    with pytest.raises(NotImplementedError, match="images_histories_enabled"):
        writer_module.project_video_to_file(video, network, tmp_path / "projection.npz", images_histories_enabled=True)
    with pytest.raises(ValueError, match="must be square.*48 x 32"):
        writer_module.project_video_to_file(video, network, tmp_path / "projection.npz")
    with pytest.raises(ValueError, match="Couldn't read input video"):
        writer_module.project_video_to_file(network, network, tmp_path / "projection.npz")
    assert not (tmp_path / "projection.npz").exists()


# ---- the ops ----


def test_ops_have_fake_tensor_registrations_and_the_right_shapes() -> None:
    with FakeTensorMode():
        def empty(*shape: int) -> torch.Tensor:
            return torch.empty(shape, dtype=torch.float32, device="cuda")

        out = empty(3, 32, 8, 8)
        for noise_batch in (1, 3):
            grad_x, grad_noise = torch.ops.gance.noise_bias_lrelu_backward_noise(out, out, empty(1), noise_batch)
            assert grad_x.shape == out.shape and grad_noise.shape == (noise_batch, 1, 8, 8) and grad_noise.dtype == torch.float32
        planes = empty(3, 1, 64, 64)
        reg = torch.ops.gance.noise_regularizer(planes)
        assert reg.shape == (3,) and reg.dtype == torch.float32 and reg.device.type == "cuda"
        assert torch.ops.gance.noise_regularizer_backward(reg, planes).shape == planes.shape
        image, target = empty(2, 3, 512, 512), empty(2, 3, 256, 256)
        dist = torch.ops.gance.pyramid_distance(image, target)
        assert dist.shape == (2,) and dist.dtype == torch.float32
        assert torch.ops.gance.pyramid_distance_backward(dist, image, target).shape == image.shape
    for op in (torch_ops.noise_regularizer, torch_ops.pyramid_distance, torch_ops.noise_bias_lrelu):
        assert op._backward_fn is not None  # pylint: disable=protected-access


# ---- the restatements themselves ----


def test_restatements_against_hand_computed_values() -> None:
    plane = torch.arange(16, dtype=torch.float64).reshape(1, 1, 4, 4)
    along_w = sum(float(plane[0, 0, y, x] * plane[0, 0, y, (x - 1) % 4]) for y in range(4) for x in range(4)) / 16
    along_h = sum(float(plane[0, 0, y, x] * plane[0, 0, (y - 1) % 4, x]) for y in range(4) for x in range(4)) / 16
    assert float(projection_ref.noise_regularizer(plane)) == pytest.approx(along_w ** 2 + along_h ** 2)
    assert len(projection_ref.noise_regularizer(torch.zeros(2, 1, 1024, 1024))) == 2
    image = torch.full((1, 3, 16, 16), 0.2, dtype=torch.float64)
    target = torch.full((1, 3, 16, 16), 102.0, dtype=torch.float64)  # (0.2 + 1) * 127.5 = 153: d = 0.2 at both levels
    assert float(projection_ref.pyramid_distance(image, target)) == pytest.approx(2 * 0.2 ** 2)
    big = torch.full((1, 3, 512, 512), 0.2, dtype=torch.float64)
    assert float(projection_ref.pyramid_distance(big, torch.full((1, 3, 256, 256), 102.0, dtype=torch.float64))) == pytest.approx(6 * 0.2 ** 2)
