"""
GPU tests of the projector (gance_amd/stylegan2/projector.py) and the writer (gance_amd/projection/projector_file_writer.py):
one whole step against the float64 restatement of tests/projection_ref.py, convergence of a short run, the distance hook,
and video -> projection file -> reader end to end.

One step: the loss and every gradient against the float64 step that takes the leaky ReLU slope signs of the run under test
(tests/grad_ref.py says why: at most 8 flips, each below 1e-4 of its layer's maximum). The bar is
grad_ref.GRADIENT_BAR_FACTOR = 8 times the error of the same restatement in float32 on the CPU, per dlatent row and per plane.

Convergence is a condition, not a measurement: per frame the final distance of w alone is at most 0.5 x the step-0 distance.
The float64 restatement of exactly this run (projection_ref.run_projection, 16^2, make_stress_variables(16, seed=3), 100 steps,
seed 0, this module's targets) ends at the ratios recorded in CONVERGENCE_RESTATEMENT below; the GPU's figures are printed beside them.
"""

from pathlib import Path
from typing import List

import numpy as np
import pytest
import torch

import grad_ref
import projection_ref
from grad_ref import cuda
from gance_amd import network_file
from gance_amd.network_interface.network_functions import LoadedNetwork
from gance_amd.projection import projection_file_reader as reader_module
from gance_amd.projection import projection_visualization
from gance_amd.projection.projector_file_writer import project_video_to_file
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.stylegan2.projector import Projector
from gance_amd.video.mjpeg_avi import MjpegAviWriter

pytestmark = pytest.mark.gpu

# The float64 restatement of the convergence run on the CPU (projection_ref.run_projection, 74 s): distance of w alone
# 0.01976915 -> 0.00321091 and 0.0123798 -> 0.00236093, regulariser sums 0.1327 -> 1.06e-6 and 0.0671 -> 1.04e-5.
# On one MI355X the run under test ends at 0.16242 x and 0.19071 x with the same sums to five digits.
CONVERGENCE_RESTATEMENT = (0.16242027, 0.19070792)  # final / step-0 distance per frame


def _step_inputs(variables, resolution: int, fmap_base: int, seed: int):  # type: ignore[no-untyped-def]
    rng = np.random.RandomState(seed)
    spec = sg2_spec.make_spec(resolution, fmap_base)
    w = rng.randn(2, 1, 512).astype(np.float32)
    planes = [rng.randn(2, 1, 1 << conv.res_log2, 1 << conv.res_log2).astype(np.float32) for conv in spec.convs]
    ramp = np.linspace(0.0, 1.0, resolution)
    smooth = 96.0 + 64.0 * np.sin(4.0 * ramp)[None, :, None, None] + 48.0 * ramp[None, None, :, None]
    targets = np.clip(smooth + 24.0 * rng.randn(2, resolution, resolution, 3), 0, 255).astype(np.uint8)
    return w, planes, targets


@pytest.mark.parametrize("resolution, fmap_base", [(16, sg2_spec.FMAP_BASE), (64, sg2_spec.FMAP_BASE_CONFIG_E)], ids=["16-f", "64-e"])
def test_one_whole_step(resolution: int, fmap_base: int) -> None:
    variables = sg2_spec.make_stress_variables(resolution, seed=3, fmap_base=fmap_base)  # (a random-init network has noise strength 0)
    w, planes, targets = _step_inputs(variables, resolution, fmap_base, seed=resolution)

    projector = Projector(num_steps=10)
    projector.set_network((variables, resolution))
    projector.start(targets)
    projector.set_variables(cuda(w), [cuda(plane) for plane in planes])
    leaf_w, leaf_planes = projector.variables
    assert all(leaf.requires_grad and leaf.is_leaf for leaf in (leaf_w, *leaf_planes))
    activations: List[torch.Tensor] = []
    _, distance, regularizer = projector.loss_terms(collect=activations)
    loss = (distance + projector.regularize_noise_weight * regularizer).sum()
    grads = torch.autograd.grad(loss, [leaf_w, *leaf_planes])

    plain64 = projection_ref.projector_step(variables, resolution, w, planes, targets, torch.float64, fmap_base)
    want64 = projection_ref.projector_step(
        variables, resolution, w, planes, targets, torch.float64, fmap_base, signs=projection_ref.check_signs(activations, plain64.activations, "the run")
    )
    own32 = projection_ref.projector_step(variables, resolution, w, planes, targets, torch.float32, fmap_base)
    own64 = projection_ref.projector_step(
        variables, resolution, w, planes, targets, torch.float64, fmap_base,
        signs=projection_ref.check_signs(own32.activations, plain64.activations, "the float32 restatement"),
    )
    failures = []

    def bar(what: str, error: float, own: float) -> None:
        limit = grad_ref.GRADIENT_BAR_FACTOR * own
        print(f"step {resolution}: {what}: error {error:.3e}, float32 restatement {own:.3e}, ratio {error / own if own else float('inf'):.2f}")
        if not (np.isfinite(error) and error <= limit):
            failures.append(f"{what}: {error:.3e} > {limit:.3e}")

    def scalar_error(got, want) -> float:  # type: ignore[no-untyped-def]
        return abs(float(got.detach()) - float(want)) / abs(float(want))

    bar("loss", scalar_error(loss, want64.loss), scalar_error(own32.loss, own64.loss))
    for index in range(2):
        bar(f"distance[{index}]", scalar_error(distance[index], want64.distance[index]), scalar_error(own32.distance[index], own64.distance[index]))
        bar(f"regulariser[{index}]", scalar_error(regularizer[index], want64.regularizer[index]), scalar_error(own32.regularizer[index], own64.regularizer[index]))
    bar("grad_w, worst row", projection_ref.sample_error(grads[0], want64.grad_w), projection_ref.sample_error(own32.grad_w, own64.grad_w))
    for layer, (got, want, mine32, mine64) in enumerate(zip(grads[1:], want64.grad_planes, own32.grad_planes, own64.grad_planes)):
        bar(f"grad_plane {layer}, worst sample", projection_ref.sample_error(got, want), projection_ref.sample_error(mine32, mine64))
    assert not failures, "; ".join(failures)


@pytest.fixture(scope="module")
def stress16():  # type: ignore[no-untyped-def]
    variables = sg2_spec.make_stress_variables(16, seed=3)
    return variables, projection_ref.convergence_targets(variables, 16)


def _run(projector: Projector, targets: np.ndarray):  # type: ignore[no-untyped-def]
    """(step-0 distance of w alone, final distance of w alone, step-0 regulariser sum, final one), each [B] on the host."""
    projector.start(targets)
    with torch.no_grad():
        _, distance0, regularizer0 = projector.loss_terms()
    while projector.get_cur_step() < projector.num_steps:
        projector.step()
    with torch.no_grad():
        _, distance1, regularizer1 = projector.loss_terms()
    return distance0.cpu().numpy(), distance1.cpu().numpy(), regularizer0.cpu().numpy(), regularizer1.cpu().numpy()


def test_convergence(stress16) -> None:  # type: ignore[no-untyped-def]
    variables, targets = stress16
    projector = Projector(num_steps=100, seed=0)
    projector.set_network((variables, 16))
    distance0, distance1, regularizer0, regularizer1 = _run(projector, targets)
    print(f"convergence 16^2 B=2 100 steps: distance {distance0} -> {distance1} (x {distance1 / distance0}, float64 restatement x {CONVERGENCE_RESTATEMENT}); "
          f"regulariser sum {regularizer0} -> {regularizer1}")
    assert projector.get_cur_step() == 100
    assert np.all(distance1 <= 0.5 * distance0), (distance0, distance1)
    assert np.all(regularizer1 < regularizer0), (regularizer0, regularizer1)
    for plane in projector.get_noises():
        assert np.abs(plane.mean(axis=(1, 2, 3))).max() < 1e-5
        assert np.abs(np.sqrt((plane.astype(np.float64) ** 2).mean(axis=(1, 2, 3))) - 1.0).max() < 1e-5
    dlatents = projector.get_dlatents()
    assert dlatents.shape == (2, 6, 512) and np.array_equal(dlatents[:, 0], dlatents[:, 5])
    assert projector.get_images().shape == (2, 3, 16, 16)
    assert [noise.shape for noise in projector.get_noises()] == [(2, 1, side, side) for side in (4, 8, 8, 16, 16)]


def test_distance_hook(stress16) -> None:  # type: ignore[no-untyped-def]
    variables, targets = stress16
    calls = []

    def mse(images: torch.Tensor, targets_u8: torch.Tensor) -> torch.Tensor:
        assert images.shape == (2, 3, 16, 16) and targets_u8.shape == (2, 16, 16, 3) and targets_u8.dtype == torch.uint8
        calls.append(1)
        want = targets_u8.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0
        return ((images - want) ** 2).mean(dim=(1, 2, 3))

    projector = Projector(num_steps=40, distance=mse, seed=0)
    projector.set_network((variables, 16))
    distance0, distance1, _, _ = _run(projector, targets)
    print(f"hook (MSE) 16^2 40 steps: {distance0} -> {distance1}")
    assert len(calls) == 42 and np.all(distance1 < distance0)


def test_noise_planes_keep_their_identity(stress16) -> None:  # type: ignore[no-untyped-def]
    """A plane that requires grad reaches the op as itself: its .grad is filled by a backward through DifferentiableSynthesis."""
    from gance_amd.stylegan2.differentiable import DifferentiableSynthesis  # pylint: disable=import-outside-toplevel

    variables, _ = stress16
    synthesis = DifferentiableSynthesis(variables, 16, device=0)
    plane = torch.randn((1, 1, 8, 8), device="cuda", requires_grad=True)
    conv = synthesis.convs[1]
    assert synthesis._noise(conv, {conv.layer_idx: plane}, 2) is plane  # pylint: disable=protected-access
    image = synthesis(torch.zeros((2, synthesis.num_layers, 512), device="cuda"), noise={conv.layer_idx: plane})
    image.square().sum().backward()
    assert plane.grad is not None and float(plane.grad.abs().max()) > 0


def test_video_to_projection_file(tmp_path: Path) -> None:
    side, steps = 32, 20
    network_path, video_path, projection_path = tmp_path / "network.pkl", tmp_path / "frames.avi", tmp_path / "projection.npz"
    network_file.write_random_network(network_path, side, seed=5)
    network = LoadedNetwork(network_path, max_batch=4)
    try:
        dlatents = np.random.RandomState(6).randn(3, 1, 512).astype(np.float32).repeat(network.engine.num_layers, axis=1)
        frames = network.create_images_matrix(dlatents)
        data, offsets = torch.ops.gance.jpeg_encode(torch.from_numpy(frames).cuda(), 95)
        data, offsets = data.cpu().numpy(), offsets.cpu().numpy()
        with MjpegAviWriter(video_path, side, 30.0) as writer:
            for index in range(3):
                writer.add_frame(data[offsets[index] : offsets[index + 1]].tobytes())

        project_video_to_file(video_path, network_path, projection_path, steps_per_projection=steps, frames_per_batch=2)

        with reader_module.ProjectionFileReader(projection_path) as reader:
            attributes = reader.projection_attributes
            assert attributes.complete is True and attributes.steps_in_projection == steps
            assert attributes.projection_frame_count == 3 and attributes.original_frame_count == 3
            assert attributes.original_fps == 30.0 and attributes.projection_fps == 30.0
            assert list(attributes.original_width_height) == [side, side] and list(attributes.projection_width_height) == [side, side]
            assert attributes.original_target_path == str(video_path) and attributes.original_network_path == str(network_path)
            assert len(attributes.target_md5_hash) == 32 and len(attributes.network_md5_hash) == 32
            assert [list(shape) for shape in attributes.noises_shapes] == [[1, 1, s, s] for s in (4, 8, 8, 16, 16, 32, 32)]
            assert attributes.latents_histories_enabled is True
            latents = np.stack(list(reader.final_latents))
            finals, targets = np.stack(list(reader.final_images)), np.stack(list(reader.target_images))
            histories = [np.stack(list(history)) for history in reader.latents_histories]
        assert latents.shape == (3, network.engine.num_layers, 512) and finals.shape == targets.shape == (3, side, side, 3)
        assert [history.shape for history in histories] == [(steps, network.engine.num_layers, 512)] * 3
        assert all(np.array_equal(history[-1], latents[index]) for index, history in enumerate(histories))
        assert np.abs(targets.astype(int) - frames.astype(int)).mean() < 4.0  # the JPEG's loss only
        reader_module.verify_projection_file_assumptions(projection_path)
        # a random-init network's noise strengths are zero: the engine's image of the stored latents IS the image with the optimised planes
        engine_images = network.create_images_matrix(latents)
        assert np.abs(finals.astype(int) - engine_images.astype(int)).max() <= 1
    finally:
        network.stop()
    chunks = list(projection_visualization.final_latents_frame_chunks(projection_path, video_height=128, chunk_frames=2))
    assert [first for first, _ in chunks] == [0, 2] and sum(int(chunk.shape[0]) for _, chunk in chunks) == 3
    assert all(chunk.dtype == torch.uint8 and chunk.is_cuda for _, chunk in chunks)
