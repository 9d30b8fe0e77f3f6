"""
Config-e generators (fmap_base = 8 << 10) on the GPU, against the fp64 oracle (oracle/stylegan2_ref.py takes every shape from the
variables, so it runs config-e unchanged).

  * Whole chain at 64^2 (the smallest network where the configs differ: 512 -> 256 / 256 -> 256) and at 256^2 (adds 256 -> 128,
    128 -> 128, 128 -> 64, 64 -> 64), every-term and stress networks, 1 / 3 / 16 frames per call (the kernel form is a function of
    the batch: the launch names must differ between the batches), float image and bytes, on the w entry (Engine.synthesize_w) and
    the z entry (LoadedNetwork.create_images_vector on a file written by write_random_network(fmap_base=8 << 10)).
  * The 512^2 and 1024^2 layers of the 1024^2 network IN ISOLATION, by the method of tests/test_isolated_layers_gpu.py: the
    layer's own input as the kernels left it (debug_activation_after(n - 1)), promoted to fp64, through ONE oracle layer, against
    debug_activation_after(n), for conv layers 14 ... 17 (1-based): 64 -> 32 up and 32 -> 32 at 512^2 (channel shapes config-f has
    at 1024^2, at half the side), 32 -> 16 up and 16 -> 16 at 1024^2 (conv16_mfma.hip: stride-1 and transposed tiles on
    v_mfma_f32_16x16x4_f32; upfir16_fused.hip with one channel tile and four chunks). Batches 1, 3 and the smallest batch at which
    the plan runs the 32 -> 16 up layer as one fused launch (read from gance_engine_describe_plan for the device's CU count);
    conv_form "auto" / "direct", up_form "auto" / "split"; every-term and stress networks, and the every-term network with a noise
    plane per sample at strength 0.5 (the method of tests/test_isolated_noise_gpu.py, planes read back with debug_noise).
    A tile seam or an image edge handled wrongly is an error of order 1 here. And 17 frames, every-term and loud networks, conv
    layers 14 and 15 only: the one batch at which the default plan on 256 CUs runs the 64 -> 32 up layer in the pair form of the
    fused up kernel (convTFp13_512x512_64->32/16x, between convV12+rgb and convV14+rgb; at 16 and at 18 frames it is "/s3").
    tests/test_isolated_coverage.py holds these batches against the planner (LARGE_CASES of tests/isolated_config_e_cases.py).
  * conv_form "winograd" / "winograd43" on the 512^2 network, 2 frames: the smallest network with a 32-channel last layer, which
    those forms end in convW14+rgb / convV14+rgb and torgb_512x512 (measured: image error 7.8e-6 / 8.6e-6).
  * The frame-emitting launch (conv16+torgb_1024x1024_16->16: conv, ToRGB 16 -> 3, + upsampled 512^2 image + bias, uint8) by the
    method of tests/test_isolated_image_gpu.py: layer 17's activation (tap: the unfused launch) and debug_image_after of the 512^2
    stage through ONE fp64 torgb_layer against the float image of a whole untapped call; ceilings 2e-5 / 1e-4 (stress) and
    FP32_MARGIN = 4 x the float32 oracle step's own error; the call's bytes equal convert_images_to_uint8 of its float image
    exactly; three bytes-only calls return those bytes; more than 30 % of them unsaturated on the every-term network (dlatent seeds
    chosen on the float32 CPU oracle: SEEDS).
  * A MultiNetwork holding a config-e and a config-f network at 64^2: a 12-frame stream alternating between them is bit-equal,
    frame by frame, to each network's own engine at the same call size (the two must not share an activation workspace).

Measured on an MI355X (256 CUs), every configuration below; the inputs are seeded. Isolated error: the 16-channel layers (32 -> 16
up as convTF15/16 and as convT15 + fir15, 16 -> 16 as conv16) 2.5e-7 ... 1.1e-6; 64 -> 32 up at 512^2 (convT13, /s3) 2.7e-7 ... 5.9e-7;
32 -> 32 at 512^2 direct 5.4e-7 ... 1.6e-6, F(4x4,3x3) 8.9e-7 ... 4.0e-6; sensitivity to another sample's plane 0.28 ... 0.65.
The frame-emitting launch: 1.6e-7 ... 2.1e-7, 0.64 ... 1.32 times the float32 oracle step's error; bytes exact; 38.6 % ... 66.5 % of
them unsaturated. On 256 CUs the 32 -> 16 up layer is one fused launch from 2 frames per call. The 17-frame rows: convTFp13/16x
2.6e-7 ... 3.8e-7, convV14+rgb behind it 1.1e-6 ... 4.7e-6, sensitivity 0.27 ... 0.38.

Bars are the project's: 2e-5 per layer in isolation, 1e-4 on the stress network, 1e-4 on the whole-chain float image, bytes within
1 LSB on fewer than 1e-3 of them (tests/test_synthesis_gpu.py).
"""

import ctypes
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from gance_amd import hip_lib, network_file
from gance_amd.network_interface import network_functions
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref
from test_isolated_noise_gpu import with_other_plane

pytestmark = pytest.mark.gpu

CONFIG_E = 8 << 10
LARGE = 1024
TOLERANCE = 2e-5
STRESS_TOLERANCE = 1e-4
IMAGE_TOLERANCE = 1e-4
FP32_MARGIN = 4.0
MIN_UNSATURATED = 0.3
SENSITIVITY = 0.1
NOISE_SEED = 23
BATCHES = (1, 3, 16)
# rows of the 16 latents that go through the fp64 oracle (most of these tests' time): every row of the 1- and 3-frame calls, the
# first three and the last of the 16-frame call (its kernels take one sample per block or GEMM column range: the ends of the batch)
ORACLE_ROWS = [0, 1, 2, 15]
FIRST_LAYER = 14  # conv layers 14 ... 17 (1-based): Conv0_up / Conv1 of 512^2 and 1024^2
UP_16 = "convTF15_1024x1024_32->16/16"
# 17 frames: the one batch at which the default plan on 256 CUs runs the 64 -> 32 up layer in the pair form of the fused up kernel
# (layers 9, 11 and 13 leave "/s3" for "/16x" at exactly 17 frames: tests/isolated_config_e_cases.py). Only conv layers 14 and 15
# (1-based) are checked there: the 1024^2 layers keep their one form from 2 frames up, and their 17-frame activations are over a
# gigabyte each to read back.
PAIR_FORM_BATCH = 17
PAIR_FORM_LAST_LAYER = 15
UP_32_PAIR_FORM = "convTFp13_512x512_64->32/16x"
LAST = "conv16+torgb_1024x1024_16->16"

# dlatents = RandomState(seed).randn(batch, 18, 512) of the frame-emitting checks on the every-term 1024^2 network: batch -> the
# first seed from 11 + batch up whose frames the float32 CPU oracle leaves at least 35 % unsaturated (stress network: 11 + batch)
SEEDS = {
    1: 15,  # 66.5 % (seeds 12, 13, 14: 24.9 %, 32.5 %, 17.6 %)
    2: 14,  # 38.6 % (seed 13: 34.1 %)
    3: 15,  # 51.4 % (seed 14: 33.4 %)
}


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    knobs = sorted(key for key in os.environ if key.startswith("GANCE_TUNE_"))
    if knobs:
        pytest.fail(f"{', '.join(knobs)} set: these checks are of the forms the product selects by itself; unset every GANCE_TUNE_* variable")
    return hip_lib.load_library()


def _rel(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.abs(got - want).max() / np.abs(want).max())


def _conv_launches(engine) -> dict:
    """{layer_idx: launch name} of the conv launches of the engine's last call (profiling on)."""
    names = {}
    for step in engine.steps():
        if step.name.startswith("conv"):
            kind = step.name.split("_")[0]
            names[int("".join(ch for ch in kind.split("+")[0] if ch.isdigit()))] = step.name
    return names


_VARIABLES: dict = {}


def _variables(network: str, resolution: int) -> dict:
    """The config-e generators, made once per session. "loud": the every-term one with noise_strength = 0.5 * (-1) ** layer_idx."""
    key = (network, resolution)
    if key not in _VARIABLES:
        if network == "stress":
            _VARIABLES[key] = sg2_spec.make_stress_variables(resolution, seed=0, fmap_base=CONFIG_E)
        else:
            variables = dict(sg2_spec.make_random_variables(resolution, seed=3, perturb=True, fmap_base=CONFIG_E))
            if network == "loud":
                for conv in sg2_spec.make_spec(resolution, fmap_base=CONFIG_E).convs:
                    name = f"G_synthesis/{conv.scope}/noise_strength"
                    variables[name] = np.full_like(variables[name], 0.5 * (-1) ** conv.layer_idx)
            _VARIABLES[key] = variables
    return _VARIABLES[key]


def _check_frames(frames: np.ndarray, image: np.ndarray, want: torch.Tensor, stress: bool, where: str) -> None:
    want_np = want.numpy()
    assert image.shape == want_np.shape and np.isfinite(image).all(), where
    err = float(np.abs(image - want_np).max())
    scale = float(np.abs(want_np).max()) if stress else 1.0  # (the stress network's bar is relative to the image range)
    print(f"  {where}: max|image - oracle| = {err:.2e}" + (f" on a range of {scale:.2f}" if stress else ""))
    assert err < IMAGE_TOLERANCE * scale, f"{where}: max |image - oracle| = {err} (range {scale})"
    want_u8 = ref.convert_images_to_uint8(want)
    assert frames.shape == want_u8.shape and frames.dtype == np.uint8, where
    diff = np.abs(frames.astype(np.int16) - want_u8.astype(np.int16))
    assert int(diff.max()) <= 1 and float((diff > 0).mean()) < 1e-3, f"{where}: bytes differ by {int(diff.max())} LSB on {float((diff > 0).mean()):.2e}"


# ---- the whole chain ----


@pytest.mark.parametrize("network", ["every_term", "stress"])
@pytest.mark.parametrize("resolution", [64, 256])
def test_whole_chain_matches_oracle_on_the_w_entry(library, resolution: int, network: str) -> None:
    spec = sg2_spec.make_spec(resolution, fmap_base=CONFIG_E)
    variables = _variables(network, resolution)
    dlatents = np.random.RandomState(7).randn(max(BATCHES), spec.num_layers, 512).astype(np.float32)
    want = ref.synthesize_w(dlatents[ORACLE_ROWS], variables, resolution)  # (once, shared by the three calls)
    launches = {}
    print(f"\nconfig-e {network} network {resolution}^2, w entry:")
    engine = hip_lib.Engine(variables, resolution, max_batch=max(BATCHES), profile=True)
    try:
        assert engine.fmap_base == CONFIG_E
        for batch in BATCHES:
            frames, image = engine.synthesize_w(dlatents[:batch], want_float=True)
            launches[batch] = _conv_launches(engine)
            rows = [i for i, s in enumerate(ORACLE_ROWS) if s < batch]
            checked = [ORACLE_ROWS[i] for i in rows]
            assert np.isfinite(image).all()
            _check_frames(frames[checked], image[checked], want[rows], network == "stress", f"{batch} frames")
    finally:
        engine.close()
    for batch in BATCHES:
        for conv in spec.convs:
            side = 2 ** conv.res_log2
            assert launches[batch][conv.layer_idx].split("/")[0].endswith(f"_{side}x{side}_{conv.cin}->{conv.cout}"), launches[batch]
    assert len({tuple(sorted(names.items())) for names in launches.values()}) >= 2, f"one set of kernel forms at every batch: {launches[1]}"


@pytest.mark.parametrize("resolution", [64, 256])
def test_whole_chain_matches_oracle_on_the_z_entry(library, resolution: int, tmp_path: Path) -> None:
    path = tmp_path / "config_e.pkl"
    network_file.write_random_network(path, resolution, seed=2, fmap_base=CONFIG_E)
    variables = sg2_spec.make_random_variables(resolution, seed=2, fmap_base=CONFIG_E)
    z = np.random.RandomState(9).randn(max(BATCHES), 512).astype(np.float32)
    want = ref.synthesize_z(z[ORACLE_ROWS], variables, resolution, truncation_psi=network_functions.TRUNCATION_PSI)
    print(f"\nconfig-e random-init network {resolution}^2, z entry:")
    network = network_functions.LoadedNetwork(path, max_batch=max(BATCHES), device=0)
    try:
        assert network.engine.fmap_base == CONFIG_E and network.resolution == resolution
        for batch in BATCHES:
            frames = network.create_images_vector(z[:batch])
            again, image = network.engine.synthesize_z(z[:batch], truncation_psi=network_functions.TRUNCATION_PSI, want_float=True)
            assert np.array_equal(again, frames), f"{batch} frames: the engine's own z call differs from create_images_vector"
            rows = [i for i, s in enumerate(ORACLE_ROWS) if s < batch]
            checked = [ORACLE_ROWS[i] for i in rows]
            assert np.isfinite(image).all()
            _check_frames(frames[checked], image[checked], want[rows], False, f"{batch} frames")
    finally:
        network.stop()


# ---- the 32-channel last layer with a Winograd form forced (the smallest network that has one: 512^2) ----

FORCED_LAST = {"winograd": "convW14+rgb_512x512_32->32", "winograd43": "convV14+rgb_512x512_32->32"}
_FORCED_ORACLE: list = []


@pytest.mark.parametrize("conv_form", sorted(FORCED_LAST))
def test_forced_winograd_forms_end_a_512_network_in_the_epilogue_channel_sum(library, conv_form: str) -> None:
    """
    conv_form "winograd" / "winograd43" on a network whose last layer has 32 channels: that layer runs on the 16x16x4 kernel's
    32-channel geometry / in F(4x4,3x3) form with the ToRGB channel sum in its epilogue (no launch absorbs the whole ToRGB),
    the two frames against the fp64 oracle at the whole-chain bars.
    """
    resolution, batch = 512, 2
    spec = sg2_spec.make_spec(resolution, fmap_base=CONFIG_E)
    variables = _variables("every_term", resolution)
    dlatents = np.random.RandomState(7).randn(batch, spec.num_layers, 512).astype(np.float32)
    if not _FORCED_ORACLE:  # (once, shared by the two forms)
        _FORCED_ORACLE.append(ref.synthesize_w(dlatents, variables, resolution))
    engine = hip_lib.Engine(variables, resolution, max_batch=batch, conv_form=conv_form, profile=True)
    try:
        assert engine.fmap_base == CONFIG_E
        frames, image = engine.synthesize_w(dlatents, want_float=True)
        whole_call = [step.name for step in engine.steps()]
    finally:
        engine.close()
    print(f"\nconfig-e every_term network {resolution}^2, conv_form={conv_form}:")
    conv_launches = [name for name in whole_call if name.startswith("conv")]
    assert conv_launches[-1] == FORCED_LAST[conv_form] and whole_call[-1] == "torgb_512x512", whole_call[-3:]
    assert not any("+torgb" in name for name in whole_call), whole_call
    _check_frames(frames, image, _FORCED_ORACLE[0], False, f"{batch} frames")


# ---- the 512^2 and 1024^2 layers in isolation ----


def _fused_up_batch(library, num_cus: int) -> int:
    """The smallest batch whose default plan on `num_cus` CUs runs the 32 -> 16 up layer as one fused launch."""
    out = ctypes.create_string_buffer(1 << 16)
    config = hip_lib.EngineConfig(LARGE, 64, 0, hip_lib.GANCE_FLAG_FMAP_BASE_8K)
    for batch in range(1, 65):
        assert library.gance_engine_describe_plan(ctypes.byref(config), num_cus, batch, out, ctypes.c_uint64(len(out))) == 0
        if UP_16 in out.value.decode().split():
            return batch
    pytest.fail(f"no batch up to 64 runs {UP_16} on {num_cus} CUs")
    return 0


# (network, conv_form, up_form, batch; batch 0 = _fused_up_batch)
ISOLATED = [
    ("every_term", "auto", "auto", 1),
    ("every_term", "auto", "auto", 3),
    ("every_term", "auto", "auto", 0),
    ("every_term", "direct", "split", 1),
    ("every_term", "direct", "split", 3),
    ("every_term", "direct", "auto", 0),
    ("every_term", "auto", "split", 0),
    ("stress", "auto", "auto", 0),
    ("stress", "direct", "split", 3),
    ("loud", "auto", "auto", 0),
    ("loud", "direct", "split", 3),
    ("every_term", "auto", "auto", PAIR_FORM_BATCH),
    ("loud", "auto", "auto", PAIR_FORM_BATCH),
]


@pytest.mark.parametrize("network,conv_form,up_form,batch", ISOLATED, ids=[f"{n}-{c}-{u}-{b or 'fused'}" for n, c, u, b in ISOLATED])
def test_layers_512_and_1024_in_isolation(library, network: str, conv_form: str, up_form: str, batch: int) -> None:
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    fused_batch = _fused_up_batch(library, num_cus)
    last_layer = PAIR_FORM_LAST_LAYER if batch == PAIR_FORM_BATCH else 17
    batch = batch or fused_batch
    spec = sg2_spec.make_spec(LARGE, fmap_base=CONFIG_E)
    variables = _variables(network, LARGE)
    ceiling = STRESS_TOLERANCE if network == "stress" else TOLERANCE
    per_sample_noise = network == "loud"
    dlatents = np.random.RandomState(11 + batch).randn(batch, spec.num_layers, 512).astype(np.float32)
    samples = sorted({0, batch - 1})
    rows: dict = {}  # (conv n, sample) -> (isolated error, sensitivity or None)
    tapped: dict = {}
    engine = hip_lib.Engine(variables, LARGE, max_batch=batch, conv_form=conv_form, up_form=up_form, profile=True)
    try:
        if per_sample_noise:
            engine.randomize_noise(seed=NOISE_SEED, count=batch)
        x = engine.debug_activation_after(dlatents, FIRST_LAYER - 1)[samples].copy()
        assert len(spec.convs) == 17
        for n in range(FIRST_LAYER, last_layer + 1):
            conv = spec.convs[n - 1]
            got = engine.debug_activation_after(dlatents, n)[samples].copy()
            tapped[n] = _conv_launches(engine)[conv.layer_idx]
            assert np.isfinite(got).all() and got.shape == (len(samples), conv.cout, 2 ** conv.res_log2, 2 ** conv.res_log2)
            for i, s in enumerate(samples):
                override, plane = None, None
                if per_sample_noise:
                    plane = engine.debug_noise(conv.layer_idx, s)
                    override = {conv.layer_idx: torch.from_numpy(plane[None, None])}
                with torch.no_grad():
                    want = ref.synthesis_layer(
                        torch.from_numpy(x[i:i + 1]).double(), torch.from_numpy(dlatents[s:s + 1]).double(), variables, conv, noise_override=override
                    ).numpy()[0]
                sensitivity = None
                if per_sample_noise:  # the oracle given the neighbouring sample's plane must answer differently (the stored one in a one-frame call)
                    stored = np.asarray(variables[f"G_synthesis/noise{conv.layer_idx}"], dtype=np.float32).reshape(plane.shape)
                    other = engine.debug_noise(conv.layer_idx, (s - 1) % batch) if batch > 1 else stored
                    strength = float(variables[f"G_synthesis/{conv.scope}/noise_strength"])
                    sensitivity = _rel(with_other_plane(want, plane, other, strength), want)
                rows[(n, s)] = (_rel(got[i], want), sensitivity)
            x = got
        engine.synthesize_w(dlatents)
        launches = _conv_launches(engine)
        whole_call = [step.name for step in engine.steps()]
    finally:
        engine.close()

    print(f"\nconfig-e isolated layers, {network} network, conv_form={conv_form}, up_form={up_form}, batch {batch} ({num_cus} CUs):")
    for (n, s), (err, sens) in sorted(rows.items()):
        print(f"  conv {n:2d} {spec.convs[n - 1].scope:18s} {tapped[n]:34s} sample {s}: {err:.2e}" + ("" if sens is None else f" {sens:.2f}"))
    for (n, s), (err, sens) in sorted(rows.items()):
        assert err < ceiling, f"conv layer {n} ({spec.convs[n - 1].scope}, {tapped[n]}), sample {s}: isolated error {err:.2e}"
        assert sens is None or sens > SENSITIVITY, f"conv layer {n}, sample {s}: another plane moves the oracle layer by only {sens:.3f}"
    # the forms the checks were meant to reach
    for n in range(FIRST_LAYER, min(last_layer, 16) + 1):  # (the tap on the last layer runs it unfused: below)
        assert tapped[n] == launches[spec.convs[n - 1].layer_idx], f"layer {n}: {tapped[n]} stopped, {launches[spec.convs[n - 1].layer_idx]} in the whole call"
    assert last_layer < 17 or tapped[17] == "conv16_1024x1024_16->16", tapped[17]
    assert launches[16] == LAST and whole_call[-1] == LAST, whole_call[-3:]
    fused = up_form == "auto" and batch >= fused_batch
    assert launches[15] == (UP_16 if fused else "convT15_1024x1024_32->16"), launches[15]
    assert ("fir15_1024x1024" in whole_call) == (not fused)
    if conv_form == "direct":
        assert launches[14] == "conv14_512x512_32->32", launches[14]
    if up_form == "split":
        assert launches[13] == "convT13_512x512_64->32", launches[13]
    if batch == PAIR_FORM_BATCH and up_form == "auto" and num_cus == 256:
        assert launches[13] == UP_32_PAIR_FORM and "fir13_512x512" not in whole_call, launches[13]


# ---- the frame-emitting launch ----

EMITTING = [("every_term", "auto", 1), ("every_term", "auto", 3), ("every_term", "direct", 2), ("stress", "auto", 2)]


@pytest.mark.parametrize("network,conv_form,batch", EMITTING, ids=[f"{n}-{c}-{b}" for n, c, b in EMITTING])
def test_frame_emitting_launch_in_isolation(library, network: str, conv_form: str, batch: int) -> None:
    spec = sg2_spec.make_spec(LARGE, fmap_base=CONFIG_E)
    variables = _variables(network, LARGE)
    ceiling = STRESS_TOLERANCE if network == "stress" else TOLERANCE
    seed = 11 + batch if network == "stress" else SEEDS[batch]
    dlatents = np.random.RandomState(seed).randn(batch, spec.num_layers, 512).astype(np.float32)
    samples = sorted({0, batch - 1})
    w64 = torch.from_numpy(dlatents[samples]).double()
    n = len(spec.convs)  # 17: the 1024^2 Conv1
    engine = hip_lib.Engine(variables, LARGE, max_batch=batch, conv_form=conv_form, profile=True)
    try:
        frames, image = engine.synthesize_w(dlatents, want_float=True)
        whole_call = [step.name for step in engine.steps()]
        x = engine.debug_activation_after(dlatents, n)[samples].copy()
        y_prev = engine.debug_image_after(dlatents, n - 1)[samples].copy()  # (stopped after the up layer: the 512^2 image as a whole call makes it)
    finally:
        engine.close()
    assert whole_call[-1] == LAST and "torgb_1024x1024" not in whole_call, whole_call[-3:]
    assert x.shape == (len(samples), 16, LARGE, LARGE) and y_prev.shape == (len(samples), 3, LARGE // 2, LARGE // 2)
    with torch.no_grad():
        xt, yt = torch.from_numpy(x), torch.from_numpy(y_prev)
        want = ref.torgb_layer(xt.double(), yt.double(), w64, variables, 10).numpy()
        want32 = ref.torgb_layer(xt, yt, w64.float(), variables, 10).numpy()
    # the bytes, on an engine that replays its calls from graphs (a profiled one launches every call eagerly)
    engine = hip_lib.Engine(variables, LARGE, max_batch=batch, conv_form=conv_form)
    try:
        frames_again, image_again = engine.synthesize_w(dlatents, want_float=True)
        bytes_only = [engine.synthesize_w(dlatents) for _ in range(3)]  # (warm-up, capture + launch, replay)
    finally:
        engine.close()
    unsaturated = float(((frames > 0) & (frames < 255)).mean())
    print(f"\nconfig-e frame-emitting launch, {network} network, conv_form={conv_form}, batch {batch}, {unsaturated:.1%} of the bytes unsaturated: error, err32, ratio")
    rows = []
    for i, s in enumerate(samples):
        err, err32 = _rel(image[s], want[i]), _rel(want32[i], want[i])
        rows.append((s, err, err32))
        print(f"  sample {s}: {err:.2e} {err32:.2e} {err / err32:5.2f}")
    for s, err, err32 in rows:
        assert err < ceiling, f"sample {s}: isolated error {err:.2e}"
        assert err <= FP32_MARGIN * err32, f"sample {s}: isolated error {err:.2e} is {err / err32:.1f} x the float32 oracle step's {err32:.2e}"
    assert np.isfinite(image).all() and frames.dtype == np.uint8 and frames.shape == (batch, LARGE, LARGE, 3)
    assert np.array_equal(frames, ref.convert_images_to_uint8(torch.from_numpy(image))), "the bytes are not the float image's"
    assert np.array_equal(image_again, image) and np.array_equal(frames_again, frames), "a second engine's call differs"
    for i, again in enumerate(bytes_only):
        assert np.array_equal(again, frames), f"bytes-only call {i + 1} of 3 differs from the bytes of the call that also returned the image"
    if network != "stress":
        assert unsaturated > MIN_UNSATURATED, f"only {unsaturated:.1%} of the bytes are unsaturated: the byte checks have little power"


# ---- two configs resident ----


def test_a_multinetwork_switches_between_a_config_e_and_a_config_f_network(library, tmp_path: Path) -> None:
    resolution, max_batch = 64, 4
    paths, variables = [], []
    for index, fmap_base in enumerate((CONFIG_E, 16 << 10)):
        variables.append(sg2_spec.make_random_variables(resolution, seed=20 + index, perturb=True, fmap_base=fmap_base))
        paths.append(tmp_path / f"network_{index}.pkl")
        network_file.save_network(paths[-1], resolution, variables[-1])
    num_layers = sg2_spec.make_spec(resolution).num_layers
    rng = np.random.RandomState(5)
    stream = [(k % 2, rng.randn((1, 1, 3, 3)[k % 4], num_layers, 512).astype(np.float32)) for k in range(12)]
    with network_functions.MultiNetwork(paths, max_batch=max_batch, device=0) as multi:
        assert multi is not None
        got = [multi.indexed_create_images_generic(index, data) for index, data in stream]
    for index in (0, 1):
        engine = hip_lib.Engine(variables[index], resolution, max_batch=max_batch, device=0)
        try:
            assert engine.fmap_base == (CONFIG_E, 16 << 10)[index]
            for k, (which, data) in enumerate(stream):
                if which == index:
                    assert np.array_equal(got[k], engine.synthesize_w(data)), f"frame {k} (network {index}, {len(data)} per call)"
        finally:
            engine.close()
    assert not np.array_equal(got[0], got[1])
