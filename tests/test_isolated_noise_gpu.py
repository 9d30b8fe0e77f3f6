"""
Every conv layer checked IN ISOLATION, in each form the product runs it in, WITH A NOISE PLANE PER SAMPLE: the way the product runs by
default (create_images_vector and the noise-blend stream call gance_engine_randomize_noise before every engine call), where sample b
of a launch reads its plane at noise + b * noise_b_stride. The sibling modules (tests/test_isolated_small_layers_gpu.py,
tests/test_isolated_layers_gpu.py) run the stored buffers, stride 0, and every kernel family does the per-sample indexing with
arithmetic of its own: a slip there gives every frame after the first the wrong noise and leaves those modules green.

Per case: engine.randomize_noise(seed, count=batch); the planes of the checked layers and samples are read back with debug_noise; the
layer's own input as the kernels left it (debug_activation_after(n - 1); the 4x4 constant for the first layer), promoted to fp64, goes
through ONE oracle layer (stylegan2_ref.synthesis_layer) fed the very planes the engine drew, and the kernel's output
(debug_activation_after(n)) is compared with that.

The networks are the every-term ones of the sibling modules (seed 3, perturb=True) with each conv layer's noise_strength set to
0.5 * (-1) ** layer_idx. The drawn strengths are N(0, 0.05), as small as -0.0001 at layer 15, where no check can see a misplaced row;
at 0.5 the noise term is of the size of the convolution, which also gives the in-plane row and column addressing of every form a
sensitive check.

Cases (tests/isolated_small_cases.py, held against the planner by tests/test_isolated_coverage.py):
  * layers 0 ... 10, 128^2 network: NOISE_CASES, every (layer, form) of FORMS once, at the LARGEST batch that still selects it.
    convT3 and convVG10 exist only at one frame: they are run all the same, because their launches switch to the drawn buffer, but a
    stride cannot show in a call of one sample;
  * layers 11 ... 16, 1024^2 network, one form each over 2 ... 64 frames: LARGE_NOISE_CASES, 9 frames (one row segment at 1024^2,
    the geometry of 64-frame calls) and 2 frames with conv_form="direct" (the conv_mfma.hip tiles; the debug tap on conv16+torgb
    runs the unfused launch, so that layer's name in the stopped call is the whole call's without "+torgb"). A case of 3 frames
    (4 row segments) was measured and passed (figures below) and was then left out for its time: see "Time".
Samples: every sample of the call for layers up to 16^2 (several samples share a tile or a GEMM column tile there); the last two
(batch - 2, batch - 1) for the larger layers, whose kernels take one sample per block, so that any b > 0 shows a stride error and two
adjacent ones a parity-dependent one; sample 0 of a one-frame call.

Bars, per layer and sample:
  * error = max|got - want| / max|want| < 2e-5, the ceiling of the sibling modules (a wrong plane is an error of order 0.1);
  * sensitivity, from the oracle alone: the same oracle layer given the plane of sample (s - 1) mod batch (the stored buffer in a
    one-frame call) must differ from `want` by more than 0.1 of max|want|. Where a layer falls short its strength is to be raised,
    never the 0.1 lowered. The convolution is nearly all of an oracle layer's time, and the layer ends in an invertible step
    (leaky ReLU x sqrt 2 of conv + plane x strength + bias), so its result for another plane is worked out from `want`
    (with_other_plane; tests/test_isolated_coverage.py holds that to a second oracle call). The condition also guards the
    read-back: were debug_noise to return one plane for every sample, the sensitivity would be zero.
The layer's launch name in the stopped call equals its name in a whole synthesize_w call made with the noise still randomized, and on
256 CUs the name of the case table. At 7 frames, after restore_noise(), layer 7's activation is bit-identical to what it was before
randomize_noise.

test_frames_of_a_64_frame_call_equal_the_same_frames_alone is the production batch end to end: frames 1, 31 and 63 of a 64-frame
1024^2 call against the same z alone with the sample id it had in the batch, under the bar of _assert_same_frames in
tests/test_synthesis_gpu.py (at most 1 LSB, on fewer than 1e-3 of the bytes). One-frame and 64-frame calls run different forms of
most layers, so this checks the plane offsets at the top of the batch without an oracle.

Measured on an MI355X (256 CUs) over the twelve cases as committed; the inputs are seeded. Error per form family, over every
(layer, sample) checked:
  * two-pass up (convT1, convT3, convT5):                    2.2e-7 ... 3.2e-7
  * scatter-GEMM up (convTG1, TG3, TG7, TG9):                2.8e-7 ... 6.4e-7
  * fused up "/16" (convTF5, convTF7):                       7.0e-7 ... 8.8e-7
  * split-operand up "/s3" (layers 5, 7, 9, 11, 13, 15):     2.5e-7 ... 8.0e-7
  * direct (conv0, conv2, conv4; conv12, conv14, conv16):    2.0e-7 ... 1.5e-6
  * F(4x4,3x3) fused (convV6+rgb ... convV16+rgb):           3.0e-6 ... 1.1e-5 (K = 288: <= 4.3e-6; K = 4608: 8.1e-6 ... 1.0e-5)
  * F(4x4,3x3) GEMM form (convVG2 ... convVG10):             2.6e-6 ... 8.8e-6
Sensitivity: 0.16 ... 0.78 over all 401 rows (layers 11 ... 16: 0.27 ... 0.51); no layer needed a larger strength. Frames 1, 31, 63
of the 64-frame call against the same z alone: at most 1 LSB, on 1.4e-4 ... 1.9e-4 of the bytes. A case of 3 frames of layers
11 ... 16, since left out, passed with figures inside these ranges.

WHAT THE CHECK FOUND. With the interpolation points 0, +-1, +-2, infinity the GEMM form measured 3.8e-6 ... 2.2e-5, and three of
the 64 samples of convVG2_8x8_512->512 missed the bar: 2.12e-5 (sample 4), 2.18e-5 (32), 2.09e-5 (53). No plane error (those are
0.36 and more, below) but the rounding of fp32 F(4x4,3x3) at K = 9 x 512: the white noise at strength 0.5 makes every layer's input
spatially rough, which the input transform amplifies where a smooth input cancels (on the quiet networks of the sibling modules
F(4x4,3x3) measures 5.0e-7 ... 1.5e-6). A float32 numpy restatement of F(4x4,3x3) on the oracle's input of layers 2 and 4 gave the
same level (largest of 16 samples 1.3e-5 and 1.9e-5) and 5.0e-6 and 6.4e-6 with the points 0, 1, -1, 1/2, -2, infinity.
gemm_forms.hip now takes those points (its three transforms are plain code; the hand-scheduled fused kernel keeps +-2 and, with one
sample per block and at most 1.1e-5, holds the bar); the figures above are with them. The bar stayed where it was.

The tests can fail: a local build whose layer_noise() reports a stride of 0 while returning the drawn buffer (every launch reads
sample 0's plane, in bounds) fails every case of two frames or more and the 64-frame test (up to 255 LSB, a third of the bytes); the
one-frame case passes. In that build debug_noise reads through the same stride and returns sample 0's plane for every sample, so the
cases fail on the sensitivity condition (0.000); with the read-back alone kept honest they fail on the error of every sample b > 0
(0.36 ... 0.64) and of no sample 0. (Run before the change of points, which touches neither the stride nor the read-back.)

Time, from --durations of runs of the whole GPU suite on one machine: the suite without this module 480 s. The module as first
written (a second oracle call for the sensitivity, an engine per case, the 3-frame case) 83 s; with the sensitivity worked out from
`want` 65 s. Both are more than a tenth of the suite, so the nine small cases share one engine and the 3-frame case of layers
11 ... 16 is left out (13.6 s): 36.5 s and 43.9 s as committed in two runs (the 9-frame case 13 ... 16 s, the direct one
11 ... 13 s, the 64-frame one 9 ... 10 s, about a second each of the rest). What remains is mostly the fp64 oracle of the 64-sample
layers and of two samples of each 1024^2-network layer, and the host copies of whole-batch activations.
"""

import os

import numpy as np
import pytest
import torch

import isolated_small_cases as cases
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

SMALL, LARGE = 128, 1024
TOLERANCE = 2e-5
SENSITIVITY = 0.1  # of max|want|: what the oracle layer must change by when it is given another sample's plane
NOISE_SEED = 23
EVERY_SAMPLE_UP_TO = 4  # layer_idx of the 16^2 Conv1
ORACLE_CHUNK = 8  # samples per oracle call (the oracle holds a modulated fp64 weight per sample: 19 MB each at 512 -> 512)
RESTORE_CASE = (7, 7)  # (frames per call, layer_idx) of the restore check


def _launches(engine) -> dict:
    """{layer_idx: launch name} of the conv launches of the engine's last call (profiling on)."""
    return cases.conv_launches(step.name for step in engine.steps())


def _rel(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.abs(got - want).max() / np.abs(want).max())


_VARIABLES: dict = {}


def _loud_variables(resolution: int) -> dict:
    """The every-term generator of the sibling modules with noise_strength = 0.5 * (-1) ** layer_idx, made once per session."""
    if resolution not in _VARIABLES:
        variables = dict(sg2_spec.make_random_variables(resolution, seed=3, perturb=True))
        for conv in sg2_spec.make_spec(resolution).convs:
            key = f"G_synthesis/{conv.scope}/noise_strength"
            variables[key] = np.full_like(variables[key], 0.5 * (-1) ** conv.layer_idx)
        _VARIABLES[resolution] = variables
    return _VARIABLES[resolution]


def with_other_plane(want: np.ndarray, own: np.ndarray, other: np.ndarray, strength: float) -> np.ndarray:
    """
    What stylegan2_ref.synthesis_layer returns for the noise plane `other` [H, W], from its fp64 result `want` [C, H, W] for the plane
    `own`: want = lrelu(pre) * sqrt 2 with pre = conv + own * strength + bias, and leaky ReLU is invertible.
    """
    pre = np.where(want > 0, want, want / 0.2) / np.sqrt(2.0) + (other.astype(np.float64) - own.astype(np.float64)) * strength
    return np.where(pre > 0, pre, 0.2 * pre) * np.sqrt(2.0)


def _samples(layer_idx: int, batch: int) -> list:
    """The samples of a call of `batch` frames that are checked at the layer."""
    if layer_idx <= EVERY_SAMPLE_UP_TO:
        return list(range(batch))
    return list(range(max(batch - 2, 0), batch))


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    knobs = sorted(key for key in os.environ if key.startswith("GANCE_TUNE_"))
    if knobs:
        pytest.fail(f"{', '.join(knobs)} set: these checks are of the forms the product selects by itself; unset every GANCE_TUNE_* variable")
    return hip_lib.load_library()


@pytest.fixture(scope="module")
def small_engine(library):
    """One 128^2 engine for the nine small cases: a layer's form depends on the call's batch, not on max_batch (the name assertions
    guard that), and every case leaves it on the stored buffers."""
    engine = hip_lib.Engine(_loud_variables(SMALL), SMALL, max_batch=cases.MAX_BATCH, profile=True)
    yield engine
    engine.close()


def _check_layers(engine, resolution: int, conv_form: str, batch: int, layers: list, expected: dict) -> None:
    """
    The isolated check of `layers` (layer_idx, ascending) in a call of `batch` frames with a noise plane per sample, on `engine`
    (profiling on, the stored buffers in use). `expected`: {layer_idx: launch name} the whole call must show on 256 CUs.
    """
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    spec = sg2_spec.make_spec(resolution)
    variables = _loud_variables(resolution)
    dlatents = np.random.RandomState(11 + batch).randn(batch, spec.num_layers, 512).astype(np.float32)
    rows: dict = {}  # (layer_idx, sample) -> (isolated error, sensitivity)
    tapped: dict = {}  # layer_idx -> its launch name in the call that stopped after it
    kept: dict = {}  # n -> (samples, the output of conv layer n (1-based) at those samples): only the last one read

    def activation(n: int, samples: list) -> np.ndarray:
        if n == 0:
            return np.repeat(np.asarray(variables["G_synthesis/4x4/Const/const"], dtype=np.float32), len(samples), axis=0)
        if n not in kept:
            full = engine.debug_activation_after(dlatents, n)
            tapped[n - 1] = _launches(engine).get(n - 1)
            assert np.isfinite(full).all()
            keep = _samples(n - 1, batch)  # (what layer n - 1 is checked at; layer n reads the same samples or fewer)
            kept.clear()
            kept[n] = (keep, full[keep].copy())
        keep, values = kept[n]
        return values[[keep.index(s) for s in samples]]

    try:
        restore = RESTORE_CASE[1] + 1 if (resolution, batch) == (SMALL, RESTORE_CASE[0]) else 0
        before = engine.debug_activation_after(dlatents, restore) if restore else None
        engine.randomize_noise(seed=NOISE_SEED, count=batch)
        for idx in layers:
            conv = spec.convs[idx]
            assert conv.layer_idx == idx
            samples = _samples(idx, batch)
            plane = {s: engine.debug_noise(idx, s) for s in sorted(set(samples) | {(s - 1) % batch for s in samples})}
            stored = np.asarray(variables[f"G_synthesis/noise{idx}"], dtype=np.float32).reshape(plane[samples[0]].shape)
            strength = float(variables[f"G_synthesis/{conv.scope}/noise_strength"])
            x = activation(idx, samples)  # (debug taps count conv layers from 1: the output of layer idx - 1)
            got = activation(idx + 1, samples)
            for first in range(0, len(samples), ORACLE_CHUNK):
                chunk = samples[first:first + ORACLE_CHUNK]
                xi = torch.from_numpy(x[first:first + ORACLE_CHUNK]).double()
                wi = torch.from_numpy(dlatents[chunk]).double()
                own = {idx: torch.from_numpy(np.stack([plane[s] for s in chunk])[:, None])}
                with torch.no_grad():
                    want = ref.synthesis_layer(xi, wi, variables, conv, noise_override=own).numpy()
                for i, s in enumerate(chunk):
                    # the neighbouring sample's plane; in a one-frame call, the stored buffer
                    other = plane[(s - 1) % batch] if batch > 1 else stored
                    wrong = with_other_plane(want[i], plane[s], other, strength)
                    assert got[first + i].shape == want[i].shape
                    rows[(idx, s)] = (_rel(got[first + i], want[i]), _rel(wrong, want[i]))
        engine.synthesize_w(dlatents)  # the whole call, noise still randomized
        launches = _launches(engine)
        if restore:
            engine.restore_noise()
            after = engine.debug_activation_after(dlatents, restore)
    finally:
        engine.restore_noise()

    print(f"\nisolated layers, a noise plane per sample, {resolution}^2 network, conv_form={conv_form}, batch {batch} ({num_cus} CUs): error, sensitivity")
    for (idx, s), (err, sens) in sorted(rows.items()):
        print(f"  conv {idx + 1:2d} {spec.convs[idx].scope:18s} {launches.get(idx, '?'):32s} sample {s:2d}: {err:.2e} {sens:.2f}")
    for idx in layers:
        whole = launches[idx].replace("+torgb", "") if conv_form == "direct" else launches[idx]  # (the tap on conv+torgb runs it unfused)
        assert tapped[idx] == whole, f"layer {idx}: {tapped[idx]} in the call stopped after it, {launches[idx]} in the whole call"
        if num_cus == cases.NUM_CUS:
            assert launches[idx] == expected[idx], f"layer {idx} at {batch} frames: {launches[idx]}"
    misses = []  # every miss of the call is reported, so that one layer's does not hide another's
    for (idx, s), (err, sens) in sorted(rows.items()):
        where = f"conv layer {idx + 1} ({spec.convs[idx].scope}, {launches[idx]}), sample {s} of {batch}"
        if not sens > SENSITIVITY:
            misses.append(f"{where}: another plane moves the oracle layer by only {sens:.3f} of its range")
        if not err < TOLERANCE:
            misses.append(f"{where}: isolated error {err:.2e}")
    assert not misses, "\n".join(misses)
    if restore:
        assert np.array_equal(after, before), f"layer {RESTORE_CASE[1]} after restore_noise() differs from before randomize_noise()"


@pytest.mark.parametrize("batch,layers", cases.NOISE_CASES, ids=[str(batch) for batch, _ in cases.NOISE_CASES])
def test_layers_4_to_128_in_isolation_with_a_noise_plane_per_sample(small_engine, batch: int, layers: list) -> None:
    assert len(sg2_spec.make_spec(SMALL).convs) == cases.LAST_SMALL_LAYER + 1
    _check_layers(small_engine, SMALL, "auto", batch, layers, {idx: cases.expected_name(idx, batch) for idx in layers})


@pytest.mark.parametrize("conv_form,batch", cases.LARGE_NOISE_CASES, ids=[f"{f}-{b}" for f, b in cases.LARGE_NOISE_CASES])
def test_layers_256_to_1024_in_isolation_with_a_noise_plane_per_sample(library, conv_form: str, batch: int) -> None:
    layers = sorted(cases.LARGE_NOISE_FORMS[conv_form])
    assert layers == list(range(cases.LAST_SMALL_LAYER + 1, len(sg2_spec.make_spec(LARGE).convs)))
    engine = hip_lib.Engine(_loud_variables(LARGE), LARGE, max_batch=batch, conv_form=conv_form, profile=True)
    try:
        _check_layers(engine, LARGE, conv_form, batch, layers, cases.LARGE_NOISE_FORMS[conv_form])
    finally:
        engine.close()


def test_frames_of_a_64_frame_call_equal_the_same_frames_alone(library) -> None:
    batch = 64
    z = np.random.RandomState(5).randn(batch, 512).astype(np.float32)
    engine = hip_lib.Engine(_loud_variables(LARGE), LARGE, max_batch=batch)
    try:
        engine.randomize_noise(seed=NOISE_SEED, count=batch)
        frames = engine.synthesize_z(z)
        alone = {}
        for k in (1, 31, 63):  # frame k alone, with the sample id it had in the batch
            engine.randomize_noise(seed=NOISE_SEED, count=1, first_sample=k)
            alone[k] = engine.synthesize_z(z[k:k + 1])[0]
    finally:
        engine.close()
    for k, frame in alone.items():
        diff = np.abs(frame.astype(np.int16) - frames[k].astype(np.int16))
        print(f"frame {k} of {batch} against the same z alone: max {int(diff.max())} LSB, {float((diff > 0).mean()):.2e} of the bytes differ")
    for k, frame in alone.items():
        diff = np.abs(frame.astype(np.int16) - frames[k].astype(np.int16))
        assert int(diff.max()) <= 1 and float((diff > 0).mean()) < 1e-3, f"frame {k}"
