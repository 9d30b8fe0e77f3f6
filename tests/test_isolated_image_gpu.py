"""
The image branch checked IN ISOLATION, one resolution at a time, in every form the product runs it in: ToRGB (the modulated 1x1
conv), upsample_2d of the skip image, bias, and the uint8 conversion. The inputs are the ones the kernels left: the plain activation
of the conv in front (debug_activation_after(n)) and the previous resolution's production image (debug_image_after(n - 1): the call
stopped after the up layer, so the Conv1 before it ran as in a whole call); promoted to fp64 they go through ONE oracle step
(stylegan2_ref.torgb_layer, the function the full oracle chain calls). Compared with that:
  * the production image: debug_image_after(n + 1) (stopped after the next up layer: layer n in its production launch, the next
    layer's style on its stores where the plan has that), at the network's last resolution the float image of a whole call;
  * the unscaled form: debug_image_after(n) (the same layer as the call's last: no next-style scale). Whether the two are
    bit-identical is printed.
The cases are the table of tests/isolated_image_cases.py, which tests/test_isolated_coverage.py holds against the planner: all
twelve (resolution, form) launches of calls of 1 ... 64 frames on 256 CUs, and the two more forms of conv_form="direct". The launch
names of the calls (profiled steps) are asserted against the table when the device has 256 CUs.

Bars, per resolution and sample, on error = max|got - want| / max|want|:
  * ceiling 2e-5, 1e-4 on the stress network (the project's layer-wise ceilings);
  * error <= FP32_MARGIN = 4 times err32, the error of the same oracle step evaluated in float32 on the CPU from the same fp32
    inputs, against the fp64 result. Kernel and float32 oracle sum the same <= 512 fp32 products in a different order (the "+rgb"
    sums run on v_mfma_f32_16x16x4_f32, true fp32, from the register values whose rounded copies the tap returns), then add the
    same four-tap upsample and the bias; a maximum over 48 ... 3e6 outputs is a stable statistic, so a factor of four covers the
    order, while a coefficient or operand that loses mantissa bits lands well above it.
Bytes, exact (no kernel's byte path may differ from its own float image):
  * the frames of a want_float call equal convert_images_to_uint8 of the float image the same call returned, bit for bit
    (__fmul_rn then __fadd_rn, clamp, truncate, against torch's separate fp32 multiply and add);
  * three bytes-only calls (the third replayed from the captured graph) return the same bytes: at 1024^2 the pass that stores no
    fp32 image (skip_y_store), in the direct form conv16+torgb;
  * on the networks that are not the stress one more than 30 % of the call's bytes are unsaturated, so that the check has power
    (the dlatent seeds below were chosen on the CPU oracle for that: SEEDS).

Measured on the CPU alone: err32 of the every-term networks at one frame, the float32 chain's own activation and image as inputs:
1.7e-7 ... 7.6e-7 over the nine resolutions (largest at 4^2), so the fp32 bar is 6.6e-7 ... 3.0e-6.
Measured on an MI355X (256 CUs) over every configuration below, error / err32 / their ratio:
  * the small kernel (4^2 ... 128^2):              1.1e-7 ... 2.8e-7 / 1.8e-7 ... 6.0e-7 / 0.32 ... 1.26
  * "convV<n>+rgb" + torgb_kernel (16 ... 1 partial images, 32^2 ... 1024^2; the stress network's rows are among them):
                                                   1.2e-7 ... 3.2e-7 / 1.2e-7 ... 7.0e-7 / 0.35 ... 1.20
  * plain torgb_kernel (direct form, 256^2, 512^2): 1.9e-7 ... 4.7e-7 / 1.9e-7 ... 5.9e-7 / 0.75 ... 1.20
  * "conv16+torgb" (direct form, 1024^2):           3.1e-7 ... 4.6e-7 / 2.6e-7 ... 5.1e-7 / 0.92 ... 1.18
No family needed more than FP32_MARGIN. The unscaled form was bit-identical to the production image in every row but the direct
form's 1024^2 one (there the stopped call runs the unfused launch: engine_plan.h), which met the same bars. The bytes were exact
everywhere; 35 % ... 55 % of them unsaturated on the networks that are not the stress one.
Builds with one defect each, through this test and through tests/test_synthesis_gpu.py::test_matrix_path_matches_oracle:
  (a) torgb_kernel sums partials - 1 images: every "+rgb" row 7e-2 ... 8e-1, 10 of the 12 cases fail here (the two without
      a "+rgb" launch cannot see it); the whole-image test fails too (1.6 ... 2.7 on the image).
  (b) torgb_kernel's fourth pixel reads ta[1] / ta[2]: every torgb_kernel row with a skip image 3.6e-2 ... 5.0e-1, 11 of 12 cases
      fail here (all but the one-frame 128^2 call, which runs only the small kernel); the whole-image test fails too (0.7 ... 1.6).
  (c) winograd64_rgb_coef_kernel clears the low 8 mantissa bits of each coefficient: every "+rgb" row 1.1e-6 ... 1.6e-5, that is
      8.4 ... 42 times err32, and all 10 cases with such a launch fail here on the fp32 bar alone (the ceilings pass), while the
      whole-image test PASSES all six cases: on the three that run a "+rgb" launch max|image - oracle| is 5.0e-5 ... 9.2e-5 under its
      1e-4 (honest build 6.6e-6 ... 9.4e-6), the bytes 1 LSB off on 2.6e-4 ... 5.9e-4 of the pixels under its 1e-3. With 6 bits cleared the "+rgb" rows are 1.4 ... 10.6 times err32
      (9 cases fail here), with 4 bits 0.7 ... 2.9 times (nothing fails: below what a different order of summation may cost).
"""

import os

import numpy as np
import pytest
import torch

import isolated_image_cases as cases
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

TOLERANCE = 2e-5
STRESS_TOLERANCE = 1e-4
FP32_MARGIN = 4.0  # times the float32 oracle step's own error: see above
MIN_UNSATURATED = 0.3

# dlatents = RandomState(seed).randn(batch, W, 512) of each call: (network, network resolution, conv_form, batch) -> seed, the
# first seed from 11 + batch up whose frames the float32 CPU oracle leaves at least 35 % unsaturated, with that share (stress network: 11 + batch)
SEEDS = {
    ("every_term", 128, "auto", 1): 13,  # 40.8 % (seed 12: 20.1 %)
    ("every_term", 128, "auto", 2): 13,  # 40.5 %
    ("every_term", 128, "auto", 4): 15,  # 54.7 %
    ("every_term", 128, "auto", 16): 27,  # 36.0 %
    ("every_term", 128, "auto", 64): 76,  # 35.0 % (seed 75: 33.9 %)
    ("every_term", 1024, "auto", 1): 12,  # 48.4 %
    ("every_term", 1024, "auto", 3): 15,  # 55.3 % (seed 14: 25.7 %)
    ("every_term", 1024, "direct", 2): 13,  # 46.6 %
    ("stylegan_init", 128, "auto", 16): 27,  # 52.4 %
    ("stylegan_init", 1024, "auto", 1): 12,  # 39.6 %
}


def _seed(network: str, resolution: int, conv_form: str, batch: int) -> int:
    return 11 + batch if network == "stress" else SEEDS[(network, resolution, conv_form, batch)]


def _rel(got: np.ndarray, want: np.ndarray) -> float:
    return float(np.abs(got - want).max() / np.abs(want).max())


_VARIABLES: dict = {}


def _variables(network: str, resolution: int) -> dict:
    """The generators of the isolated conv checks (tests/test_isolated_layers_gpu.py), made once per session."""
    if (network, resolution) not in _VARIABLES:
        if network == "stress":
            _VARIABLES[(network, resolution)] = sg2_spec.make_stress_variables(resolution, seed=0)
        else:
            _VARIABLES[(network, resolution)] = sg2_spec.make_random_variables(resolution, seed=3, perturb=network == "every_term")
    return _VARIABLES[(network, resolution)]


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    knobs = sorted(key for key in os.environ if key.startswith("GANCE_TUNE_"))
    if knobs:
        pytest.fail(f"{', '.join(knobs)} set: these checks are of the forms the product selects by itself; unset every GANCE_TUNE_* variable")
    return hip_lib.load_library()


def _case(resolution: int, conv_form: str, batch: int) -> tuple:
    return [case for case in cases.CASES if case[:3] == (resolution, conv_form, batch)][0]


# every term on at every case of the table; StyleGAN2's own init (no noise, no biases: the network bench.py times) and the stress
# network at one case of each network resolution
CONFIGS = [("every_term",) + case for case in cases.CASES] + [
    ("stylegan_init",) + _case(128, "auto", 16),
    ("stylegan_init",) + _case(1024, "auto", 1),
    ("stress",) + _case(128, "auto", 4),
    ("stress",) + _case(1024, "auto", 3),
]


def _check_names(names: list, resolution: int, batch: int, conv_form: str, where: str, stopped: bool = False) -> str:
    """The image launches of `resolution` among a call's profiled launch names, held against the table; returns "conv + torgb"."""
    torgb, conv = cases.image_launches(names)[resolution]
    name, _ = cases.expected_form(resolution, batch, conv_form)
    if stopped and name is not None and "+torgb" in name:  # (a debug tap on the last layer runs the unfused launch: engine_plan.h)
        name = None
    kind = conv.split("_")[0]
    if name is None:
        assert "+" not in kind and torgb != "", f"{where}: {conv} / {torgb}"
    else:
        assert conv == name and (torgb == "") == ("+torgb" in name), f"{where}: {conv} / {torgb}"
    return f"{kind}{' + ' + torgb if torgb else ''}"


@pytest.mark.parametrize("network,resolution,conv_form,batch,checked", CONFIGS, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in CONFIGS])
def test_image_branch_in_isolation_on_the_default_kernels(library, network: str, resolution: int, conv_form: str, batch: int, checked: list) -> None:
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    on_table = num_cus == cases.NUM_CUS
    spec = sg2_spec.make_spec(resolution)
    variables = _variables(network, resolution)
    ceiling = STRESS_TOLERANCE if network == "stress" else TOLERANCE
    samples = [batch - 1] if batch == 64 else sorted({0, batch - 1})
    dlatents = np.random.RandomState(_seed(network, resolution, conv_form, batch)).randn(batch, spec.num_layers, 512).astype(np.float32)
    w64 = torch.from_numpy(dlatents[samples]).double()
    rows: list = []  # (resolution, form, launches, sample, error, err32)
    identical: dict = {}

    engine = hip_lib.Engine(variables, resolution, max_batch=batch, conv_form=conv_form, profile=True)
    try:
        frames, image = engine.synthesize_w(dlatents, want_float=True)
        whole_call = [step.name for step in engine.steps()]
        produced: dict = {}  # conv layers run -> the skip image that call left, samples only
        for r in checked:
            n = cases.conv1_index(r) + 1  # (debug taps count conv layers from 1)
            assert spec.convs[n - 1].res_log2 == r.bit_length() - 1 and not spec.convs[n - 1].up
            x = engine.debug_activation_after(dlatents, n)[samples].copy()
            if n > 1 and n - 1 not in produced:
                produced[n - 1] = engine.debug_image_after(dlatents, n - 1)[samples].copy()
            y_prev = produced.get(n - 1)
            unscaled = engine.debug_image_after(dlatents, n)[samples].copy()
            launches = {"unscaled": _check_names([s.name for s in engine.steps()], r, batch, conv_form, f"{r}^2, stopped after its conv", stopped=True) if on_table
                        else "?"}
            if n < len(spec.convs):
                produced[n + 1] = engine.debug_image_after(dlatents, n + 1)[samples].copy()
                names = [s.name for s in engine.steps()]
                production = produced[n + 1]
            else:
                names, production = whole_call, image[samples]
            launches["production"] = _check_names(names, r, batch, conv_form, f"{r}^2, production") if on_table else "?"
            assert x.shape[2:] == (r, r) and production.shape == unscaled.shape == (len(samples), 3, r, r)
            assert (y_prev is None) == (r == 4)
            assert np.isfinite(x).all() and np.isfinite(production).all() and np.isfinite(unscaled).all()
            identical[r] = bool(np.array_equal(production, unscaled))
            with torch.no_grad():
                xt, yt = torch.from_numpy(x), None if y_prev is None else torch.from_numpy(y_prev)
                want = ref.torgb_layer(xt.double(), None if yt is None else yt.double(), w64, variables, r.bit_length() - 1).numpy()
                want32 = ref.torgb_layer(xt, yt, w64.float(), variables, r.bit_length() - 1).numpy()
            assert want32.dtype == np.float32 and want.shape == production.shape
            for i, s in enumerate(samples):
                err32 = _rel(want32[i], want[i])
                rows.append((r, "production", launches["production"], s, _rel(production[i], want[i]), err32))
                rows.append((r, "unscaled", launches["unscaled"], s, _rel(unscaled[i], want[i]), err32))
        if on_table:  # the whole call ran the forms of the table at every resolution
            for r in cases.FORMS:
                if r <= resolution:
                    _check_names(whole_call, r, batch, conv_form, f"{r}^2, whole call")
    finally:
        engine.close()

    # the bytes, on an engine that replays its calls from graphs (a profiled one launches every call eagerly)
    engine = hip_lib.Engine(variables, resolution, max_batch=batch, conv_form=conv_form)
    try:
        frames_again, image_again = engine.synthesize_w(dlatents, want_float=True)
        bytes_only = [engine.synthesize_w(dlatents) for _ in range(3)]  # (warm-up, capture + launch, replay)
    finally:
        engine.close()
    unsaturated = float(((frames > 0) & (frames < 255)).mean())

    print(f"\nisolated image branch, {network} network {resolution}^2, conv_form={conv_form}, batch {batch} ({num_cus} CUs), "
          f"{unsaturated:.1%} of the bytes unsaturated: error, err32, error / err32")
    for r, form, launch, s, err, err32 in rows:
        print(f"  {r:4d}^2 {form:10s} {launch:32s} sample {s:2d}: {err:.2e} {err32:.2e} {err / err32:5.2f}"
              f"{'' if form == 'unscaled' else '  (unscaled form bit-identical)' if identical[r] else '  (unscaled form differs)'}")

    for r, form, launch, s, err, err32 in rows:
        where = f"{r}^2 image ({form}: {launch}), sample {s}"
        assert err < ceiling, f"{where}: isolated error {err:.2e}"
        assert err <= FP32_MARGIN * err32, f"{where}: isolated error {err:.2e} is {err / err32:.1f} x the float32 oracle step's {err32:.2e}"

    assert np.isfinite(image).all() and frames.dtype == np.uint8 and frames.shape == (batch, resolution, resolution, 3)
    assert np.array_equal(frames, ref.convert_images_to_uint8(torch.from_numpy(image))), "the bytes are not the float image's"
    assert np.array_equal(image_again, image) and np.array_equal(frames_again, frames), "a second engine's call differs"
    for i, again in enumerate(bytes_only):
        assert np.array_equal(again, frames), f"bytes-only call {i + 1} of 3 differs from the bytes of the call that also returned the image"
    if network != "stress":
        assert unsaturated > MIN_UNSATURATED, f"only {unsaturated:.1%} of the bytes are unsaturated: the byte checks have little power"
