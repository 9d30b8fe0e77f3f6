"""
The 64^2 ... 256^2 conv layers of config-e generators (fmap_base = 8 << 10), and the image branch at 64^2 ... 512^2, checked IN
ISOLATION in every form the product selects for them by itself (conv_form / up_form "auto", no GANCE_TUNE_* knob). Config-e halves
the channel counts a resolution earlier than config-f, which puts forms into the DEFAULT plan that a config-f call reaches only
through overrides: the F(2x2,3x3) launches with the ToRGB sum in their epilogue ("convW8+rgb", "convW10+rgb"), the direct form at
64^2 ... 256^2 ("conv<n>" + "finish<n>"), and the pair-form fused up launches ("/16x"), which layers 9 and 11 take at exactly 17
frames. The cases are the table of tests/isolated_config_e_cases.py, which tests/test_isolated_coverage.py holds against the
planner: all 27 (layer, form) launches of layers 7 ... 16 (layer_idx) over 1 ... 64 frames on 256 CUs; layers 7 ... 12 are checked
here on the 256^2 network (the smallest that holds them, planned like the 1024^2 one), layers 13 ... 16 in
tests/test_config_e_gpu.py on the 1024^2 network.

Conv layers, by the method of tests/test_isolated_small_layers_gpu.py: the layer's own input as the kernels left it
(debug_activation_after(n - 1)), promoted to fp64, through ONE oracle layer (stylegan2_ref.synthesis_layer), against
debug_activation_after(n), for samples {0, batch - 1}.
  * every-term network at every batch of CASES (the first batch of each form; all of layers 7 ... 12 at 1 and at 64 frames);
  * stress network at 1, 17 and 64 frames, all of layers 7 ... 12;
  * "loud" network (noise_strength = 0.5 * (-1) ** layer_idx) with a noise plane per sample (engine.randomize_noise(seed,
    count=batch)) at every batch of NOISE_CASES (the last batch of each form), the planes read back with debug_noise; the oracle
    layer given the neighbouring sample's plane (the stored one in a one-frame call) must differ by more than 0.1 of its range
    (with_other_plane of tests/test_isolated_noise_gpu.py);
  * conv_form="direct", up_form="split" at 1 and at 3 frames: the conv_mfma.hip tiles and the two-pass up at config-e's
    (channels, side) pairs.
Bars: error = max|got - want| / max|want| < 2e-5, 1e-4 on the stress network (the project's layer-wise ceilings). err32, the error
of the same oracle layer in float32 from the same input, and the ratio are printed. The tapped call's launch name equals the name
in an untapped synthesize_w, and on 256 CUs the table's name.

Image branch, by the method of tests/test_isolated_image_gpu.py: the plain activation of the conv in front
(debug_activation_after(n)) and the previous resolution's production image (debug_image_after(n - 1)) through ONE fp64
stylegan2_ref.torgb_layer, against the production image (debug_image_after(n + 1); at the 256^2 network's last resolution the float
image of a whole call) and the unscaled one (debug_image_after(n)). Cases: IMAGE_CASES, every one of the nine (resolution, form)
image launches at the first batch of its range, in the last sample of an odd call (3 and 7 frames) and of a 64-frame call;
"convV14+rgb" on the 1024^2 network. Bars: the ceilings above, and error <= FP32_MARGIN = 4 times err32 (the float32 oracle step's
own error: see tests/test_isolated_image_gpu.py for why a factor of four). Bytes, on the 256^2 network: the frames of a want_float
call equal convert_images_to_uint8 of the same call's float image exactly; three bytes-only calls return the same bytes; more than
30 % of them are unsaturated on the networks that are not the stress one (seeds chosen on the float32 CPU oracle: SEEDS).

Measured on an MI355X (256 CUs) over every configuration below; the inputs are seeded. Every one of the 27 (layer, form) pairs and of
the nine image forms appears in the printed rows with its launch name. Conv layers 7 ... 12, error / err32 / their ratio, over the
every-term, stress and loud networks:
  * scatter-GEMM up (convTG7, convTG9):                      2.7e-7 ... 4.7e-7 / 5.5e-7 ... 1.3e-6 / 0.31 ... 0.60
  * two-pass up (convT11 + fir11):                           1.9e-7 ... 5.7e-7 / 4.5e-7 ... 6.3e-7 / 0.38 ... 0.91
  * split-operand up, narrow (convTF9/s3, 5 frames):         4.4e-7 ... 6.6e-7 / 5.5e-7 ... 7.6e-7 / 0.80 ... 0.93
  * split-operand up, wide (convTFp7, 9, 11 /s3):            3.2e-7 ... 1.0e-6 / 3.6e-7 ... 1.4e-6 / 0.60 ... 1.30
  * fused up, pair form (convTFp7, 9, 11 /16x):              4.4e-7 ... 9.1e-7 / 4.2e-7 ... 1.2e-6 / 0.64 ... 1.67
  * direct (conv8, conv10, conv12 + finish; direct / split): 3.8e-7 ... 1.9e-6 / 3.5e-7 ... 8.4e-7 / 0.62 ... 3.27
  * F(2x2,3x3) with the ToRGB sum (convW8+rgb, convW10+rgb): 3.9e-7 ... 8.8e-7 / 3.4e-7 ... 5.9e-7 / 0.97 ... 1.84
  * F(4x4,3x3) GEMM form (convVG8, convVG10):                7.1e-7 ... 3.3e-6 / 3.6e-7 ... 7.2e-7 / 0.99 ... 7.73
  * F(4x4,3x3) fused (convV8+rgb, convV10+rgb, convV12+rgb): 7.0e-7 ... 8.2e-6 / 3.4e-7 ... 8.5e-7 / 1.33 ... 20.7 (every-term network:
    <= 2.6e-6; the stress and loud networks' rougher inputs cost F(4x4,3x3) its usual factor: tests/test_isolated_noise_gpu.py)
Sensitivity to the neighbouring sample's plane: 0.28 ... 0.55 over the 38 loud rows. No form came near its ceiling.
The image branch, error / err32 / their ratio:
  * stand-alone torgb_64x64 / 128x128 / 256x256 (after convVG8, convVG10, conv12): 1.5e-7 ... 4.0e-7 / 2.5e-7 ... 4.6e-7 / 0.58 ... 0.86
  * "convW<n>+rgb" + torgb (4 and 2 partial images):          1.5e-7 ... 2.8e-7 / 1.2e-7 ... 1.1e-6 / 0.26 ... 1.22
  * "convV<n>+rgb" + torgb (8, 4, 2 and 1 partial images):    1.3e-7 ... 3.2e-7 / 1.3e-7 ... 5.3e-7 / 0.32 ... 1.15
The unscaled form was bit-identical to the production image in every row. The bytes were exact everywhere; 40.6 % ... 55.0 % of them
unsaturated on the every-term 256^2 network.

The checks have power where the whole chain has none. A build whose winograd64_rgb_coef_kernel clears the low 8 mantissa bits of each
ToRGB coefficient (defect (c) of tests/test_isolated_image_gpu.py; it reaches "convW8+rgb" and "convW10+rgb", which only config-e
selects by default, and the "convV<n>+rgb" launches): the seven every-term 256^2 image cases with a "+rgb" launch FAIL here, on the
fp32 bar alone (convW8+rgb 4.0e-6 ... 6.2e-6, 10 ... 15 times err32; convW10+rgb 2.5e-6 ... 6.1e-6, 8.9 ... 21 times; convV8 / 10 / 12+rgb
2.9e-6 ... 1.2e-5, 7.4 ... 54 times; the one-frame case, which has no such launch, passes), while all four cases of
tests/test_config_e_gpu.py::test_whole_chain_matches_oracle_on_the_w_entry PASS on that build: max|image - oracle| on the every-term
networks 7.5e-5 (64^2, 16 frames), 4.5e-5 (256^2, 3 frames, the convW10+rgb call) and 8.8e-5 (256^2, 16 frames) under its 1e-4, where
the honest build has 1.0e-5, 1.1e-5 and 1.6e-5.

Time on one machine: this module 42 s (the 64-frame layer cases 3.1 ... 3.3 s each, the 64-frame image case 1.9 s, every other case
0.5 ... 1.8 s); the two 17-frame rows of tests/test_config_e_gpu.py 2.2 s and 2.6 s.
"""

import os

import numpy as np
import pytest
import torch

import isolated_config_e_cases as cases
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref
from test_config_e_gpu import CONFIG_E, _variables
from test_isolated_noise_gpu import with_other_plane

pytestmark = pytest.mark.gpu

SMALL, LARGE = 256, 1024
TOLERANCE = 2e-5
STRESS_TOLERANCE = 1e-4
FP32_MARGIN = 4.0  # times the float32 oracle step's own error (the image branch)
MIN_UNSATURATED = 0.3
SENSITIVITY = 0.1  # of max|want|: what the oracle layer must change by when it is given another sample's plane
NOISE_SEED = 23

# dlatents = RandomState(seed).randn(batch, W, 512) of each image case on the every-term networks: (network resolution, batch) ->
# seed, the first from 11 + batch up whose frames the float32 CPU oracle leaves at least 35 % unsaturated, with that share (stress
# network: 11 + batch). The 1024^2 cases check no bytes; their seeds are those of tests/test_config_e_gpu.py.
SEEDS = {
    (256, 1): 12,  # 54.1 %
    (256, 2): 13,  # 42.6 %
    (256, 3): 14,  # 40.6 %
    (256, 4): 15,  # 44.2 %
    (256, 6): 17,  # 55.0 %
    (256, 7): 18,  # 40.9 %
    (256, 8): 19,  # 45.0 %
    (256, 64): 75,  # 41.8 %
    (1024, 1): 15,
    (1024, 3): 15,
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


def _launches(engine) -> dict:
    """{layer_idx: launch name} of the conv launches of the engine's last call (profiling on)."""
    return cases.conv_launches(step.name for step in engine.steps())


# ---- conv layers 7 ... 12 ----

# (network, conv_form, up_form, frames per call, layer_idx checked)
LAYER_CONFIGS = (
    [("every_term", "auto", "auto", batch, layers) for batch, layers in cases.CASES]
    + [("stress", "auto", "auto", batch, cases.SMALL_LAYERS) for batch in (1, 17, 64)]
    + [("loud", "auto", "auto", batch, layers) for batch, layers in cases.NOISE_CASES]
    + [("every_term", "direct", "split", batch, cases.SMALL_LAYERS) for batch in (1, 3)]
)


@pytest.mark.parametrize("network,conv_form,up_form,batch,layers", LAYER_CONFIGS, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in LAYER_CONFIGS])
def test_layers_64_to_256_in_isolation(library, network: str, conv_form: str, up_form: str, batch: int, layers: list) -> None:
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    spec = sg2_spec.make_spec(SMALL, fmap_base=CONFIG_E)
    assert len(spec.convs) == cases.LAST_SMALL_LAYER + 1
    variables = _variables(network, SMALL)
    ceiling = STRESS_TOLERANCE if network == "stress" else TOLERANCE
    per_sample_noise = network == "loud"
    default_forms = (conv_form, up_form) == ("auto", "auto")
    dlatents = np.random.RandomState(11 + batch).randn(batch, spec.num_layers, 512).astype(np.float32)
    samples = sorted({0, batch - 1})
    rows: dict = {}  # (layer_idx, sample) -> (isolated error, err32, sensitivity or None)
    tapped: dict = {}  # layer_idx -> its launch name in the call that stopped after it
    kept: dict = {}  # n -> the output of conv layer n (1-based) at `samples`: only the last one read

    engine = hip_lib.Engine(variables, SMALL, max_batch=batch, conv_form=conv_form, up_form=up_form, profile=True)

    def activation(n: int) -> np.ndarray:
        if n not in kept:
            full = engine.debug_activation_after(dlatents, n)
            tapped[n - 1] = _launches(engine).get(n - 1)
            kept.clear()
            kept[n] = full[samples].copy()
        return kept[n]

    try:
        assert engine.fmap_base == CONFIG_E
        if per_sample_noise:
            engine.randomize_noise(seed=NOISE_SEED, count=batch)
        for idx in layers:
            conv = spec.convs[idx]
            assert conv.layer_idx == idx
            x = activation(idx)  # (debug taps count conv layers from 1: the output of layer idx - 1)
            got = activation(idx + 1)
            side = 2 ** conv.res_log2
            assert np.isfinite(got).all() and got.shape == (len(samples), conv.cout, side, side) and x.shape[1] == conv.cin
            for i, s in enumerate(samples):
                override, plane = None, None
                if per_sample_noise:
                    plane = engine.debug_noise(idx, s)
                    override = {idx: torch.from_numpy(plane[None, None])}
                xi, wi = torch.from_numpy(x[i:i + 1]), torch.from_numpy(dlatents[s:s + 1])
                with torch.no_grad():
                    want = ref.synthesis_layer(xi.double(), wi.double(), variables, conv, noise_override=override).numpy()[0]
                    want32 = ref.synthesis_layer(xi, wi, variables, conv, noise_override=override).numpy()[0]
                assert want32.dtype == np.float32
                sensitivity = None
                if per_sample_noise:  # the oracle given the neighbouring sample's plane (the stored one in a one-frame call)
                    stored = np.asarray(variables[f"G_synthesis/noise{idx}"], dtype=np.float32).reshape(plane.shape)
                    other = engine.debug_noise(idx, (s - 1) % batch) if batch > 1 else stored
                    strength = float(variables[f"G_synthesis/{conv.scope}/noise_strength"])
                    sensitivity = _rel(with_other_plane(want, plane, other, strength), want)
                rows[(idx, s)] = (_rel(got[i], want), _rel(want32, want), sensitivity)
        engine.synthesize_w(dlatents)  # the untapped call (noise still randomized on the loud network)
        whole_call = [step.name for step in engine.steps()]
        launches = cases.conv_launches(whole_call)
    finally:
        engine.close()

    print(f"\nconfig-e isolated layers, {network} network {SMALL}^2, conv_form={conv_form}, up_form={up_form}, batch {batch} ({num_cus} CUs): "
          f"error, err32, error / err32{', sensitivity' if per_sample_noise else ''}")
    for (idx, s), (err, err32, sens) in sorted(rows.items()):
        print(f"  conv {idx + 1:2d} {spec.convs[idx].scope:16s} {launches.get(idx, '?'):32s} sample {s:2d}: {err:.2e} {err32:.2e} {err / err32:5.2f}"
              + ("" if sens is None else f" {sens:.2f}"))
    for idx in layers:
        assert tapped[idx] == launches[idx], f"layer {idx}: {tapped[idx]} in the call stopped after it, {launches[idx]} in the whole call"
        conv = spec.convs[idx]
        side = 2 ** conv.res_log2
        assert launches[idx].split("/")[0].endswith(f"_{side}x{side}_{conv.cin}->{conv.cout}"), launches[idx]
        if default_forms:
            if num_cus == cases.NUM_CUS:
                assert launches[idx] == cases.expected_name(idx, batch), f"layer {idx} at {batch} frames: {launches[idx]}"
        elif conv.up:  # up_form="split": two passes
            assert "/" not in launches[idx] and f"fir{idx}_{side}x{side}" in whole_call, launches[idx]
        else:  # conv_form="direct": the conv_mfma.hip tiles
            assert launches[idx] == f"conv{idx}_{side}x{side}_{conv.cin}->{conv.cout}", launches[idx]
    misses = []  # every miss of the call is reported, so that one layer's does not hide another's
    for (idx, s), (err, _, sens) in sorted(rows.items()):
        where = f"conv layer {idx + 1} ({spec.convs[idx].scope}, {launches[idx]}), sample {s} of {batch}"
        if not err < ceiling:
            misses.append(f"{where}: isolated error {err:.2e}")
        if sens is not None and not sens > SENSITIVITY:
            misses.append(f"{where}: another plane moves the oracle layer by only {sens:.3f} of its range")
    assert not misses, "\n".join(misses)


# ---- the image branch at 64^2 ... 512^2 ----

# every term on at every case of the table; the stress network at the two odd calls of the 256^2 network (both "convW<n>+rgb"
# launches, "convV10+rgb" and "convV12+rgb") and at the odd call of the 1024^2 one
IMAGE_CONFIGS = [("every_term",) + case for case in cases.IMAGE_CASES] + [
    ("stress",) + case for case in cases.IMAGE_CASES if case[:2] in ((SMALL, 3), (SMALL, 7), (LARGE, 3))
]


def _check_names(names: list, resolution: int, batch: int, where: str) -> str:
    """The image launches of `resolution` among a call's profiled launch names, held against the table; returns "conv + torgb"."""
    torgb, conv = cases.image_launches(names)[resolution]
    name, _ = cases.expected_form(resolution, batch)
    kind = conv.split("_")[0]
    assert torgb == f"torgb_{resolution}x{resolution}", f"{where}: {conv} / {torgb}"  # (no config-e layer up to 512^2 absorbs its whole ToRGB)
    if name is None:
        assert "+" not in kind, f"{where}: {conv} / {torgb}"
    else:
        assert conv == name, f"{where}: {conv} / {torgb}"
    return f"{kind} + {torgb}"


@pytest.mark.parametrize("network,resolution,batch,checked", IMAGE_CONFIGS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in IMAGE_CONFIGS])
def test_image_branch_64_to_512_in_isolation(library, network: str, resolution: int, batch: int, checked: list) -> None:
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    on_table = num_cus == cases.NUM_CUS
    spec = sg2_spec.make_spec(resolution, fmap_base=CONFIG_E)
    variables = _variables(network, resolution)
    ceiling = STRESS_TOLERANCE if network == "stress" else TOLERANCE
    check_bytes = resolution == SMALL  # (the 1024^2 network's bytes: tests/test_config_e_gpu.py::test_frame_emitting_launch_in_isolation)
    samples = [batch - 1] if batch == 64 else sorted({0, batch - 1})
    seed = 11 + batch if network == "stress" else SEEDS[(resolution, batch)]
    dlatents = np.random.RandomState(seed).randn(batch, spec.num_layers, 512).astype(np.float32)
    w64 = torch.from_numpy(dlatents[samples]).double()
    rows: list = []  # (resolution, form, launches, sample, error, err32)
    identical: dict = {}

    def names_of(engine, r: int, where: str) -> str:
        names = [step.name for step in engine.steps()]
        if on_table:
            return _check_names(names, r, batch, where)
        torgb, conv = cases.image_launches(names)[r]  # (another CU count: the names are printed, the numerics checked)
        return f"{conv.split('_')[0]} + {torgb}"

    engine = hip_lib.Engine(variables, resolution, max_batch=batch, profile=True)
    try:
        assert engine.fmap_base == CONFIG_E
        if check_bytes:
            frames, image = engine.synthesize_w(dlatents, want_float=True)
        else:
            frames, image = engine.synthesize_w(dlatents), None
        whole_call = [step.name for step in engine.steps()]
        produced: dict = {}  # conv layers run -> the skip image that call left, samples only
        for r in checked:
            n = cases.conv1_index(r) + 1  # (debug taps count conv layers from 1)
            assert spec.convs[n - 1].res_log2 == r.bit_length() - 1 and not spec.convs[n - 1].up
            x = engine.debug_activation_after(dlatents, n)[samples].copy()
            if n - 1 not in produced:
                produced[n - 1] = engine.debug_image_after(dlatents, n - 1)[samples].copy()
            y_prev = produced[n - 1]
            unscaled = engine.debug_image_after(dlatents, n)[samples].copy()
            launches = {"unscaled": names_of(engine, r, f"{r}^2, stopped after its conv")}
            if n < len(spec.convs):
                produced[n + 1] = engine.debug_image_after(dlatents, n + 1)[samples].copy()
                launches["production"] = names_of(engine, r, f"{r}^2, production")
                production = produced[n + 1]
            else:
                launches["production"] = _check_names(whole_call, r, batch, f"{r}^2, production") if on_table else "the whole call"
                production = image[samples]
            assert x.shape == (len(samples), spec.convs[n - 1].cout, r, r) and production.shape == unscaled.shape == (len(samples), 3, r, r)
            assert y_prev.shape == (len(samples), 3, r // 2, r // 2)
            assert np.isfinite(x).all() and np.isfinite(production).all() and np.isfinite(unscaled).all()
            identical[r] = bool(np.array_equal(production, unscaled))
            with torch.no_grad():
                xt, yt = torch.from_numpy(x), torch.from_numpy(y_prev)
                want = ref.torgb_layer(xt.double(), yt.double(), w64, variables, r.bit_length() - 1).numpy()
                want32 = ref.torgb_layer(xt, yt, w64.float(), variables, r.bit_length() - 1).numpy()
            assert want32.dtype == np.float32 and want.shape == production.shape
            for i, s in enumerate(samples):
                err32 = _rel(want32[i], want[i])
                rows.append((r, "production", launches["production"], s, _rel(production[i], want[i]), err32))
                rows.append((r, "unscaled", launches["unscaled"], s, _rel(unscaled[i], want[i]), err32))
        if on_table:  # the whole call ran the forms of the table at every resolution
            for r in cases.IMAGE_FORMS:
                if r <= resolution:
                    _check_names(whole_call, r, batch, f"{r}^2, whole call")
    finally:
        engine.close()

    unsaturated = float(((frames > 0) & (frames < 255)).mean())
    print(f"\nconfig-e isolated image branch, {network} network {resolution}^2, batch {batch} ({num_cus} CUs), "
          f"{unsaturated:.1%} of the bytes unsaturated: error, err32, error / err32")
    for r, form, launch, s, err, err32 in rows:
        print(f"  {r:4d}^2 {form:10s} {launch:28s} sample {s:2d}: {err:.2e} {err32:.2e} {err / err32:5.2f}"
              f"{'' if form == 'unscaled' else '  (unscaled form bit-identical)' if identical[r] else '  (unscaled form differs)'}")
    misses = []
    for r, form, launch, s, err, err32 in rows:
        where = f"{r}^2 image ({form}: {launch}), sample {s}"
        if not err < ceiling:
            misses.append(f"{where}: isolated error {err:.2e}")
        if not err <= FP32_MARGIN * err32:
            misses.append(f"{where}: isolated error {err:.2e} is {err / err32:.1f} x the float32 oracle step's {err32:.2e}")
    assert not misses, "\n".join(misses)
    assert frames.dtype == np.uint8 and frames.shape == (batch, resolution, resolution, 3)
    if not check_bytes:
        return

    # the bytes, on an engine that replays its calls from graphs (a profiled one launches every call eagerly)
    engine = hip_lib.Engine(variables, resolution, max_batch=batch)
    try:
        frames_again, image_again = engine.synthesize_w(dlatents, want_float=True)
        bytes_only = [engine.synthesize_w(dlatents) for _ in range(3)]  # (warm-up, capture + launch, replay)
    finally:
        engine.close()
    assert np.isfinite(image).all()
    assert np.array_equal(frames, ref.convert_images_to_uint8(torch.from_numpy(image))), "the bytes are not the float image's"
    assert np.array_equal(image_again, image) and np.array_equal(frames_again, frames), "a second engine's call differs"
    for i, again in enumerate(bytes_only):
        assert np.array_equal(again, frames), f"bytes-only call {i + 1} of 3 differs from the bytes of the call that also returned the image"
    if network != "stress":
        assert unsaturated > MIN_UNSATURATED, f"only {unsaturated:.1%} of the bytes are unsaturated: the byte checks have little power"
