"""
The part of a call in front of the first convolution checked IN ISOLATION, kernel by kernel, against float64: the eight launches of
mapping_dense_kernel (pixel-norm of z in the first), broadcast_truncate_kernel, styles_kernel and demod_kernel
(gance_amd/csrc/aux_kernels.hip) with their host-side preparation in gance_engine_create (the scaled mapping weights, the `A`
matrix and `bias1 = mod_bias + 1`, the `blk_row` table, the `w2` pool summed over the nine taps in fp32).

Each stage is read back through a debug tap (Engine.debug_mapping_after, debug_dlatents, debug_read_style, debug_read_demod) and
judged against ONE oracle step applied to the float32 values the kernels left in front of it (tests/front_end_ref.py: the functions
the whole oracle chain calls). Error: max|got - ref64| / max|ref64| of one layer's [B, n] block. Bar: 8 x the error of the float32
restatement on the same inputs, never below 2^-23. tests/test_front_end.py holds the same judge to a list of wrong restatements on
these inputs, the case table to the networks' layers, and the set of taps to the planner.

Networks and batches (front_end_ref.NETWORKS): the 128^2 config-f stress and perturbed random networks at 1, 7, 8, 9, 17 and 64
frames (skinny_block walks samples in groups of eight with a remainder); the 1024^2 config-f network at 1 and 9 (128-, 64- and
32-channel layers: K / 8 = 16 ... 4); the 1024^2 config-e network at 3 and 9 (16-channel layers: a half-filled demod block, a
half-filled style block with a blk_row entry of its own). Every layer and every sample of each is judged. The w-calls stop after
conv layer 1: styles and demod of every layer run in front of it.

Measured on an MI355X (256 CUs), error / float32 restatement / their ratio (the bar is at ratio 8), the ranges over every tensor of
the stage:
  * one mapping layer (8 layers x 10 inputs, and the zero sample's row), stress network:  9.2e-8 ... 5.2e-7 / 9.2e-8 ... 8.8e-7 / 0.26 ... 1.36
                                                              perturbed random network:  9.1e-8 ... 3.9e-7 / 9.1e-8 ... 9.9e-7 / 0.25 ... 1.15
    the zero sample's row of layer 1 is the float32 restatement to the bit (9.2e-8, ratio 1.00, bar 7.4e-7);
  * z -> layer 8 against g_mapping, stress:    6.5e-7 ... 9.3e-7 / 8.9e-7 ... 1.1e-6 / 0.61 ... 1.00
                                    perturbed: 5.4e-7 ... 8.7e-7 / 8.4e-7 ... 1.5e-6 / 0.37 ... 0.95
    (eight layers accumulate to about twice one layer's error, in the kernels as in float32 on the CPU);
  * truncation (6 psi x 2 batches): 0 ... 1.1e-7, equal to the float32 restatement's error in every case (ratio 1.00; psi = 0 exact);
  * styles, stress-128-f (17 layers x 6 batches):   5.2e-8 ... 1.2e-7 / 9.6e-8 ... 3.4e-7 / 0.24 ... 0.89
            perturb-128-f:                          1.3e-7 ... 2.4e-7 / 2.4e-7 ... 1.0e-6 / 0.17 ... 0.77
            perturb-1024-f (26 layers x 2 batches): 9.0e-8 ... 2.1e-7 / 2.6e-7 ... 1.0e-6 / 0.15 ... 0.71
            perturb-1024-e:                         1.1e-7 ... 1.9e-7 / 2.5e-7 ... 8.5e-7 / 0.17 ... 0.68
    (bias1 = mod_bias + 1 is rounded once on the host where the restatement rounds twice per value);
  * demodulation, stress-128-f (11 layers x 6 batches): 5.8e-8 ... 1.7e-7 / 5.4e-8 ... 1.5e-7 / 0.61 ... 2.41
                  perturb-128-f:                        1.1e-7 ... 1.8e-7 / 1.2e-7 ... 1.7e-7 / 0.86 ... 1.29
                  perturb-1024-f (17 layers x 2):       9.0e-8 ... 1.7e-7 / 8.7e-8 ... 1.5e-7 / 0.69 ... 1.41
                  perturb-1024-e:                       8.1e-8 ... 1.6e-7 / 8.4e-8 ... 1.6e-7 / 0.82 ... 1.30
                  the epsilon case (3 layers):          9.0e-8 ... 9.9e-8 / 9.3e-8 ... 1.0e-7 / 0.88 ... 1.06
    (the 2.41 is one layer of the one-frame stress call, 1.3e-7 against a restatement that happened to land at 5.4e-8);
  * a sample's mapping output, dlatents, styles and demodulation are the same bits at positions 0, 7, 8 and 63 of a 64-frame call
    and alone, and two runs of a call give the same bits.
Nothing in the four kernels or their host preparation had to change: the fp32 host sum of w2 over the nine taps, 1.0f / sqrtf against
the restatement's rsqrt and the block-tree reduction of the pixel-norm all sit at the float32 restatement's own error.
"""

from typing import Dict, Iterator, List

import ctypes

import numpy as np
import pytest
import torch

import front_end_ref as fe
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec

pytestmark = pytest.mark.gpu

_F32P = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def engines() -> Iterator[Dict[str, hip_lib.Engine]]:
    """The engines of the module by network name, each made when a test first asks for it, all closed at the end."""
    if not torch.cuda.is_available():
        pytest.fail("test marked gpu but no HIP device is visible")

    class Engines(dict):
        def __missing__(self, name: str) -> hip_lib.Engine:
            if name == "epsilon":
                network = fe.NETWORKS[fe.EPSILON_NETWORK]
                self[name] = hip_lib.Engine(fe.epsilon_case().variables, network.resolution, max_batch=fe.EPSILON_MAX_BATCH, device=0)
            else:
                network = fe.NETWORKS[name]
                self[name] = hip_lib.Engine(fe.variables_of(name), network.resolution, max_batch=network.max_batch, device=0)
            return self[name]

    made = Engines()
    yield made
    for engine in made.values():
        engine.close()


def _summary(stage: str, figures: List[fe.Figures]) -> None:
    errors, owns, ratios = [f.error for f in figures], [f.own for f in figures], [f.ratio for f in figures]
    print(f"{stage}: {len(figures)} tensors, error {min(errors):.1e} ... {max(errors):.1e}, float32 restatement {min(owns):.1e} ... {max(owns):.1e}, "
          f"ratio {min(ratios):.2f} ... {max(ratios):.2f}")


# ---- mapping ----


@pytest.mark.parametrize("network", fe.MAPPING_NETWORKS)
def test_every_mapping_layer_matches_float64(engines: Dict[str, hip_lib.Engine], network: str) -> None:
    engine, variables = engines[network], fe.variables_of(network)
    failures: List[str] = []
    layers: List[fe.Figures] = []
    chains: List[fe.Figures] = []
    for label, z in fe.mapping_cases():
        outputs = [engine.debug_mapping_after(z, n) for n in range(1, sg2_spec.MAPPING_LAYERS + 1)]
        assert all(output.shape == (z.shape[0], 512) and np.all(np.isfinite(output)) for output in outputs), label
        for n, got in enumerate(outputs, start=1):
            x = z if n == 1 else outputs[n - 2]  # the kernels' own output of the layer before
            layers.append(fe.judge(f"{network} mapping, {label}, layer {n}", got, fe.dense(x, variables, n, torch.float64), fe.dense(x, variables, n, torch.float32), failures))
        # the whole chain z -> layer 8 against g_mapping's row: the accumulation over eight layers, beside the per-layer figures
        chains.append(fe.judge(f"{network} mapping, {label}, z -> layer 8", outputs[-1], fe.mapping_chain(z, variables, torch.float64)[-1],
                               fe.mapping_chain(z, variables, torch.float32)[-1], failures))
        if "zero sample" in label:
            # the all-zero sample: 0 * rsqrt(0 + 1e-8) = 0, so layer 1 leaves lrelu(bias * lrmul) * sqrt(2) alone. Judged as a tensor of
            # its own: no sum of 512 products stands in front of the gain here (tests/test_front_end.py: the gain variant)
            row = slice(fe.ZERO_SAMPLE, fe.ZERO_SAMPLE + 1)
            bias_only = fe.dense(np.zeros((1, 512), dtype=np.float32), variables, 1, torch.float64)
            assert torch.equal(bias_only, fe.dense(z, variables, 1, torch.float64)[row])
            layers.append(fe.judge(f"{network} mapping, the zero sample's row of layer 1", outputs[0][row], bias_only,
                                   fe.dense(z[row], variables, 1, torch.float32), failures))
    _summary(f"{network} mapping, one layer", layers)
    _summary(f"{network} mapping, z -> layer 8", chains)
    assert not failures, "; ".join(failures)


# ---- truncation ----


def test_truncation_matches_float64_and_broadcasts_bit_equal_rows(engines: Dict[str, hip_lib.Engine]) -> None:
    network = fe.TRUNCATION_NETWORK
    engine, variables = engines[network], fe.variables_of(network)
    failures: List[str] = []
    figures: List[fe.Figures] = []
    for batch in fe.TRUNCATION_BATCHES:
        z = fe.mapping_z(batch)
        mapped = engine.debug_mapping_after(z, sg2_spec.MAPPING_LAYERS)
        for psi in fe.TRUNCATION_PSIS:
            dlatents = engine.debug_dlatents(z, psi)
            assert dlatents.shape == (batch, engine.num_layers, 512)
            assert all(np.array_equal(dlatents[:, row], dlatents[:, 0]) for row in range(1, engine.num_layers)), (batch, psi)
            if psi == 0.0:
                assert np.array_equal(dlatents[:, 0], np.broadcast_to(variables["dlatent_avg"], (batch, 512))), batch
            if psi == 1.0:  # (not asked to the bit: a + (w - a) rounds twice)
                assert np.abs(dlatents[:, 0] - mapped).max() <= 2.0 ** -22 * np.abs(mapped).max()
            figures.append(fe.judge(f"truncation, batch {batch}, psi {psi}", dlatents, fe.truncation(mapped, variables, psi, engine.num_layers, torch.float64),
                                    fe.truncation(mapped, variables, psi, engine.num_layers, torch.float32), failures))
    _summary("truncation", figures)
    assert not failures, "; ".join(failures)


# ---- styles and demodulation ----


def _styles_of_call(engine: hip_lib.Engine, spec: sg2_spec.SynthesisSpec, dlatents: np.ndarray) -> Dict[tuple, np.ndarray]:
    """{(kind, index): style [B, cin]} of every layer, from one w-call stopped after conv layer 1."""
    batch = engine.debug_run_front_end(dlatents)
    return {(kind, index): engine.debug_read_style(batch, kind, index) for kind, index, _, _ in fe.style_layers(spec)}


@pytest.mark.parametrize("network,batch", fe.STYLE_CASES)
def test_every_style_matches_float64(engines: Dict[str, hip_lib.Engine], network: str, batch: int) -> None:
    engine, spec, variables = engines[network], fe.spec_of(network), fe.variables_of(network)
    dlatents = fe.dlatents_of(network, batch)
    styles = _styles_of_call(engine, spec, dlatents)
    failures: List[str] = []
    figures = []
    for kind, index, scope, row in fe.style_layers(spec):
        got = styles[(kind, index)]
        assert got.shape == (batch, (spec.convs if kind == "conv" else spec.torgbs)[index].cin)
        figures.append(fe.judge(f"{network} batch {batch} style of {kind} {index} ({scope})", got, fe.style(dlatents[:, row], variables, scope, torch.float64),
                                fe.style(dlatents[:, row], variables, scope, torch.float32), failures))
    _summary(f"{network} batch {batch} styles", figures)
    assert not failures, "; ".join(failures)


def _judge_demod(label: str, engine: hip_lib.Engine, spec: sg2_spec.SynthesisSpec, variables: dict, dlatents: np.ndarray, convs, failures: List[str]) -> List[fe.Figures]:
    """Every sample's demodulation of the given conv layers against float64 from the kernels' own float32 styles and the raw weights."""
    batch = engine.debug_run_front_end(dlatents)
    figures = []
    for index in convs:
        conv = spec.convs[index]
        styles, got = engine.debug_read_style(batch, "conv", index), engine.debug_read_demod(batch, index)
        assert got.shape == (batch, conv.cout) and np.all(np.isfinite(got)) and np.all(got > 0), (label, index)
        figures.append(fe.judge(f"{label} demod of conv {index} ({conv.scope})", got, fe.demod(styles, variables, conv.scope, torch.float64),
                                fe.demod(styles, variables, conv.scope, torch.float32), failures))
    _summary(f"{label} demod", figures)
    return figures


@pytest.mark.parametrize("network,batch,convs", fe.DEMOD_CASES, ids=[f"{name}-{batch}-convs{convs[0]}to{convs[-1]}" for name, batch, convs in fe.DEMOD_CASES])
def test_every_demodulation_matches_float64(engines: Dict[str, hip_lib.Engine], network: str, batch: int, convs: tuple) -> None:
    failures: List[str] = []
    _judge_demod(f"{network} batch {batch}", engines[network], fe.spec_of(network), fe.variables_of(network), fe.dlatents_of(network, batch), convs, failures)
    assert not failures, "; ".join(failures)


def test_demodulation_where_the_epsilon_is_half_the_sum(engines: Dict[str, hip_lib.Engine]) -> None:
    case = fe.epsilon_case()
    engine, spec = engines["epsilon"], fe.spec_of(fe.EPSILON_NETWORK)
    failures: List[str] = []
    _judge_demod("epsilon case", engine, spec, case.variables, case.dlatents, case.convs, failures)
    for index in case.convs:  # (the call of _judge_demod is the engine's last)
        conv = spec.convs[index]
        styles, got = engine.debug_read_style(fe.EPSILON_BATCH, "conv", index), engine.debug_read_demod(fe.EPSILON_BATCH, index)
        share = np.delete(fe.epsilon_share(styles, case.variables, conv.scope), fe.EPSILON_ZERO_SAMPLE, axis=0)
        print(f"epsilon case conv {index}: 1e-8 is {share.min():.2f} ... {share.max():.2f} of the sum under the root of the kernel's styles")
        assert np.mean((share > 0.1) & (share < 0.9)) > 0.9
        # the sample whose dlatent rows are zero: bias1 = -1 + 1 = 0 exactly, s = 0, d = 1 / sqrt(1e-8) to float32 rounding
        assert not styles[fe.EPSILON_ZERO_SAMPLE].any()
        zero = got[fe.EPSILON_ZERO_SAMPLE].astype(np.float64)
        assert np.all(np.isfinite(zero)) and np.abs(zero * np.sqrt(1e-8) - 1.0).max() <= 4 * 2.0 ** -23, index  # (1e-8f, the sum, the root, the quotient: an ulp each at the most)
    assert not failures, "; ".join(failures)


# ---- bits ----


def test_a_sample_does_not_depend_on_the_batch_it_comes_in(engines: Dict[str, hip_lib.Engine]) -> None:
    network = "stress-128-f"
    engine, spec = engines[network], fe.spec_of(network)
    z_one, z_many = fe.mapping_z(1), fe.mapping_z(64).copy()
    w_one, w_many = fe.dlatents_of(network, 1), fe.dlatents_of(network, 64).copy()
    for position in fe.BIT_POSITIONS:
        z_many[position], w_many[position] = z_one[0], w_one[0]
    for n in (1, 8):
        alone, together = engine.debug_mapping_after(z_one, n), engine.debug_mapping_after(z_many, n)
        assert all(np.array_equal(together[position], alone[0]) for position in fe.BIT_POSITIONS), n
        assert np.array_equal(together, engine.debug_mapping_after(z_many, n))  # two runs of the same call
    alone, together = engine.debug_dlatents(z_one, 0.7), engine.debug_dlatents(z_many, 0.7)
    assert all(np.array_equal(together[position], alone[0]) for position in fe.BIT_POSITIONS)
    assert np.array_equal(together, engine.debug_dlatents(z_many, 0.7))

    def front_end(dlatents: np.ndarray) -> Dict[tuple, np.ndarray]:
        values = _styles_of_call(engine, spec, dlatents)
        values.update({("demod", index): engine.debug_read_demod(dlatents.shape[0], index) for index in range(len(spec.convs))})
        return values

    alone, together, again = front_end(w_one), front_end(w_many), front_end(w_many)
    assert np.array_equal(engine.debug_style(w_one, "torgb", 1), alone[("torgb", 1)]) and np.array_equal(engine.debug_demod(w_one, 3), alone[("demod", 3)])
    assert sorted(alone) == sorted(together) and len(alone) == 2 * len(spec.convs) + len(spec.torgbs)
    for key, values in together.items():
        assert all(np.array_equal(values[position], alone[key][0]) for position in fe.BIT_POSITIONS), key
        assert np.array_equal(values, again[key]), key
        assert not np.array_equal(values[1], values[0]), key  # (the other samples are other samples)


# ---- validation ----


def test_the_taps_refuse_bad_arguments_and_write_nothing(engines: Dict[str, hip_lib.Engine]) -> None:
    network = "stress-128-f"
    engine, other, spec = engines[network], engines["perturb-128-f"], fe.spec_of(network)
    lib, handle = hip_lib.load_library(), engine._handle  # pylint: disable=protected-access
    assert engine.num_layers == spec.num_layers == 12 and engine.max_batch == 64
    out = np.full(65 * 12 * 512, 7.0, dtype=np.float32)
    z = fe.mapping_z(64)
    z_pointer, pointer, invalid = z.ctypes.data_as(_F32P), out.ctypes.data_as(_F32P), 1  # GANCE_ERR_INVALID_ARGUMENT
    room = ctypes.c_uint64(out.size)
    assert engine.debug_run_front_end(fe.dlatents_of(network, 7)) == 7
    refused = [
        # a NULL engine, input or output
        lib.gance_engine_debug_mapping(None, z_pointer, 1, 8, pointer, room),
        lib.gance_engine_debug_mapping(handle, None, 1, 8, pointer, room),
        lib.gance_engine_debug_mapping(handle, z_pointer, 1, 8, None, room),
        lib.gance_engine_debug_dlatents(None, z_pointer, 1, 0.7, pointer, room),
        lib.gance_engine_debug_dlatents(handle, z_pointer, 1, 0.7, None, room),
        lib.gance_engine_debug_read_style(None, 0, 0, 7, pointer, room),
        lib.gance_engine_debug_read_style(handle, 0, 0, 7, None, room),
        lib.gance_engine_debug_read_demod(None, 0, 7, pointer, room),
        lib.gance_engine_debug_read_demod(handle, 0, 7, None, room),
        # a layer out of range
        lib.gance_engine_debug_mapping(handle, z_pointer, 1, 0, pointer, room),
        lib.gance_engine_debug_mapping(handle, z_pointer, 1, 9, pointer, room),
        lib.gance_engine_debug_read_style(handle, 0, len(spec.convs), 7, pointer, room),
        lib.gance_engine_debug_read_style(handle, 1, len(spec.torgbs), 7, pointer, room),
        lib.gance_engine_debug_read_style(handle, 0, -1, 7, pointer, room),
        lib.gance_engine_debug_read_style(handle, 2, 0, 7, pointer, room),
        lib.gance_engine_debug_read_demod(handle, len(spec.convs), 7, pointer, room),
        lib.gance_engine_debug_read_demod(handle, -1, 7, pointer, room),
        # a batch outside [1, max_batch], or not the last call's
        lib.gance_engine_debug_mapping(handle, z_pointer, 65, 8, pointer, room),
        lib.gance_engine_debug_mapping(handle, z_pointer, 0, 8, pointer, room),
        lib.gance_engine_debug_dlatents(handle, z_pointer, 65, 0.7, pointer, room),
        lib.gance_engine_debug_read_style(handle, 0, 0, 65, pointer, room),
        lib.gance_engine_debug_read_style(handle, 0, 0, 8, pointer, room),
        lib.gance_engine_debug_read_demod(handle, 0, 65, pointer, room),
        lib.gance_engine_debug_read_demod(handle, 0, 6, pointer, room),
        # an output buffer one float too small
        lib.gance_engine_debug_mapping(handle, z_pointer, 64, 8, pointer, ctypes.c_uint64(64 * 512 - 1)),
        lib.gance_engine_debug_dlatents(handle, z_pointer, 64, 0.7, pointer, ctypes.c_uint64(64 * 12 * 512 - 1)),
        lib.gance_engine_debug_read_style(handle, 0, 0, 7, pointer, ctypes.c_uint64(7 * 512 - 1)),
        lib.gance_engine_debug_read_demod(handle, len(spec.convs) - 1, 7, pointer, ctypes.c_uint64(7 * 256 - 1)),
    ]
    assert refused == [invalid] * len(refused), refused
    assert np.all(out == 7.0)
    # the two 128^2 engines share one workspace: after the other's call the styles there are not this engine's
    assert engine.debug_read_style(7, "conv", 0).shape == (7, 512)
    other.debug_run_front_end(fe.dlatents_of("perturb-128-f", 7))
    with pytest.raises(hip_lib.GanceHipError) as error:
        engine.debug_read_style(7, "conv", 0)
    assert error.value.status == invalid
    assert other.debug_read_demod(7, 0).shape == (7, 512)
    # ... and the engine still runs a whole call after all that
    frames = engine.synthesize_w(fe.dlatents_of(network, 1))
    assert frames.shape == (1, 128, 128, 3)
