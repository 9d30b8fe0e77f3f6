"""
CPU tests of tests/front_end_ref.py, the reference of the device tests of the front end (tests/test_front_end_gpu.py): mapping
network, truncation, styles and demodulation.

- The restatements composed end to end ARE the chain: ref.g_mapping, ref.truncate and the style and demodulation inside
  ref.modulated_conv2d_layer, to the bit, in float64 and float32.
- The bars are not vacuous: the judge of the device tests rejects each of a list of deliberately wrong float32 restatements, by
  at least 2 x its bar, on the inputs the device tests use. That is a condition on the inputs (the bar is 8 x the float32
  restatement's own error whatever comes of it): a variant that is not rejected calls for other inputs.
- The taps cover the plan: the launches of a call that belong to no layer are exactly `styles` and `demod`, for both 1024^2
  networks at 1 ... 64 frames (with the mapping launches and `truncate`, which gance_engine_describe_plan does not list: they
  are in front of a z call only). A layer's launches are `conv...`, `torgb...` and the second launch of a conv step that has
  one (`finish<N>`, `fir<N>`: config-e's default plan has them), held to stand right behind its conv launch. A new front-end
  kernel fails here until it has a tap.
- The case table reaches every layer, and the epsilon case has the epsilon under its root that it claims.
"""

import json
import os
import subprocess
import sys
from typing import Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import front_end_ref as fe
import isolated_small_cases as small_cases
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

# ---- the restatements equal the chain ----

CHAIN_NETWORKS = ((32, sg2_spec.FMAP_BASE), (64, sg2_spec.FMAP_BASE_CONFIG_E))  # (config-e differs from config-f from 64^2 on)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32), ids=("float64", "float32"))
@pytest.mark.parametrize("resolution,fmap_base", CHAIN_NETWORKS, ids=("32-f", "64-e"))
def test_the_restatements_composed_are_the_chain(resolution: int, fmap_base: int, dtype: torch.dtype, monkeypatch: pytest.MonkeyPatch) -> None:
    spec = sg2_spec.make_spec(resolution, fmap_base)
    variables = sg2_spec.make_stress_variables(resolution, seed=resolution, fmap_base=fmap_base)
    z = np.random.RandomState(resolution).randn(3, 512).astype(np.float32)
    with torch.no_grad():
        mapped = ref.g_mapping(torch.from_numpy(z).to(dtype), variables, spec.num_layers)
        dlatents = ref.truncate(mapped, variables, 0.7)
    chain = fe.mapping_chain(z, variables, dtype)
    assert len(chain) == 8 and torch.equal(chain[-1], mapped[:, 0]) and torch.equal(mapped, chain[-1][:, None, :].repeat(1, spec.num_layers, 1))
    assert torch.equal(fe.truncation(chain[-1], variables, 0.7, spec.num_layers, dtype), dlatents)
    assert torch.equal(fe.truncation(chain[-1], variables, 0.0, spec.num_layers, dtype)[1, 3], ref._t(variables, "dlatent_avg", dtype))  # pylint: disable=protected-access

    # the style and the demodulation that ref.modulated_conv2d_layer computes on its way through g_synthesis, by scope
    seen = {}
    real_style, real_demodulation = ref.layer_style, ref.layer_demodulation

    def spy_style(y, spied_variables, scope):
        seen[scope] = [real_style(y, spied_variables, scope), None]
        return seen[scope][0]

    def spy_demodulation(s, w, modulated=None):
        scope = next(scope for scope, (style, _) in seen.items() if style is s)
        assert modulated is not None  # (the layer hands over its own product)
        seen[scope][1] = real_demodulation(s, w, modulated=modulated)
        return seen[scope][1]

    monkeypatch.setattr(ref, "layer_style", spy_style)
    monkeypatch.setattr(ref, "layer_demodulation", spy_demodulation)
    rows = torch.from_numpy(np.random.RandomState(resolution + 1).randn(3, spec.num_layers, 512).astype(np.float32)).to(dtype)
    with torch.no_grad():
        ref.g_synthesis(rows, variables, resolution)
    monkeypatch.undo()
    assert sorted(seen) == sorted(f"G_synthesis/{scope}" for _, _, scope, _ in fe.style_layers(spec))
    for kind, _, scope, row in fe.style_layers(spec):
        in_chain_style, in_chain_demod = seen[f"G_synthesis/{scope}"]
        restated = fe.style(rows[:, row], variables, scope, dtype)
        assert torch.equal(restated, in_chain_style), scope
        if kind == "conv":
            assert torch.equal(fe.demod(restated, variables, scope, dtype, chunk=2), in_chain_demod), scope
        else:
            assert in_chain_demod is None, scope  # (a ToRGB does not demodulate)


# ---- the bars are not vacuous: deliberately wrong float32 restatements ----


def wrong_dense(x: np.ndarray, variables: ref.Variables, n: int, epsilon: float = 1e-8, epsilon_outside: bool = False,
                gain: float = float(np.sqrt(2.0)), lrmul_on_bias: bool = True) -> torch.Tensor:
    """Dense layer n in float32, written out; with the defaults it is fe.dense(..., float32) to the bit."""
    x = torch.from_numpy(np.asarray(x, dtype=np.float32))
    if n == 1:
        mean_square = (x ** 2).mean(dim=1, keepdim=True)
        x = x / (torch.sqrt(mean_square) + epsilon) if epsilon_outside else x * torch.rsqrt(mean_square + epsilon)
    w = torch.from_numpy(variables[f"G_mapping/Dense{n - 1}/weight"]) * (1.0 / np.sqrt(512.0) * 0.01)
    b = torch.from_numpy(variables[f"G_mapping/Dense{n - 1}/bias"]) * (0.01 if lrmul_on_bias else 1.0)
    return F.leaky_relu(x @ w + b.reshape(1, -1), 0.2) * gain


def wrong_truncation(mapped: torch.Tensor, variables: ref.Variables, psi: float, num_layers: int, shift: int = 0) -> torch.Tensor:
    avg = torch.from_numpy(np.roll(variables["dlatent_avg"], -shift))[None, None]  # shift 1: element k reads avg[k + 1]
    dlatents = mapped[:, None, :].repeat(1, num_layers, 1)
    return avg + (dlatents - avg) * psi


def wrong_style(dlatents: np.ndarray, variables: ref.Variables, scope: str, row: int, plus_one: bool = True, dropped_slice: Optional[int] = None) -> torch.Tensor:
    y = torch.from_numpy(dlatents[:, row])
    mod_w = torch.from_numpy(variables[f"G_synthesis/{scope}/mod_weight"]) * (1.0 / np.sqrt(512.0))
    if dropped_slice is not None:  # one of the eight k-slices of the 512-long sum
        mod_w = mod_w.clone()
        mod_w[dropped_slice * 64 : (dropped_slice + 1) * 64] = 0.0
    s = y @ mod_w + torch.from_numpy(variables[f"G_synthesis/{scope}/mod_bias"])[None]
    return s + 1.0 if plus_one else s


def wrong_demod(styles: torch.Tensor, variables: ref.Variables, scope: str, epsilon: float = 1e-8, epsilon_outside: bool = False,
                dropped_tap: Optional[int] = None, dropped_slice: Optional[int] = None) -> torch.Tensor:
    raw = torch.from_numpy(variables[f"G_synthesis/{scope}/weight"])  # [3, 3, I, O]
    w = raw * (1.0 / np.sqrt(float(9 * raw.shape[2])))
    results = []
    for first in range(0, styles.shape[0], 8):
        ww = w[None] * styles[first : first + 8, None, None, :, None]
        if dropped_tap is not None:
            ww = ww.clone()
            ww[:, dropped_tap // 3, dropped_tap % 3] = 0.0
        if dropped_slice is not None:  # one of the eight k-slices of the sum over input channels
            width = raw.shape[2] // 8
            ww = ww.clone()
            ww[:, :, :, dropped_slice * width : (dropped_slice + 1) * width] = 0.0
        total = (ww ** 2).sum(dim=(1, 2, 3))
        results.append(1.0 / (torch.sqrt(total) + epsilon) if epsilon_outside else torch.rsqrt(total + epsilon))
    return torch.cat(results)


REJECTED = 2.0  # every variant is this many times over its bar


def _rejected(label: str, wrong: torch.Tensor, want64: torch.Tensor, want32: torch.Tensor, right: torch.Tensor) -> None:
    assert torch.equal(right, want32), f"{label}: the variant's code with nothing wrong is not the float32 restatement"
    figures = fe.measure(wrong, want64, want32)
    print(f"{label}: error {figures.error:.3e} over bar {figures.bar:.3e} = {figures.error / figures.bar:.1f}")
    assert not figures.passed and figures.error >= REJECTED * figures.bar, label


@pytest.mark.parametrize("network", fe.MAPPING_NETWORKS)
def test_the_judge_rejects_wrong_mapping_layers(network: str) -> None:
    variables = fe.variables_of(network)
    for batch in fe.MAPPING_BATCHES:
        # the epsilons where the device test has them show: z times 1e-3
        z = fe.mapping_z(batch, 1e-3)
        want64, want32 = fe.dense(z, variables, 1, torch.float64), fe.dense(z, variables, 1, torch.float32)
        right = wrong_dense(z, variables, 1)
        _rejected(f"{network} batch {batch}: pixel-norm epsilon 1e-7", wrong_dense(z, variables, 1, epsilon=1e-7), want64, want32, right)
        _rejected(f"{network} batch {batch}: pixel-norm epsilon outside the root", wrong_dense(z, variables, 1, epsilon_outside=True), want64, want32, right)
        # lrmul in every layer, each on the float32 chain's output of the layer before it
        chain = [torch.from_numpy(fe.mapping_z(batch))] + fe.mapping_chain(fe.mapping_z(batch), variables, torch.float32)
        for n in range(1, 9):
            x = chain[n - 1].numpy()
            want64, want32 = fe.dense(x, variables, n, torch.float64), fe.dense(x, variables, n, torch.float32)
            right = wrong_dense(x, variables, n)
            _rejected(f"{network} batch {batch} layer {n}: lrmul on the weight only", wrong_dense(x, variables, n, lrmul_on_bias=False), want64, want32, right)
    # The gain: 1.41421f is 2.5e-6 short of sqrt(2), and a float32 sum of 512 products of N(0, 1) inputs is itself 3e-7 ... 7e-7 of
    # the tensor's maximum off (bars of 2.4e-6 ... 5.6e-6: that variant is 0.4 ... 1.1 of them at every layer and batch above). The
    # all-zero sample's row of layer 1 has no sum, only bias * lrmul, leaky ReLU and the gain (float32 restatement 9e-8 off): the
    # device test judges that row as a tensor of its own, and there the variant shows. One kernel runs all eight layers.
    z = fe.mapping_z_with_a_zero_sample()[fe.ZERO_SAMPLE : fe.ZERO_SAMPLE + 1]
    want64, want32 = fe.dense(z, variables, 1, torch.float64), fe.dense(z, variables, 1, torch.float32)
    _rejected(f"{network} the zero sample's row of layer 1: gain 1.41421f", wrong_dense(z, variables, 1, gain=float(np.float32(1.41421))), want64, want32,
              wrong_dense(z, variables, 1))


def test_the_judge_rejects_a_truncation_that_reads_the_next_element_of_the_average() -> None:
    variables = fe.variables_of(fe.TRUNCATION_NETWORK)
    num_layers = fe.spec_of(fe.TRUNCATION_NETWORK).num_layers
    assert np.std(variables["dlatent_avg"]) > 0.25  # (not constant)
    for batch in fe.TRUNCATION_BATCHES:
        mapped = fe.mapping_chain(fe.mapping_z(batch), variables, torch.float32)[-1]
        for psi in fe.TRUNCATION_PSIS:
            if psi == 1.0:  # (the average cancels: a + (w - a) = w whichever element a is)
                continue
            want64, want32 = (fe.truncation(mapped, variables, psi, num_layers, dtype) for dtype in (torch.float64, torch.float32))
            _rejected(f"batch {batch} psi {psi}: avg[k + 1]", wrong_truncation(mapped, variables, psi, num_layers, shift=1), want64, want32,
                      wrong_truncation(mapped, variables, psi, num_layers))


STYLE_VARIANT_CASES = [("stress-128-f", 9), ("perturb-128-f", 9), ("perturb-1024-e", 3)]


@pytest.mark.parametrize("network,batch", STYLE_VARIANT_CASES)
def test_the_judge_rejects_wrong_styles(network: str, batch: int) -> None:
    assert (network, batch) in fe.STYLE_CASES
    spec, variables, dlatents = fe.spec_of(network), fe.variables_of(network), fe.dlatents_of(network, batch)
    for kind, index, scope, row in fe.style_layers(spec):
        label = f"{network} batch {batch} {kind} {index}"
        want64, want32 = (fe.style(dlatents[:, row], variables, scope, dtype) for dtype in (torch.float64, torch.float32))
        right = wrong_style(dlatents, variables, scope, row)
        if network.startswith("stress"):  # (mod_bias ~ N(0, 3): where a missing + 1 is smallest against the style's maximum)
            _rejected(f"{label}: no + 1", wrong_style(dlatents, variables, scope, row, plus_one=False), want64, want32, right)
        if row + 1 < spec.num_layers:
            _rejected(f"{label}: dlatent row + 1", wrong_style(dlatents, variables, scope, row + 1), want64, want32, right)
        if kind == "torgb":  # the row of the Conv1 of the same resolution
            _rejected(f"{label}: the conv's dlatent row", wrong_style(dlatents, variables, scope, row - 1), want64, want32, right)
        for dropped in (0, 7):
            _rejected(f"{label}: k-slice {dropped} dropped", wrong_style(dlatents, variables, scope, row, dropped_slice=dropped), want64, want32, right)


@pytest.mark.parametrize("network,batch", [("stress-128-f", 7), ("perturb-1024-e", 3)])
def test_the_judge_rejects_wrong_demodulation(network: str, batch: int) -> None:
    assert any(case[:2] == (network, batch) for case in fe.DEMOD_CASES)
    spec, variables, dlatents = fe.spec_of(network), fe.variables_of(network), fe.dlatents_of(network, batch)
    for index, conv in enumerate(spec.convs):
        label = f"{network} batch {batch} conv {index}"
        styles = fe.style(dlatents[:, conv.layer_idx], variables, conv.scope, torch.float32)
        want64, want32 = (fe.demod(styles, variables, conv.scope, dtype) for dtype in (torch.float64, torch.float32))
        right = wrong_demod(styles, variables, conv.scope)
        for tap in (0, 4, 8):
            _rejected(f"{label}: tap {tap} left out of w2", wrong_demod(styles, variables, conv.scope, dropped_tap=tap), want64, want32, right)
        for dropped in (0, 7):
            _rejected(f"{label}: k-slice {dropped} dropped", wrong_demod(styles, variables, conv.scope, dropped_slice=dropped), want64, want32, right)


def test_the_epsilon_case_is_what_it_claims_and_shows_a_wrong_epsilon() -> None:
    case = fe.epsilon_case()
    spec = fe.spec_of(fe.EPSILON_NETWORK)
    assert [spec.convs[i].scope for i in case.convs] == ["4x4/Conv", "16x16/Conv1", "128x128/Conv1"]
    assert [(spec.convs[i].cin, spec.convs[i].cout) for i in case.convs] == [(512, 512), (512, 512), (256, 256)]
    assert case.dlatents.shape[0] == fe.EPSILON_BATCH <= fe.EPSILON_MAX_BATCH
    for index in case.convs:
        conv = spec.convs[index]
        assert np.all(case.variables[f"G_synthesis/{conv.scope}/mod_bias"] == -1.0)
        assert not np.any(case.dlatents[fe.EPSILON_ZERO_SAMPLE, conv.layer_idx]) and np.all(np.any(case.dlatents[:, conv.layer_idx], axis=1)[np.arange(fe.EPSILON_BATCH) != fe.EPSILON_ZERO_SAMPLE])
        styles = fe.style(case.dlatents[:, conv.layer_idx], case.variables, conv.scope, torch.float32)
        # (mod_bias + 1 = 0 exactly, as in the engine's bias1: the float32 style is the affine part alone, and zero for the zero rows)
        assert not styles[fe.EPSILON_ZERO_SAMPLE].any()
        share = fe.epsilon_share(styles, case.variables, conv.scope)
        others = np.delete(share, fe.EPSILON_ZERO_SAMPLE, axis=0)
        print(f"conv {index}: dlatent row times {case.scales[index]:.3e}; 1e-8 is {others.min():.2f} ... {others.max():.2f} of the sum under the root")
        assert np.all(share[fe.EPSILON_ZERO_SAMPLE] == 1.0)
        assert np.mean((others > 0.1) & (others < 0.9)) > 0.9  # (asked for: at least one layer with such an element)
        want64, want32 = (fe.demod(styles, case.variables, conv.scope, dtype) for dtype in (torch.float64, torch.float32))
        assert np.all(np.isfinite(want32.numpy())) and abs(float(want64[fe.EPSILON_ZERO_SAMPLE, 0]) - 1e4) < 1e-6
        right = wrong_demod(styles, case.variables, conv.scope)
        _rejected(f"conv {index}: demodulation epsilon 1e-7", wrong_demod(styles, case.variables, conv.scope, epsilon=1e-7), want64, want32, right)
        _rejected(f"conv {index}: demodulation epsilon outside the root", wrong_demod(styles, case.variables, conv.scope, epsilon_outside=True), want64, want32, right)


# ---- the case table ----


def test_the_case_table_is_well_formed() -> None:
    assert [(n.resolution, n.fmap_base, n.max_batch) for n in fe.NETWORKS.values()] == [
        (128, sg2_spec.FMAP_BASE, 64), (128, sg2_spec.FMAP_BASE, 64), (1024, sg2_spec.FMAP_BASE, 9), (1024, sg2_spec.FMAP_BASE_CONFIG_E, 9),
    ]
    assert [n.kind for n in fe.NETWORKS.values()] == ["stress", "perturb", "perturb", "perturb"]
    for name, network in fe.NETWORKS.items():
        assert all(1 <= batch <= network.max_batch for batch in network.batches), name
        assert sg2_spec.fmap_base_of(fe.variables_of(name), network.resolution) == network.fmap_base, name
    for name in ("stress-128-f", "perturb-128-f"):
        assert fe.NETWORKS[name].batches == (1, 7, 8, 9, 17, 64)
    assert fe.NETWORKS["perturb-1024-f"].batches == (1, 9) and fe.NETWORKS["perturb-1024-e"].batches == (3, 9)
    # every conv and every ToRGB of each network in a style case, every conv in a demod case (the device test walks
    # style_layers(spec) and spec.convs for each of these cases)
    assert fe.STYLE_CASES == [(name, batch) for name, network in fe.NETWORKS.items() for batch in network.batches]
    assert {7, 8, 9} <= {batch for _, batch in fe.STYLE_CASES}
    for name, batch in fe.STYLE_CASES:  # (a 64-frame call's demod is spread over two cases)
        covered = [index for case_name, case_batch, convs in fe.DEMOD_CASES if (case_name, case_batch) == (name, batch) for index in convs]
        assert covered == list(range(len(fe.spec_of(name).convs))), (name, batch)
    assert {case[:2] for case in fe.DEMOD_CASES} == set(fe.STYLE_CASES)
    for name in fe.NETWORKS:
        spec = fe.spec_of(name)
        layers = fe.style_layers(spec)
        assert [(kind, index) for kind, index, _, _ in layers] == [("conv", i) for i in range(len(spec.convs))] + [("torgb", i) for i in range(len(spec.torgbs))]
        assert all(row == (spec.convs[index].layer_idx if kind == "conv" else spec.torgbs[index].dlatent_row) for kind, index, _, row in layers)
    # what each network is there for
    channels = {name: sorted({conv.cin for conv in fe.spec_of(name).convs} | {conv.cout for conv in fe.spec_of(name).convs}) for name in fe.NETWORKS}
    assert channels["stress-128-f"] == channels["perturb-128-f"] == [256, 512]
    assert channels["perturb-1024-f"] == [32, 64, 128, 256, 512] and channels["perturb-1024-e"] == [16, 32, 64, 128, 256, 512]
    # per-row-distinct dlatents, the same draws at every scale of z
    dlatents = fe.dlatents_of("perturb-1024-e", 3)
    assert len({row.tobytes() for sample in dlatents for row in sample}) == dlatents.shape[0] * dlatents.shape[1]
    assert np.allclose(fe.mapping_z(5, 1e3), fe.mapping_z(5) * 1e3, rtol=1e-6)
    assert fe.MAPPING_BATCHES == (1, 5, 64) and fe.MAPPING_SCALES == (1.0, 1e-3, 1e3) and fe.TRUNCATION_BATCHES == (1, 64)
    assert fe.TRUNCATION_PSIS == (0.0, 0.5, 0.7, 1.0, 1.2, -0.5) and fe.BIT_POSITIONS == (0, 7, 8, 63)
    zero = fe.mapping_z_with_a_zero_sample()
    assert zero.shape == (5, 512) and not zero[2].any() and all(zero[i].any() for i in (0, 1, 3, 4))


# ---- the taps cover the plan ----

# gance_engine_describe_plan in a fresh child, every GANCE_TUNE_* variable stripped (the knobs are read once per process), as
# tests/test_isolated_coverage.py calls it
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
num_cus, max_batch = int(sys.argv[2]), int(sys.argv[3])
out = ctypes.create_string_buffer(1 << 16)
plans = {}
for resolution, flags in json.loads(sys.argv[4]):
    config = (ctypes.c_int32 * 4)(resolution, max_batch, 0, flags)  # gance_engine_config: resolution, max_batch, device, flags
    plans[f"{resolution}/{flags}"] = {}
    for batch in range(1, max_batch + 1):
        status = lib.gance_engine_describe_plan(config, ctypes.c_int32(num_cus), ctypes.c_int32(batch), out, ctypes.c_uint64(len(out)))
        assert status == 0, status
        plans[f"{resolution}/{flags}"][batch] = out.value.decode().split()
print(json.dumps(plans))
"""


def _belongs_to_a_layer(name: str) -> bool:
    """conv... and torgb... launches, and the second launch of a conv layer's step (engine_plan.h, name_step: finish<N>, fir<N>)."""
    return name.startswith(("conv", "torgb", "finish", "fir"))


def test_the_launches_in_front_of_the_layers_are_the_two_with_a_tap() -> None:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    env = {key: value for key, value in os.environ.items() if not key.startswith("GANCE_TUNE_")}
    child = subprocess.run(
        [sys.executable, "-c", _CHILD, str(hip_lib.LIBRARY_PATH), str(small_cases.NUM_CUS), "64",
         json.dumps([[1024, 0], [1024, hip_lib.GANCE_FLAG_FMAP_BASE_8K]])],
        check=True, env=env, capture_output=True, text=True, timeout=120,
    )
    plans = json.loads(child.stdout)
    assert sorted(plans) == ["1024/0", f"1024/{hip_lib.GANCE_FLAG_FMAP_BASE_8K}"]
    for key, by_batch in plans.items():
        assert sorted(int(batch) for batch in by_batch) == list(range(1, 65))
        for batch, names in by_batch.items():
            assert [name for name in names if not _belongs_to_a_layer(name)] == ["styles", "demod"], (key, batch)
            assert names[:2] == ["styles", "demod"], (key, batch)
            # ... and a second launch never stands alone: its conv launch is right in front of it
            for position, name in enumerate(names):
                if name.startswith(("finish", "fir")):
                    layer = int("".join(ch for ch in name.split("_")[0] if ch.isdigit()))
                    assert set(small_cases.conv_launches([names[position - 1]])) == {layer}, (key, batch, name)
