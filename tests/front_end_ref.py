"""
Reference for the part of a call in front of the first convolution (tests/test_front_end.py, tests/test_front_end_gpu.py): the
eight dense layers of the mapping network, truncation, and the style and demodulation vectors of every layer.

Each restatement is the function the whole chain calls, of `oracle/stylegan2_ref.py` (`mapping_dense_layer`, `truncate`,
`layer_style`, `layer_demodulation`), applied to ONE stage's input: the float32 values the kernels left in front of that stage,
promoted to float64, or kept in float32 for the yardstick. So a stage is judged on its own arithmetic, not on what reached it.

The error measure is `grad_ref.relative_error` of one tensor: max|got - ref64| / max|ref64|, where a tensor is one stage's
[B, n] block of one layer (the layers of the stress network differ in scale by 100 x: never the whole styles buffer).
The bar is `grad_ref.GRADIENT_BAR_FACTOR` (8) x the error of the float32 restatement on the same inputs, and never below
2^-23: one float32 ulp of the tensor's maximum, without which an elementwise stage whose float32 restatement happens to be
exact (truncation with psi = 0) would get a zero bar. No bar is taken from the output of the code under test.

The seeded inputs of the device tests are made here, so that the CPU test can hold them to the conditions they are there for.
"""

import functools
from typing import Dict, List, NamedTuple, Tuple, Union

import numpy as np
import torch

import grad_ref
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

ULP = 2.0 ** -23
BAR_FACTOR = grad_ref.GRADIENT_BAR_FACTOR
DEMOD_EPSILON = 1e-8
Array = Union[np.ndarray, torch.Tensor]


class Network(NamedTuple):
    """A network of the device tests: how it is made, the engine's max_batch and the batches of its style and demod cases."""

    kind: str  # "stress": make_stress_variables, "perturb": make_random_variables(perturb=True)
    resolution: int
    fmap_base: int
    seed: int
    max_batch: int
    batches: Tuple[int, ...]


# The 128^2 config-f networks: channels 512 ... 256, every remainder class of the eight-sample groups that matters (1, 7, 8, 9, 17)
# and the largest call the product issues (64). The 1024^2 config-f network: the 128-, 64- and 32-channel layers (K / 8 = 16 ... 4),
# one full group and a group of one. The 1024^2 config-e network: the 16-channel layers (cout < 32: a half-filled demod block;
# cin = 16: K / 8 = 2 and a half-filled style block).
NETWORKS: Dict[str, Network] = {
    "stress-128-f": Network("stress", 128, sg2_spec.FMAP_BASE, 41, 64, (1, 7, 8, 9, 17, 64)),
    "perturb-128-f": Network("perturb", 128, sg2_spec.FMAP_BASE, 42, 64, (1, 7, 8, 9, 17, 64)),
    "perturb-1024-f": Network("perturb", 1024, sg2_spec.FMAP_BASE, 43, 9, (1, 9)),
    "perturb-1024-e": Network("perturb", 1024, sg2_spec.FMAP_BASE_CONFIG_E, 44, 9, (3, 9)),
}
STYLE_CASES: List[Tuple[str, int]] = [(name, batch) for name, network in NETWORKS.items() for batch in network.batches]


def _demod_cases() -> List[Tuple[str, int, Tuple[int, ...]]]:
    """(network, batch, conv indices): every conv layer at every batch; a 64-frame call's in two cases (the float64 restatement
    of 64 samples of a 512 x 512 layer is 1.2 GB of modulated weights, walked eight samples at a time: half a second a layer)."""
    cases = []
    for name, batch in STYLE_CASES:
        convs = tuple(range(len(sg2_spec.make_spec(NETWORKS[name].resolution, NETWORKS[name].fmap_base).convs)))
        half = len(convs) // 2
        cases += [(name, batch, convs[:half]), (name, batch, convs[half:])] if batch >= 64 else [(name, batch, convs)]
    return cases


DEMOD_CASES = _demod_cases()

MAPPING_NETWORKS = ("stress-128-f", "perturb-128-f")
MAPPING_BATCHES = (1, 5, 64)
MAPPING_SCALES = (1.0, 1e-3, 1e3)  # the pixel-norm has to absorb the scale: at 1e-3 mean(z^2) ~ 1e-6 and its 1e-8 is 1 % of the sum
TRUNCATION_NETWORK = "stress-128-f"  # dlatent_avg ~ N(0, 0.5)
TRUNCATION_PSIS = (0.0, 0.5, 0.7, 1.0, 1.2, -0.5)
TRUNCATION_BATCHES = (1, 64)
BIT_POSITIONS = (0, 7, 8, 63)  # where one sample is put in a 64-frame call, and alone


def spec_of(name: str) -> sg2_spec.SynthesisSpec:
    network = NETWORKS[name]
    return sg2_spec.make_spec(network.resolution, network.fmap_base)


@functools.lru_cache(maxsize=None)
def variables_of(name: str) -> ref.Variables:
    """A network's variables, made once per process."""
    network = NETWORKS[name]
    if network.kind == "stress":
        return sg2_spec.make_stress_variables(network.resolution, seed=network.seed, fmap_base=network.fmap_base)
    return sg2_spec.make_random_variables(network.resolution, seed=network.seed, perturb=True, fmap_base=network.fmap_base)


# ---- the restatements: one stage each, in float64 (the reference) or float32 (the yardstick) ----


def _tensor(values: Array, dtype: torch.dtype) -> torch.Tensor:
    if isinstance(values, torch.Tensor):
        return values.detach().cpu().to(dtype)
    return torch.from_numpy(np.ascontiguousarray(values)).to(dtype)


def dense(x: Array, variables: ref.Variables, n: int, dtype: torch.dtype) -> torch.Tensor:
    """Dense layer n (1 ... 8) of the mapping network on x [B, 512]: layer 1 takes z and normalises it first."""
    with torch.no_grad():
        return ref.mapping_dense_layer(_tensor(x, dtype), variables, n - 1, normalize=n == 1)


def mapping_chain(z: Array, variables: ref.Variables, dtype: torch.dtype) -> List[torch.Tensor]:
    """The outputs of all eight dense layers, each from the one before it in `dtype` (the last is g_mapping's row)."""
    outputs, x = [], _tensor(z, dtype)
    for n in range(1, sg2_spec.MAPPING_LAYERS + 1):
        x = dense(x, variables, n, dtype)
        outputs.append(x)
    return outputs


def truncation(mapped: Array, variables: ref.Variables, psi: float, num_layers: int, dtype: torch.dtype) -> torch.Tensor:
    """The dlatents [B, num_layers, 512] from the mapping network's output [B, 512]: g_mapping's broadcast, then `truncate`."""
    with torch.no_grad():
        return ref.truncate(_tensor(mapped, dtype)[:, None, :].repeat(1, num_layers, 1), variables, psi)


def style(dlatent_row: Array, variables: ref.Variables, scope: str, dtype: torch.dtype) -> torch.Tensor:
    """The style [B, cin] of the layer at G_synthesis/`scope` from its dlatent row [B, 512]."""
    with torch.no_grad():
        return ref.layer_style(_tensor(dlatent_row, dtype), variables, f"G_synthesis/{scope}")


def demod(styles: Array, variables: ref.Variables, scope: str, dtype: torch.dtype, chunk: int = 8) -> torch.Tensor:
    """The demodulation coefficients [B, cout] of the conv layer at G_synthesis/`scope` from its style [B, cin] (the modulated
    weights of `chunk` samples at a time: a 512 x 512 layer's are 19 MB per sample in float64)."""
    s = _tensor(styles, dtype)
    with torch.no_grad():
        w = ref._get_weight(ref._t(variables, f"G_synthesis/{scope}/weight", dtype))  # pylint: disable=protected-access
        return torch.cat([ref.layer_demodulation(s[first : first + chunk], w) for first in range(0, s.shape[0], chunk)])


def style_layers(spec: sg2_spec.SynthesisSpec) -> List[Tuple[str, int, str, int]]:
    """(kind, index, scope, dlatent row) of every layer that has a style: the conv layers, then the ToRGBs."""
    layers = [("conv", index, conv.scope, conv.layer_idx) for index, conv in enumerate(spec.convs)]
    return layers + [("torgb", index, rgb.scope, rgb.dlatent_row) for index, rgb in enumerate(spec.torgbs)]


# ---- the judge ----


class Figures(NamedTuple):
    error: float  # of the values judged, against the float64 restatement
    own: float  # of the float32 restatement, against the same
    bar: float

    @property
    def ratio(self) -> float:
        if self.own == 0.0:  # (truncation with psi = 0: the float32 restatement is exact, and so must the kernel be to show a ratio)
            return 0.0 if self.error == 0.0 else float("inf")
        return self.error / self.own

    @property
    def passed(self) -> bool:
        return bool(np.isfinite(self.error) and self.error <= self.bar)


def measure(got: Array, want64: torch.Tensor, want32: torch.Tensor) -> Figures:
    assert want64.dtype == torch.float64 and want32.dtype == torch.float32 and tuple(want64.shape) == tuple(want32.shape)
    got = _tensor(got, torch.float64)
    assert tuple(got.shape) == tuple(want64.shape), (tuple(got.shape), tuple(want64.shape))
    own = grad_ref.relative_error(want32, want64)
    return Figures(grad_ref.relative_error(got, want64), own, max(BAR_FACTOR * own, ULP))


def judge(label: str, got: Array, want64: torch.Tensor, want32: torch.Tensor, failures: List[str]) -> Figures:
    """Print one tensor's figures, then note a failure: the caller asserts on `failures` once everything of a case is on record."""
    figures = measure(got, want64, want32)
    print(f"{label}: error {figures.error:.3e}, float32 restatement {figures.own:.3e}, ratio {figures.ratio:.2f}, bar {figures.bar:.3e}")
    if not figures.passed:
        failures.append(f"{label}: {figures.error:.3e} > {figures.bar:.3e}")
    return figures


# ---- the seeded inputs of the device tests ----


def mapping_z(batch: int, scale: float = 1.0) -> np.ndarray:
    """z [batch, 512] ~ N(0, 1) times `scale` (the same draws at every scale)."""
    return (np.random.RandomState(7000 + batch).randn(batch, sg2_spec.LATENT_SIZE) * scale).astype(np.float32)


ZERO_SAMPLE = 2


def mapping_z_with_a_zero_sample() -> np.ndarray:
    """Five samples, the middle one all zero: its pixel-norm is 0 * rsqrt(1e-8) = 0 and its output the bias-only result."""
    z = mapping_z(5).copy()
    z[ZERO_SAMPLE] = 0.0
    return z


def mapping_cases() -> List[Tuple[str, np.ndarray]]:
    cases = [(f"batch {batch} scale {scale:g}", mapping_z(batch, scale)) for batch in MAPPING_BATCHES for scale in MAPPING_SCALES]
    return cases + [("batch 5 with a zero sample", mapping_z_with_a_zero_sample())]


def dlatents_of(name: str, batch: int) -> np.ndarray:
    """dlatents [batch, W, 512] drawn independently per row: a layer that reads the wrong row gets other values."""
    num_layers = spec_of(name).num_layers
    return np.random.RandomState(NETWORKS[name].seed * 1000 + batch).randn(batch, num_layers, sg2_spec.DLATENT_SIZE).astype(np.float32)


# ---- the epsilon case of the demodulation ----

EPSILON_NETWORK = "perturb-128-f"
EPSILON_CONVS = (0, 4, 10)  # the 4x4 layer, a 512-channel layer (16x16 Conv1), a 256-channel layer (128x128 Conv1)
EPSILON_BATCH = 9
EPSILON_ZERO_SAMPLE = 4
EPSILON_MAX_BATCH = 9


class EpsilonCase(NamedTuple):
    variables: ref.Variables
    dlatents: np.ndarray  # [EPSILON_BATCH, W, 512]
    convs: Tuple[int, ...]
    scales: Dict[int, float]  # per conv index: what its dlatent row was multiplied by


def _sum_under_the_root(styles: Array, variables: ref.Variables, scope: str) -> torch.Tensor:
    """sum over taps and input channels of (w s)^2, [B, cout], in float64."""
    s = _tensor(styles, torch.float64)
    w = ref._get_weight(ref._t(variables, f"G_synthesis/{scope}/weight", torch.float64))  # pylint: disable=protected-access
    return torch.cat([(ref.modulate_weight(w, s[i : i + 8]) ** 2).sum(dim=(1, 2, 3)) for i in range(0, s.shape[0], 8)])


@functools.lru_cache(maxsize=None)
def epsilon_case() -> EpsilonCase:
    """
    A copy of the 128^2 random network with mod_bias = -1 on three layers, so that their style is the affine part alone and
    shrinks with the dlatent row. Each of those rows is scaled so that the median (over samples and output channels) of
    sum (w s)^2 is 1e-8, the epsilon under the root: the scale is derived here, in float64, from the sum at scale 1. Sample
    EPSILON_ZERO_SAMPLE has those rows exactly zero: s = 0 and d = 1 / sqrt(1e-8).
    """
    spec = spec_of(EPSILON_NETWORK)
    variables = dict(variables_of(EPSILON_NETWORK))
    dlatents = dlatents_of(EPSILON_NETWORK, EPSILON_BATCH).copy()
    scales = {}
    for index in EPSILON_CONVS:
        conv = spec.convs[index]
        scope = f"G_synthesis/{conv.scope}"
        variables[f"{scope}/mod_bias"] = np.full((conv.cin,), -1.0, dtype=np.float32)
        unit = _sum_under_the_root(style(dlatents[:, conv.layer_idx], variables, conv.scope, torch.float64), variables, conv.scope)
        scales[index] = float(np.sqrt(DEMOD_EPSILON / float(unit.median())))  # (the sum is quadratic in the row)
        dlatents[:, conv.layer_idx] *= np.float32(scales[index])
        dlatents[EPSILON_ZERO_SAMPLE, conv.layer_idx] = 0.0
    return EpsilonCase(variables, dlatents, EPSILON_CONVS, scales)


def epsilon_share(styles: Array, variables: ref.Variables, scope: str) -> np.ndarray:
    """What 1e-8 contributes to the sum under the root, per (sample, output channel), in float64."""
    total = _sum_under_the_root(styles, variables, scope)
    return (DEMOD_EPSILON / (total + DEMOD_EPSILON)).numpy()
