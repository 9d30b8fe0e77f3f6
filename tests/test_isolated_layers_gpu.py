"""
Every 256^2 ... 1024^2 conv layer of the 1024^2 generator checked IN ISOLATION, in the form the product runs it (default selection:
conv_form / up_form "auto", no GANCE_TUNE_* knobs): the layer's own input as the kernels left it (debug_activation_after(n - 1)),
promoted to fp64, goes through ONE oracle layer (stylegan2_ref.synthesis_layer, the function the full oracle chain calls), and the
kernel's output (debug_activation_after(n)) is compared with that. The chain's upstream error (1.3e-6 ... 1.8e-6 of a layer's range
against the full fp64 chain) is not in the comparison, so a much tighter bar holds than the layer-wise tests against the chain can use.

What this reaches that the other tests do not: the 1024^2 Conv0_up (Cin = 64: two chunks of 32 channels, the chunk loop's one trip per
step) and the 512^2 one in the split-operand form (upfir_split.hip) at every row-segment count its planner produces for 1024^2 calls of
one to nine frames (16 / 8 / 4 / 2 / 1 on 256 CUs: each segment behind its own priming step), with pre-scaled input (the F(4x4,3x3)
launch before it stores its output times this layer's style) and, with conv_form="direct", plain input; and the F(4x4,3x3) Conv1
launches with the ToRGB channel sum in their epilogue ("convV...+rgb") at 256^2 ... 1024^2. Stopping after layer n drops only
layer n's own next-style pre-scale (engine.hip: `li + 1 < limit`); the pre-scaled stores are still checked, through the layer that
reads them.

Bars, per layer and sample, on max|got - want| / max|want|:
  * 2e-5 for every layer (the layer-wise bar of tests/test_synthesis_gpu.py), 1e-4 on the stress network (its bar there);
  * SPLIT_UP_TOLERANCE for the split-operand up layers ("/s3"), stress network included: a kernel that silently drops one of its six
    part products (narrower than fp32) must fail here. Measured on the MI355X over every configuration below: honest 2.1e-7 ... 8.7e-7
    (worst: the 256^2 layer at 3 frames), a build without the x2 w0 product 2.8e-6 ... 5.4e-6 (best: the 256^2 layer, plain input). The
    two are only 3.2x apart, so the bar sits at their geometric middle, 1.5e-6: 1.7x the worst honest error, 0.55x the smallest
    dropped-term error. The inputs are seeded and the kernels sum in a fixed order, so the honest errors repeat exactly.
  * the F(4x4,3x3) Conv1 layers keep 2e-5: measured honest 5.0e-7 ... 1.5e-6 (stress network 2.2e-6 ... 3.5e-6), the size of a dropped
    split term, so no tighter bar separates right from subtly wrong there.
In the direct form the 1024^2 Conv1 fuses its ToRGB and stores no activation; a debug tap on it runs the unfused launch (engine.hip).
"""

import numpy as np
import pytest
import torch

from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec
from oracle import stylegan2_ref as ref

pytestmark = pytest.mark.gpu

RESOLUTION = 1024
FIRST_LAYER = 12  # conv layers 12 ... 17 (1-based): Conv0_up / Conv1 of 256^2, 512^2, 1024^2
TOLERANCE = 2e-5
STRESS_TOLERANCE = 1e-4
SPLIT_UP_TOLERANCE = 1.5e-6  # (honest <= 8.7e-7, one dropped part product >= 2.8e-6: see above)


def _upfirs_plan(batch: int, cout: int, h: int, num_cus: int) -> tuple:
    """(segments, blocks) of a split-operand up launch: upfirs_plan in gance_amd/csrc/upfir_split.hip restated (16 output channels
    per block, 64-column strips, steps of 8 rows, segments of >= 16 rows, powers of two, until every CU has a block)."""
    base = batch * (cout // 16) * (h // 64)
    segs, best = 1, -(-base // num_cus) * h
    n = 2
    while h // n >= 16 and (h // n) % 8 == 0 and base * (n // 2) < num_cus:
        cost = -(-(base * n) // num_cus) * (h // n + 8)
        if cost < best:
            best, segs = cost, n
        n *= 2
    return segs, base * segs


def _batches_by_segment_count(num_cus: int) -> list:
    """[(segments, batch)] of the 1024^2 Conv0_up (64 -> 32 channels, 512^2 input): the smallest batch <= 9 for each segment count
    the planner produces, where the engine takes the split form (blocks for 9/16 of the CUs), most segments first."""
    found: dict = {}
    for batch in range(1, 10):
        segs, blocks = _upfirs_plan(batch, 32, RESOLUTION // 2, num_cus)
        if blocks >= num_cus * 9 // 16:
            found.setdefault(segs, batch)
    return sorted(found.items(), reverse=True)


def _launches(engine) -> dict:
    """{layer_idx: launch name} of the conv launches of the engine's last call (profiling on)."""
    names = {}
    for step in engine.steps():
        if step.name.startswith("conv"):
            kind = step.name.split("_")[0]
            names[int("".join(ch for ch in kind.split("+")[0] if ch.isdigit()))] = step.name
    return names


_VARIABLES: dict = {}


def _variables(network: str) -> dict:
    """The 1024^2 generators, made once per session."""
    if network not in _VARIABLES:
        if network == "stress":
            _VARIABLES[network] = sg2_spec.make_stress_variables(RESOLUTION, seed=0)
        else:
            _VARIABLES[network] = sg2_spec.make_random_variables(RESOLUTION, seed=3, perturb=network == "every_term")
    return _VARIABLES[network]


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    return hip_lib.load_library()


# (network, conv_form, rank): the batch is the rank-th entry of _batches_by_segment_count; random init with every term on at the
# 16 / 4 / 1-segment batches, StyleGAN2's own init (no noise, no biases: the network bench.py times) at the 8 / 2-segment ones
CONFIGS = [
    ("every_term", "auto", 0),
    ("stylegan_init", "auto", 1),
    ("every_term", "auto", 2),
    ("stylegan_init", "auto", 3),
    ("every_term", "auto", 4),
    ("every_term", "direct", 1),
    ("stress", "auto", 0),
]


@pytest.mark.parametrize("network,conv_form,rank", CONFIGS, ids=[f"{n}-{f}-{r}" for n, f, r in CONFIGS])
def test_layers_256_to_1024_in_isolation_on_the_default_kernels(library, network: str, conv_form: str, rank: int) -> None:
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = _batches_by_segment_count(num_cus)
    if num_cus == 256:
        assert plan == [(16, 1), (8, 2), (4, 3), (2, 5), (1, 9)]
    segs, batch = plan[min(rank, len(plan) - 1)]
    last_rank = min(rank, len(plan) - 1) == len(plan) - 1
    spec = sg2_spec.make_spec(RESOLUTION)
    variables = _variables(network)
    ceiling = STRESS_TOLERANCE if network == "stress" else TOLERANCE
    dlatents = np.random.RandomState(11 + rank).randn(batch, spec.num_layers, 512).astype(np.float32)
    samples = sorted({batch - 1} | ({0} if last_rank and conv_form == "auto" and network != "stress" else set()))
    engine = hip_lib.Engine(variables, RESOLUTION, max_batch=batch, conv_form=conv_form, profile=True)
    errors: dict = {}  # (conv n, sample) -> isolated error
    try:
        x = engine.debug_activation_after(dlatents, FIRST_LAYER - 1)[samples].copy()
        for n in range(FIRST_LAYER, len(spec.convs) + 1):
            got = engine.debug_activation_after(dlatents, n)[samples].copy()
            conv = spec.convs[n - 1]
            for i, s in enumerate(samples):
                with torch.no_grad():
                    want = ref.synthesis_layer(torch.from_numpy(x[i:i + 1]).double(), torch.from_numpy(dlatents[s:s + 1]).double(), variables, conv)
                want = want.numpy()[0]
                assert got[i].shape == want.shape
                errors[(n, s)] = float(np.abs(got[i] - want).max() / np.abs(want).max())
            x = got
        engine.synthesize_w(dlatents)
        launches = _launches(engine)
    finally:
        engine.close()

    print(f"\nisolated layers, {network} network, conv_form={conv_form}, batch {batch} ({segs} row segments at 1024^2, {num_cus} CUs):")
    for (n, s), err in sorted(errors.items()):
        print(f"  conv {n:2d} {spec.convs[n - 1].scope:18s} {launches.get(n - 1, '?'):32s} sample {s}: {err:.2e}")
    for (n, s), err in errors.items():
        assert err < ceiling, f"conv layer {n} ({spec.convs[n - 1].scope}, {launches.get(n - 1)}), sample {s}: isolated error {err:.2e}"
        if launches.get(n - 1, "").endswith("/s3"):
            assert err < SPLIT_UP_TOLERANCE, f"split-operand up layer {n} ({launches[n - 1]}), sample {s}: isolated error {err:.2e}"

    # the forms the checks were meant to reach: the split-operand up kernel on the 512^2 and 1024^2 Conv0_up, pre-scaled input where
    # F(4x4,3x3) launches with the ToRGB channel sum run the Conv1 before them, plain input in the direct form
    for n in (14, 16):
        name = launches[spec.convs[n - 1].layer_idx]
        assert name.endswith("/s3"), name
        assert name.startswith("convTFp") == (conv_form == "auto"), name
    if conv_form == "auto":
        for n in (13, 15, 17):
            name = launches[spec.convs[n - 1].layer_idx]
            assert name.startswith("convV") and not name.startswith("convVG") and "+rgb" in name.split("_")[0], name
