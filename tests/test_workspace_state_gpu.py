"""
What one workspace keeps between calls: its zero borders and nothing else.

Every convolution family reads out-of-image taps as exact zeros without a bounds test, which holds only while the borders of the
activation planes and of the parity planes, zeroed once when the workspace is created, are never written; and every engine of one
(device, resolution, max_batch, config) shares that workspace whatever its forms, so a form chosen at one batch leaves its state to
the form chosen at the next. The isolated layer checks run each form on a workspace of its own and never see a border; here one
workspace goes through the forms the way the product stream puts it through them. Two debug taps do the looking:
Engine.debug_border_residue (border words that are not zero / border words scanned / planes, per layer and buffer, over the
buffers' whole capacity) and Engine.debug_poison_scratch (2^20 into every scratch cell that is not border; with include_borders,
private workspaces only, into the borders too). No GANCE_TUNE_* knob may be set, as in the isolated modules.

(a) test_the_taps_themselves, 32^2, max_batch 3, private workspace: a fresh engine scans clean; "scanned" is planes x the border
    words of a plane counted in Python (tests/workspace_state_cases.py, per class for the parity planes); poison leaves the scan
    clean and the next calls bit-equal to a pristine engine's; poison with borders makes nonzero == scanned in every buffer (NaN
    counts, -0 does not); that mode is refused on a shared workspace.
(b) test_borders_stay_zero_after_every_production_form (the four networks of workspace_state_cases.NETWORKS: every batch of the
    isolated case tables once in a seeded shuffled order, then descending; on the 1024^2 config-f network a conv_form="direct"
    engine of other weights takes turns) and test_borders_stay_zero_after_every_forced_form (the eleven forced conv_form x up_form
    engines of the 128^2 network on ONE workspace at 1, 5 and 64 frames): after every call every count is zero, else the failure
    names layer, buffer and the call before it. On 256 CUs the profiled launch names are held to the three case tables
    (workspace_state_cases.name_misses, itself held to the planner by tests/test_workspace_state_cases.py).
(c) test_results_do_not_depend_on_the_history_of_the_workspace: per batch one fresh private-workspace engine of the same
    max_batch makes ONE synthesize_w(want_float=True) call: the reference. A seasoned engine then goes through the order of (b)
    with an engine of other weights and forms (direct, split) taking turns on its workspace; between the calls: synthesize_z at
    two psi, the device entry on a side stream, a debug_activation_after stop, a randomize_noise -> restore_noise round trip (their
    references: one more pristine engine), the bytes-only host entry three times (eager, capture, replay) with the other engine
    and a poison between capture and replay; then poison and every batch again. Every result, bytes and fp32 image, must be
    array_equal to its reference: no tolerance. The forced forms are held the same way in the (b) test, against their own first
    results: a second round in another order after a poison.

Measured on an MI355X (256 CUs, so with the launch names held to the tables). Every border count was zero after every call, and
every result bit-equal to its reference: no kernel had to change.
  (a) 32^2, max_batch 3: 86016 (4^2) ... 516096 (32^2) activation border words scanned per layer in 1536 planes, 3133440 (8^2 up
      layer) and 9031680 (32^2 up layer, 49152 planes: 4 classes x 24 units x 512 channels) parity-plane border words, all zero when fresh and after the
      poison, all counted after the poison with borders; 1.6 s.
  (b) f-128: 20 calls, 1.2 s; e-256: 22 calls, 1.0 s; f-1024: 20 calls (10 of them the direct engine's), 1.7 s; e-1024: 8 calls,
      0.8 s; forced forms: 66 calls of 11 engines, 5.3 s (creating the eleven engines is most of it).
  (c) f-128: 70 calls, 7.7 s, of which 6.0 s go to the eleven pristine engines of the references; e-256: 76 calls, 6.8 s (5.2 s);
      f-1024: 28 calls, 3.8 s (2.3 s); e-1024: 28 calls, 3.6 s (1.8 s). Creating an engine costs 0.5 s of weight arrangement on
      the host, 1 s on a busy one: within a run of the whole suite the two ten-batch cases took 11.4 s and 10.7 s, the forced forms 7.7 s.
The checks bite: on a build whose fir_epilogue_kernel also stores 1e-3 into row 1, column 3 of its own output plane (a border cell,
in bounds) all ten tests fail. (b) after its first call, naming the Conv0_up layers that ran two-pass or in scatter-GEMM form at that
batch (f-128 at 8 frames: layers 1 and 3, 4096 border words each; e-1024 at 3 frames: layers 1, 3, 5, 7, 9); (c) at its third call,
the first that meets another form's leftovers: 886 ... 17097 fp32 pixels off by 7.0e-4 ... 1.3e-3, a sixth of a grey level, which the
1-LSB-in-1e-3-of-the-bytes comparison of the older history checks lets through.
"""

import os
import time

import numpy as np
import pytest
import torch

import workspace_state_cases as cases
from gance_amd import hip_lib
from gance_amd.stylegan2 import spec as sg2_spec

pytestmark = pytest.mark.gpu

CONFIG_E = sg2_spec.FMAP_BASE_CONFIG_E
FMAP_BASE = {"f": sg2_spec.FMAP_BASE, "e": CONFIG_E}
TAP_RESOLUTION, TAP_MAX_BATCH = 32, 3
STOP_AFTER = 7  # conv layers of the debug_activation_after stop: through the 32^2 Conv1
NOISE_SEED = 9


@pytest.fixture(scope="module")
def library():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")
    knobs = sorted(key for key in os.environ if key.startswith("GANCE_TUNE_"))
    if knobs:
        pytest.fail(f"{', '.join(knobs)} set: these checks are of the forms the product selects by itself; unset every GANCE_TUNE_* variable")
    return hip_lib.load_library()


_VARIABLES: dict = {}


def _variables(config: str, resolution: int, seed: int = 3) -> dict:
    """The every-term generators (perturb=True), made once per session; seed 4: the "other weights"."""
    key = (config, resolution, seed)
    if key not in _VARIABLES:
        _VARIABLES[key] = sg2_spec.make_random_variables(resolution, seed=seed, perturb=True, fmap_base=FMAP_BASE[config])
    return _VARIABLES[key]


def _dlatents(spec, count: int, seed: int) -> np.ndarray:
    return np.random.RandomState(seed).randn(count, spec.num_layers, 512).astype(np.float32)


def _dirty(engine, spec) -> list:
    """["layer, buffer: n of m border words"] of every buffer of the engine's workspace that holds a border word that is not zero."""
    found = []
    for conv, row in zip(spec.convs, engine.debug_border_residue()):
        for buffer, (nonzero, scanned, _) in (("activation", row[:3]), ("parity planes", row[3:])):
            if nonzero:
                side = 2 ** conv.res_log2
                found.append(f"conv layer {conv.layer_idx} ({conv.scope}, {side}x{side}), {buffer}: {int(nonzero)} of {int(scanned)} border words are not zero")
    return found


def _require_clean(engine, spec, after: str) -> None:
    found = _dirty(engine, spec)
    assert not found, f"after {after}:\n" + "\n".join(found)


def _expected_scan(spec, max_batch: int, residue: np.ndarray) -> None:
    """"scanned" of every buffer is planes x the border words of a plane, by the geometry of tests/workspace_state_cases.py."""
    assert residue.shape == (len(spec.convs), 6) and residue.dtype == np.uint64
    for conv, row in zip(spec.convs, residue.astype(np.int64)):
        side = 2 ** conv.res_log2
        assert row[2] == max_batch * conv.cout, (conv.scope, row)
        assert row[1] == row[2] * cases.act_border_words(side), (conv.scope, row)
        if not conv.up:
            assert not row[3:].any(), (conv.scope, row)
            continue
        h = side // 2
        per_class, rest = divmod(int(row[5]), 4)
        assert rest == 0 and per_class % conv.cout == 0 and per_class >= max_batch * conv.cout, (conv.scope, row)  # (units: split-K slabs x samples)
        assert row[4] == per_class * sum(cases.parity_border_words(h, py, px) for py in (0, 1) for px in (0, 1)), (conv.scope, row)


# ---- (a) the taps ----


def test_the_taps_themselves(library) -> None:
    spec = sg2_spec.make_spec(TAP_RESOLUTION)
    variables = _variables("f", TAP_RESOLUTION)
    dlatents = _dlatents(spec, TAP_MAX_BATCH, 5)
    pristine = hip_lib.Engine(variables, TAP_RESOLUTION, max_batch=TAP_MAX_BATCH, private_workspace=True)
    try:
        want = {batch: pristine.synthesize_w(dlatents[:batch], want_float=True) for batch in (TAP_MAX_BATCH, 1, 2)}
    finally:
        pristine.close()
    engine = hip_lib.Engine(variables, TAP_RESOLUTION, max_batch=TAP_MAX_BATCH, private_workspace=True)
    try:
        fresh = engine.debug_border_residue()
        assert not fresh[:, [0, 3]].any(), fresh
        _expected_scan(spec, TAP_MAX_BATCH, fresh)
        assert sum(conv.up for conv in spec.convs) == 3 and (fresh[:, 4] > 0).sum() == 3
        engine.debug_poison_scratch(cases.POISON)
        assert np.array_equal(engine.debug_border_residue(), fresh)
        for batch in (TAP_MAX_BATCH, 1, 2):
            frames, image = engine.synthesize_w(dlatents[:batch], want_float=True)
            assert np.isfinite(image).all() and float(np.abs(image).max()) < 1e3, batch
            assert np.array_equal(image, want[batch][1]) and np.array_equal(frames, want[batch][0]), f"{batch} frames after the poison"
            assert np.array_equal(engine.debug_border_residue(), fresh), batch
        for value, counted in ((cases.POISON, True), (float("nan"), True), (-0.0, False)):
            engine.debug_poison_scratch(value, include_borders=True)
            residue = engine.debug_border_residue()
            assert np.array_equal(residue[:, [1, 2, 4, 5]], fresh[:, [1, 2, 4, 5]])
            for nonzero, scanned in ((0, 1), (3, 4)):
                assert np.array_equal(residue[:, nonzero], residue[:, scanned] if counted else np.zeros_like(residue[:, scanned])), (value, residue)
    finally:
        engine.close()  # (its borders are gone: nothing else may run on this workspace)
    shared = hip_lib.Engine(variables, TAP_RESOLUTION, max_batch=TAP_MAX_BATCH)
    try:
        with pytest.raises(hip_lib.GanceHipError) as refusal:
            shared.debug_poison_scratch(cases.POISON, include_borders=True)
        assert refusal.value.status == 1 and "PRIVATE_WORKSPACE" in str(refusal.value)
        assert np.array_equal(shared.debug_border_residue(), fresh)
        frames, image = shared.synthesize_w(dlatents, want_float=True)
        assert np.array_equal(image, want[TAP_MAX_BATCH][1]) and np.array_equal(frames, want[TAP_MAX_BATCH][0])
    finally:
        shared.close()


# ---- (b) the borders after every form ----


def _conv_names(names) -> str:
    return " ".join(name.split("_")[0] for name in names if name.startswith("conv"))


@pytest.mark.parametrize("name", list(cases.NETWORKS))
def test_borders_stay_zero_after_every_production_form(library, name: str) -> None:
    network = cases.NETWORKS[name]
    on_table = torch.cuda.get_device_properties(0).multi_processor_count == cases.NUM_CUS
    spec = sg2_spec.make_spec(network.resolution, fmap_base=FMAP_BASE[network.config])
    dlatents = _dlatents(spec, network.max_batch, 31)
    started = time.perf_counter()
    engine = hip_lib.Engine(_variables(network.config, network.resolution), network.resolution, max_batch=network.max_batch, profile=True)
    other, calls = None, 0
    try:
        if name == "f-1024":  # other weights, forced forms, the same workspace
            other = hip_lib.Engine(_variables(network.config, network.resolution, seed=4), network.resolution, max_batch=network.max_batch, conv_form="direct")
        _expected_scan(spec, network.max_batch, engine.debug_border_residue())
        _require_clean(engine, spec, "the creation of the workspace")
        for batch in cases.call_order(network.batches):
            frames = engine.synthesize_w(dlatents[:batch])
            names = [step.name for step in engine.steps()]
            calls += 1
            assert frames.shape == (batch, network.resolution, network.resolution, 3)
            _require_clean(engine, spec, f"call {calls}, {batch} frames: {_conv_names(names)}")
            if on_table:
                misses = cases.name_misses(network.config, network.resolution, batch, names)
                assert not misses, "\n".join(misses)
            if other is not None:
                other.synthesize_w(dlatents[:batch])
                calls += 1
                _require_clean(engine, spec, f"call {calls}, {batch} frames on the conv_form=\"direct\" engine")
    finally:
        engine.close()
        if other is not None:
            other.close()
    held = "their launch names held to the case tables" if on_table else f"launch names not held: not {cases.NUM_CUS} CUs"
    print(f"\n{name}: {calls} calls, every border word zero after each, {held} ({time.perf_counter() - started:.1f} s)")


def test_borders_stay_zero_after_every_forced_form(library) -> None:
    resolution, max_batch = cases.FORCED_RESOLUTION, cases.FORCED_MAX_BATCH
    spec = sg2_spec.make_spec(resolution)
    dlatents = _dlatents(spec, max_batch, 32)
    started = time.perf_counter()
    engines, first, calls = [], {}, 0
    try:
        for conv_form, up_form in cases.FORCED_FORMS:
            engines.append(((conv_form, up_form), hip_lib.Engine(_variables("f", resolution), resolution, max_batch=max_batch, conv_form=conv_form, up_form=up_form)))
        scanner = engines[0][1]  # (one workspace: any of them scans it)
        _require_clean(scanner, spec, "the creation of the workspace")
        for batch in cases.FORCED_BATCHES:
            for forms, engine in engines:
                first[(forms, batch)] = engine.synthesize_w(dlatents[:batch], want_float=True)
                calls += 1
                assert np.isfinite(first[(forms, batch)][1]).all(), (forms, batch)
                _require_clean(scanner, spec, f"call {calls}: {batch} frames, conv_form={forms[0]}, up_form={forms[1]}")
        assert not np.array_equal(first[(("direct", "split"), 5)][1], first[(("winograd43", "fused"), 5)][1])  # (the forms do differ)
        scanner.debug_poison_scratch(cases.POISON)
        for batch in reversed(cases.FORCED_BATCHES):  # the other way round, from poisoned scratch
            for forms, engine in reversed(engines):
                frames, image = engine.synthesize_w(dlatents[:batch], want_float=True)
                calls += 1
                where = f"call {calls}: {batch} frames, conv_form={forms[0]}, up_form={forms[1]}, second round"
                assert np.array_equal(image, first[(forms, batch)][1]) and np.array_equal(frames, first[(forms, batch)][0]), where
                _require_clean(scanner, spec, where)
    finally:
        for _, engine in engines:
            engine.close()
    print(f"\nforced forms: {calls} calls of {len(engines)} engines on one workspace, every border word zero after each ({time.perf_counter() - started:.1f} s)")


# ---- (c) history independence, to the bit ----


def _pristine(variables, network, dlatents: np.ndarray):
    """One call of a fresh engine on a workspace nobody else has used."""
    engine = hip_lib.Engine(variables, network.resolution, max_batch=network.max_batch, private_workspace=True)
    try:
        return engine.synthesize_w(dlatents, want_float=True)
    finally:
        engine.close()


def _same(got, want, where: str) -> None:
    frames, image = got
    assert np.isfinite(image).all(), f"{where}: the image is not finite"
    differing = int((image != want[1]).sum())
    assert differing == 0, f"{where}: {differing} of {image.size} fp32 pixels differ from the pristine engine's, by up to {float(np.abs(image - want[1]).max()):.3e}"
    assert np.array_equal(frames, want[0]), f"{where}: {int((frames != want[0]).sum())} bytes differ from the pristine engine's"


@pytest.mark.parametrize("name", list(cases.NETWORKS))
def test_results_do_not_depend_on_the_history_of_the_workspace(library, name: str) -> None:
    network = cases.NETWORKS[name]
    spec = sg2_spec.make_spec(network.resolution, fmap_base=FMAP_BASE[network.config])
    variables = _variables(network.config, network.resolution)
    dlatents = _dlatents(spec, network.max_batch, 31)
    other_dlatents = _dlatents(spec, network.max_batch, 33)
    batches = network.history_batches
    middle = batches[len(batches) // 2]
    z = np.random.RandomState(34).randn(middle, 512).astype(np.float32)
    psis = (0.7, 1.2)
    started = time.perf_counter()

    want = {batch: _pristine(variables, network, dlatents[:batch]) for batch in batches}
    extras = hip_lib.Engine(variables, network.resolution, max_batch=network.max_batch, private_workspace=True)
    try:
        want_z = {psi: extras.synthesize_z(z, truncation_psi=psi, want_float=True) for psi in psis}
        want_activation = extras.debug_activation_after(dlatents[:middle], STOP_AFTER)
        extras.randomize_noise(seed=NOISE_SEED, count=middle)
        want_noisy = extras.synthesize_w(dlatents[:middle], want_float=True)
    finally:
        extras.close()
    assert not np.array_equal(want_noisy[1], want[middle][1]) and not np.array_equal(want_z[0.7][1], want_z[1.2][1])
    referenced = time.perf_counter()

    seasoned = hip_lib.Engine(variables, network.resolution, max_batch=network.max_batch)
    other = hip_lib.Engine(_variables(network.config, network.resolution, seed=4), network.resolution, max_batch=network.max_batch, conv_form="direct", up_form="split")
    calls, other_first = 0, {}

    def check(batch: int, what: str) -> None:
        nonlocal calls
        calls += 1
        _same(seasoned.synthesize_w(dlatents[:batch], want_float=True), want[batch], f"call {calls}, {batch} frames, {what}")

    def disturb(batch: int) -> None:
        nonlocal calls
        calls += 1
        got = other.synthesize_w(other_dlatents[:batch], want_float=True)
        _same(got, other_first.setdefault(batch, got), f"call {calls}, {batch} frames on the other engine")

    def z_call(psi: float) -> None:
        nonlocal calls
        calls += 1
        _same(seasoned.synthesize_z(z, truncation_psi=psi, want_float=True), want_z[psi], f"call {calls}, synthesize_z of {middle} frames at psi {psi}")

    def device_call(batch: int) -> None:
        nonlocal calls
        calls += 1
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            d_w = torch.from_numpy(dlatents[:batch]).cuda()
            d_u8 = torch.empty((batch, network.resolution, network.resolution, 3), dtype=torch.uint8, device="cuda")
            d_f32 = torch.empty((batch, 3, network.resolution, network.resolution), dtype=torch.float32, device="cuda")
            seasoned.synthesize_w_device(d_w.data_ptr(), batch, d_u8.data_ptr(), d_f32.data_ptr(), side.cuda_stream)
        side.synchronize()
        _same((d_u8.cpu().numpy(), d_f32.cpu().numpy()), want[batch], f"call {calls}, {batch} frames through the device entry on a side stream")

    def stopped_call() -> None:
        nonlocal calls
        calls += 1
        got = seasoned.debug_activation_after(dlatents[:middle], STOP_AFTER)
        assert np.array_equal(got, want_activation), f"call {calls}: the activation after {STOP_AFTER} conv layers differs from the pristine engine's"

    def noisy_call() -> None:
        nonlocal calls
        calls += 1
        seasoned.randomize_noise(seed=NOISE_SEED, count=middle)
        try:
            _same(seasoned.synthesize_w(dlatents[:middle], want_float=True), want_noisy, f"call {calls}, {middle} frames with a noise plane per sample")
        finally:
            seasoned.restore_noise()

    between = [lambda: z_call(psis[0]), lambda: device_call(middle), stopped_call, noisy_call, lambda: z_call(psis[1]), lambda: device_call(batches[0])]
    try:
        order = cases.call_order(batches)
        for i, batch in enumerate(order):
            check(batch, "seasoning")
            disturb(order[(i + 1) % len(order)])
            if i < len(between):
                between[i]()
                _require_clean(seasoned, spec, f"call {calls}")
        # the bytes-only host entry at one batch: eager, capture and launch, then the replay of that graph from poisoned scratch
        for i in range(3):
            if i == 2:
                disturb(batches[-1])
                seasoned.debug_poison_scratch(cases.POISON)
            calls += 1
            frames = seasoned.synthesize_w(dlatents[:middle])
            assert np.array_equal(frames, want[middle][0]), f"call {calls}, bytes-only call {i + 1} of 3 of {middle} frames: {int((frames != want[middle][0]).sum())} bytes differ"
        seasoned.debug_poison_scratch(cases.POISON)
        for batch in sorted(batches):  # no form reads scratch it did not write in that call
            check(batch, "after the poison")
            disturb(batch)
        _require_clean(seasoned, spec, f"call {calls}")
    finally:
        seasoned.close()
        other.close()
    ended = time.perf_counter()
    print(f"\n{name}: {calls} calls on one workspace, each bit-equal to its pristine reference "
          f"(references {referenced - started:.1f} s, calls {ended - referenced:.1f} s)")
