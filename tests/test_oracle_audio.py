"""
CPU tests pinning the audio -> latent ORACLE (oracle/audio_ref.py) against golden vectors captured
from the reference's own code (oracle/make_goldens.py; fixtures in tests/golden/).
"""

import hashlib

import numpy as np
import pytest

from gance_amd import synthetic
from oracle import audio_ref

BLEND_CASES = [
    "blend_n60_seed0_roll_k3",
    "blend_n60_seed1_noroll_k1",
    "blend_n60_seed2_roll_k1",
    "blend_n240_seed3_roll_k3",
    "blend_n1800_seed7_roll_k3",
    "blend_n9000_seed11_roll_k3",
]
FLOAT_TOL = dict(rtol=1e-10, atol=1e-10)


def load_case(golden_dir, name):
    golden = np.load(golden_dir / f"{name}.npz")
    num_frames, vector_length, num_projection, seed, roll, num_networks, stride, depth = (int(v) for v in golden["meta"])
    alpha, amp_lo, amp_hi = (float(v) for v in golden["alpha_amp"])
    audio = synthetic.synthetic_audio(num_frames, vector_length, seed=seed)
    latents = synthetic.synthetic_final_latents(num_projection, vector_length, seed=seed + 4)
    config = dict(
        num_frames=num_frames, vector_length=vector_length, roll=bool(roll), num_networks=num_networks,
        stride=stride, depth=depth, alpha=alpha, amp=(amp_lo, amp_hi),
    )
    return golden, audio, latents, config


def check_stage(golden, key: str, array: np.ndarray, stride: int, **tol) -> None:
    flat = np.asarray(array).reshape(-1)
    tol = tol or FLOAT_TOL
    np.testing.assert_allclose(flat[::stride], golden[f"{key}_sample"], **tol)
    lo, hi, total, size = golden[f"{key}_stats"]
    assert flat.size == int(size)
    np.testing.assert_allclose([flat.min(), flat.max()], [lo, hi], **tol)
    np.testing.assert_allclose(flat.sum(dtype=np.float64), total, rtol=1e-9, atol=1e-6)


@pytest.mark.parametrize("name", BLEND_CASES)
def test_every_stage_matches_the_reference_goldens(golden_dir, name: str) -> None:
    golden, audio, latents, cfg = load_case(golden_dir, name)
    L, stride = cfg["vector_length"], cfg["stride"]
    stages = audio_ref.create_spectrogram_stages(audio, L, cfg["amp"], cfg["roll"])
    check_stage(golden, "db", stages.db, stride)
    check_stage(golden, "scaled", stages.scaled, stride)
    check_stage(golden, "smoothed_time", stages.smoothed_time, stride)
    check_stage(golden, "smoothed", stages.smoothed, stride)
    check_stage(golden, "final", stages.final, stride)
    # float32 RMS: bit-exact (same summation order as librosa's numpy call)
    assert np.array_equal(stages.raw_rms, golden["raw_rms"]) and stages.raw_rms.dtype == golden["raw_rms"].dtype
    smoothed, rolling = audio_ref.smoothed_rolling_average(stages.raw_rms, 3, 7, 3)
    np.testing.assert_allclose(rolling, golden["rolling_average"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(smoothed, golden["rolling_smoothed"], rtol=1e-13, atol=1e-16)
    # integer stages: exact
    assert np.array_equal(audio_ref.quantize_to_indices(smoothed, 3), golden["roll_values"])
    if cfg["roll"]:
        assert np.array_equal(stages.roll_values, golden["roll_values"])

    result = audio_ref.alpha_blend_projection_file(
        latents, cfg["alpha"], cfg["roll"], cfg["amp"], cfg["depth"], audio, L, list(range(cfg["num_networks"]))
    )
    assert np.array_equal(result.network_indices, golden["network_indices"])
    assert result.combined.shape == (18, cfg["num_frames"] * L) and result.combined.dtype == np.float64
    assert result.projected.dtype == np.float32
    check_stage(golden, "combined_row0", result.combined[0], stride)
    check_stage(golden, "combined_row_depth", result.combined[cfg["depth"]], stride, rtol=0, atol=0)
    check_stage(golden, "projected_row0", result.projected[0], stride, rtol=0, atol=0)
    for row in range(1, cfg["depth"]):
        assert np.array_equal(result.combined[row], result.combined[0])


NOISE_CASES = ["noise_n60_seed0_roll_k3", "noise_n600_seed5_noroll_k2"]


@pytest.mark.parametrize("name", NOISE_CASES)
def test_noise_blend_matches_the_reference_goldens(golden_dir, name: str) -> None:
    """noise-blend: the noise source is the same library calls, so float32 stages are bit-equal."""
    golden = np.load(golden_dir / f"{name}.npz")
    num_frames, vector_length, seed, roll, num_networks, stride = (int(v) for v in golden["meta"])
    alpha, amp_lo, amp_hi = (float(v) for v in golden["alpha_amp"])
    audio = synthetic.synthetic_audio(num_frames, vector_length, seed=seed)
    result = audio_ref.alpha_blend_vectors_max_rms_power_audio(
        alpha, bool(roll), (amp_lo, amp_hi), audio, vector_length, list(range(num_networks))
    )
    assert result.noise.dtype == np.float32 and result.combined.dtype == np.float64
    assert np.array_equal(result.noise[::stride], golden["noise_sample"])
    assert np.array_equal([result.noise.min(), result.noise.max()], golden["noise_stats"][:2])
    assert np.array_equal(result.network_indices, golden["network_indices"])
    check_stage(golden, "spectrogram", result.spectrogram, stride)
    check_stage(golden, "combined", result.combined, stride)
    assert np.array_equal(audio_ref.gaussian_data(vector_length, num_frames)[::stride], golden["gaussian_default_sample"])
    assert np.array_equal(audio_ref.gaussian_data(vector_length, num_frames, 3, 2)[::stride], golden["gaussian_both_sample"])


def test_array_helpers_match_the_reference_goldens(golden_dir) -> None:
    golden = np.load(golden_dir / "vector_helpers.npz")
    data = golden["data"]
    assert np.array_equal(audio_ref.rotate_vectors_over_time(data, 64, golden["rolls"]), golden["rotated"])
    np.testing.assert_allclose(audio_ref.smooth_across_vectors(data, 8, 7, 3), golden["smooth_across_7_3"], **FLOAT_TOL)
    np.testing.assert_allclose(audio_ref.smooth_each_vector(data, 64, 5, 3), golden["smooth_each_5_3"], **FLOAT_TOL)
    np.testing.assert_allclose(audio_ref.smooth_each_vector(data, 64), golden["smooth_each_default"], **FLOAT_TOL)
    assert np.array_equal(audio_ref.duplicate_to_vector_count(data, 64, 18), golden["duplicated_x3"])
    assert np.array_equal(audio_ref.sub_vectors(golden["matrices"], 32), golden["sub_vectors_matrix"])
    assert golden["sub_vectors_matrix"].shape == (5, 18, 32)  # test/test_vector_sources_common.py:66-83
    assert np.array_equal(audio_ref.sub_vectors(data, 64), golden["sub_vectors_vector"])
    assert np.array_equal(audio_ref.quantize_to_indices(golden["ramp"], 3), golden["quantized_3"])
    assert np.array_equal(audio_ref.quantize_to_indices(golden["ramp"], 5), golden["quantized_5"])
    resampled = audio_ref.reshape_spectrogram_to_vectors(golden["resample_255_input"].reshape(3, 255).T, 512, None)
    np.testing.assert_allclose(resampled, golden["resample_255_to_512"], **FLOAT_TOL)
    with pytest.raises(ValueError):
        audio_ref.duplicate_to_vector_count(data, 64, 20)  # vsc:318-331


def test_pairwise_sum_restatement_is_numpy_bit_for_bit() -> None:
    import pandas as pd

    # numpy feeds add.reduce in buffers of this many values; the restatement (and the HIP kernel) assume 8192
    assert np.getbufsize() == audio_ref.NUMPY_REDUCE_BLOCK == 8192
    rng = np.random.RandomState(0)
    orders_differ = []
    for n in (1, 7, 8, 9, 100, 128, 129, 512, 1000, 1800, 4097, 8192, 8193, 9000, 15361, 16385, 20000, 100000):
        values = (rng.randn(n) * rng.rand() * 10).astype(np.float32)
        total = audio_ref.numpy_pairwise_sum_f32(values)
        assert total == np.add.reduce(values), n
        # pandas' float32 mean (the rolling average's fill value) is that sum over the count, in float32
        assert np.float32(total / np.float32(n)) == pd.Series(values).mean(), n
        if audio_ref._pairwise_sum_f32(values) != total:  # pylint: disable=protected-access
            orders_differ.append(n)
    # one pairwise tree over the whole series is numpy's order only up to one block: the cases above separate them
    assert orders_differ and min(orders_differ) > 8192, orders_differ


def test_rolling_mean_restatement_is_pandas_bit_for_bit() -> None:
    import pandas as pd

    rng = np.random.RandomState(1)
    for n in (3, 4, 10, 1800):
        values = np.abs(rng.randn(n)).astype(np.float32)
        want = pd.Series(values).rolling(3).mean().to_numpy()
        got = audio_ref.pandas_rolling_mean_kahan(values, 3)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[2:], want[2:])


def test_rms_known_answer_shape_of_reference_test() -> None:
    """Mirror of test/test_dynamic_model_switching.py:15-39: one RMS value per 1000-sample vector."""
    audio = synthetic.synthetic_audio(4, 1000, seed=3)
    rms = audio_ref.compute_raw_rms(audio[:1000], 1000)
    assert rms.shape == (1,)
    assert np.isclose(rms[0], np.sqrt(np.mean(audio[:1000].astype(np.float64) ** 2)), rtol=1e-6)


def test_live_reference_agrees_on_fresh_inputs(golden_dir) -> None:
    """
    Beyond the blend cases: a seed, amplitude range and network count that no other fixture covers, against what the
    reference returned for it (tests/golden/blend_n90_seed99_roll_k4.npz, oracle/make_goldens.py fresh_seed_case).
    """
    golden = np.load(golden_dir / "blend_n90_seed99_roll_k4.npz")
    num_frames, L = 90, 512
    audio = synthetic.synthetic_audio(num_frames, L, seed=99)
    latents = synthetic.synthetic_final_latents(num_frames // 3, L, seed=5)
    got = audio_ref.alpha_blend_projection_file(latents, 0.4, True, (-1, 1), 10, audio, L, [0, 1, 2, 3])
    np.testing.assert_allclose(got.spectrogram, golden["spectrogram"], **FLOAT_TOL)
    projected = np.ascontiguousarray(got.projected)
    digest, dtype, shape = (str(v) for v in golden["projected_digest"])
    assert (str(projected.dtype), str(projected.shape)) == (dtype, shape)
    assert hashlib.sha256(projected.tobytes()).hexdigest() == digest
    # the rows past the blend depth are the projected latents themselves (in the reference, bit for bit); the others blended
    combined, copies = np.asarray(got.combined), golden["combined_copy_rows"]
    assert combined.shape == tuple(golden["combined_shape"]) and len(copies) > 0
    for row in copies:
        assert np.array_equal(combined[row], projected[row])
    check_stage(golden, "blended", np.delete(combined, copies, axis=0), int(golden["meta"][0]))
    assert np.array_equal(got.network_indices, golden["network_indices"])
