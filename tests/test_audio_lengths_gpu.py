"""
GPU parity tests of the audio -> latent path at a song's length, against the CPU oracle on fresh inputs.

The benchmark and the other audio tests stop at N = 1800 frames; a song at 60 fps is ten times that. Two length
thresholds live in the kernels and are crossed here:
- past 8192 frames, pandas' float32 `Series.mean()` (the fill value of the rolling mean's NaN head) is numpy's
  add.reduce, which sums blocks of 8192 values pairwise and adds the block sums one after another;
- past kChainStaged = 15360 frames, reduce_chain_kernel reads the per-frame series from HBM instead of LDS.
The long cases use seeds whose fill value depends on the summation order (asserted on the CPU first), so a kernel
summing the whole series as one pairwise tree fails them.

Bars as in test_blend_gpu.py: integer stages and the float32 RMS bit-exact; the rolling mean to 1e-15 relative (its
two head entries, a float32 value widened, exactly); the Savitzky-Golay stages to 1e-12 relative; the float64
spectrogram stages to 1e-7 absolute (1e-6 for dB); the float32 latents to 1e-5 absolute.
"""

import numpy as np
import pandas as pd
import pytest
import torch

from gance_amd import hip_lib, synthetic
from gance_amd.data_into_network_visualization import visualization_inputs
from gance_amd.vector_sources import vector_reduction
from oracle import audio_ref

pytestmark = pytest.mark.gpu

L = 512
FLOAT_ATOL = 1e-7


def whole_tree_mean_differs(series: np.ndarray) -> bool:
    """True when one pairwise tree over the whole float32 series gives another mean than pandas (numpy's blocked order)."""
    whole_tree = np.float32(audio_ref._pairwise_sum_f32(series) / np.float32(len(series)))  # pylint: disable=protected-access
    return bool(whole_tree != pd.Series(series).mean())


@pytest.mark.parametrize("num_frames,seed,mult,num_networks,separates", [
    (7, 24, 7, 2, False),        # the minimum frame count (savgol window 7)
    (8193, 30, 3, 3, True),      # the first length numpy sums in two blocks
    (15360, 35, 8, 4, True),     # the longest series staged in LDS
    (15361, 41, 15361, 3, True),  # the shortest series read from HBM; prime, so one projected latent for all frames
    (18001, 31, 47, 5, True),    # 5 minutes at 60 fps, odd, not a multiple of the 4- and 8-frame launch groupings
])
def test_blend_matches_oracle_at_song_length(num_frames, seed, mult, num_networks, separates) -> None:
    alpha, amp, depth = 0.25, (-5.0, 5.0), 12
    audio = synthetic.synthetic_audio(num_frames, L, seed=seed)
    latents = synthetic.synthetic_final_latents(num_frames // mult, L, seed=seed + 1)
    stages = audio_ref.create_spectrogram_stages(audio, L, amp, True)
    if separates:
        assert whole_tree_mean_differs(stages.raw_rms), "this input does not tell the two summation orders apart"
    smoothed_want, rolling_want = audio_ref.smoothed_rolling_average(stages.raw_rms, 3, 7, 3)
    # only latent row 0 enters the blend (the others are copies of it): the oracle on that row alone, blend_depth 1,
    # returns the blend row and the projected row without tiling 18 rows of N * L values
    want = audio_ref.alpha_blend_projection_file(latents[:1], alpha, True, amp, 1, audio, L, list(range(num_networks)))

    blend = hip_lib.Blend(num_frames, num_frames // mult, alpha, True, amp, depth, num_networks, latent_depth=latents.shape[0])
    try:
        d_audio = torch.from_numpy(audio).cuda()
        d_row0 = torch.from_numpy(np.ascontiguousarray(latents[0])).cuda()
        d_dlat = torch.empty((num_frames, latents.shape[0], L), dtype=torch.float32, device="cuda")
        d_idx = torch.empty((num_frames,), dtype=torch.int32, device="cuda")
        blend.run_device(
            d_audio.data_ptr(), audio.size, d_row0.data_ptr(), d_dlat.data_ptr(), d_idx.data_ptr(), debug_stages=True,
            stream=torch.cuda.current_stream().cuda_stream,
        )
        torch.cuda.synchronize()
        # per-frame series: bit-exact integers and float32
        raw_rms = blend.read_stage("raw_rms")
        assert raw_rms.dtype == np.float32 and np.array_equal(raw_rms, stages.raw_rms)
        roll_values = blend.read_stage("roll_values")
        assert np.array_equal(roll_values, stages.roll_values)
        assert np.array_equal(blend.read_stage("roll_cumulative"), np.cumsum(stages.roll_values) % L)
        assert np.array_equal(d_idx.cpu().numpy(), want.network_indices)
        assert np.array_equal(blend.read_stage("network_indices"), want.network_indices)
        rolling = blend.read_stage("rolling_average")
        assert rolling[0] == rolling_want[0] and rolling[1] == rolling_want[1], "fill value of the NaN head"
        np.testing.assert_allclose(rolling, rolling_want, rtol=1e-15, atol=0)
        np.testing.assert_allclose(blend.read_stage("rolling_smoothed"), smoothed_want, rtol=1e-12, atol=1e-15)
        index_smoothed_want = audio_ref.smoothed_rolling_average(stages.raw_rms, 3, 3, 2)[0]
        np.testing.assert_allclose(blend.read_stage("index_smoothed"), index_smoothed_want, rtol=1e-12, atol=1e-15)
        # float64 spectrogram stages
        np.testing.assert_allclose(blend.read_stage("db").T, stages.db, rtol=0, atol=1e-6)
        for stage in ("scaled", "smoothed_time", "smoothed", "final"):
            np.testing.assert_allclose(blend.read_stage(stage).reshape(-1), getattr(stages, stage), rtol=0, atol=FLOAT_ATOL, err_msg=stage)
        np.testing.assert_allclose(blend.read_stage("rolled").reshape(-1), stages.rolled, rtol=0, atol=FLOAT_ATOL * 50)
        # the latents: rows < depth = float32(blend row), rows >= depth = the projected row, bit for bit
        for row in (0, depth - 1):
            np.testing.assert_allclose(d_dlat[:, row, :].cpu().numpy().reshape(-1), want.combined[0].astype(np.float32), rtol=0, atol=1e-5)
        for row in (depth, 17):
            assert np.array_equal(d_dlat[:, row, :].cpu().numpy().reshape(-1), want.projected[0])
    finally:
        blend.close()


def test_noise_blend_past_the_lds_staged_length() -> None:
    """alpha_blend_vectors_max_rms_power_audio runs the same chain kernel: its roll amounts and indices at N > 15360."""
    num_frames, seed, num_networks, alpha, amp = 15361, 41, 3, 0.25, (-5, 5)
    audio = synthetic.synthetic_audio(num_frames, L, seed=seed)
    stages = audio_ref.create_spectrogram_stages(audio, L, amp, True)
    assert whole_tree_mean_differs(stages.raw_rms), "this input does not tell the two summation orders apart"
    want = audio_ref.alpha_blend_vectors_max_rms_power_audio(alpha, True, amp, audio, L, list(range(num_networks)))
    out = visualization_inputs.alpha_blend_vectors_max_rms_power_audio(alpha, True, amp, audio, L, list(range(num_networks)))
    assert np.array_equal(out.network_indices.result.data, want.network_indices)
    np.testing.assert_allclose(out.a_vectors.data, want.spectrogram, rtol=0, atol=FLOAT_ATOL)
    result = visualization_inputs.alpha_blend_vectors_max_rms_power_audio_device(alpha, True, amp, audio, L, num_networks, keep_stages=True)
    try:
        assert np.array_equal(result.blend.read_stage("roll_values"), stages.roll_values)
        assert np.array_equal(result.network_indices.cpu().numpy(), want.network_indices)
        rolling_want = audio_ref.smoothed_rolling_average(stages.raw_rms, 3, 7, 3)[1]
        np.testing.assert_allclose(result.blend.read_stage("rolling_average"), rolling_want, rtol=1e-15, atol=0)
    finally:
        result.blend.close()


@pytest.mark.parametrize("num_frames,seed", [(9000, 11), (15361, 41)])
def test_standalone_rms_rolling_average_at_song_length(num_frames, seed) -> None:
    audio = synthetic.synthetic_audio(num_frames, L, seed=seed)
    raw_want = audio_ref.compute_raw_rms(audio, L)
    assert whole_tree_mean_differs(raw_want), "this input does not tell the two summation orders apart"
    smoothed_want, rolling_want = audio_ref.smoothed_rolling_average(raw_want)
    layers = vector_reduction.reduce_vector_rms_rolling_average(audio, L)
    assert np.array_equal(layers.layers[1].data, raw_want)
    assert np.array_equal(layers.layers[0].data, rolling_want)
    np.testing.assert_allclose(layers.result.data, smoothed_want, rtol=1e-13, atol=0)
    quantized = vector_reduction.quantize_results_layers(layers, [0, 1, 2])
    assert np.array_equal(quantized.result.data, audio_ref.quantize_to_indices(smoothed_want, 3))


def test_standalone_rms_of_frames_longer_than_one_block() -> None:
    """Frames of 9000 samples: numpy sums each frame's squares in blocks of 8192 too (librosa's np.mean over a frame)."""
    frame_length, hop = 9000, 512
    audio = synthetic.synthetic_audio(60, L, seed=5)
    want = audio_ref.compute_raw_rms(audio, frame_length)
    whole_tree = np.array([
        np.sqrt(np.float32(audio_ref._pairwise_sum_f32(np.abs(audio[t * hop : t * hop + frame_length]) ** 2) / np.float32(frame_length)))  # pylint: disable=protected-access
        for t in range(len(want))
    ])
    assert np.any(whole_tree != want), "this input does not tell the two summation orders apart"
    layers = vector_reduction.reduce_vector_rms_rolling_average(audio, frame_length)
    assert layers.layers[1].data.dtype == np.float32 and np.array_equal(layers.layers[1].data, want)
    rolling_max = vector_reduction.reduce_vector_rms_rolling_max(audio, frame_length)
    assert np.array_equal(rolling_max.layers[0].data, want)
