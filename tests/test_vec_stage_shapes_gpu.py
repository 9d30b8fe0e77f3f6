"""
The stand-alone audio stages (`hip_lib.vec_*` over the `gance_vec_*` kernels of gance_amd/csrc/audio.hip) at every shape of
tests/vec_stage_cases.py, each against a reference that does not share the kernel's numerics (tests/vec_stage_ref.py: exact
rational Savitzky-Golay weights, long-double Fourier operator and DFT; oracle.audio_ref and scipy.ndimage for the stages whose
operation order IS the contract).

Bars come from the arithmetic, with S = sum_j |c_j x_j| the absolute dot product of an output:
  Savitzky-Golay   (w + 4) 2^-53 S        a w-term fp64 dot product, one rounding of each table entry, one of the result
  resample         (n_in + 4) 2^-53 S     the same over n_in terms
  spectrogram      8.686 (m + 4) 2^-53 sum |x_n w_n| / |X_k| dB per bin, plus the same for the bin holding the maximum
  raw RMS, rolling maximum, remap, quantize   bit for bit
  rolling mean     rtol 1e-15 (the same operation order; a division the compiler may not reorder)
  min-max          4 ulp of |x scale| + |offset|: the offset may be contracted into an fma
  mirrors          the 1e-9 of tests/test_standalone_api_gpu.py against oracle.audio_ref (1e-8 through the dB stage)
Every figure is printed before it is asserted.
"""

import numpy as np
import pytest
import torch
from scipy.ndimage import maximum_filter1d
from scipy.signal import resample

import vec_stage_cases as cases
import vec_stage_ref as ref
from gance_amd import apply_spectrogram, hip_lib
from gance_amd.vector_sources import vector_sources_common
from oracle import audio_ref

pytestmark = pytest.mark.gpu

TOL = dict(rtol=0.0, atol=1e-9)


@pytest.fixture(scope="module", autouse=True)
def gpu() -> None:
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; the product path has no CPU fallback")


def report(name: str, error: np.ndarray, bar: np.ndarray) -> None:
    """Print the worst observed error against its bar, then hold every output to it."""
    error, bar = np.asarray(error, dtype=np.float64), np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(error))
    assert np.all(np.isfinite(error)), name
    ratio = np.where(bar > 0, error / np.where(bar > 0, bar, 1.0), np.where(error > 0, np.inf, 0.0))
    worst = int(np.argmax(ratio))
    print(f"{name}: worst error / bar {ratio.flat[worst]:.3f} (error {error.flat[worst]:.3e}, bar {bar.flat[worst]:.3e}) at {np.unravel_index(worst, ratio.shape)}")
    assert np.all(error <= bar), name


# ---- Savitzky-Golay -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("count,length,axis,w,p", cases.SAVGOL_CASES)
def test_savgol(count: int, length: int, axis: int, w: int, p: int) -> None:
    data = cases.matrix(count, length, seed=w * 1000 + p)
    got = hip_lib.vec_savgol(data, axis, w, p)
    assert got.shape == data.shape and got.dtype == np.float64
    want, scale = ref.savgol(data, axis, w, p)
    report(f"savgol {(count, length, axis, w, p)}", np.abs(got - want), ref.savgol_bar(w, scale))


def test_savgol_mirrors_on_lines_equal_to_the_window() -> None:
    count, length, _, w, p = cases.SAVGOL_CASES[0]
    data = cases.matrix(count, length, seed=1).reshape(-1)
    got = vector_sources_common.smooth_across_vectors(data, length, window_length=w, polyorder=p)
    want = audio_ref.smooth_across_vectors(data, length, w, p)
    print(f"smooth_across_vectors {(count, length, w, p)}: {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, **TOL)
    count, length, _, w, p = cases.SAVGOL_CASES[2]
    data = cases.matrix(count, length, seed=2).reshape(-1)
    got = vector_sources_common.smooth_each_vector(data, length, window_length=w, polyorder=p)
    want = audio_ref.smooth_each_vector(data, length, w, p)
    print(f"smooth_each_vector {(count, length, w, p)}: {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, **TOL)


# ---- Fourier resample ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("count,n_in,n_out", cases.RESAMPLE_CASES)
def test_fourier_resample(count: int, n_in: int, n_out: int) -> None:
    data = cases.matrix(count, n_in, seed=n_in * 100 + n_out)
    got = hip_lib.vec_fourier_resample(data, n_out)
    assert got.shape == (count, n_out) and got.dtype == np.float64
    want, scale = ref.fourier_resample(data, n_out)
    report(f"resample {(count, n_in, n_out)}", np.abs(got - want), ref.resample_bar(n_in, scale))


@pytest.mark.parametrize("count,n_in,n_out", cases.RESAMPLE_REFUSED)
def test_fourier_resample_refuses_lengths_past_its_limits(count: int, n_in: int, n_out: int) -> None:
    with pytest.raises(ValueError):
        hip_lib.vec_fourier_resample(np.zeros((count, n_in)), n_out)


def test_resample_mirror_odd_to_even_downwards() -> None:
    count, n_in, n_out = cases.MIRROR_RESAMPLE
    data = cases.matrix(count, n_in, seed=3)
    got = vector_sources_common.scale_vectors_to_length_resample(data.reshape(-1), n_in, n_out)
    want = resample(data, n_out, axis=1).reshape(-1)
    print(f"scale_vectors_to_length_resample {n_in} -> {n_out}: {np.abs(got - want).max():.3e}")
    assert got.shape == (count * n_out,)
    np.testing.assert_allclose(got, want, **TOL)


# ---- spectrogram --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("short", (0, 1), ids=("exact", "one_less"))
@pytest.mark.parametrize("L,frames,truncate", cases.SPECTROGRAM_CASES)
def test_spectrogram(L: int, frames: int, truncate: bool, short: int) -> None:
    """`short`: one sample fewer than the windows need, which drops the last frame."""
    audio = cases.audio_of(L, cases.spectrogram_samples(L, frames) - short)
    got = hip_lib.vec_spectrogram(audio, L, truncate=truncate)
    want, magnitude, scale = ref.spectrogram(audio, L, truncate)
    bins = (L - 2) // 2 if truncate else L - 2
    assert got.shape == want.shape == (bins, frames - short) and got.dtype == np.float64
    report(f"spectrogram L = {L} truncate = {truncate} frames = {frames - short}", np.abs(got - want), ref.spectrogram_bar_db(L, magnitude, scale))


@pytest.mark.parametrize("truncate", (True, False))
def test_spectrogram_refuses_tables_past_the_lds_limit(truncate: bool) -> None:
    L = cases.SPECTROGRAM_REFUSED_LENGTH
    with pytest.raises(ValueError, match="2732"):
        hip_lib.vec_spectrogram(cases.audio_of(L, cases.spectrogram_samples(L, 2)), L, truncate=truncate)


@pytest.mark.parametrize("L", cases.SMOOTH_SCALE_LENGTHS)
def test_smooth_scale_mirror(L: int) -> None:
    audio = cases.audio_of(L, cases.SMOOTH_SCALE_FRAMES * L)
    got = apply_spectrogram.compute_spectrogram_smooth_scale(audio, L, (-2, 2))
    want = audio_ref.compute_spectrogram_smooth_scale(audio, L, (-2, 2))
    print(f"compute_spectrogram_smooth_scale L = {L}: {np.abs(got - want).max():.3e}")
    assert got.shape == want.shape == (cases.SMOOTH_SCALE_FRAMES * L,)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8)


# ---- RMS, rolling mean, rolling maximum ---------------------------------------------------------------------------------


@pytest.mark.parametrize("rolling_window,w,p", cases.ROLLING_CASES)
@pytest.mark.parametrize("L", cases.RMS_VECTOR_LENGTHS)
def test_rms_rolling_average(L: int, rolling_window: int, w: int, p: int) -> None:
    audio = cases.audio_of(L, cases.hop_samples(L, cases.RMS_HOPS))
    raw, rolling, smoothed = hip_lib.vec_rms_rolling_average(audio, L, rolling_window, w, p)
    want_raw = audio_ref.compute_raw_rms(audio, L)
    assert raw.dtype == np.float32 and raw.shape == want_raw.shape == (cases.RMS_HOPS,)
    print(f"raw RMS L = {L}: {int(np.sum(raw != want_raw))} of {raw.size} values differ")
    assert np.array_equal(raw, want_raw)
    _, want_rolling = audio_ref.smoothed_rolling_average(want_raw, rolling_window, w, p)
    print(f"rolling mean L = {L} window = {rolling_window}: relative {np.abs(rolling / want_rolling - 1).max():.3e}")
    assert rolling.dtype == np.float64
    np.testing.assert_allclose(rolling, want_rolling, rtol=1e-15, atol=0)
    if rolling_window > cases.RMS_HOPS:
        assert np.all(rolling == rolling[0])  # nothing but the fill value
    # the filter stage alone: on the series the kernel itself filtered
    want_smoothed, scale = ref.savgol_lines(rolling[None, :], w, p)
    report(f"smoothed L = {L} {(rolling_window, w, p)}", np.abs(smoothed[None, :] - want_smoothed), ref.savgol_bar(w, scale))


@pytest.mark.parametrize("hops,size", cases.ROLLING_MAX_HOPS)
@pytest.mark.parametrize("L", cases.ROLLING_MAX_VECTOR_LENGTHS)
def test_rms_rolling_max(L: int, hops: int, size: int) -> None:
    audio = cases.audio_of(L, cases.hop_samples(L, hops))
    raw, got = hip_lib.vec_rms_rolling_max(audio, L)
    want_raw, want = audio_ref.reduce_vector_rms_rolling_max(audio, L)
    assert raw.shape == got.shape == (hops,) and raw.dtype == got.dtype == np.float32
    if size > 0:
        assert np.array_equal(want, maximum_filter1d(input=want_raw, size=size))
    print(f"rolling max L = {L} hops = {hops} size = {size}: {int(np.sum(raw != want_raw))} raw, {int(np.sum(got != want))} filtered values differ")
    assert np.array_equal(raw, want_raw) and np.array_equal(got, want)


# ---- min-max, remap, quantize -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,count", cases.MINMAX_CASES)
def test_minmax_scale(name: str, count: int) -> None:
    data = cases.minmax_input(name, count)
    got = hip_lib.vec_minmax_scale(data, cases.MINMAX_RANGE)
    want = audio_ref.minmax_scale_1d(data, cases.MINMAX_RANGE)
    lo, hi = cases.MINMAX_RANGE
    spread = data.max() - data.min()
    scale = (hi - lo) / (spread if spread != 0.0 else 1.0)
    offset = lo - data.min() * scale
    assert got.shape == data.shape and got.dtype == np.float64
    report(f"minmax {name} {count}", np.abs(got - want), 4 * np.spacing(np.abs(data * scale) + abs(offset)))


@pytest.mark.parametrize("bad", cases.MINMAX_REFUSED, ids=("nan", "plus_inf", "minus_inf"))
def test_minmax_scale_refuses_a_non_finite_last_element(bad: float) -> None:
    data = cases.minmax_input("random", 1000)
    data[-1] = bad
    with pytest.raises(ValueError):
        hip_lib.vec_minmax_scale(data, cases.MINMAX_RANGE)


@pytest.mark.parametrize("count", cases.REMAP_COUNTS)
def test_remap(count: int) -> None:
    (x_lo, x_hi), (y_lo, y_hi) = cases.REMAP_INPUT_RANGE, cases.REMAP_OUTPUT_RANGE
    data = np.random.RandomState(count).uniform(x_lo, x_hi, size=count)
    data[0] = x_lo
    data[-1] = x_hi if count > 1 else x_lo
    got = hip_lib.vec_remap(data, cases.REMAP_INPUT_RANGE, cases.REMAP_OUTPUT_RANGE)
    slope = (y_hi - y_lo) / (x_hi - x_lo)  # scipy.interpolate.interp1d's linear form, as oracle.audio_ref.quantize_to_indices states it
    want = slope * (data - x_lo) + y_lo
    print(f"remap {count}: {int(np.sum(got != want))} of {count} values differ")
    assert got.shape == (count,) and got.dtype == np.float64 and np.array_equal(got, want)
    assert got[0] == y_lo and (count == 1 or got[-1] == y_hi)


def test_quantize_sends_ties_to_even() -> None:
    values, num_indices, want = cases.QUANTIZE_TIES
    got = hip_lib.vec_quantize(np.array(values), num_indices)
    print(f"quantize ties: {got.tolist()}")
    assert got.dtype == np.int64 and got.tolist() == list(want)
    assert audio_ref.quantize_to_indices(np.array(values), num_indices).tolist() == list(want)


@pytest.mark.parametrize("count,num_indices", cases.QUANTIZE_CASES)
def test_quantize(count: int, num_indices: int) -> None:
    data = np.random.RandomState(count + num_indices).randn(count)
    got = hip_lib.vec_quantize(data, num_indices)
    want = audio_ref.quantize_to_indices(data, num_indices)
    print(f"quantize {count} K = {num_indices}: {int(np.sum(got != want))} values differ")
    assert got.shape == (count,) and got.dtype == np.int64 and np.array_equal(got, want)
    assert got.min() == 0 and got.max() == num_indices - 1
