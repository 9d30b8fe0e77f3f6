"""
CPU checks behind the isolated tests of the stand-alone audio stages (tests/test_vec_stage_shapes_gpu.py): that the case
tables of tests/vec_stage_cases.py reach the branches they claim, computed from the shapes alone, and that the two operator
tables libgance_hip builds on the host (read through the host-only taps `hip_lib.savgol_table` and
`hip_lib.fourier_resample_matrix`) are the operators of tests/vec_stage_ref.py. No GPU involved.

The Savitzky-Golay table is a long-double Gram-Schmidt whose error is not known a priori, so it is measured here against
the exact rational weights: worst |table - exact| / max |row| over the table, per (window_length, polyorder):

    p =       0         1         2         3       w // 2     w - 1     other
    w =   1   0
    w =   3   5.55e-17  5.55e-17  2.71e-20
    w =   5   5.55e-17  5.55e-17  6.83e-17  5.15e-17            8.13e-20
    w =   7   5.55e-17  5.55e-17  5.55e-17  5.55e-17            8.13e-20
    w =   9   5.55e-17  7.63e-17  5.61e-17  7.96e-17  7.19e-17  1.08e-19
    w =  11   2.78e-17  9.62e-17  7.65e-17  8.54e-17  6.17e-17  9.06e-20
    w =  19                       7.52e-17
    w =  25   2.08e-17  9.75e-17  9.21e-17  8.76e-17  7.69e-17  6.78e-20
    w =  51   1.39e-17  1.02e-16  9.45e-17  1.04e-16  8.64e-17  1.36e-19  (51, 10) 8.94e-17
    w = 101   1.21e-17  9.58e-17  9.51e-17  1.08e-16  8.41e-17  1.90e-19  (101, 10) 1.04e-16

The worst is 1.082e-16 at (101, 3), and SAVGOL_TABLE_BAR is 8 times that. One rounding to double of an exact entry is up to
2^-53 = 1.11e-16 on this scale, so the table is the exact operator rounded to double at every order the entry points accept,
including the ones where scipy's own polyfit edge rows are 1e-3 .. 1 away from the exact weights.

What this measurement found first: built by Gram-Schmidt on the monomials x^k, the table was 2.99e-12 off at (51, 25) and
8.9e-3 off at (101, 50), past the 1e-12 that counts as a defect; every other pair above was at the level it has now. savgol_table now
orthogonalises x Q_{k-1} instead (gance_amd/csrc/audio.hip), which brought those two to 8.64e-17 and 8.41e-17.
"""

import ctypes
import warnings

import numpy as np
import pytest
from scipy.signal import resample, savgol_filter

import vec_stage_cases as cases
import vec_stage_ref as ref
from gance_amd import hip_lib
from oracle import audio_ref

SAVGOL_TABLE_BAR = 8 * 1.082e-16  # 8 x the worst measured value of the table in the module docstring
TOL = 1e-9  # the product's parity promise against scipy (tests/test_standalone_api_gpu.py)

SAVGOL_GRID = tuple(
    sorted(
        {(w, p) for w in (1, 3, 5, 7, 9, 11, 25, 51, 101) for p in (0, 1, 2, 3, w // 2, w - 1) if p < w}
        | {(w, p) for _, _, _, w, p in cases.SAVGOL_CASES}
        | {(w, p) for _, w, p in cases.ROLLING_CASES}
    )
)
RESAMPLE_GRID = tuple(
    sorted(
        {(n_in, n_out) for n_in in (*range(1, 10), 24, 25) for n_out in (*range(1, 10), 16, 24, 25, 50)}
        | {(n_in, n_out) for _, n_in, n_out in cases.RESAMPLE_CASES}
    )
)


@pytest.fixture(scope="module")
def library() -> ctypes.CDLL:
    if not hip_lib.LIBRARY_PATH.exists():
        import __graft_entry__  # pylint: disable=import-outside-toplevel

        __graft_entry__.build()
    return hip_lib.load_library()


# ---- the tables reach what they claim ---------------------------------------------------------------------------------


def test_spectrogram_cases_reach_every_trip_count_and_the_lds_limit() -> None:
    trips = set()
    for L, frames, truncate in cases.SPECTROGRAM_CASES:
        m = L - 2
        assert L >= 4 and m % 2 == 0 and frames == 5
        bins = m // 2 if truncate else m
        trips.add(-(-bins // cases.BLOCK))
        samples = cases.spectrogram_samples(L, frames)
        assert (samples - m) // L + 1 == frames and (samples - 1 - m) // L + 1 == frames - 1  # exactly enough, and one less drops a frame
    assert {1, 2, 3} <= trips
    truncated_bins = {(L - 2) // 2 for L in cases.SPECTROGRAM_LENGTHS}
    assert {1, cases.BLOCK, cases.BLOCK + 1} <= truncated_bins and any(bins % 2 == 0 and bins > 2 for bins in truncated_bins - {cases.BLOCK})
    assert 2 * cases.BLOCK + 2 in {L - 2 for L in cases.SPECTROGRAM_LENGTHS}  # 514 bins untruncated: the third trip holds two bins
    largest = max(cases.SPECTROGRAM_LENGTHS)
    assert 3 * (largest - 2) * 8 <= 64 * 1024 < 3 * (largest + 2 - 2) * 8 and cases.SPECTROGRAM_REFUSED_LENGTH == largest + 2
    assert {L for L, _, truncate in cases.SPECTROGRAM_CASES if truncate} == {L for L, _, truncate in cases.SPECTROGRAM_CASES if not truncate}


def test_resample_cases_reach_every_parity_class_in_each_direction() -> None:
    classes = {(np.sign(n_out - n_in), n_in % 2, n_out % 2) for _, n_in, n_out in cases.RESAMPLE_CASES if n_in > 1 and n_out > 1}
    assert {(direction, a, b) for direction in (-1, 1) for a in (0, 1) for b in (0, 1)} | {(0, 0, 0), (0, 1, 1)} <= classes
    assert any(n_in == 1 for _, n_in, _ in cases.RESAMPLE_CASES) and any(n_out == 1 for _, _, n_out in cases.RESAMPLE_CASES)
    assert any(count * n_out == 2 * cases.BLOCK + 1 for count, _, n_out in cases.RESAMPLE_CASES)
    assert max(n_in for _, n_in, _ in cases.RESAMPLE_CASES) == 8192
    assert {(n_in, n_out) for _, n_in, n_out in cases.RESAMPLE_REFUSED} == {(8193, 3), (3, 65537)}
    assert cases.MIRROR_RESAMPLE[1:] == (13, 8)


def test_savgol_cases_reach_every_branch_of_the_line() -> None:
    lines = [(count if axis == 0 else length, w, p) for count, length, axis, w, p in cases.SAVGOL_CASES]
    for line, w, p in lines:
        assert w % 2 == 1 and 0 <= p < w <= line
    assert any(line == w and w > 1 for line, w, _ in lines)  # one interior sample, every other one an edge row
    assert any(w == 1 for _, w, _ in lines)
    assert any(p == w - 1 and w > 1 for _, w, p in lines)
    assert any(line > 512 and w == 51 for line, w, _ in lines)
    assert {axis for _, _, axis, _, _ in cases.SAVGOL_CASES} == {0, 1}
    assert any(axis == 0 and length > 1 and count >= 300 for count, length, axis, _, _ in cases.SAVGOL_CASES)  # strided lines
    assert {(51, 10), (101, 10)} <= {(w, p) for _, w, p in lines}


def test_element_counts_fall_on_both_sides_of_a_block() -> None:
    counts = [count * length for count, length, _, _, _ in cases.SAVGOL_CASES]
    counts += [count * n_out for count, _, n_out in cases.RESAMPLE_CASES]
    counts += list(cases.REMAP_COUNTS) + [count for _, count in cases.MINMAX_CASES]
    remainders = {count % cases.BLOCK for count in counts if count > cases.BLOCK - 1}
    assert {cases.BLOCK - 1, 0, 1} <= remainders
    assert 1 in counts and 1 in cases.REMAP_COUNTS
    assert max(count for _, count in cases.MINMAX_CASES) == cases.BLOCK * cases.BLOCK + 1  # the second grid-stride trip, one element


def test_rms_and_rolling_cases_reach_every_path_of_the_sums() -> None:
    lengths = set(cases.RMS_VECTOR_LENGTHS)
    assert {1, 7, 8, 127, 128, 129, 512, 1000, audio_ref.NUMPY_REDUCE_BLOCK, audio_ref.NUMPY_REDUCE_BLOCK + 1} == lengths
    windows = {window for window, _, _ in cases.ROLLING_CASES}
    assert 1 in windows and cases.RMS_HOPS in windows and max(windows) > cases.RMS_HOPS
    assert all(w <= cases.RMS_HOPS for _, w, _ in cases.ROLLING_CASES)
    for length in lengths:
        assert 1 + (cases.hop_samples(length, cases.RMS_HOPS) - length) // cases.HOP == cases.RMS_HOPS
        assert 1 + (cases.hop_samples(length, cases.RMS_HOPS) - 1 - length) // cases.HOP == cases.RMS_HOPS - 1
    assert [(hops, hops // 80) for hops, _ in cases.ROLLING_MAX_HOPS] == list(cases.ROLLING_MAX_HOPS)
    assert {size for _, size in cases.ROLLING_MAX_HOPS} == {0, 1, 2, 3, 5}


def test_audio_of_is_a_prefix_of_the_synthetic_track() -> None:
    from gance_amd import synthetic  # pylint: disable=import-outside-toplevel

    audio = cases.audio_of(66, cases.spectrogram_samples(66, 5))
    assert audio.dtype == np.float32 and audio.shape == (4 * 66 + 64,)
    assert np.array_equal(audio, synthetic.synthetic_audio(6, 66, seed=66)[: audio.size])
    assert cases.audio_of(1, cases.hop_samples(1, 20)).shape == (1 + 19 * 512,)


# ---- the Fourier resample operator ------------------------------------------------------------------------------------


def test_the_long_double_resample_matrix_is_scipys_operator() -> None:
    """The reference itself against scipy.signal.resample of the unit impulses: an FFT of at most 50 points in double, 1e-14."""
    worst = 0.0
    for n_in, n_out in RESAMPLE_GRID:
        if n_in > 50:
            continue
        want = resample(np.eye(n_in), n_out, axis=1)
        worst = max(worst, float(np.abs(ref.fourier_resample_matrix(n_in, n_out) - want).max()))
    print(f"long-double matrix against scipy.signal.resample: {worst:.3e}")
    assert worst <= 1e-14


def test_fourier_resample_matrix_is_the_long_double_operator(library: ctypes.CDLL) -> None:
    """Bar: 4 ulp of the largest entry, what tests/test_music.py allows a table built with libm."""
    assert library is not None
    worst = 0.0
    for n_in, n_out in RESAMPLE_GRID:
        got = hip_lib.fourier_resample_matrix(n_in, n_out)
        want = ref.fourier_resample_matrix(n_in, n_out)
        assert got.shape == want.shape == (n_in, n_out) and got.dtype == np.float64
        error = float(np.abs(got.astype(ref.LD) - want).max())
        bar = 4 * float(np.spacing(np.float64(np.abs(want).max())))
        worst = max(worst, error / bar)
        assert error <= bar, (n_in, n_out, error, bar)
    print(f"resample matrix: worst error / bar {worst:.3f} over {len(RESAMPLE_GRID)} length pairs")
    with pytest.raises(ValueError):
        hip_lib.fourier_resample_matrix(0, 4)


# ---- the Savitzky-Golay operator --------------------------------------------------------------------------------------


def test_exact_weights_are_a_projection() -> None:
    """What makes them least-squares weights: H reproduces every polynomial up to the order, and its rows sum to one."""
    for w, p in ((5, 2), (7, 3), (9, 8), (51, 10)):
        rows, denominator = ref.savgol_weights(w, p)
        h = w // 2
        for i, row in enumerate(rows):
            for degree in range(p + 1):
                assert sum(weight * (j - h) ** degree for j, weight in enumerate(row)) == denominator * (i - h) ** degree
        assert rows[h] == rows[h][::-1]
    assert ref.savgol_table_exact(5, 2)[:5] == [ref.Fraction(n, 35) for n in (-3, 12, 17, 12, -3)]  # the textbook quadratic taps


def test_savgol_table_is_the_exact_operator(library: ctypes.CDLL) -> None:
    assert library is not None
    worst = 0.0
    for w, p in SAVGOL_GRID:
        table = hip_lib.savgol_table(w, p)
        assert table.shape == (w + (w // 2) * w,) and table.dtype == np.float64
        error = ref.table_error(table, w, p)
        print(f"    ({w:3d}, {p:3d})  {error:.2e}")
        worst = max(worst, error)
        assert error <= SAVGOL_TABLE_BAR, (w, p, error)
    print(f"Savitzky-Golay table: worst {worst:.3e}, bar {SAVGOL_TABLE_BAR:.3e}")
    assert SAVGOL_TABLE_BAR <= 1e-12


def scipy_table(w: int, p: int) -> np.ndarray:
    """scipy's interior coefficients and polyfit edge rows in the library's layout, from its response to the unit impulses."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # np.polyfit's RankWarning at high orders
        response = savgol_filter(np.eye(w), w, p, axis=0, mode="interp")  # a line as long as the window: row i is H[i]
    h = w // 2
    return np.concatenate([response[h]] + [response[i] for i in range(h)])


def test_savgol_table_keeps_scipy_parity_where_scipy_is_right(library: ctypes.CDLL) -> None:
    """Wherever scipy is within 1e-9 of the exact weights, the table is within 1e-9 of scipy."""
    assert library is not None
    trusted = []
    for w, p in SAVGOL_GRID:
        theirs = scipy_table(w, p)
        exact = np.array([float(value) for value in ref.savgol_table_exact(w, p)])
        if np.abs(theirs - exact).max() <= TOL:
            trusted.append((w, p))
            assert np.abs(hip_lib.savgol_table(w, p) - theirs).max() <= TOL, (w, p)
    print(f"scipy within {TOL} of the exact weights at {len(trusted)} of {len(SAVGOL_GRID)} pairs; not at {sorted(set(SAVGOL_GRID) - set(trusted))}")
    assert {(7, 3), (5, 2), (51, 2), (11, 3)} <= set(trusted)  # the orders the path itself uses are among them


def test_the_savgol_tap_checks_its_arguments(library: ctypes.CDLL) -> None:
    for w, p in ((4, 2), (0, 0), (-3, 0), (5, 5), (5, -1)):
        with pytest.raises(ValueError):
            hip_lib.savgol_table(w, p)
    out = np.full(8, 7.0)
    pointer = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert library.gance_debug_savgol_table(3, 1, pointer, ctypes.c_uint64(8)) == 1  # the table holds 3 + 1 * 3 = 6 values
    assert b"6 values" in library.gance_last_error() and np.all(out == 7.0)
    assert library.gance_debug_savgol_table(3, 1, None, ctypes.c_uint64(6)) == 1
    assert library.gance_debug_savgol_table(3, 1, pointer, ctypes.c_uint64(6)) == 0 and np.all(out[6:] == 7.0)
    np.testing.assert_allclose(out[:3], [1 / 3] * 3, rtol=1e-15)
    assert "gance_debug_savgol_table" in hip_lib.ADDED_WITHIN_ABI and library.gance_abi_version() == 6


# ---- the spectrogram ----------------------------------------------------------------------------------------------------


def test_spectrogram_refuses_tables_past_the_lds_limit_before_touching_a_device(library: ctypes.CDLL) -> None:
    """GANCE_ERR_INVALID_ARGUMENT, not GANCE_ERR_NO_DEVICE or a launch error: the pointers are never looked at."""
    L = cases.SPECTROGRAM_REFUSED_LENGTH
    for truncate in (1, 0):
        status = library.gance_vec_spectrogram2_f64(ctypes.c_void_p(256), ctypes.c_uint64(5 * L), L, truncate, ctypes.c_void_p(512), None)
        assert status == 1
        assert b"2732" in library.gance_last_error()


def test_spectrogram_inputs_keep_the_bar_under_a_microdecibel() -> None:
    """
    The dB bar of the GPU test is relative to |X_k|: it only means something where no bin is lost in cancellation. On these
    inputs it stays under 1e-6 dB at every bin, and the oracle's pocketfft route agrees with the long-double DFT within it.
    """
    worst_bar, worst_oracle = 0.0, 0.0
    for L, frames, truncate in cases.SPECTROGRAM_CASES:
        audio = cases.audio_of(L, cases.spectrogram_samples(L, frames))
        db, magnitude, scale = ref.spectrogram(audio, L, truncate)
        bins = (L - 2) // 2 if truncate else L - 2
        assert db.shape == magnitude.shape == (bins, frames) and scale.shape == (frames,) and db.max() == 0.0
        bar = ref.spectrogram_bar_db(L, magnitude, scale)
        print(f"    L = {L:4d} truncate = {truncate!s:5}: largest bar {bar.max():.2e} dB, lowest bin {db.min():.1f} dB")
        worst_bar = max(worst_bar, float(bar.max()))
        assert bar.max() < 1e-6, (L, truncate)
        if truncate:
            difference = np.abs(audio_ref.compute_spectrogram(audio, L) - db)
            worst_oracle = max(worst_oracle, float(difference.max()))
            assert np.all(difference <= bar), (L, float((difference / bar).max()))
    print(f"spectrogram: largest bar {worst_bar:.2e} dB; oracle against the long-double DFT {worst_oracle:.2e} dB")
