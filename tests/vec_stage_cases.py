"""
The shapes of the isolated checks of the stand-alone audio stages (`gance_vec_*` of gance_amd/csrc/audio.hip), shared by
tests/test_vec_stage_cases.py (which checks from the shapes alone that the tables reach the branches they claim, and
checks the host tables) and tests/test_vec_stage_shapes_gpu.py (which runs them). Each case is the smallest shape that
reaches its branch; the branch stands beside it.

Left out on purpose: a constant series through the quantizer. Its remap is 0 / 0 in the reference as well
(oracle/audio_ref.py, quantize_to_indices: "min == max is undefined"), so there is nothing to hold the kernel to.
"""

import numpy as np

from gance_amd import synthetic

BLOCK = 256  # threads per block of every element-wise gance_vec_* kernel, and of dft_magnitude_kernel
HOP = 512  # librosa's default hop, whatever the frame length

# Savitzky-Golay (num_vectors N, vector_length L, axis, window_length w, polyorder p); axis 0 filters lines of N samples
SAVGOL_CASES = (
    (7, 5, 0, 7, 3),  # a line exactly as long as the window: one interior sample, every other one an edge row
    (3, 8, 1, 1, 0),  # window 1: the identity, no edge rows at all
    (2, 9, 1, 9, 8),  # the interpolating order p = w - 1, on a line equal to the window
    (33, 31, 0, 5, 2),  # 1023 elements: one short of four blocks, strided lines
    (33, 31, 1, 5, 2),  # ... and the same along the contiguous axis
    (2, 600, 1, 51, 2),  # the default window on a line past 512
    (300, 3, 0, 7, 3),  # long strided lines, 900 elements (no multiple of 256)
    (2, 64, 1, 51, 10),  # an order at which scipy's own edge fit is 1e-3 off
    (2, 128, 1, 101, 10),  # an order at which scipy's own edge fit is about 0.6 off (256 elements: exactly one block)
)

# Fourier resample (num_vectors N, in_length, out_length)
RESAMPLE_CASES = (
    tuple((2, n_in, n_out) for n_in in (7, 8) for n_out in (7, 8, 12, 13))  # equal lengths and up, every parity pair
    + tuple((2, n_in, n_out) for n_in in (12, 13) for n_out in (7, 8))  # down, every parity pair
    + (
        (5, 1, 4),  # a single input sample: only the mean term
        (5, 6, 1),  # a single output sample
        (3, 100, 171),  # 513 outputs: one past two blocks
        (2, 1000, 37),  # long lines down to a short odd one
        (1, 8192, 3),  # the length limit of the entry point
    )
)
RESAMPLE_REFUSED = ((1, 8193, 3), (1, 3, 65537))  # one past each limit: ValueError

# spectrogram (vector_length L, frames, truncate): window m = L - 2, bins m / 2 (truncate) or m; one block of 256 threads per
# frame, thread k takes bins k, k + 256, ...
SPECTROGRAM_LENGTHS = (
    4,  # the shortest: a window of 2 samples, 1 bin
    6,  # 2 bins
    64,  # 31 bins
    66,  # 32 bins: an even bin count
    514,  # 256 bins: exactly one block, one trip; 512 bins untruncated, two full trips
    516,  # 257 bins: the second trip; 514 bins untruncated, three trips
    1000,  # the reference's own test length
    1024,  # 511 bins, two trips; 1022 untruncated, four
    2732,  # the largest tables that fit the 64 KiB of LDS a launch may take
)
SPECTROGRAM_FRAMES = 5
SPECTROGRAM_CASES = tuple((L, SPECTROGRAM_FRAMES, truncate) for L in SPECTROGRAM_LENGTHS for truncate in (True, False))
SPECTROGRAM_REFUSED_LENGTH = 2734  # 3 * 2732 * 8 bytes > 64 KiB: ValueError before anything is launched

# mirrors of the reference's functions (gance_amd/apply_spectrogram.py, gance_amd/vector_sources/vector_sources_common.py)
SMOOTH_SCALE_LENGTHS = (66, 1000)  # compute_spectrogram_smooth_scale(audio, L, (-2, 2)): even and odd bin counts into the resample
SMOOTH_SCALE_FRAMES = 12
MIRROR_RESAMPLE = (3, 13, 8)  # scale_vectors_to_length_resample, odd to even downwards

# RMS and rolling average: a series of RMS_HOPS values, frames of vector_length samples every 512
RMS_VECTOR_LENGTHS = (
    1,  # one sample per frame
    7,  # numpy's plain loop (fewer than 8 values)
    8,  # the first length on the unrolled path
    127,  # the unrolled path with a tail of 7
    128,  # the longest run summed without a split
    129,  # the first split (64 + 65)
    512,  # the hop itself
    1000,  # the reference's own test length; frames overlap
    8192,  # exactly one block of numpy's reduction buffer
    8193,  # the second block: one value added to the running total
)
RMS_HOPS = 20
# (rolling_window, savgol window_length, savgol polyorder)
ROLLING_CASES = (
    (1, 1, 0),  # a window of one value: no NaN head; filter window 1
    (3, 7, 3),  # the defaults
    (20, 5, 2),  # a window as long as the series: one computed value, nineteen fill values
    (25, 19, 2),  # a window longer than the series: every value is the fill value
)

# rolling maximum: (hops, size of the maximum filter = hops // 80), each at vector_length 512 and 1000
ROLLING_MAX_HOPS = (
    (79, 0),  # below 80 values: a copy
    (80, 1),  # size 1: the identity through the filter kernel
    (160, 2),  # even size: the window leans left
    (241, 3),  # odd size
    (400, 5),  # reflection two samples deep; two blocks
)
ROLLING_MAX_VECTOR_LENGTHS = (512, 1000)

# min-max scale: (name, count); range (-5, 5). 256 blocks x 256 threads stride over the array, so 65537 takes a second trip
MINMAX_RANGE = (-5.0, 5.0)
MINMAX_CASES = (("one", 1), ("constant", 1000), ("second_trip", 65537), ("negative", 300))
MINMAX_REFUSED = (np.nan, np.inf, -np.inf)  # each as the LAST element of 1000: ValueError

# remap: counts, input range (-2, 5) onto the reversed output range (10, -3)
REMAP_COUNTS = (1, 255, 257)
REMAP_INPUT_RANGE, REMAP_OUTPUT_RANGE = (-2.0, 5.0), (10.0, -3.0)

# quantize
QUANTIZE_TIES = ((0.0, 0.5, 1.5, 2.5, 3.0), 4, (0, 0, 2, 2, 3))  # exact .5 ties go to the even integer
QUANTIZE_CASES = ((2, 3), (20000, 5), (20000, 1))  # (count, K); K = 1 gives all zeros


def matrix(rows: int, columns: int, seed: int) -> np.ndarray:
    """Seeded standard-normal float64 [rows][columns]."""
    return np.random.RandomState(seed).randn(rows, columns)


def audio_of(vector_length: int, num_samples: int) -> np.ndarray:
    """The first `num_samples` samples of `synthetic_audio(frames + 1, L, seed=L)`, frames = the whole frames that many samples span."""
    frames = -(-num_samples // vector_length)
    return synthetic.synthetic_audio(frames + 1, vector_length, seed=vector_length)[:num_samples]


def spectrogram_samples(vector_length: int, frames: int) -> int:
    """The fewest samples that give `frames` windows of L - 2 samples every L; one less drops a frame."""
    return (frames - 1) * vector_length + vector_length - 2


def hop_samples(vector_length: int, hops: int) -> int:
    """The fewest samples that give `hops` RMS values."""
    return vector_length + (hops - 1) * HOP


def minmax_input(name: str, count: int) -> np.ndarray:
    if name == "constant":
        return np.full(count, 0.3)
    data = np.random.RandomState(count).randn(count) * 7.0
    if name == "negative":
        data = -np.abs(data) - 1.0
    return data
