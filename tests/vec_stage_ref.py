"""
References for the isolated checks of the stand-alone audio stages that do NOT go through scipy's numerics
(tests/test_vec_stage_cases.py, tests/test_vec_stage_shapes_gpu.py):

  Savitzky-Golay    the least-squares weights in exact rational arithmetic (integer abscissae), applied to the data exactly
                    (a double is a rational) and rounded once
  Fourier resample  the operator by direct long-double sums of scipy.signal.resample's documented steps, applied in long double
  spectrogram       periodic Hann window and a direct DFT in long double, the angle k n mod m reduced in integers

Every function also returns the error scale S of each output, the absolute dot product sum_j |c_j x_j|: what one rounding
error per term is relative to, and so what the bars of the GPU tests are written in.
"""

import functools
from fractions import Fraction
from math import lcm
from typing import List, Tuple

import numpy as np

LD = np.longdouble
TWO_PI = 2 * LD("3.14159265358979323846264338327950288419716939937510")
EPS = 2.0**-53  # one rounding of a double


# ---- Savitzky-Golay ---------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def savgol_weights(window_length: int, polyorder: int) -> Tuple[Tuple[Tuple[int, ...], ...], int]:
    """
    Rows 0 .. w // 2 of the hat matrix H = A (A^T A)^-1 A^T of the least-squares fit of a polynomial of degree p to w equally
    spaced samples (A[j][k] = x_j^k, x_j = j - w // 2): H[i][j] is the weight of sample j in the fitted value at position i.
    Row w // 2 holds the interior taps, rows i < w // 2 the edge fit of scipy.signal.savgol_filter's mode "interp".
    Exact: returned as integer numerators over one common denominator.

    H = sum_k q_k(x_i) q_k(x_j) / <q_k, q_k> over the first p + 1 monic polynomials orthogonal on the points, which come
    from the three-term recurrence q_{k+1} = (x - a_k) q_k - b_k q_{k-1}, a_k = <x q_k, q_k> / <q_k, q_k>,
    b_k = <q_k, q_k> / <q_{k-1}, q_{k-1}>, all in rationals.
    """
    w, p, h = window_length, polyorder, window_length // 2
    assert w >= 1 and w % 2 == 1 and 0 <= p < w
    points = [Fraction(j - h) for j in range(w)]
    previous, current = [Fraction(0)] * w, [Fraction(1)] * w
    previous_norm = Fraction(1)
    integer_polynomials, norms = [], []
    for k in range(p + 1):
        norm = sum(value * value for value in current)
        scale = lcm(*(value.denominator for value in current))
        as_integers = [int(value * scale) for value in current]
        integer_polynomials.append(as_integers)
        norms.append(sum(value * value for value in as_integers))
        if k == p:
            break
        a = sum(x * value * value for x, value in zip(points, current)) / norm
        b = norm / previous_norm if k > 0 else Fraction(0)
        previous, current = current, [(x - a) * value - b * old for x, value, old in zip(points, current, previous)]
        previous_norm = norm
    denominator = lcm(*norms)
    rows = []
    for i in range(h + 1):
        row = [0] * w
        for q, norm in zip(integer_polynomials, norms):
            factor = q[i] * (denominator // norm)
            for j in range(w):
                row[j] += factor * q[j]
        rows.append(tuple(row))
    return tuple(rows), denominator


def savgol_table_exact(window_length: int, polyorder: int) -> List[Fraction]:
    """The layout of libgance_hip's table: w interior taps, then w // 2 edge rows of w weights, as exact rationals."""
    rows, denominator = savgol_weights(window_length, polyorder)
    h = window_length // 2
    return [Fraction(value, denominator) for row in (rows[h],) + rows[:h] for value in row]


def table_error(table: np.ndarray, window_length: int, polyorder: int) -> float:
    """max over the table of |entry - exact| / max |row|, the differences taken exactly."""
    exact = savgol_table_exact(window_length, polyorder)
    assert len(exact) == table.size
    worst = Fraction(0)
    for start in range(0, len(exact), window_length):
        row = exact[start : start + window_length]
        largest = max(abs(value) for value in row)
        for value, got in zip(row, table[start : start + window_length]):
            worst = max(worst, abs(Fraction(float(got)) - value) / largest)
    return float(worst)


def _exact_integers(values: np.ndarray) -> Tuple[List[int], int]:
    """Doubles as integers times one power of two: values[i] == integers[i] * 2 ** low exactly."""
    mantissas, exponents = np.frexp(np.asarray(values, dtype=np.float64))
    low = int(exponents.min()) - 53
    return [int(np.ldexp(m, 53)) << (int(e) - 53 - low) for m, e in zip(mantissas, exponents)], low


def savgol_lines(lines: np.ndarray, window_length: int, polyorder: int) -> Tuple[np.ndarray, np.ndarray]:
    """
    scipy.signal.savgol_filter(mode="interp") along axis 1 of [count][n], exactly, rounded once to float64; and S per output.
    Positions h <= i < n - h take the interior taps, the first h the edge rows on the first w samples, the last h the same rows
    mirrored on the last w samples.
    """
    lines = np.asarray(lines, dtype=np.float64)
    assert lines.ndim == 2 and np.all(np.isfinite(lines))
    w, h, n = window_length, window_length // 2, lines.shape[1]
    assert w <= n
    rows, denominator = savgol_weights(window_length, polyorder)
    float_rows = [[abs(float(Fraction(value, denominator))) for value in row] for row in rows]
    out, scale = np.empty_like(lines), np.empty_like(lines)
    for index, line in enumerate(lines):
        integers, low = _exact_integers(line)
        absolute = np.abs(line)
        unit = Fraction(2) ** low / denominator
        for i in range(n):
            if i < h:
                row, samples = i, range(0, w)
            elif i >= n - h:
                row, samples = n - 1 - i, range(n - 1, n - 1 - w, -1)
            else:
                row, samples = h, range(i - h, i + h + 1)
            total = sum(weight * integers[j] for weight, j in zip(rows[row], samples))
            out[index, i] = float(total * unit)  # Fraction -> float rounds correctly, once
            scale[index, i] = float(sum(LD(weight) * LD(absolute[j]) for weight, j in zip(float_rows[row], samples)))
    return out, scale


def savgol(data: np.ndarray, axis: int, window_length: int, polyorder: int) -> Tuple[np.ndarray, np.ndarray]:
    """`savgol_lines` along `axis` of a 2-D array."""
    if axis == 0:
        out, scale = savgol_lines(np.asarray(data).T, window_length, polyorder)
        return np.ascontiguousarray(out.T), np.ascontiguousarray(scale.T)
    return savgol_lines(data, window_length, polyorder)


def savgol_bar(window_length: int, scale: np.ndarray) -> np.ndarray:
    """A w-term fp64 dot product, one rounding of each table entry, one of the result."""
    return (window_length + 4) * EPS * scale


# ---- Fourier resample -------------------------------------------------------------------------------------------


def _unit_circle(numerators: np.ndarray, period: int) -> Tuple[np.ndarray, np.ndarray]:
    """cos and sin of 2 pi r / period in long double, r reduced modulo the period in integers first."""
    angle = TWO_PI * (np.asarray(numerators, dtype=np.int64) % period).astype(LD) / LD(period)
    return np.cos(angle), np.sin(angle)


@functools.lru_cache(maxsize=None)
def fourier_resample_matrix(n_in: int, n_out: int) -> np.ndarray:
    """
    scipy.signal.resample of a real line as the long-double matrix M[n][j] (y = x M), from the library's documented steps:
    X = rfft(x); keep the first min(n_in, n_out) // 2 + 1 terms; when N = min(n_in, n_out) is even, the term at N / 2 is
    doubled going down (it stands for both +N/2 and -N/2 of the input) and halved going up (it is split between the two);
    irfft to n_out points, whose own Nyquist term (n_out even, k = n_out / 2) is real and counted once while every other
    term k > 0 counts twice (itself and its conjugate); scale by n_out / n_in, which with irfft's 1 / n_out leaves 1 / n_in.
    """
    smaller = min(n_in, n_out)
    kept = smaller // 2 + 1
    n, j = np.arange(n_in, dtype=np.int64), np.arange(n_out, dtype=np.int64)
    total = np.ones((n_in, n_out), dtype=LD)  # k = 0: the mean
    for k in range(1, kept):
        x_cos, x_sin = _unit_circle(k * n, n_in)  # X_k of the unit impulse at n: exp(-2 pi i k n / n_in)
        re, im = x_cos, -x_sin
        if smaller % 2 == 0 and k == smaller // 2:
            factor = LD(2) if n_out < n_in else LD(0.5) if n_in < n_out else LD(1)
            re, im = re * factor, im * factor
        out_cos, out_sin = _unit_circle(k * j, n_out)  # the output term: Re(Y_k exp(+2 pi i k j / n_out))
        if n_out % 2 == 0 and k == n_out // 2:
            total += np.outer(re, out_cos)
        else:
            total += 2 * (np.outer(re, out_cos) - np.outer(im, out_sin))
    return total / LD(n_in)


def fourier_resample(data: np.ndarray, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """Every row of [count][n_in] resampled to n_out points in long double, rounded once; and S per output."""
    lines = np.asarray(data, dtype=np.float64).astype(LD)
    operator = fourier_resample_matrix(lines.shape[1], n_out)
    return (lines @ operator).astype(np.float64), (np.abs(lines) @ np.abs(operator)).astype(np.float64)


def resample_bar(n_in: int, scale: np.ndarray) -> np.ndarray:
    """An n_in-term fp64 dot product, one rounding of each matrix entry, one of the result."""
    return (n_in + 4) * EPS * scale


# ---- spectrogram ------------------------------------------------------------------------------------------------


_WINDOW_CACHE: dict = {}  # the samples of one window -> (|X_k| for every k < m, sum_n |x_n w_n|); computed once, shared, never changed


def _dft_magnitudes(audio: np.ndarray, vector_length: int) -> Tuple[np.ndarray, np.ndarray]:
    """|X_k| for every bin k < m of every window, long double [frames][m], and sum_n |x_n w_n| per window."""
    m = vector_length - 2
    frames = (audio.size - m) // vector_length + 1
    keys = [audio[t * vector_length : t * vector_length + m].tobytes() for t in range(frames)]
    missing = sorted(set(key for key in keys if key not in _WINDOW_CACHE))
    if missing:
        n = np.arange(m, dtype=np.int64)
        circle_cos, circle_sin = _unit_circle(n, m)
        window = LD(0.5) - LD(0.5) * circle_cos  # np.hanning(m + 1)[:-1]: periodic
        windowed = np.stack([np.frombuffer(key, dtype=np.float32).astype(LD) * window for key in missing])  # [windows][m]
        magnitude = np.empty((len(missing), m), dtype=LD)
        for first in range(0, m, 256):
            k = np.arange(first, min(first + 256, m), dtype=np.int64)
            index = np.outer(k, n) % m  # the angle of exp(-2 pi i k n / m), reduced before the long-double cos / sin
            re = windowed @ circle_cos[index].T
            im = -(windowed @ circle_sin[index].T)
            magnitude[:, first : first + k.size] = np.hypot(re, im)
        for key, row, line in zip(missing, magnitude, windowed):
            row.setflags(write=False)
            _WINDOW_CACHE[key] = (row, np.abs(line).sum())
    return np.stack([_WINDOW_CACHE[key][0] for key in keys]), np.array([_WINDOW_CACHE[key][1] for key in keys], dtype=LD)


def spectrogram(audio: np.ndarray, vector_length: int, truncate: bool) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """
    compute_spectrogram of float32 mono samples: windows of m = L - 2 samples every L, periodic Hann, DFT, the first m // 2 bins
    (or all m with truncate off), 20 log10(|X| / max |X|) against the maximum over everything kept, transposed to [bins][frames].
    Returns (dB float64, |X| float64 [bins][frames], S float64 [frames]): S = sum_n |x_n w_n|, the absolute dot product of every
    bin of the frame (the twiddles have modulus 1).
    """
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    m = vector_length - 2
    assert vector_length >= 4 and m % 2 == 0 and audio.ndim == 1 and audio.size >= m
    magnitude, scale = _dft_magnitudes(audio, vector_length)
    kept = magnitude[:, : m // 2 if truncate else m]
    db = LD(20) * np.log10(kept / kept.max())
    return np.ascontiguousarray(db.T.astype(np.float64)), np.ascontiguousarray(kept.T.astype(np.float64)), scale.astype(np.float64)


def spectrogram_bar_db(vector_length: int, magnitude: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """
    dB per bin: an m-term fp64 dot product with rounded window and twiddles leaves |X_k| off by (m + 4) 2^-53 S, which is
    20 / ln 10 = 8.686 times that over |X_k| in dB; the maximum the bin is divided by carries the same from its own frame.
    """
    m = vector_length - 2
    relative = (m + 4) * EPS * scale[None, :] / magnitude
    return 8.686 * (relative + relative.flat[np.argmax(magnitude)])
