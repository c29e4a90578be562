"""Running-median detrending restated in numpy from the definition alone
(include/pulsarutils_hip.h, "running-median detrending").

Running median: ``w`` odd, ``h = (w - 1) // 2``; ``out[r][i]`` is the median of ``x[r][clip(i + k, 0,
n - 1)]``, ``k = -h .. h`` - an element of the window, ordered by value with -0 before +0, +-inf
ordinary values; a window that holds a NaN gives the canonical quiet NaN.

Plan: ``d = max(1, W // min_points)``, ``w = 2 ((W // d) // 2) + 1``.

Baseline: ``nblk = n // d`` block sums (``d`` samples added in order to 0.0, float64), ``mean = sum /
d``, ``med`` = the running median of ``mean`` at width ``w``; per sample, one float64 operation each,

    u = (2 i - d + 1) / (2 d),  b0 = clip(floor(u), 0, nblk - 2),  t = clip(u - b0, 0, 1)
    base = med[b0] + t (med[b0 + 1] - med[b0])                    (med[0] for nblk == 1)

with ``med[b0]`` itself where ``t == 0`` and ``med[b0 + 1]`` itself where ``t == 1``,

and ``out[i] = (T)((double)x[i] - base)``.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

_KEY = {np.dtype(np.float32): (np.uint32, 31), np.dtype(np.float64): (np.uint64, 63)}


def to_keys(x):
    """Unsigned keys whose integer order is the order of the values, -0 before +0."""
    x = np.ascontiguousarray(x)
    ut, top = _KEY[x.dtype]
    b = x.view(ut)
    sign = (b >> ut(top)).astype(bool)
    return np.where(sign, ~b, b | (ut(1) << ut(top)))


def from_keys(k, dtype):
    ut, top = _KEY[np.dtype(dtype)]
    k = np.ascontiguousarray(k, dtype=ut)
    return np.where((k >> ut(top)).astype(bool), k ^ (ut(1) << ut(top)), ~k).astype(ut).view(dtype)


def running_median(x, w):
    """The running median of every row of float32 / float64 ``x`` (1-D: one row), same dtype."""
    x = np.asarray(x)
    if x.dtype not in _KEY:
        raise ValueError("running_median: float32 or float64")
    w = int(w)
    if w < 1 or w % 2 == 0:
        raise ValueError("running_median: w odd and >= 1")
    h = (w - 1) // 2
    rows = np.atleast_2d(x)
    pad = np.pad(rows, ((0, 0), (h, h)), mode="edge")
    win = sliding_window_view(pad, w, axis=1)
    med = from_keys(np.sort(sliding_window_view(to_keys(pad), w, axis=1), axis=-1)[..., h], x.dtype)
    med = np.where(np.isnan(win).any(axis=-1), np.array(np.nan, x.dtype), med)  # np.nan: the canonical quiet NaN
    return med.reshape(x.shape)


def detrend_plan(width_samples, min_points=101):
    W, mp = int(width_samples), int(min_points)
    if W < 1 or mp < 1:
        raise ValueError("detrend_plan: width_samples >= 1 and min_points >= 1")
    d = max(1, W // mp)
    return d, 2 * ((W // d) // 2) + 1


def block_means(x, d):
    """float64 (rows, n // d): d samples added in order to 0.0, divided by d."""
    x = np.atleast_2d(np.asarray(x))
    nblk = x.shape[1] // d
    s = np.zeros((x.shape[0], nblk))
    for j in range(d):
        s = s + x[:, j:nblk * d:d].astype(np.float64)
    return s / np.float64(d)


def interpolate(med, n, d):
    """The baseline of ``n`` samples from float64 ``med`` (rows, nblk), nblk = n // d."""
    med = np.atleast_2d(np.asarray(med, dtype=np.float64))
    nblk = med.shape[1]
    assert nblk == n // d and nblk >= 1
    if nblk == 1:
        return np.repeat(med[:, :1], n, axis=1)
    i = np.arange(n, dtype=np.int64)
    u = (2 * i - d + 1).astype(np.float64) / np.float64(2 * d)
    b0 = np.clip(np.floor(u).astype(np.int64), 0, nblk - 2)
    t = np.clip(u - b0.astype(np.float64), 0.0, 1.0)
    m0, m1 = med[:, b0], med[:, b0 + 1]
    with np.errstate(invalid="ignore"):
        return np.where(t == 0.0, m0, np.where(t == 1.0, m1, m0 + t * (m1 - m0)))


def baseline(x, width_samples, min_points=101):
    """float64 baseline of every row of ``x`` (1-D: one row), the shape of ``x``."""
    x = np.asarray(x)
    d, w = detrend_plan(width_samples, min_points)
    rows = np.atleast_2d(x)
    if rows.shape[1] // d < 1:
        raise ValueError("baseline: fewer samples than one block")
    med = running_median(block_means(rows, d), w)
    return interpolate(med, rows.shape[1], d).reshape(x.shape)


def apply(x, med, d):
    """(T)((double)x - base) of rows ``x`` with the medians ``med`` of blocks of ``d`` samples."""
    x = np.asarray(x)
    rows = np.atleast_2d(x)
    with np.errstate(invalid="ignore"):
        return (rows.astype(np.float64) - interpolate(med, rows.shape[1], d)).astype(x.dtype).reshape(x.shape)


def detrend(x, width_samples, min_points=101):
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return (x.astype(np.float64) - baseline(x, width_samples, min_points)).astype(x.dtype)


def same_bits(a, b):
    """a and b have the same dtype, shape and bits."""
    a, b = np.asarray(a), np.asarray(b)
    ut = _KEY[a.dtype][0]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(ut),
                                                                        np.ascontiguousarray(b).view(ut))


def same_bits_or_nan(a, b):
    """As same_bits, but a NaN made by arithmetic matches any NaN (its sign and payload are
    unspecified)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return same_bits(a[ok], b[ok])


def red_noise_series(amplitude=0.8, n=65536, period=250.37, duty=0.02, seed=5):
    """(white, red): unit noise plus a top-hat pulse, and the same with two slow sinusoids and a
    random walk added; float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    white = rng.standard_normal(n) + amplitude * (((t / period) % 1.0) < duty)
    red = (6.0 * np.sin(2 * np.pi * t / 3100.0 + 0.3) + 4.0 * np.sin(2 * np.pi * t / 7777.0)
           + 15.0 * np.cumsum(rng.standard_normal(n)) / np.sqrt(n))
    return white.astype(np.float32), (white + red).astype(np.float32)
