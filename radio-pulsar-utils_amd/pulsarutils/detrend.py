"""Running-median detrending: take the red noise out of a time series before it is folded.

A slow wander of the baseline (receiver gain, sky, a random walk) inflates a series' standard
deviation and spills into every fold of :mod:`pulsarutils.ffa`.  The baseline here is a running
median of block means, interpolated linearly between the block centres and subtracted.  The
reference has no counterpart; the definition is this project's own and claims parity with no other
package (include/pulsarutils_hip.h has it in full; tests/detrend_oracle.py restates it in numpy,
bit for bit).

**Running median** (``pu_running_median``): ``w`` odd, ``h = (w - 1) // 2``; ``out[i]`` is the median
of ``x[clip(i + k, 0, n - 1)]``, ``k = -h .. h`` (the edge sample is repeated, as
``scipy.ndimage.median_filter(mode="nearest")`` does).  It is an element of the window; -0 sorts
before +0, +-inf are ordinary values and a window that holds a NaN gives NaN.

**Plan** (:func:`detrend_plan`): a width of ``W`` samples gives blocks of ``d = max(1, W //
min_points)`` samples and a median over ``w = 2 ((W // d) // 2) + 1`` of them: between
``min_points`` and ``2 min_points`` block means, whatever ``W`` is.

**Baseline**: ``nblk = n // d`` block means (``pu_rebin_time``'s float64 sums over ``d``), their
running median ``med`` at width ``w``, and per sample, in float64, ``u = (2 i - d + 1) / (2 d)``, ``b0 =
clip(floor(u), 0, nblk - 2)``, ``t = clip(u - b0, 0, 1)``, ``base = med[b0] + t (med[b0 + 1] -
med[b0])`` (the median itself at ``t = 0`` and ``t = 1``; ``med[0]`` for one block);
``pu_detrend_apply`` subtracts it.

The width must be many pulse widths - a median over a window that a pulse fills a good part of
takes the pulse for baseline and eats it - and well below the time scale of nothing you want to
keep: everything slower than the width goes.

Conventions are ``periodicity``'s: numpy in -> numpy out, CUDA tensor in -> tensors out, a 1-D
array is one row; float32 and float64 series keep their type, any other becomes float64.
:func:`detrend_plan` and :func:`describe` need no GPU; the rest runs HIP kernels and raises
``HipBackendError`` without the library or a GPU.
"""
import ctypes

import numpy as np

from . import _hip

MAX_WIDTH = 2047   # pu_running_median's limit on w
DESCRIBE_FIELDS = ("tile", "lds_bytes", "w_max")
_FLOATS = (_hip.PU_F32, _hip.PU_F64)


def detrend_plan(width_samples, min_points=101):
    """``(d, w)`` for a width of ``width_samples`` samples: the block length and the odd width of
    the median over block means.  Host only."""
    W, mp = int(width_samples), int(min_points)
    if W < 1 or mp < 1:
        raise ValueError("detrend_plan: width_samples and min_points must be >= 1")
    d = max(1, W // mp)
    w = 2 * ((W // d) // 2) + 1
    if w > MAX_WIDTH:
        raise ValueError(f"detrend_plan: min_points {mp} gives a median over {w} blocks, above the kernel's limit of "
                         f"{MAX_WIDTH}")
    return d, w


def describe(dtype, w):
    """pu_running_median_describe, on the host alone: a dict of ``DESCRIBE_FIELDS`` - the outputs
    of a workgroup, its LDS bytes at this ``dtype`` (numpy float32 / float64) and ``w``, and the
    limit on ``w``."""
    code = {np.dtype(np.float32): _hip.PU_F32, np.dtype(np.float64): _hip.PU_F64}.get(np.dtype(dtype), -1)
    info = np.zeros(len(DESCRIBE_FIELDS), np.int64)
    _hip.check(_hip.lib().pu_running_median_describe(code, int(w), info.ctypes.data_as(ctypes.c_void_p), info.size),
               "pu_running_median_describe")
    return dict(zip(DESCRIBE_FIELDS, info.tolist()))


# ------------------------------------------------------------------ the device stages

def _check_width(w):
    w = int(w)
    if w < 1 or w % 2 == 0 or w > MAX_WIDTH:
        raise ValueError(f"running_median: w must be odd and in 1 .. {MAX_WIDTH}, got {w}")
    return w


def _running_median_device(x, w):
    """pu_running_median of a 2-D row-major float32 / float64 device tensor; a new tensor."""
    t = _hip.torch()
    out = t.empty(x.shape, dtype=x.dtype, device=x.device)
    if x.shape[0]:
        _hip.check(_hip.lib().pu_running_median(_hip.ptr(x), _hip.dtype_code(x.dtype), x.shape[0], x.shape[1],
                                                _hip.row_stride(x), w, _hip.ptr(out), x.shape[1], _hip.stream_ptr()),
                   "pu_running_median")
    return out


def _medians_device(x, d, w):
    """float64 (rows, n // d): the running median at width ``w`` of the means of blocks of ``d``."""
    from .dedispersion import _rebin_time_device
    t = _hip.torch()
    if x.shape[0] == 0:
        return t.empty((0, x.shape[1] // d), dtype=t.float64, device=x.device)
    sums = _rebin_time_device(x, d)
    # a tensor divisor: one IEEE division per mean (a Python scalar would be multiplied by as 1 / d)
    return _running_median_device(sums / t.full((), float(d), dtype=t.float64, device=x.device), w)


def _apply_device(x, med, d, out):
    """pu_detrend_apply: ``out`` (may be ``x``) = ``x`` minus the baseline interpolated from ``med``."""
    if x.shape[0]:
        _hip.check(_hip.lib().pu_detrend_apply(_hip.ptr(x), _hip.dtype_code(x.dtype), x.shape[0], x.shape[1],
                                               _hip.row_stride(x), _hip.ptr(med), med.shape[1], med.shape[1], d,
                                               _hip.ptr(out), _hip.row_stride(out), _hip.stream_ptr()), "pu_detrend_apply")
    return out


def _plan_for(what, n, width_samples, min_points):
    d, w = detrend_plan(width_samples, min_points)
    if n // d < 1:
        raise ValueError(f"{what}: a series of {n} samples has no block of {d}")
    return d, w


def _detrend_device(x, width_samples, min_points=101, in_place=False):
    """The detrended rows of a 2-D row-major float32 / float64 device tensor (``x`` itself with
    ``in_place``)."""
    t = _hip.torch()
    d, w = _plan_for("detrend", x.shape[1], width_samples, min_points)
    out = x if in_place else t.empty(x.shape, dtype=x.dtype, device=x.device)
    return _apply_device(x, _medians_device(x, d, w), d, out)


def _result(y, one_d, as_numpy):
    if one_d:
        y = y[0]
    return y.cpu().numpy() if as_numpy else y


def running_median(series, w):
    """The running median of width ``w`` (odd, at most 2047) of every row, in the rows' type."""
    w = _check_width(w)
    x, one_d, as_numpy = _hip.as_rows(series, "running_median: series must be (rows, nsamples) or 1-D", _FLOATS)
    if x.shape[1] < 1:
        raise ValueError("running_median: an empty series")
    return _result(_running_median_device(x, w), one_d, as_numpy)


def baseline(series, width_samples, min_points=101):
    """The baseline :func:`detrend` subtracts: float64, the shape of ``series``."""
    t = _hip.require_gpu()
    x, one_d, as_numpy = _hip.as_rows(series, "baseline: series must be (rows, nsamples) or 1-D", _FLOATS)
    d, w = _plan_for("baseline", x.shape[1], width_samples, min_points)
    med = _medians_device(x, d, w)
    # the one implementation of the interpolation is pu_detrend_apply's: -0 - base is -base in
    # every bit (+0 for base = -0, -0 for base = +0), and negating gives base back
    zero = t.full(x.shape, -0.0, dtype=t.float64, device=x.device)
    return _result(_apply_device(zero, med, d, zero).neg_(), one_d, as_numpy)


def detrend(series, width_samples, min_points=101):
    """``series`` minus its :func:`baseline` at a width of ``width_samples`` samples, in the
    series' type (the subtraction is float64, rounded once)."""
    x, one_d, as_numpy = _hip.as_rows(series, "detrend: series must be (rows, nsamples) or 1-D", _FLOATS)
    return _result(_detrend_device(x, width_samples, min_points), one_d, as_numpy)


__all__ = ["detrend_plan", "describe", "running_median", "baseline", "detrend"]
