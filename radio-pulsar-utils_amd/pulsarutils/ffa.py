"""The fast folding algorithm (FFA): a time-domain search for long-period, narrow pulses.

``periodicity_search`` sums at most 32 harmonics incoherently, and a pulse with a duty cycle of
half a per cent has two hundred; ``folding.frequency_search`` folds coherently but gives every
trial its own pass over the series.  The FFA folds ``m`` rows of ``p`` bins at all ``m`` periods
between ``p`` and ``p + 1`` bins at once, sharing partial folds in a tree of ``log2 m`` levels, and
a boxcar matched filter scores every folded profile.  The reference has no counterpart, and the
definition is this project's own: it claims parity with no other package.

**Definitions** (include/pulsarutils_hip.h has them in full; tests/ffa_oracle.py restates them in
numpy, bit for bit).  ``rdiv(a, b) = (2a + b) // (2b)``.

Transform (``pu_ffa``): ``x[i][j] = series[i p + j]``, ``m`` rows; ``F(x) = x`` for one row, else
``nh = m // 2``, ``nt = m - nh``, ``H = F(x[:nh])``, ``T = F(x[nh:])`` and ``F[s][j] = H[h][j] +
T[t][(j + b) % p]`` with ``h = rdiv(s (nh - 1), m - 1)``, ``t = rdiv(s (nt - 1), m - 1)``, ``b = s -
t``: float32 adds, head operand on the left.  Row ``s`` folds at ``p + s / (m - 1)`` bins.
:func:`ffa_tables` gives the same tree level by level, as the kernels walk it.

S/N: for a profile ``v``, a width ``w`` and the series' noise ``sigma``: ``(B_w - w T / p) /
(sqrt(m w (1 - w / p)) sigma)`` with ``T`` the profile's sum and ``B_w`` its largest circular
window sum of ``w`` bins; ``peak`` is the first bin of that window.  A Gaussian S/N of one trial: no
false-alarm model over the trials is built.

A search covers a range of periods with integer downsampling factors (:func:`ffa_plan`): factor
``d`` sums ``d`` samples (``pu_rebin_time``, float64) and folds at base periods from ``bins_min``
bins up to where the next factor takes over.  Each downsampled row is normalised by its own mean
and standard deviation.  With ``detrend_width`` (seconds) the series first loses its red noise: a
running-median baseline of that width (:mod:`pulsarutils.detrend`) is subtracted once, from the
float64 series, before any downsampling.  The width must be many pulse widths, or the median
takes the pulse for baseline and eats it.  Without it the rows are folded as they come.

Known limits: detrending is off by default and its width is the caller's choice (no estimate of
the red noise's time scale is made); integer downsampling factors only; no acceleration; no plots
and no command-line tool.

Conventions are ``periodicity``'s: numpy in -> numpy out, CUDA tensor in -> tensors out, a 1-D
array is one row.  Importable without a GPU: :func:`ffa_tables`, :func:`trial_periods`,
:func:`default_widths`, :func:`ffa_plan` and :func:`describe` are pure numpy or host-only; the rest
runs HIP kernels and raises ``HipBackendError`` without the library or a GPU.
"""
import ctypes
import math

import numpy as np

from . import _hip

MAX_BINS = 2048    # pu_ffa's limit on p
MAX_WIDTHS = 16    # widths of one call
_WS_BYTES = 4 << 30  # pu_ffa's workspace per call: more rows go in batches
_MAX_ROWS_M = (1 << 31) - 1  # rows x m of one call
DESCRIBE_FIELDS = ("depth", "lds_levels", "block_rows", "workspace_bytes", "global_levels", "p_max", "lds_bytes",
                   "traffic_bytes")


def _rdiv(a, b):
    return (2 * a + b) // (2 * b)


def ffa_tables(m):
    """The tree of the transform of ``m`` rows, bottom level first: a list of ``ceil(log2 m)``
    tuples ``(head, tail, rot)`` of int64 arrays of ``m`` entries.  A level makes row ``g`` of its
    output plane as ``below[head[g]] + roll(below[tail[g]], -rot[g])`` (``[(j + rot) % p]``), or
    copies ``below[head[g]]`` where ``tail[g] == -1`` (a block of one row: only at the bottom
    level).  The blocks of a level are the top-down halvings of ``[0, m)``, stored in place; the
    tables do not depend on ``p``."""
    m = int(m)
    if m < 1:
        raise ValueError("ffa_tables: m must be >= 1")
    depth = (m - 1).bit_length()
    blocks = [(0, m)]
    per_depth = []
    for _ in range(depth):
        per_depth.append(blocks)
        nxt = []
        for start, size in blocks:
            nh = size // 2
            nxt += [(start, size)] if size == 1 else [(start, nh), (start + nh, size - nh)]
        blocks = nxt
    levels = []
    for blocks in reversed(per_depth):
        head, tail, rot = np.zeros(m, np.int64), np.full(m, -1, np.int64), np.zeros(m, np.int64)
        for start, size in blocks:
            if size == 1:
                head[start] = start
                continue
            nh = size // 2
            nt = size - nh
            s = np.arange(size, dtype=np.int64)
            h, t = _rdiv(s * (nh - 1), size - 1), _rdiv(s * (nt - 1), size - 1)
            head[start:start + size] = start + h
            tail[start:start + size] = start + nh + t
            rot[start:start + size] = s - t
        levels.append((head, tail, rot))
    return levels


def trial_periods(p, m, sample_time=1.0):
    """The periods of the ``m`` rows of a transform at base period ``p``: ``(p + s / (m - 1))
    sample_time``, ``s = 0 .. m - 1`` (``p sample_time`` alone for ``m = 1``); float64."""
    p, m = int(p), int(m)
    if p < 2 or m < 1:
        raise ValueError("trial_periods: p >= 2 and m >= 1")
    if m == 1:
        return np.array([p * float(sample_time)])
    return (p + np.arange(m, dtype=np.float64) / (m - 1)) * float(sample_time)


def default_widths(p):
    """Boxcar widths in bins for a profile of ``p`` bins: 1, 2, 3, 4, 6, 9, 13, 19 .. - each
    ``max(w + 1, floor(1.5 w))`` after the last - while ``w <= p // 4``, at least ``[1]``, at most
    16 of them.  int32."""
    p = int(p)
    if p < 2:
        raise ValueError("default_widths: p must be >= 2")
    out, w = [], 1
    while w <= max(1, p // 4) and w < p and len(out) < MAX_WIDTHS:
        out.append(w)
        w = max(w + 1, (3 * w) // 2)
    return np.asarray(out, dtype=np.int32)


def ffa_plan(n, sample_time, period_min, period_max, bins_min=240, bins_max=260, min_rows=8):
    """The steps ``(d, p_first, p_stop)`` of a search of ``n`` samples from ``period_min`` to
    ``period_max`` (seconds): downsample by the integer factor ``d``, then fold at the base
    periods ``p_first <= p < p_stop`` bins.  The first factor is ``max(1, floor(period_min /
    (bins_min sample_time)))``, the factor after ``d`` is ``d' = max(d + 1, floor(d bins_max /
    bins_min))``, and ``d`` takes ``p = bins_min .. ceil(bins_min d' / d) - 1``, so consecutive
    factors tile the period axis without a gap (a small ``d`` simply takes more base periods); the
    last factor is the last whose first period ``bins_min d sample_time`` is not above
    ``period_max``.  Base periods that leave fewer than ``min_rows`` rows (``(n // d) // p``) are
    dropped.  ``ValueError`` for an empty plan's arguments or a base period above the kernel's
    limit of 2048 bins."""
    n, bins_min, bins_max, min_rows = int(n), int(bins_min), int(bins_max), int(min_rows)
    sample_time, period_min, period_max = float(sample_time), float(period_min), float(period_max)
    if n < 1 or not sample_time > 0 or not period_min > 0 or not period_max >= period_min:
        raise ValueError("ffa_plan: n and sample_time positive, 0 < period_min <= period_max")
    if bins_min < 2 or bins_max <= bins_min or min_rows < 1:
        raise ValueError("ffa_plan: 2 <= bins_min < bins_max and min_rows >= 1")
    eps = 1.0 + 1e-12  # a period given as bins x sample_time lands on its own step
    d = max(1, int(math.floor(period_min / (bins_min * sample_time) * eps)))
    plan = []
    while bins_min * d * sample_time <= period_max * eps:
        dn = max(d + 1, (d * bins_max) // bins_min)
        p_stop = -((-bins_min * dn) // d)
        if p_stop - 1 > MAX_BINS:
            raise ValueError(f"ffa_plan: downsampling factor {d} needs base periods up to {p_stop - 1} bins, above the "
                             f"kernel's limit of {MAX_BINS}: lower bins_min")
        p_stop = min(p_stop, (n // d) // min_rows + 1)
        if p_stop > bins_min:
            plan.append((d, bins_min, p_stop))
        d = dn
    return plan


def describe(rows, m, p, nwidths=0, want_out=True):
    """pu_ffa_describe: the level split and workspace of a ``pu_ffa`` call, on the host alone - a
    dict of ``DESCRIBE_FIELDS``.  ``block_rows`` is the rows ``B`` of an LDS block at this ``p``."""
    info = np.zeros(len(DESCRIBE_FIELDS), np.int64)
    _hip.check(_hip.lib().pu_ffa_describe(int(rows), int(m), int(p), int(nwidths), int(bool(want_out)),
                                          info.ctypes.data_as(ctypes.c_void_p), info.size), "pu_ffa_describe")
    return dict(zip(DESCRIBE_FIELDS, info.tolist()))


# ------------------------------------------------------------------ the device stages

def _series(series, what):
    """(float32 2-D device tensor, the input was 1-D, the input was numpy)."""
    t = _hip.require_gpu()
    x, one_d, as_numpy = _hip.as_rows(series, f"{what}: series must be (rows, nsamples) or 1-D", (_hip.PU_F32, _hip.PU_F64))
    if x.dtype != t.float32:
        x = x.to(t.float32)
    return x, one_d, as_numpy


def _widths(widths, p):
    w = default_widths(p) if widths is None else np.ascontiguousarray(np.atleast_1d(widths), dtype=np.int32)
    if w.ndim != 1 or not 1 <= w.size <= MAX_WIDTHS or w.min() < 1 or w.max() >= p:
        raise ValueError(f"widths: 1 to {MAX_WIDTHS} integers in 1 .. p - 1 = {p - 1}")
    return w


def _rows_per_call(rows, m, p, nwidths, want_out):
    def ws(r):
        return describe(r, m, p, nwidths, want_out)["workspace_bytes"]
    per_row = ws(2) - ws(1)  # 0: the transform alone with every level in LDS, which no workspace limits
    return max(1, min(rows, _MAX_ROWS_M // m, _WS_BYTES // per_row if per_row else rows))


def _ffa_device(x, p, want_out, widths=None, sigma=None, want_peak=True):
    """pu_ffa of a 2-D row-major float32 device tensor: ``(out or None, snr or None, peak or
    None)``, ``m = n // p``; ``widths``: host int32 array or None (no S/N); ``sigma``: float64 device
    tensor (rows,) or None."""
    t = _hip.torch()
    lib = _hip.lib()
    rows, n = x.shape
    p = int(p)
    if p < 2 or p > MAX_BINS:
        raise ValueError(f"p must be in 2 .. {MAX_BINS}, got {p}")
    m = n // p
    if m < 1:
        raise ValueError(f"a series of {n} samples has no row of {p} bins")
    nw = 0 if widths is None else int(widths.size)
    out = t.empty((rows, m, p), dtype=t.float32, device=x.device) if want_out else None
    snr = t.empty((rows, m, nw), dtype=t.float32, device=x.device) if nw else None
    peak = t.empty((rows, m, nw), dtype=t.int32, device=x.device) if nw and want_peak else None
    if rows == 0:
        return out, snr, peak
    per = _rows_per_call(rows, m, p, nw, want_out)
    buf, wp, wsb = _hip.workspace(describe(per, m, p, nw, want_out)["workspace_bytes"], x.device)
    wptr = widths.ctypes.data_as(ctypes.c_void_p) if nw else None
    for r0 in range(0, rows, per):
        k = min(per, rows - r0)
        _hip.check(lib.pu_ffa(_hip.ptr(x[r0:]), k, _hip.row_stride(x), m, p, _hip.ptr(out[r0:]) if want_out else None, m * p,
                              wptr, nw, _hip.ptr(sigma[r0:]) if sigma is not None else None,
                              _hip.ptr(snr[r0:]) if nw else None, _hip.ptr(peak[r0:]) if peak is not None else None, wp,
                              wsb, _hip.stream_ptr()), "pu_ffa")
    return out, snr, peak


def _sigma_device(sigma, rows, device):
    if sigma is None:
        return None
    t = _hip.torch()
    s = sigma if isinstance(sigma, t.Tensor) else t.from_numpy(np.ascontiguousarray(np.atleast_1d(sigma), dtype=np.float64))
    s = s.to(device=device, dtype=t.float64).reshape(-1).contiguous()
    if s.numel() == 1 and rows != 1:
        s = s.expand(rows).contiguous()
    if s.numel() != rows:
        raise ValueError(f"sigma: one value per row ({rows}), got {s.numel()}")
    return s


def ffa_transform(series, p):
    """The transform of each row's first ``m p`` samples, ``m = n // p``: float32 ``(rows, m, p)``
    (``(m, p)`` for a 1-D series); row ``s`` is the fold at :func:`trial_periods` ``(p, m)[s]``."""
    x, one_d, as_numpy = _series(series, "ffa_transform")
    out, _, _ = _ffa_device(x, p, True)
    if one_d:
        out = out[0]
    return out.cpu().numpy() if as_numpy else out


def ffa_snr(series, p, widths=None, sigma=None):
    """``(snr, peak)`` of every trial period and width: float32 and int32 ``(rows, m, nwidths)``
    (``(m, nwidths)`` for a 1-D series).  ``widths``: bins, default :func:`default_widths`;
    ``sigma``: the rows' noise per sample (one value per row, or one for all; default 1).  Only the
    S/N leaves the device's kernels: the top level of the tree is formed where it is scored."""
    x, one_d, as_numpy = _series(series, "ffa_snr")
    w = _widths(widths, int(p))
    _, snr, peak = _ffa_device(x, p, False, w, _sigma_device(sigma, x.shape[0], x.device))
    if one_d:
        snr, peak = snr[0], peak[0]
    return (snr.cpu().numpy(), peak.cpu().numpy()) if as_numpy else (snr, peak)


def _downsampled(x64, d):
    """(float32 rows of n // d samples: d samples summed in float64, minus the row's mean;
    float64 per-row standard deviation, inf for a constant row: its S/N is 0)."""
    from .dedispersion import _rebin_time_device
    t = _hip.torch()
    y = x64 if d == 1 else _rebin_time_device(x64, d)
    y = y - y.mean(dim=1, keepdim=True)
    sd = y.std(dim=1, unbiased=False)
    sd = t.where(sd > 0, sd, t.full_like(sd, math.inf))
    return y.to(t.float32), sd


def _detrended(what, x64, sample_time, detrend_width, detrend_min_points):
    """``x64`` (float64 rows, a copy this module owns) minus its running-median baseline of
    ``detrend_width`` seconds, in place; untouched for ``None``."""
    if detrend_width is None:
        return x64
    from .detrend import _detrend_device
    width = float(detrend_width)
    if not width > 0:
        raise ValueError(f"{what}: detrend_width must be positive seconds or None")
    return _detrend_device(x64, max(1, int(np.rint(width / sample_time))), detrend_min_points, in_place=True)


def _plan_steps(what, x, sample_time, period_min, period_max, bins_min, bins_max, min_rows):
    plan = ffa_plan(x.shape[1], sample_time, period_min, period_max, bins_min, bins_max, min_rows)
    if not plan:
        raise ValueError(f"{what}: no base period between {period_min} and {period_max} s leaves {min_rows} rows of "
                         f"{x.shape[1]} samples")
    return plan


def _best_widths(z, sd, p, widths):
    """One step of a search on the device, from :func:`_downsampled`'s rows: (best S/N over the
    widths, its index, its peak), each (rows, m') with the duplicate last trial dropped (m' = m - 1;
    m for m = 1), and the widths."""
    w = _widths(widths, p)
    _, snr, peak = _ffa_device(z, p, False, w, sd)
    if snr.shape[1] > 1:
        snr, peak = snr[:, :-1], peak[:, :-1]
    best, k = snr.max(dim=2)
    return best, k, peak.gather(2, k.unsqueeze(2)).squeeze(2), w


def ffa_periodogram(series, sample_time, period_min, period_max, bins_min=240, bins_max=260, min_rows=8, widths=None,
                    detrend_width=None, detrend_min_points=101):
    """The S/N of one series (or a few rows) at every trial period of :func:`ffa_plan`.  Per step
    ``(d, p)`` the rows are downsampled by ``d``, normalised by their mean and standard deviation
    and scored by :func:`ffa_snr` at ``widths`` (default :func:`default_widths` ``(p)``); the last
    trial of each base period is dropped (it is the first of the next).  ``detrend_width``
    (seconds; None: none) subtracts a running-median baseline of that width first
    (``detrend.detrend`` at ``max(1, rint(detrend_width / sample_time))`` samples and
    ``detrend_min_points``).  Returns a dict: ``period``
    (s, ``(ntrials,)``, ascending within a step), ``snr`` (best over the widths, float32
    ``(rows, ntrials)`` or ``(ntrials,)``), ``width`` (s, of that best, the shape of ``snr``) and
    ``dsfactor`` (int64 ``(ntrials,)``)."""
    t = _hip.torch()
    x, one_d, as_numpy = _series(series, "ffa_periodogram")
    sample_time = float(sample_time)
    plan = _plan_steps("ffa_periodogram", x, sample_time, period_min, period_max, bins_min, bins_max, min_rows)
    x64 = _detrended("ffa_periodogram", x.to(t.float64), sample_time, detrend_width, detrend_min_points)
    periods, snrs, wids, dsf = [], [], [], []
    for d, p0, p1 in plan:
        z, sd = _downsampled(x64, d)
        for p in range(p0, p1):
            best, k, _, w = _best_widths(z, sd, p, widths)
            m = (x.shape[1] // d) // p
            per = trial_periods(p, m, d * sample_time)
            periods.append(per[:-1] if m > 1 else per)
            snrs.append(best)
            wids.append(t.from_numpy(w.astype(np.float64) * d * sample_time).to(x.device)[k])
            dsf.append(np.full(best.shape[1], d, np.int64))
    snr, wid = t.cat(snrs, dim=1), t.cat(wids, dim=1)
    if one_d:
        snr, wid = snr[0], wid[0]
    if as_numpy:
        snr, wid = snr.cpu().numpy(), wid.cpu().numpy()
    return {"period": np.concatenate(periods), "snr": snr, "width": wid, "dsfactor": np.concatenate(dsf)}


def ffa_search(series, sample_time, period_min, period_max, sigma=7.0, bins_min=240, bins_max=260, min_rows=8,
               widths=None, sift=True, detrend_width=None, detrend_min_points=101):
    """Search a plane ``(ndm, n)`` (or one series) for pulses of periods ``period_min ..
    period_max`` seconds with the FFA.

    Per step ``(d, p)`` of :func:`ffa_plan` every row is downsampled, normalised and scored as in
    :func:`ffa_periodogram`; on the device a trial is kept when its best S/N over the widths is
    above ``sigma``, above its left neighbour among the step's trials and not below its right one,
    and only those leave the device.  ``detrend_width`` (seconds; None: none) subtracts a
    running-median baseline of that width from every row first, as in :func:`ffa_periodogram`; it
    must be many pulse widths.

    Returns a table, strongest first: ``period`` (s), ``freq`` (Hz), ``row``, ``snr``, ``width``
    (s, of the best boxcar), ``peak_phase`` (the phase in [0, 1) of the boxcar's centre, phase 0
    at the series' first sample), ``dsfactor`` and ``nabsorbed``.  ``sift=True`` passes the list
    through ``periodicity.sift_candidates`` (``logp := -snr``, ``tobs = n sample_time``), which
    absorbs a signal's harmonics, sub-harmonics and its detections at neighbouring steps and
    rows; otherwise ``nabsorbed`` is 0."""
    from .periodicity import sift_candidates
    from .table import make_table
    t = _hip.torch()
    x, _, _ = _series(series, "ffa_search")
    sample_time, thr = float(sample_time), float(sigma)
    n = x.shape[1]
    plan = _plan_steps("ffa_search", x, sample_time, period_min, period_max, bins_min, bins_max, min_rows)
    x64 = _detrended("ffa_search", x.to(t.float64), sample_time, detrend_width, detrend_min_points)
    cols = {c: [] for c in ("period", "row", "snr", "width", "peak_phase", "dsfactor")}
    for d, p0, p1 in plan:
        z, sd = _downsampled(x64, d)
        for p in range(p0, p1):
            best, k, peak, w = _best_widths(z, sd, p, widths)
            edge = t.full_like(best[:, :1], -math.inf)
            keep = (best > thr) & (best > t.cat((edge, best[:, :-1]), dim=1)) & (best >= t.cat((best[:, 1:], edge), dim=1))
            idx = keep.nonzero()
            if idx.shape[0] == 0:
                continue
            r, s = idx[:, 0], idx[:, 1]
            r_h, s_h = r.cpu().numpy(), s.cpu().numpy()
            k_h = k[r, s].cpu().numpy()
            m = (n // d) // p
            cols["period"].append(trial_periods(p, m, d * sample_time)[s_h])
            cols["row"].append(r_h.astype(np.int64))
            cols["snr"].append(best[r, s].cpu().numpy().astype(np.float64))
            cols["width"].append(w[k_h].astype(np.float64) * d * sample_time)
            cols["peak_phase"].append(((peak[r, s].cpu().numpy() + 0.5 * w[k_h]) / p) % 1.0)
            cols["dsfactor"].append(np.full(r_h.size, d, np.int64))
    empty = {"period": np.float64, "row": np.int64, "snr": np.float64, "width": np.float64, "peak_phase": np.float64,
             "dsfactor": np.int64}
    cols = {c: np.concatenate(v) if v else np.zeros(0, empty[c]) for c, v in cols.items()}
    cols["freq"] = 1.0 / cols["period"]
    if sift:
        cols["logp"] = -cols["snr"]
        cols = sift_candidates(cols, n * sample_time)
        del cols["logp"]
    else:
        order = np.argsort(-cols["snr"], kind="stable")
        cols = {c: v[order] for c, v in cols.items()}
        cols["nabsorbed"] = np.zeros(order.size, np.int64)
    names = ("period", "freq", "row", "snr", "width", "peak_phase", "dsfactor", "nabsorbed")
    return make_table({c: cols[c] for c in names})


__all__ = ["ffa_tables", "trial_periods", "default_widths", "ffa_plan", "describe", "ffa_transform", "ffa_snr",
           "ffa_periodogram", "ffa_search"]
