"""Host restatement of the pulse-frequency search (include/pulsarutils_hip.h, pu_fold_trials and
pu_profile_chi2; pulsarutils/folding.py fold_trials / frequency_search): the fold of
tests/fold_oracle.py one trial at a time, the NaN rule of a trial whose phase cannot be binned,
and the epoch-folding chi^2 with ``math.fsum``.

Test infrastructure only.  Nothing here imports ``pulsarutils.folding`` (the code under test).
tests/test_period_oracle.py pins these functions against facts."""
import math

import numpy as np

import fold_oracle as fo

U = 2.0 ** -53


def trial_is_bad(n, dphase, phase0=0.0, first_sample=0):
    """The trials the device masks: a non-finite phase0 / dphase, or |p| >= 2^52 at either end of
    the chunk (p in the float64 steps of the bin rule)."""
    with np.errstate(all="ignore"):
        dp, p0 = np.float64(dphase), np.float64(phase0)
        pa = p0 + np.float64(first_sample) * dp
        pb = p0 + np.float64(first_sample + max(n - 1, 0)) * dp
        return not (np.isfinite(dp) and np.isfinite(p0) and abs(pa) < 2.0 ** 52 and abs(pb) < 2.0 ** 52)


def fold_trials(x, dphases, nbin, phase0s=None, first_sample=0, exact=False):
    """Fold of ``x`` (rows, n) at every trial -> (sums (rows, F, nbin), counts (F, nbin), abs_sums
    or None): ``fold_oracle.fold_exact`` per trial (integer-valued ``x``, ``exact=True``) or
    ``fold_oracle.fold_fsum``.  A bad trial has NaN sums and zero counts."""
    x = np.atleast_2d(np.asarray(x))
    dphases = np.atleast_1d(np.asarray(dphases, dtype=np.float64))
    phase0s = np.zeros_like(dphases) if phase0s is None else np.broadcast_to(np.asarray(phase0s, np.float64), dphases.shape)
    rows, n = x.shape
    sums = np.zeros((rows, dphases.size, nbin))
    counts = np.zeros((dphases.size, nbin), np.int64)
    abs_sums = None if exact else np.zeros((rows, dphases.size, nbin))
    done = {}
    for k, (dp, p0) in enumerate(zip(dphases.tolist(), phase0s.tolist())):
        if trial_is_bad(n, dp, p0, first_sample):
            sums[:, k] = np.nan
            continue
        if (dp, p0) not in done:
            done[(dp, p0)] = (fo.fold_exact if exact else fo.fold_fsum)(x, dp, nbin, p0, first_sample)
        res = done[(dp, p0)]
        sums[:, k], counts[k] = res[0], res[1]
        if not exact:
            abs_sums[:, k] = res[2]
    return sums, counts, abs_sums


def chi2(sums, counts, mean, var):
    """(chi2, dof) of one profile (``sums``, ``counts``: (nbin,)): the sum over the bins with
    counts > 0 of (s - c mean)^2 / (c var) by ``math.fsum``; dof = those bins - 1.  NaN when
    ``var`` is not > 0 or a sum of any bin, empty ones included, is not finite."""
    s = [float(v) for v in np.asarray(sums).ravel()]
    c = [int(v) for v in np.asarray(counts).ravel()]
    hit = [b for b in range(len(c)) if c[b] > 0]
    dof = len(hit) - 1
    if not float(var) > 0 or not all(math.isfinite(v) for v in s):
        return math.nan, dof
    return math.fsum((s[b] - c[b] * float(mean)) ** 2 / (c[b] * float(var)) for b in hit), dof


def chi2_all(sums, counts, mean, var):
    """``chi2`` of every (row, trial) of ``sums`` (rows, F, nbin) -> (chi2 (rows, F), dof (F,))."""
    sums = np.asarray(sums)
    rows, nf, _ = sums.shape
    out = np.zeros((rows, nf))
    dof = np.zeros(nf, np.int32)
    for k in range(nf):
        for r in range(rows):
            out[r, k], dof[k] = chi2(sums[r, k], counts[k], mean[r], var[r])
    return out, dof


def chi2_tolerance(nbin, sums, counts, mean, var, sums_err=None):
    """The bound on ``|chi2(device) - chi2(oracle)|`` for one profile, from the operation count.

    With u = 2^-53, a term is T = d^2 / (c var), d = s - c mean.  The device rounds c mean
    (error <= u |c mean|) and the subtraction (<= u |d|), so its d is off by at most
    e_d = u (|c mean| + |d|) + e_s, where e_s is what the device's s may differ from the oracle's
    by (``sums_err``; 0 when both read the same sums).  Squaring, the product c var and the
    division each add one relative rounding: |T' - T| <= (2 |d| e_d + e_d^2) / (c var) + 3 u T
    to first order; we allow 4 u T for the second-order terms.  The sequential sum of at most
    nbin non-negative terms adds at most (nbin - 1) u sum T.  The oracle's own terms carry the
    same e_d and 3 u T (its fsum is exact to one rounding, u sum T), so the term part is
    doubled: tol = sum_b [2 (2 |d| e_d + e_d^2) / (c var) + 8 u T] + (nbin + 1) u sum T."""
    s = np.asarray(sums, dtype=np.float64)
    c = np.asarray(counts, dtype=np.float64)
    hit = c > 0
    s, c = s[hit], c[hit]
    es = np.zeros_like(s) if sums_err is None else np.asarray(sums_err, dtype=np.float64)[hit]
    d = np.abs(s - c * mean)
    ed = U * (np.abs(c * mean) + d) + es
    term = d * d / (c * var)
    return float(np.sum(2.0 * (2.0 * d * ed + ed * ed) / (c * var) + 8.0 * U * term) + (nbin + 1) * U * np.sum(term))
