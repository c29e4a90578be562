"""Host restatement of the folding and Z^2_n / H definitions (include/pulsarutils_hip.h, pu_fold
and pu_h_test; pulsarutils/folding.py): the bin rule, the fold as ``np.add.at`` per channel
(``math.fsum`` per bin for float input), and Z^2 / H with ``math.fsum`` for every sum and
exact-integer phases.

Test infrastructure only.  Nothing here imports ``pulsarutils.folding`` (the code under test).
tests/test_fold_oracle.py pins these functions against facts."""
import math

import numpy as np


def bins(nsamples, dphase, nbin, phase0=0.0, first_sample=0, return_frac=False):
    """b(t) for t = 0 .. nsamples - 1: three float64 steps, each rounded once."""
    idx = np.arange(first_sample, first_sample + nsamples, dtype=np.int64).astype(np.float64)
    prod = idx * np.float64(dphase)
    p = np.float64(phase0) + prod
    f = p - np.floor(p)
    b = np.minimum((f * np.float64(nbin)).astype(np.int64), nbin - 1)
    return (b, f) if return_frac else b


def fold_exact(x, dphase, nbin, phase0=0.0, first_sample=0):
    """Fold of integer-valued ``x`` (nchan, n): ``np.add.at`` per channel in int64 -> (float64
    sums, int64 counts).  Exact while the sums stay below 2^53."""
    x = np.atleast_2d(np.asarray(x))
    b = bins(x.shape[1], dphase, nbin, phase0, first_sample)
    sums = np.zeros((x.shape[0], nbin), np.int64)
    for c in range(x.shape[0]):
        np.add.at(sums[c], b, x[c].astype(np.int64))
    counts = np.zeros(nbin, np.int64)
    np.add.at(counts, b, 1)
    return sums.astype(np.float64), counts


def fold_fsum(x, dphase, nbin, phase0=0.0, first_sample=0):
    """Fold of float ``x`` (nchan, n) with every bin's sum exactly rounded (``math.fsum``) ->
    (sums, counts, abs_sums): ``abs_sums[c, b]`` = the fsum of ``|x|`` over the bin."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    b = bins(x.shape[1], dphase, nbin, phase0, first_sample)
    order = np.argsort(b, kind="stable")
    sb = b[order]
    starts = np.searchsorted(sb, np.arange(nbin), side="left")
    ends = np.searchsorted(sb, np.arange(nbin), side="right")
    sums = np.zeros((x.shape[0], nbin))
    abs_sums = np.zeros((x.shape[0], nbin))
    for c in range(x.shape[0]):
        row = x[c][order]
        for k in range(nbin):
            if ends[k] > starts[k]:
                seg = row[starts[k]:ends[k]]
                sums[c, k] = math.fsum(seg)
                abs_sums[c, k] = math.fsum(np.abs(seg))
    return sums, (ends - starts).astype(np.int64), abs_sums


def z2_all(p, nmax):
    """``Z^2_1 .. Z^2_nmax`` of one profile (list of floats): NaN when the profile holds a
    non-finite value or its sum is not > 0."""
    p = [float(v) for v in np.asarray(p).ravel()]
    n = len(p)
    if not all(math.isfinite(v) for v in p):
        return [math.nan] * nmax
    tot = math.fsum(p)
    if not tot > 0:
        return [math.nan] * nmax
    powers = []
    for k in range(1, nmax + 1):
        ck = math.fsum(p[j] * math.cos(2.0 * math.pi * ((k * j) % n) / n) for j in range(n))
        sk = math.fsum(p[j] * math.sin(2.0 * math.pi * ((k * j) % n) / n) for j in range(n))
        powers.append(ck * ck + sk * sk)
    return [2.0 / tot * math.fsum(powers[:m]) for m in range(1, nmax + 1)]


def z2_all_fast(p, nmax):
    """``z2_all`` for long profiles: the same exact-integer phases and fsum for the sum over
    bins (numpy products, ``math.fsum`` of each product vector), seconds instead of minutes."""
    p = np.asarray(p, dtype=np.float64).ravel()
    n = p.size
    if not np.isfinite(p).all():
        return [math.nan] * nmax
    tot = math.fsum(p)
    if not tot > 0:
        return [math.nan] * nmax
    j = np.arange(n, dtype=np.int64)
    tab_c = np.array([math.cos(2.0 * math.pi * r / n) for r in range(n)])
    tab_s = np.array([math.sin(2.0 * math.pi * r / n) for r in range(n)])
    # harmonic n - k reads the table mirrored (cos the same, sin negated): C_{n-k} = C_k and
    # S_{n-k} = -S_k, so its power is harmonic k's and only k <= n / 2 is summed
    powers = []
    for k in range(1, nmax + 1):
        if 2 * k > n:
            powers.append(powers[n - k - 1])
            continue
        r = (k * j) % n
        ck = math.fsum((p * tab_c[r]).tolist())
        sk = math.fsum((p * tab_s[r]).tolist())
        powers.append(ck * ck + sk * sk)
    cum, out = [], []
    for m in range(nmax):
        cum.append(powers[m])
        out.append(2.0 / tot * math.fsum(cum))
    return out


def h_from_z2(zs):
    """(H, M, the list of H_m) from ``Z^2_1 ..``: H_m = Z^2_m - 4 m + 4, M the first maximum;
    (NaN, 0, []) for a NaN profile."""
    if any(math.isnan(z) for z in zs):
        return math.nan, 0, []
    hm = [z - 4.0 * m + 4.0 for m, z in enumerate(zs, start=1)]
    best = max(hm)
    return best, hm.index(best) + 1, hm


def z2_tolerance(n, m, tot):
    """The bound on ``|Z^2_m(device) - Z^2_m(oracle)|``: each of C_k, S_k is an n-term dot
    product bounded by P with error <= (n + 2) 2^-53 P; squared, scaled by 2 / P and summed
    over k <= m that is 8 m (n + 2) 2^-53 P, doubled for the oracle's own error."""
    return 16.0 * m * (n + 2) * 2.0 ** -53 * tot
