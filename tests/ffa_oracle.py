"""The fast folding transform and its S/N, restated in numpy from the definition alone
(include/pulsarutils_hip.h, "fast folding"): the recursion, not the level tables the kernels walk.

``rdiv(a, b) = (2a + b) // (2b)``.  ``F(x) = x`` for one row; otherwise ``nh = m // 2``, ``nt = m -
nh``, ``H = F(x[:nh])``, ``T = F(x[nh:])`` and for ``s = 0 .. m - 1``

    h = rdiv(s (nh - 1), m - 1),  t = rdiv(s (nt - 1), m - 1),  b = s - t
    F[s][j] = H[h][j] + T[t][(j + b) % p]

in float32, head operand on the left.  S/N of a profile ``v`` at width ``w``: ``(B_w - w T / p) /
(sqrt(m w (1 - w / p)) sigma)``, ``T = sum v``, ``B_w`` the largest circular window sum, ``peak`` the
lowest bin attaining it.
"""
import math

import numpy as np


def rdiv(a, b):
    return (2 * a + b) // (2 * b)


def merge_indices(m):
    """(h, t, b) of the top merge of m >= 2 rows, int64 arrays of m."""
    nh = m // 2
    nt = m - nh
    s = np.arange(m, dtype=np.int64)
    h, t = rdiv(s * (nh - 1), m - 1), rdiv(s * (nt - 1), m - 1)
    return h, t, s - t


def ffa(x):
    """F(x) of a float32 (m, p) array, by the recursion."""
    x = np.asarray(x, dtype=np.float32)
    m, p = x.shape
    if m == 1:
        return x.copy()
    nh = m // 2
    head, tail = ffa(x[:nh]), ffa(x[nh:])
    h, t, b = merge_indices(m)
    cols = (np.arange(p, dtype=np.int64)[None, :] + b[:, None]) % p
    return head[h] + tail[t[:, None], cols]  # float32 + float32: one rounding


def ffa_series(series, p):
    """F of the first (n // p) p samples of a 1-D series."""
    series = np.asarray(series, dtype=np.float32)
    m = series.size // p
    return ffa(series[:m * p].reshape(m, p))


def apply_tables(x, tables):
    """The transform by level tables (pulsarutils.ffa.ffa_tables' layout), bottom level first."""
    cur = np.asarray(x, dtype=np.float32).copy()
    p = cur.shape[1]
    j = np.arange(p, dtype=np.int64)
    for head, tail, rot in tables:
        cols = (j[None, :] + rot[:, None]) % p
        summed = cur[head] + cur[np.maximum(tail, 0)[:, None], cols]
        cur = np.where((tail < 0)[:, None], cur[head], summed)
    return cur


def shifts(m):
    """The shift the tree gives input row i in trial s: int64 (m, m), [s, i]."""
    if m == 1:
        return np.zeros((1, 1), np.int64)
    nh = m // 2
    sh, st = shifts(nh), shifts(m - nh)
    h, t, b = merge_indices(m)
    return np.concatenate((sh[h], st[t] + b[:, None]), axis=1)


def brute_fold(x, shift):
    """out[s][j] = sum_i x[i][(j + shift[s, i]) % p], float64 in row order."""
    x = np.asarray(x, dtype=np.float64)
    m, p = x.shape
    j = np.arange(p, dtype=np.int64)
    out = np.zeros((shift.shape[0], p))
    for i in range(m):
        out += x[i][(j[None, :] + shift[:, i:i + 1]) % p]
    return out


def window_sums(v, w):
    """The p circular window sums of width w of profile v, each correctly rounded to float64
    (exact integers for integer-valued v; math.fsum otherwise)."""
    v = np.asarray(v)
    p = v.size
    if np.all(v == np.rint(v)) and np.abs(v).sum() < 2.0 ** 52:
        c = np.concatenate(([0], np.cumsum(np.concatenate((v, v)).astype(np.int64))))
        return (c[w:w + p] - c[:p]).astype(np.float64)
    vv = [float(a) for a in v] * 2
    return np.array([math.fsum(vv[b:b + w]) for b in range(p)])


def snr_exact(v, w, m, sigma=1.0):
    """(snr as float64, peak, the window sums) of profile v at width w, sums exact."""
    v = np.asarray(v)
    p = v.size
    sums = window_sums(v, w)
    total = math.fsum(float(a) for a in v)
    peak = int(np.argmax(sums))  # the first maximum
    snr = (sums[peak] - w * total / p) / (math.sqrt(m * w * (1.0 - w / p)) * sigma)
    return snr, peak, sums


def snr_table(F, widths, sigma=1.0):
    """(snr, peak) of every row of F at every width, (m, nwidths), by float64 prefix sums: for
    detection tests, not for exactness."""
    F = np.asarray(F, dtype=np.float64)
    m, p = F.shape
    c = np.concatenate((np.zeros((m, 1)), np.cumsum(np.concatenate((F, F), axis=1), axis=1)), axis=1)
    total = F.sum(axis=1)
    snr, peak = np.zeros((m, len(widths))), np.zeros((m, len(widths)), np.int64)
    for k, w in enumerate(widths):
        w = int(w)
        sums = c[:, w:w + p] - c[:, :p]
        peak[:, k] = np.argmax(sums, axis=1)
        snr[:, k] = (sums.max(axis=1) - w * total / p) / (math.sqrt(m * w * (1.0 - w / p)) * sigma)
    return snr, peak


def pulsar_series(n, period, duty, amplitude, seed, phase0=0.0):
    """Unit Gaussian noise plus a top-hat pulse of ``amplitude`` wherever the phase (t / period +
    phase0) mod 1 is below ``duty``; float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    on = ((t / period + phase0) % 1.0) < duty
    return (rng.standard_normal(n) + amplitude * on).astype(np.float32)
