"""Blind periodicity search in the Fourier domain: spectrum, harmonic sums, candidates.

``folding.frequency_search`` gives every trial frequency its own pass over the series; a blind
search takes one FFT per dedispersed series instead, takes out the red noise, sums the
harmonics so that narrow pulses are not lost, and keeps the significant peaks.  Epoch folding is
then the refinement around a few candidates.  The reference has no counterpart.

**Definitions** (include/pulsarutils_hip.h has them in full; tests/spectrum_oracle.py restates
the float32 stages in numpy, bit for bit).

``rfft`` (``pu_rfft``): ``y[t] = float32(float64(x[t]) - mean)`` for ``t < n``, 0 up to ``nfft``
(a power of two, 2^8 .. 2^24); ``spec[k] = sum_t y[t] exp(-2 pi i k t / nfft)``, ``k = 0 ..
nfft / 2``, complex64, by a hand-written float32 FFT whose bits depend on the row's samples alone.

``power_spectrum`` (``pu_spectrum_normalize``): ``P[k] = re re + im im`` for the ``nb = nfft / 2``
bins below Nyquist; every block of ``block`` bins is divided by its median / ln 2 (block 0 leaves
the DC bin out), so noise has mean about 1 and each bin is about Exp(1); bin 0 is 0.

``harmonic_sums`` (``pu_harmonic_search``): level ``l`` sums ``H = 2^l`` harmonics, indexed by the
bin ``k`` of the TOP harmonic: ``S_0[k] = N[k]``, ``S_(l+1)[k] = S_l[k] + sum_(odd m < 2H)
N[(k m + H) // (2H)]``.  The fundamental of ``S_l[k]`` is at ``k / 2^l`` bins, i.e. the frequency
resolution of a level-``l`` candidate is ``1 / (2^l T)``: summing from the top keeps the resolution
the highest harmonic has (a fundamental-based index would smear it over ``H`` bins).  A bin is a
candidate of its level when its sum is above the level's threshold, above its left neighbour and
not below its right one.  Under noise ``S_l`` is Erlang(``H``) distributed: :func:`erlang_logsf`.

Acceleration trials (``pu_resample_accel``, ``pu_rfft_accel``): a pulsar in a binary drifts across
Fourier bins; resampling the series in time at its line-of-sight acceleration ``a`` makes it
periodic again.  With ``af = a sample_time / (2 c)``, output sample ``i`` of ``n`` is input sample
``i + rint(af i (i - n))`` (nearest neighbour, clamped into the row: :func:`resample_indices`).
:func:`acceleration_search` runs the chain above over (acceleration, row) pairs, the index map
applied where the FFT's first pass loads its samples.  A constant acceleration only.

Conventions are ``folding``'s: numpy in -> numpy out, CUDA tensor in -> tensors out, a 1-D array
is one row.  Importable without a GPU: :func:`next_nfft`, :func:`harmonic_bins`,
:func:`erlang_logsf`, :func:`power_threshold`, :func:`sigma_from_logp`, :func:`logp_from_sigma`,
:func:`bin_ranges`, :func:`sift_candidates`, :func:`accel_factor`, :func:`resample_indices` and
:func:`acceleration_grid` are pure numpy; the rest runs HIP kernels and
raises ``HipBackendError`` without the library or a GPU.
"""
import ctypes
import functools
import math

import numpy as np

from . import _hip

NHARMS = (1, 2, 4, 8, 16, 32)
MIN_NFFT, MAX_NFFT = 1 << 8, 1 << 24
_FFT_WS_BYTES = 1 << 30  # pu_rfft's workspace per call (its rows; the twiddle table on top): more rows go in batches
_MAX_ROWS = 32768        # rows of one call (a launch's grid.y)


def next_nfft(n, pad=1):
    """The transform length for ``n`` samples: the smallest power of two ``>= n * pad``, at least
    2^8.  ``ValueError`` above 2^24."""
    n, pad = int(n), int(pad)
    if n < 1 or pad < 1:
        raise ValueError("next_nfft: n and pad must be positive")
    nfft = MIN_NFFT
    while nfft < n * pad:
        nfft *= 2
    if nfft > MAX_NFFT:
        raise ValueError(f"next_nfft: {n} samples x pad {pad} need more than 2^24 points")
    return nfft


def _nlev(nharm):
    if nharm not in NHARMS:
        raise ValueError(f"nharm must be one of {NHARMS}, got {nharm!r}")
    return NHARMS.index(nharm) + 1


def harmonic_bins(k, level):
    """The bins ``S_level[k]`` adds, in the order it adds them: ``k`` itself, then for ``l = 0 ..
    level - 1`` and odd ``m = 1, 3 .. 2^(l+1) - 1`` the bin ``(k m + 2^l) // 2^(l+1)``.  int64,
    shape ``k.shape + (2^level,)``."""
    level = int(level)
    if not 0 <= level <= 5:
        raise ValueError("harmonic_bins: level must be in 0 .. 5")
    k = np.asarray(k, dtype=np.int64)
    cols = [k]
    for lv in range(level):
        h = 1 << lv
        for m in range(1, 2 * h, 2):
            cols.append((k * m + h) // (2 * h))
    return np.stack(cols, axis=-1)


def erlang_logsf(s, nharm):
    """``log P(S > s)`` of the sum ``S`` of ``nharm`` Exp(1) powers: ``log(e^-s sum_(j < nharm)
    s^j / j!)``, evaluated in log space (no underflow for large ``s``).  Below the mean (``s <
    nharm``), where the tail probability is near 1, it is ``log1p(-e^-s sum_(j >= nharm) s^j /
    j!)`` instead, so small ``|log P|`` keep their relative accuracy.  float64, ``s >= 0``."""
    nharm = int(nharm)
    if nharm < 1:
        raise ValueError("erlang_logsf: nharm must be >= 1")
    s = np.asarray(s, dtype=np.float64)
    if nharm == 1:
        return -s

    def log_series(j0, j1):
        """log(e^-s sum_(j0 <= j < j1) s^j / j!) per element of s."""
        j = np.arange(j0, j1, dtype=np.float64)
        lg = np.array([math.lgamma(i + 1.0) for i in range(j0, j1)])
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = j * np.log(s)[..., None] - lg
            terms = np.where((s[..., None] == 0) & (j == 0), 0.0, terms)  # 0 log 0 = 0
            top = terms.max(axis=-1)
            return -s + top + np.log(np.exp(terms - top[..., None]).sum(axis=-1))

    upper = log_series(0, nharm)
    # s < nharm: the terms of the complement fall by at least s / j < 1 per step from j = nharm on;
    # 256 of them leave less than 2^-53 of the first for any nharm <= 32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lower = np.log1p(-np.exp(log_series(nharm, nharm + 256)))
    return np.where(s < nharm, np.where(s == 0, 0.0, lower), upper)


def power_threshold(logp, nharm):
    """The summed power ``s`` with ``erlang_logsf(s, nharm) == logp`` (``logp <= 0``), by
    bisection (remembered per ``(logp, nharm)``: a search asks for the same few every call)."""
    return _power_threshold(float(logp), int(nharm))


@functools.lru_cache(maxsize=256)
def _power_threshold(logp, nharm):
    if not logp <= 0:
        raise ValueError("power_threshold: logp must be <= 0")
    lo, hi = 0.0, max(1.0, -2.0 * logp + 4.0 * nharm)
    while float(erlang_logsf(hi, nharm)) > logp:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(erlang_logsf(mid, nharm)) > logp:
            lo = mid
        else:
            hi = mid
        if hi - lo <= 1e-15 * hi:
            break
    return 0.5 * (lo + hi)


_ERFC_MAX_SIGMA = 37.0  # erfc(37 / sqrt 2) ~ 1e-299: beyond, the asymptotic series


def logp_from_sigma(sigma):
    """``log`` of the one-sided Gaussian tail probability beyond ``sigma``: ``log(erfc(sigma /
    sqrt 2) / 2)``, by the asymptotic series ``-sigma^2 / 2 - log(sigma sqrt(2 pi)) + log(1 -
    1/sigma^2 + 3/sigma^4 - 15/sigma^6)`` where ``erfc`` would underflow."""
    sigma = float(sigma)
    if sigma <= _ERFC_MAX_SIGMA:
        return math.log(0.5 * math.erfc(sigma / math.sqrt(2.0)))
    q = 1.0 / (sigma * sigma)
    return -0.5 * sigma * sigma - math.log(sigma * math.sqrt(2.0 * math.pi)) + math.log1p(-q + 3 * q * q - 15 * q ** 3)


def sigma_from_logp(logp):
    """The inverse of :func:`logp_from_sigma` (bisection), for ``logp < log(1/2)``; 0 at and
    above ``log(1/2)``."""
    logp = float(logp)
    if not logp < math.log(0.5):
        return 0.0
    lo, hi = 0.0, 2.0
    while logp_from_sigma(hi) > logp:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if logp_from_sigma(mid) > logp:
            lo = mid
        else:
            hi = mid
        if hi - lo <= 1e-15 * hi:
            break
    return 0.5 * (lo + hi)


def bin_ranges(fmin, fmax, nfft, sample_time, nlev, nb=None):
    """``(kmin, kmax)``, int64 arrays of ``nlev`` entries: the top-harmonic bins ``kmin[l] <= k <
    kmax[l]`` whose fundamental ``k / 2^l / (nfft sample_time)`` lies in ``[fmin, fmax]``.
    ``fmin=None``: from one bin of the fundamental (``k >= 2^l``); ``fmax=None``: up to ``nb``.
    Both ends are clipped to ``[0, nb]`` (``nb`` defaults to ``nfft // 2``)."""
    nfft, nlev = int(nfft), int(nlev)
    nb = nfft // 2 if nb is None else int(nb)
    tobs = nfft * float(sample_time)
    if not tobs > 0:
        raise ValueError("bin_ranges: nfft and sample_time must be positive")
    if fmin is not None and fmax is not None and not float(fmax) >= float(fmin):
        raise ValueError("bin_ranges: fmax < fmin")
    kmin, kmax = np.zeros(nlev, np.int64), np.zeros(nlev, np.int64)
    for lv in range(nlev):
        h = 1 << lv
        lo = h if fmin is None else int(math.ceil(float(fmin) * tobs * h))
        hi = nb if fmax is None else int(math.floor(float(fmax) * tobs * h)) + 1
        kmin[lv] = min(max(lo, 0), nb)
        kmax[lv] = min(max(hi, kmin[lv]), nb)
    return kmin, kmax


def sift_candidates(cands, tobs, max_ratio=16):
    """Keep one candidate per signal.  ``cands``: a mapping of equal-length columns with at least
    ``freq`` and ``logp`` (a table of :func:`periodicity_search`).  The candidates are taken by
    ``logp`` ascending (most significant first; ties in their given order); one whose frequency
    is within ``1.5 / tobs`` of ``j f`` or ``f / j`` (``1 <= j <= max_ratio``) of an already
    accepted candidate of frequency ``f``, in any row, is dropped and counted in that
    candidate's ``nabsorbed`` (the first such in acceptance order).  Returns a dict of numpy
    columns, the accepted candidates in acceptance order, with ``nabsorbed`` (int64) added."""
    names = [c for c in (cands.colnames if hasattr(cands, "colnames") else cands.keys()) if c != "nabsorbed"]
    cols = {c: np.asarray(cands[c]) for c in names}
    freq = np.asarray(cols["freq"], dtype=np.float64)
    order = np.argsort(np.asarray(cols["logp"], dtype=np.float64), kind="stable")
    tol = 1.5 / float(tobs)
    j = np.arange(1, int(max_ratio) + 1, dtype=np.float64)
    kept, kept_f, absorbed = [], [], []
    for i in order:
        f = freq[i]
        hit = -1
        if kept:
            fa = np.asarray(kept_f)[:, None]
            near = (np.abs(f - fa * j) <= tol) | (np.abs(f - fa / j) <= tol)
            rows = np.flatnonzero(near.any(axis=1))
            if rows.size:
                hit = int(rows[0])
        if hit >= 0:
            absorbed[hit] += 1
        else:
            kept.append(int(i))
            kept_f.append(f)
            absorbed.append(0)
    idx = np.asarray(kept, dtype=np.int64)
    out = {c: v[idx] for c, v in cols.items()}
    out["nabsorbed"] = np.asarray(absorbed, dtype=np.int64)
    return out


# ------------------------------------------------------------------ acceleration trials (numpy)

C_LIGHT = 299792458.0  # m / s
MAX_ACCEL_TRIALS = 65535


def accel_factor(accel, sample_time):
    """The dimensionless factor ``af = accel * sample_time / (2 c)`` of an acceleration in m/s^2
    (float64; an array gives an array)."""
    sample_time = float(sample_time)
    if not sample_time > 0:
        raise ValueError("accel_factor: sample_time must be positive")
    return np.asarray(accel, dtype=np.float64) * sample_time / (2.0 * C_LIGHT)


def resample_indices(n, af):
    """``src``, int64 ``(n,)``: sample ``i`` of a series of ``n`` resampled at the factor ``af`` is
    sample ``src[i] = i + clamp(rint(af i (i - n)))`` of the input (nearest neighbour; the clamp
    keeps ``0 <= src <= n - 1`` for every ``af``, NaN and inf included; include/pulsarutils_hip.h).
    This is the map ``pu_resample_accel`` and ``pu_rfft_accel`` apply, step for step."""
    n = int(n)
    if n < 0 or n > MAX_NFFT:
        raise ValueError("resample_indices: n must be in [0, 2^24]")
    i = np.arange(n, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.float64(af) * (i * (i - n)).astype(np.float64)
        s = np.fmin(np.fmax(np.rint(q), -i.astype(np.float64)), (n - 1 - i).astype(np.float64))
    return i + s.astype(np.int64)


def acceleration_grid(amax, tobs, ftop, drift_bins=1.0):
    """Trial accelerations (m/s^2, float64, ascending) from ``-amax`` to ``amax`` at least:
    ``step * (-k .. k)`` with ``step = drift_bins c / (ftop tobs^2)`` and ``k = ceil(amax / step)``,
    so the grid is symmetric and contains 0.  A signal at ``ftop`` Hz (the highest harmonic to be
    summed) drifts ``ftop a tobs^2 / c`` Fourier bins under the acceleration ``a``: between two
    trials it is left with at most ``drift_bins / 2``.  ``ValueError`` for a non-positive argument
    or more than 65535 trials."""
    amax, tobs, ftop, drift_bins = float(amax), float(tobs), float(ftop), float(drift_bins)
    if not all(math.isfinite(v) and v > 0 for v in (amax, tobs, ftop, drift_bins)):
        raise ValueError("acceleration_grid: amax, tobs, ftop and drift_bins must be positive")
    step = drift_bins * C_LIGHT / (ftop * tobs * tobs)
    steps = amax / step if step > 0 else math.inf
    k = math.ceil(steps) if steps <= MAX_ACCEL_TRIALS else MAX_ACCEL_TRIALS
    if 2 * k + 1 > MAX_ACCEL_TRIALS:
        raise ValueError(f"acceleration_grid: amax / step = {steps:g} (step {step:g} m/s^2) needs more than "
                         f"{MAX_ACCEL_TRIALS} trials")
    return step * np.arange(-k, k + 1, dtype=np.float64)


# ------------------------------------------------------------------ the device stages

def _series(series, what):
    """(float32 / float64 2-D device tensor, the input was 1-D, the input was numpy)."""
    x, one_d, as_numpy = _hip.as_rows(series, f"{what}: series must be (rows, nsamples) or 1-D",
                                      (_hip.PU_F32, _hip.PU_F64))
    if x.shape[1] < 1:
        raise ValueError(f"{what}: an empty series")
    return x, one_d, as_numpy


def _check_nfft(nfft, n):
    if nfft is None:
        return next_nfft(n)
    nfft = int(nfft)
    if nfft < MIN_NFFT or nfft > MAX_NFFT or nfft & (nfft - 1) or nfft < n:
        raise ValueError(f"nfft must be a power of two in [2^8, 2^24] and >= the {n} samples, got {nfft}")
    return nfft


def _check_block(block, nb):
    block = int(block)
    if block < 16 or block > min(1024, nb) or block & (block - 1):
        raise ValueError(f"block must be a power of two in [16, min(1024, {nb})], got {block}")
    return block


_aligned = _hip.workspace  # the name callers of this module knew it by


def _rows_per_call(rows, nfft):
    per_row = max(1, _hip.lib().pu_rfft_workspace_bytes(2, nfft) - _hip.lib().pu_rfft_workspace_bytes(1, nfft))
    return max(1, min(rows, _MAX_ROWS, _FFT_WS_BYTES // per_row))


def _rfft_device(x, nfft, mean=None):
    """pu_rfft of a 2-D row-major device tensor -> complex64 (rows, nfft / 2 + 1); ``mean``: float64
    (rows,) device tensor (default: the rows' float64 sums / n)."""
    from .stats import _chunk_row_sums
    t = _hip.torch()
    lib = _hip.lib()
    rows, n = x.shape
    spec = t.empty((rows, nfft // 2 + 1), dtype=t.complex64, device=x.device)
    if rows == 0:
        return spec
    if mean is None:
        mean = _chunk_row_sums(x, 3) / float(n)
    per = _rows_per_call(rows, nfft)
    ws, wp, wsb = _hip.workspace(lib.pu_rfft_workspace_bytes(per, nfft), x.device)
    for r0 in range(0, rows, per):
        m = min(per, rows - r0)
        _hip.check(lib.pu_rfft(_hip.ptr(x[r0:]), _hip.dtype_code(x.dtype), m, n, _hip.row_stride(x),
                               _hip.ptr(mean[r0:]), nfft, _hip.ptr(spec[r0:]), spec.stride(0), wp, wsb,
                               _hip.stream_ptr()), "pu_rfft")
    return spec


def _normalize_device(spec, nb, block):
    """pu_spectrum_normalize of a complex64 (rows, >= nb) device tensor -> float32 (rows, nb)."""
    t = _hip.torch()
    rows = spec.shape[0]
    out = t.empty((rows, nb), dtype=t.float32, device=spec.device)
    for r0 in range(0, rows, _MAX_ROWS):
        m = min(_MAX_ROWS, rows - r0)
        _hip.check(_hip.lib().pu_spectrum_normalize(_hip.ptr(spec[r0:]), m, nb, spec.stride(0), block,
                                                    _hip.ptr(out[r0:]), out.stride(0), _hip.stream_ptr()),
                   "pu_spectrum_normalize")
    return out


def _harmonic_search_device(norm, nlev, thr, kmin, kmax, sums=None, cap=0):
    """pu_harmonic_search of a float32 (rows, nb) row-major device tensor (at most ``_MAX_ROWS``
    rows) -> (``SPEC_CAND_DTYPE`` records on the host: the first ``cap``, the total count).
    ``sums``: None, or a contiguous float32 (nlev, rows, nb) device tensor to fill."""
    t = _hip.torch()
    lib = _hip.lib()
    rows, nb = norm.shape
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    kmin = np.ascontiguousarray(kmin, dtype=np.int64)
    kmax = np.ascontiguousarray(kmax, dtype=np.int64)
    if thr.size != nlev or kmin.size != nlev or kmax.size != nlev:
        raise ValueError("harmonic search: thr, kmin and kmax need one entry per level")
    count = ctypes.c_int64(0)
    if rows == 0:
        return np.zeros(0, _hip.SPEC_CAND_DTYPE), 0
    ws, wp, wsb = _hip.workspace(lib.pu_harmonic_search_workspace_bytes(rows, nb, nlev), norm.device)
    cap = int(cap)
    buf = t.empty(max(1, cap) * _hip.SPEC_CAND_DTYPE.itemsize, dtype=t.uint8, device=norm.device) if cap > 0 else None
    _hip.check(lib.pu_harmonic_search(_hip.ptr(norm), rows, nb, _hip.row_stride(norm), nlev, _hip.ptr(sums),
                                      sums.stride(0) if sums is not None else 0,
                                      sums.stride(1) if sums is not None else 0,
                                      thr.ctypes.data_as(ctypes.c_void_p), kmin.ctypes.data_as(ctypes.c_void_p),
                                      kmax.ctypes.data_as(ctypes.c_void_p), _hip.ptr(buf), cap, ctypes.byref(count), wp,
                                      wsb, _hip.stream_ptr()), "pu_harmonic_search")
    got = min(cap, count.value)
    if got == 0:
        return np.zeros(0, _hip.SPEC_CAND_DTYPE), count.value
    rec = buf[:got * _hip.SPEC_CAND_DTYPE.itemsize].cpu().numpy().view(_hip.SPEC_CAND_DTYPE).copy()
    return rec, count.value


def rfft(series, nfft=None):
    """The spectrum of each row minus its mean (float64 row sums / n), zero-padded to ``nfft``
    (default :func:`next_nfft` of the length): complex64 ``(rows, nfft / 2 + 1)``, ``(nfft / 2 +
    1,)`` for a 1-D series."""
    x, one_d, as_numpy = _series(series, "rfft")
    nfft = _check_nfft(nfft, x.shape[1])
    spec = _rfft_device(x, nfft)
    if one_d:
        spec = spec[0]
    return spec.cpu().numpy() if as_numpy else spec


def power_spectrum(series, nfft=None, block=128):
    """The normalised power spectrum of each row: float32 ``(rows, nfft / 2)`` (the Nyquist bin is
    dropped), noise at mean about 1 (module docstring)."""
    x, one_d, as_numpy = _series(series, "power_spectrum")
    nfft = _check_nfft(nfft, x.shape[1])
    block = _check_block(block, nfft // 2)
    norm = _normalize_device(_rfft_device(x, nfft), nfft // 2, block)
    if one_d:
        norm = norm[0]
    return norm.cpu().numpy() if as_numpy else norm


def harmonic_sums(norm, nharm=16):
    """The harmonic sums of normalised spectra ``(rows, nb)``, levels 0 .. log2(nharm): float32
    ``(nlev, rows, nb)`` (``(nlev, nb)`` for a 1-D spectrum)."""
    nlev = _nlev(nharm)
    t = _hip.require_gpu()
    x, one_d, as_numpy = _hip.as_rows(norm, "harmonic_sums: a normalised spectrum (rows, nb) or 1-D", (_hip.PU_F32,))
    if x.shape[1] < 1:
        raise ValueError("harmonic_sums: a normalised spectrum (rows, nb) or 1-D")
    if x.dtype != t.float32:
        x = x.to(t.float32)
    rows, nb = x.shape
    sums = t.empty((nlev, rows, nb), dtype=t.float32, device=x.device)
    never = np.full(nlev, np.inf, np.float32)
    zero = np.zeros(nlev, np.int64)
    for r0 in range(0, rows, _MAX_ROWS):
        m = min(_MAX_ROWS, rows - r0)
        _harmonic_search_device(x[r0:r0 + m], nlev, never, zero, zero, sums=sums[:, r0:])
    if one_d:
        sums = sums[:, 0]
    return sums.cpu().numpy() if as_numpy else sums


def periodicity_search(series, sample_time, fmin=None, fmax=None, nharm=16, sigma=6.0, block=128, pad=1, sift=True,
                       max_candidates=4096):
    """Blind search for periodic signals in ``series`` (one dedispersed series, or a plane (ndm,
    n) such as ``dedispersion_search(show=True)``'s).

    Each row goes through :func:`rfft` at ``nfft = next_nfft(n, pad)``, :func:`power_spectrum`'s
    normalisation in blocks of ``block`` bins and the harmonic sums of 1, 2 .. ``nharm`` harmonics
    (``nharm`` in 1, 2, 4, 8, 16, 32); a local maximum of a sum is a candidate when its
    single-trial Erlang tail probability is below that of ``sigma`` Gaussian standard deviations
    and its fundamental lies in ``[fmin, fmax]`` Hz (:func:`bin_ranges`).  No sums are written to
    memory; rows go in batches whose FFT workspace stays under 1 GiB.  ``max_candidates`` sizes
    the first candidate buffer of a batch: when a batch holds more, its buffer is allocated again
    at the size the count gives, so no candidate is ever dropped.

    Returns a table with one row per candidate, most significant first: ``freq`` (Hz, of the
    fundamental: ``bin / nharm / (nfft sample_time)``), ``row``, ``nharm``, ``bin`` (of the top
    harmonic), ``power`` (the summed normalised power), ``logp`` (``erlang_logsf(power, nharm)``,
    single trial), ``sigma`` (its Gaussian equivalent) and ``nabsorbed``.  ``sift=True`` passes the
    list through :func:`sift_candidates` (``tobs = nfft sample_time``); otherwise ``nabsorbed`` is 0."""
    nlev = _nlev(nharm)
    x, _, _ = _series(series, "periodicity_search")
    rows, n = x.shape
    sample_time, nfft, nb, block, thr, kmin, kmax = _search_levels("periodicity_search", n, sample_time, fmin, fmax, nlev,
                                                                   sigma, block, pad)
    per = _rows_per_call(rows, nfft)
    found = [np.zeros(0, _hip.SPEC_CAND_DTYPE)]
    for r0 in range(0, rows, per):
        rec = _spectrum_candidates(_rfft_device(x[r0:r0 + per], nfft), nb, block, nlev, thr, kmin, kmax, max_candidates)
        rec["row"] += r0
        found.append(rec)
    return _candidate_table(np.concatenate(found), nfft * sample_time, sift)


def _search_levels(what, n, sample_time, fmin, fmax, nlev, sigma, block, pad):
    """What a search of ``n`` samples fixes before its first batch: (sample_time, nfft, nb, block,
    and per level the power threshold of ``sigma`` and the bin range of ``[fmin, fmax]``)."""
    nfft = next_nfft(n, pad)
    nb = nfft // 2
    block = _check_block(block, nb)
    sample_time = float(sample_time)
    if not sample_time > 0:
        raise ValueError(f"{what}: sample_time must be positive")
    logp_min = logp_from_sigma(float(sigma))
    thr = np.array([power_threshold(logp_min, 1 << lv) for lv in range(nlev)], np.float32)
    kmin, kmax = bin_ranges(fmin, fmax, nfft, sample_time, nlev, nb)
    return sample_time, nfft, nb, block, thr, kmin, kmax


def _spectrum_candidates(spec, nb, block, nlev, thr, kmin, kmax, max_candidates):
    """The candidate records of a batch of spectra: normalise, sum, pick (``row``: the batch's)."""
    norm = _normalize_device(spec, nb, block)
    rec, count = _harmonic_search_device(norm, nlev, thr, kmin, kmax, cap=max(1, int(max_candidates)))
    if count > rec.size:  # more than the buffer held: once more with room for all
        rec, count = _harmonic_search_device(norm, nlev, thr, kmin, kmax, cap=count)
    return rec


def _candidate_table(rec, tobs, sift, extra=None):
    """The table of :func:`periodicity_search` from ``SPEC_CAND_DTYPE`` records (``row`` already
    the caller's row); ``extra``: further columns, one entry per record."""
    from .table import make_table
    harm = (1 << rec["level"].astype(np.int64))
    power = rec["power"].astype(np.float64)
    logp = np.zeros(rec.size)
    for h in np.unique(harm):
        sel = harm == h
        logp[sel] = erlang_logsf(power[sel], int(h))
    cols = {"freq": rec["bin"].astype(np.float64) / harm / tobs, "row": rec["row"].astype(np.int64), "nharm": harm,
            "bin": rec["bin"].astype(np.int64), "power": rec["power"].astype(np.float32), "logp": logp,
            "sigma": np.array([sigma_from_logp(v) for v in logp], dtype=np.float64)}
    cols.update(extra or {})
    if sift:
        cols = sift_candidates(cols, tobs)
    else:
        order = np.argsort(logp, kind="stable")
        cols = {c: v[order] for c, v in cols.items()}
        cols["nabsorbed"] = np.zeros(rec.size, np.int64)
    return make_table(cols)


# ------------------------------------------------------------------ acceleration trials (device)

def _accel_factors(what, accel, sample_time, n, device):
    """(``af`` as a float64 device tensor (nacc,), ``accel`` was a scalar); ``ValueError`` where the
    map would stop being monotone (``|af| n > 1``) or ``accel`` is not finite."""
    t = _hip.torch()
    acc = np.asarray(accel, dtype=np.float64)
    scalar = acc.ndim == 0
    acc = acc.reshape(-1)
    af = accel_factor(acc, sample_time)
    if not np.all(np.abs(af) * n <= 1.0):  # (NaN fails too)
        raise ValueError(f"{what}: |accel| sample_time / (2 c) x {n} samples must be <= 1 and finite: beyond, "
                         "nearest-neighbour resampling is not monotone")
    return t.from_numpy(np.ascontiguousarray(af)).to(device), scalar


def _resample_device(x, af):
    """pu_resample_accel of a 2-D row-major device tensor -> (nacc, rows, n) of its dtype."""
    t = _hip.torch()
    rows, n = x.shape
    nacc = af.numel()
    out = t.empty((nacc, rows, n), dtype=x.dtype, device=x.device)
    _hip.check(_hip.lib().pu_resample_accel(_hip.ptr(x), _hip.dtype_code(x.dtype), rows, n, _hip.row_stride(x),
                                            _hip.ptr(af), nacc, _hip.ptr(out), n, _hip.stream_ptr()),
               "pu_resample_accel")
    return out


def _accel_batches(rows, nacc, nfft):
    """The (a0, a1, r0, r1) of the calls that cover nacc x rows (acceleration, row) pairs, sized as
    :func:`_rows_per_call` sizes rows: whole accelerations per call while ``rows`` fit in one, else
    one acceleration and the row batches of :func:`periodicity_search`."""
    per = _rows_per_call(rows * nacc, nfft)
    if rows <= per:
        na = per // rows
        return [(a0, min(a0 + na, nacc), 0, rows) for a0 in range(0, nacc, na)]
    return [(a, a + 1, r0, min(r0 + per, rows)) for a in range(nacc) for r0 in range(0, rows, per)]


def _rfft_accel_device(x, af, mean, nfft, ws, spec=None):
    """pu_rfft_accel of one batch: ``x`` (rows, n), ``af`` (nacc,), ``mean`` (rows,) -> complex64
    (nacc * rows, nfft / 2 + 1), pair ``a * rows + r``.  ``ws``: :func:`_hip.workspace` triple."""
    t = _hip.torch()
    rows, n = x.shape
    nacc = af.numel()
    if spec is None:
        spec = t.empty((nacc * rows, nfft // 2 + 1), dtype=t.complex64, device=x.device)
    _hip.check(_hip.lib().pu_rfft_accel(_hip.ptr(x), _hip.dtype_code(x.dtype), rows, n, _hip.row_stride(x),
                                        _hip.ptr(mean), _hip.ptr(af), nacc, nfft, _hip.ptr(spec), spec.stride(0), ws[1],
                                        ws[2], _hip.stream_ptr()),
               "pu_rfft_accel")
    return spec


def _accel_workspace(batches, nfft, device):
    lib = _hip.lib()
    return _hip.workspace(max(lib.pu_rfft_accel_workspace_bytes(r1 - r0, a1 - a0, nfft) for a0, a1, r0, r1 in batches), device)


def resample(series, accel, sample_time):
    """``series`` resampled in time at the constant line-of-sight acceleration ``accel`` (m/s^2):
    sample ``i`` of a row becomes its sample :func:`resample_indices` ``(n, accel_factor(accel,
    sample_time))[i]``, nearest neighbour.  A scalar ``accel`` gives the series' shape and dtype; an
    array of ``nacc`` gives ``(nacc, rows, n)`` (``(nacc, n)`` for a 1-D series).  ``ValueError``
    when ``|accel| sample_time / (2 c) * n > 1``."""
    x, one_d, as_numpy = _series(series, "resample")
    af, scalar = _accel_factors("resample", accel, sample_time, x.shape[1], x.device)
    out = _resample_device(x, af)
    if one_d:
        out = out[:, 0]
    if scalar:
        out = out[0]
    return out.cpu().numpy() if as_numpy else out


def rfft_accel(series, accels, sample_time, nfft=None):
    """:func:`rfft` of every row at every trial acceleration, the resampling of :func:`resample`
    applied where the transform loads its samples (no resampled series is written): complex64
    ``(nacc, rows, nfft / 2 + 1)`` (``(nacc, nfft / 2 + 1)`` for a 1-D series).  The mean taken out
    is the row's own (float64 sum / n), the same at every acceleration; with it the result has the
    bits ``pu_rfft`` gives on the resampled series."""
    from .stats import _chunk_row_sums
    t = _hip.torch()
    x, one_d, as_numpy = _series(series, "rfft_accel")
    rows, n = x.shape
    nfft = _check_nfft(nfft, n)
    af, _ = _accel_factors("rfft_accel", accels, sample_time, n, x.device)
    nacc = af.numel()
    spec = t.empty((nacc, rows, nfft // 2 + 1), dtype=t.complex64, device=x.device)
    if nacc:
        mean = _chunk_row_sums(x, 3) / float(n)
        batches = _accel_batches(rows, nacc, nfft)
        ws = _accel_workspace(batches, nfft, x.device)
        for a0, a1, r0, r1 in batches:
            if r1 - r0 == rows:
                _rfft_accel_device(x, af[a0:a1], mean, nfft, ws, spec=spec[a0:a1].view(-1, nfft // 2 + 1))
            else:
                _rfft_accel_device(x[r0:r1], af[a0:a1], mean[r0:r1], nfft, ws, spec=spec[a0, r0:r1])
    if one_d:
        spec = spec[:, 0]
    return spec.cpu().numpy() if as_numpy else spec


def acceleration_search(series, sample_time, accels=None, amax=None, fmin=None, fmax=None, nharm=16, sigma=6.0,
                        block=128, pad=1, sift=True, max_candidates=4096):
    """:func:`periodicity_search` with an acceleration axis: every row is searched at every trial
    acceleration, so a pulsar whose frequency drifts across Fourier bins (a binary) adds up again
    at the trial nearest to its line-of-sight acceleration.

    Give exactly one of ``accels`` (m/s^2, any order) and ``amax``: the latter searches
    :func:`acceleration_grid` ``(amax, n sample_time, ftop)`` with ``ftop = min(fmax nharm,
    Nyquist)`` (Nyquist when ``fmax`` is None).  The (acceleration, row) pairs go through
    ``pu_rfft_accel`` - :func:`rfft_accel`: the resampling happens in the transform's first load,
    no resampled plane is written - and then through :func:`periodicity_search`'s normalisation,
    harmonic sums and candidate rule, in batches of at most 1 GiB of FFT workspace.

    Returns :func:`periodicity_search`'s table plus ``accel`` (m/s^2, the trial's); ``row`` is the
    series' row.  ``sift=True``: :func:`sift_candidates` as there - it merges across rows, so a
    signal seen at neighbouring accelerations is absorbed into its best one.  ``accels=[0.0]``
    gives :func:`periodicity_search`'s table.  A constant acceleration only: no jerk."""
    from .stats import _chunk_row_sums
    if (accels is None) == (amax is None):
        raise ValueError("acceleration_search: give exactly one of accels and amax")
    nlev = _nlev(nharm)
    x, _, _ = _series(series, "acceleration_search")
    rows, n = x.shape
    sample_time, nfft, nb, block, thr, kmin, kmax = _search_levels("acceleration_search", n, sample_time, fmin, fmax, nlev,
                                                                   sigma, block, pad)
    if accels is None:
        nyquist = 0.5 / sample_time
        ftop = nyquist if fmax is None else min(float(fmax) * int(nharm), nyquist)
        accels = acceleration_grid(amax, n * sample_time, ftop)
    accels = np.asarray(accels, dtype=np.float64).reshape(-1)
    af, _ = _accel_factors("acceleration_search", accels, sample_time, n, x.device)
    found, found_a = [np.zeros(0, _hip.SPEC_CAND_DTYPE)], [np.zeros(0, np.int64)]
    if accels.size:
        means = {}  # per row batch, as periodicity_search takes them
        batches = _accel_batches(rows, accels.size, nfft)
        ws = _accel_workspace(batches, nfft, x.device)
        for a0, a1, r0, r1 in batches:
            if (r0, r1) not in means:
                means[r0, r1] = _chunk_row_sums(x[r0:r1], 3) / float(n)
            spec = _rfft_accel_device(x[r0:r1], af[a0:a1], means[r0, r1], nfft, ws)
            rec = _spectrum_candidates(spec, nb, block, nlev, thr, kmin, kmax, max_candidates)
            pair = rec["row"].astype(np.int64)
            found_a.append(a0 + pair // (r1 - r0))
            rec["row"] = r0 + pair % (r1 - r0)
            found.append(rec)
    return _candidate_table(np.concatenate(found), nfft * sample_time, sift,
                            extra={"accel": accels[np.concatenate(found_a)] if accels.size else np.zeros(0)})


__all__ = ["next_nfft", "harmonic_bins", "erlang_logsf", "power_threshold", "sigma_from_logp", "logp_from_sigma",
           "bin_ranges", "sift_candidates", "rfft", "power_spectrum", "harmonic_sums", "periodicity_search",
           "accel_factor", "resample_indices", "acceleration_grid", "resample", "rfft_accel", "acceleration_search"]
