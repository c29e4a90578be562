"""Host restatement of the acceleration trials (include/pulsarutils_hip.h: pu_resample_accel,
pu_rfft_accel): the nearest-neighbour index map, the gather, and the scenario the GPU test
searches (a pulse train that drifts across Fourier bins).

Test infrastructure only.  Nothing here imports ``pulsarutils.periodicity`` (the code under
test).  tests/test_accel_oracle.py pins these functions against exact rational arithmetic."""
import numpy as np

import spectrum_oracle as so

C = 299792458.0


def accel_factor(accel, sample_time):
    """``af = accel * sample_time / (2 c)``."""
    return np.float64(accel) * np.float64(sample_time) / (2.0 * C)


def resample_indices(n, af):
    """``src`` (int64, n): ``p = float64(i (i - n))`` (int64 product), ``q = af p`` (one rounding),
    ``s = fmin(fmax(rint(q), -i), n - 1 - i)``, ``src = i + int64(s)``."""
    i = np.arange(int(n), dtype=np.int64)
    p = (i * (i - int(n))).astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.float64(af) * p
        s = np.fmin(np.fmax(np.rint(q), -(i.astype(np.float64))), (int(n) - 1 - i).astype(np.float64))
    return i + s.astype(np.int64)


def resample(x, af):
    """``x`` (rows, n) or (n,) gathered along its last axis at ``resample_indices(n, af)``."""
    x = np.asarray(x)
    return x[..., resample_indices(x.shape[-1], af)]


def emitted_index(u, n, af):
    """The exact inverse of the unrounded map: the resampled-series index ``i`` (float64) with
    ``i + af i (i - n) = u``, i.e. the root of ``af i^2 + (1 - af n) i - u = 0`` that is ``u`` at
    ``af = 0`` (written so that it neither cancels nor divides by ``af``)."""
    u = np.asarray(u, dtype=np.float64)
    b = 1.0 - np.float64(af) * n
    return 2.0 * u / (b + np.sqrt(b * b + 4.0 * np.float64(af) * u))


# the detection scenario: shared by tests/test_accel_oracle.py and tests/test_gpu_accel.py
N, DT, F0, DUTY, AMP, SEED, ACCEL = 2 ** 14, 1e-3, 23.7, 0.05, 1.0, 5, 3.8e5
BLOCK, NLEV = 128, 5


def drifting_rows():
    """float32 (2, N): row 0 is unit Gaussian noise plus a pulse train of F0 Hz, DUTY and AMP that is
    periodic in the series resampled at ACCEL (received sample ``u`` shows the phase of
    ``emitted_index(u)``); row 1 is noise alone."""
    rng = np.random.default_rng(SEED)
    a = rng.standard_normal(N).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    i = emitted_index(np.arange(N), N, accel_factor(ACCEL, DT))
    a[(i * DT * F0) % 1.0 < DUTY] += np.float32(AMP)
    return np.stack([a, b])


def best_sums(row, block=BLOCK, nlev=NLEV):
    """Per level: (the largest harmonic sum over the bins ``k >= 2^level``, its bin) of one series,
    by spectrum_oracle's rfft (float64 mean taken out, rounded to complex64), normalize and
    harmonic_sums."""
    row = np.asarray(row)
    n = row.size
    mean = [row.astype(np.float64).sum() / n]
    spec = so.rfft(row[None], n, mean).astype(np.complex64)
    sums = so.harmonic_sums(so.normalize(spec, n // 2, block), nlev)[:, 0]
    out = []
    for lv in range(nlev):
        k = (1 << lv) + int(np.argmax(sums[lv, 1 << lv:]))
        out.append((float(sums[lv, k]), k))
    return out
