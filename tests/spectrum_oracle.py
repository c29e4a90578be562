"""Host restatement of the FFT periodicity search (include/pulsarutils_hip.h: pu_rfft,
pu_spectrum_normalize, pu_harmonic_search): the float64 DFT of the float32-rounded samples, and
the normalisation, the harmonic sums and the candidate rule in the exact float32 order of the
header (numpy's elementwise float32 operations round once each and never fuse).

Test infrastructure only.  Nothing here imports ``pulsarutils.periodicity`` (the code under
test).  tests/test_spectrum_oracle.py pins these functions against hand-computed facts."""
import numpy as np

F32 = np.float32
LN2 = F32(0.6931472)
CAND_DTYPE = np.dtype([("row", "<i4"), ("level", "<i4"), ("bin", "<i8"), ("power", "<f4"), ("pad", "<f4")])


def padded_samples(x, nfft, mean=None):
    """``y``: float32 (rows, nfft), ``float32(float64(x) - mean)`` then zeros."""
    x = np.atleast_2d(np.asarray(x))
    rows, n = x.shape
    mean = np.zeros(rows) if mean is None else np.asarray(mean, dtype=np.float64).reshape(rows)
    y = np.zeros((rows, int(nfft)), F32)
    y[:, :n] = (x.astype(np.float64) - mean[:, None]).astype(F32)
    return y


def rfft(x, nfft, mean=None):
    """The float64 DFT of the float32-rounded, zero-padded samples: complex128 (rows, nfft/2+1)."""
    return np.fft.rfft(padded_samples(x, nfft, mean).astype(np.float64), axis=1)


def power(spec, nb):
    """``re re + im im`` in float32 (two products, one sum) of bins 0 .. nb - 1."""
    spec = np.atleast_2d(np.asarray(spec))[:, :nb]
    re, im = spec.real.astype(F32), spec.imag.astype(F32)
    a, b = re * re, im * im
    return a + b


def normalize(spec, nb, block):
    """pu_spectrum_normalize of a complex64 spectrum (rows, >= nb): float32 (rows, nb)."""
    with np.errstate(all="ignore"):
        p = power(spec, nb)
        out = np.zeros_like(p)
        for r in range(p.shape[0]):
            for b0 in range(0, nb, block):
                blk = p[r, b0:b0 + block]
                real = blk[1:] if b0 == 0 else blk
                if not np.all(np.isfinite(real)):
                    out[r, b0:b0 + block] = np.nan
                    continue
                srt = blk.copy()
                if b0 == 0:
                    srt[0] = np.inf
                srt = np.sort(srt)
                lo, hi = srt[block // 2 - 1], srt[block // 2]
                med = lo if b0 == 0 else F32(0.5) * (lo + hi)
                if not med > 0:
                    continue
                scale = LN2 / med
                out[r, b0:b0 + block] = blk * scale
        out[:, 0] = 0
    return out


def harmonic_sums(norm, nlev):
    """float32 (nlev, rows, nb): S_0 = norm, S_(l+1)[k] = S_l[k] + the terms norm[(k m + H) // (2H)]
    for odd m ascending, added one at a time."""
    norm = np.atleast_2d(np.asarray(norm, dtype=F32))
    rows, nb = norm.shape
    k = np.arange(nb, dtype=np.int64)
    out = np.zeros((nlev, rows, nb), F32)
    s = norm.copy()
    out[0] = s
    with np.errstate(all="ignore"):
        for lv in range(nlev - 1):
            h = 1 << lv
            for m in range(1, 2 * h, 2):
                s = s + norm[:, (k * m + h) // (2 * h)]
            out[lv + 1] = s
    return out


def candidates(sums, thr, kmin, kmax):
    """The candidate records of sums (nlev, rows, nb), sorted by (row, level, bin)."""
    sums = np.asarray(sums, dtype=F32)
    nlev, rows, nb = sums.shape
    rec = []
    with np.errstate(all="ignore"):
        for r in range(rows):
            for lv in range(nlev):
                s = sums[lv, r]
                left = np.concatenate(([F32(-np.inf)], s[:-1]))
                right = np.concatenate((s[1:], [F32(-np.inf)]))
                k = np.arange(nb)
                ok = (k >= kmin[lv]) & (k < kmax[lv]) & (s > F32(thr[lv])) & (s > left) & (s >= right)
                for b in np.flatnonzero(ok):
                    rec.append((r, lv, int(b), s[b], 0.0))
    return np.array(rec, dtype=CAND_DTYPE)
