"""Folding at a pulse period and the Z^2_n / H statistics: the periodic-pulsar path.

``clean.PulseInfo`` and ``clean.dedispersion_search(info, dmmin, dmmax)`` are the API of a
*folded* profile (one turn in ``nbin`` bins, ``sample_time = 1 / pulse_freq / nbin``), and
``clean.digitize`` exists to feed the H-test of the reference's ``plot_diagnostics``
(clean.py:252-253).  The reference makes no folded profile and draws its H-versus-DM panel
with hendrics; this module makes the profile from a filterbank (:func:`fold`,
:func:`fold_file`) and returns what the panel plotted as arrays (:func:`h_curve`,
:func:`profile_stats`).  The plots themselves stay out of scope.

**The bin rule** (:func:`fold_bins`; ``pu_fold`` in include/pulsarutils_hip.h computes the
same bits on the device).  With ``dphase = sample_time * pulse_freq`` (one float64 product),
sample ``i`` of the file falls in bin::

    p = ph0 + float64(i) * dphase          # one multiply, one add, no fused multiply-add
    f = p - floor(p)
    b = min(int64(f * float64(nbin)), nbin - 1)

**Z^2_n and H** (de Jager et al. 1989, binned as hendrics / stingray do; ``pu_h_test``).  For a
profile ``p[0 .. n)``: ``P = sum p``, ``C_k, S_k = sum_j p[j] cos, sin(2 pi ((k j) mod n) / n)``,
``Z^2_m = (2 / P) sum_{k <= m} (C_k^2 + S_k^2)``, ``H = max_m (Z^2_m - 4 m + 4)`` and ``M`` the
first ``m`` that attains it.  A profile with a non-finite value or ``P`` not ``> 0`` gives NaN
(``M = 0``).

Conventions are the package's: numpy in -> numpy out, CUDA tensor in -> tensors out.
Importable without a GPU (:func:`fold_bins` is pure numpy); everything else runs HIP kernels
and raises ``HipBackendError`` without the library or a GPU.
"""
import numpy as np

from . import _hip


def fold_bins(nsamples, pulse_freq, sample_time, nbin, ph0=0.0, first_sample=0):
    """The bin (int64) of samples ``first_sample .. first_sample + nsamples - 1``: the
    documented definition of the fold, in numpy."""
    nbin = int(nbin)
    if nbin < 1:
        raise ValueError("fold_bins: nbin must be >= 1")
    dphase = float(sample_time) * float(pulse_freq)
    idx = np.arange(int(first_sample), int(first_sample) + int(nsamples), dtype=np.int64)
    prod = idx.astype(np.float64) * dphase
    p = float(ph0) + prod
    f = p - np.floor(p)
    return np.minimum((f * float(nbin)).astype(np.int64), nbin - 1)


def _fold_device(x, dphase, nbin, ph0, first_sample, sums, counts):
    """pu_fold of a 2-D row-major device tensor into device ``sums`` / ``counts``."""
    lib = _hip.lib()
    nchan, n = x.shape
    ws, wp, wsb = _hip.workspace(lib.pu_fold_workspace_bytes(nchan, n, nbin), x.device)
    _hip.check(lib.pu_fold(_hip.ptr(x), _hip.dtype_code(x.dtype), nchan, n, _hip.row_stride(x), int(first_sample),
                           float(ph0), float(dphase), int(nbin), _hip.ptr(sums), sums.stride(0), _hip.ptr(counts), wp,
                           wsb, _hip.stream_ptr()), "pu_fold")


def fold(data, pulse_freq, sample_time, nbin, ph0=0.0, first_sample=0, out=None):
    """Fold ``data`` (nchan, nsamples; a 1-D array is one channel) at ``pulse_freq``.

    Returns ``(sums, counts)``: float64 ``(nchan, nbin)`` sums of the samples of each bin and
    the int64 number of samples per bin (the same for every channel).  ``first_sample`` is
    the position of ``data``'s first sample in the series the phase counts from, so chunks of
    a file fold to partial results that add up.  ``out=(sums, counts)``: existing device
    tensors (float64 ``(nchan, nbin)`` row-major, int64 ``(nbin,)``) to accumulate into; they
    are returned.  uint8, float32 and float64 data are folded as they are, other types as
    float64.  Exact for uint8 (and for integer-valued input below 2^53); reproducible bit for
    bit otherwise (no floating-point atomics)."""
    t = _hip.require_gpu()
    x, one_d, as_numpy = _hip.as_rows(data, "fold: data must be (nchan, nsamples) or 1-D",
                                      (_hip.PU_U8, _hip.PU_F32, _hip.PU_F64))
    nbin = int(nbin)
    if nbin < 1:
        raise ValueError("fold: nbin must be >= 1")
    nchan = x.shape[0]
    if out is None:
        sums = t.zeros((nchan, nbin), dtype=t.float64, device=x.device)
        counts = t.zeros(nbin, dtype=t.int64, device=x.device)
    else:
        sums, counts = out
        ok = (isinstance(sums, t.Tensor) and isinstance(counts, t.Tensor) and sums.dtype == t.float64
              and counts.dtype == t.int64 and tuple(sums.shape) == (nchan, nbin) and tuple(counts.shape) == (nbin,)
              and sums.stride(1) == 1 and counts.is_contiguous() and sums.device == x.device
              and counts.device == x.device)
        if not ok:
            raise ValueError(f"fold: out must be a row-major float64 ({nchan}, {nbin}) tensor and a contiguous int64 "
                             f"({nbin},) tensor on {x.device}")
    _fold_device(x, float(sample_time) * float(pulse_freq), nbin, ph0, first_sample, sums, counts)
    if out is not None:
        return sums, counts
    if one_d:
        sums = sums[0]
    if as_numpy:
        return sums.cpu().numpy(), counts.cpu().numpy()
    return sums, counts


def fold_file(fname, pulse_freq, nbin=128, ph0=0.0, chunksize=2**17, clean=True, surelybad=(), tmin=0.0, tmax=None,
              zero_dm=False):
    """Fold a SIGPROC filterbank at ``pulse_freq`` (Hz) into a ``clean.PulseInfo``.

    The file is streamed in non-overlapping chunks of ``chunksize`` samples
    (``filestream.tiled_chunks``); chunk k + 1 is uploaded while chunk k is folded
    (``filestream.ChunkStream``) and all array work stays in HBM.  The phase counts from the
    file's first sample, whatever ``tmin``; samples ``i`` with ``tmin <= i * tsamp < tmax`` are folded.

    ``clean=True``: each chunk goes through ``renormalize_device`` with the
    ``get_bad_chans`` (+ ``surelybad``) mask, as in ``search_by_chunks`` (``zero_dm`` is its
    opt-in subtraction), and the float64 result is folded.  ``clean=False``: the raw samples
    are folded (exactly, for 8-bit and packed files) and the masked channels' rows are zeroed
    at the end.

    The result has ``allprofs = sums / counts`` (float64 ``(nchan, nbin)``; a bin no sample
    hit is 0), flipped when ``foff < 0`` so that channel 0 is the lowest frequency, and
    ``nbin, nchan, pulse_freq, ph0, start_freq, bandwidth, date`` set, plus the attribute
    ``counts``; it feeds ``clean.dedispersion_search(info, dmmin, dmmax)`` as it is."""
    from .clean import PulseInfo, renormalize_device
    from .filestream import ChunkStream, bad_channel_mask, tiled_chunks
    from .sigproc import FilReader
    nbin, chunksize = int(nbin), int(chunksize)
    if nbin < 1 or chunksize < 1:
        raise ValueError("fold_file: nbin and chunksize must be positive")
    t = _hip.require_gpu()
    mask = bad_channel_mask(fname, surelybad)
    fil = FilReader(fname)
    header = fil.header
    nsamples, tsamp, nchan = header["nsamples"], header["tsamp"], header["nchans"]
    i0 = min(nsamples, max(0, int(np.ceil(float(tmin) / tsamp))))
    i1 = nsamples if tmax is None else min(nsamples, max(i0, int(np.ceil(float(tmax) / tsamp))))
    dev = t.device("cuda", t.cuda.current_device())
    dphase = float(tsamp) * float(pulse_freq)
    sums = t.zeros((nchan, nbin), dtype=t.float64, device=dev)
    counts = t.zeros(nbin, dtype=t.int64, device=dev)
    with ChunkStream(fil, tiled_chunks(i0, i1, chunksize), dev, prefetch=True) as blocks:
        for istart, _, block in blocks:
            if clean:
                block, _ = renormalize_device(block, badchans_mask=mask, zero_dm=zero_dm)
            _fold_device(block, dphase, nbin, ph0, istart, sums, counts)
            del block
    s, c = sums.cpu().numpy(), counts.cpu().numpy()
    allprofs = np.zeros_like(s)
    hit = c > 0
    allprofs[:, hit] = s[:, hit] / c[hit].astype(np.float64)
    allprofs[mask] = 0.0
    if header["foff"] < 0:
        allprofs = np.ascontiguousarray(allprofs[::-1])
    info = PulseInfo()
    info.allprofs = allprofs
    info.counts = c
    info.nbin = nbin
    info.nchan = nchan
    info.pulse_freq = float(pulse_freq)
    info.ph0 = float(ph0)
    info.start_freq = header["fbottom"]
    info.bandwidth = header["bandwidth"]
    info.date = header.get("tstart")
    return info


def _h_test_device(prof, nmax, want_zs):
    """pu_h_test of a 2-D row-major float64 device tensor -> (h, m, zs or None) tensors."""
    t = _hip.torch()
    lib = _hip.lib()
    rows, n = prof.shape
    nmax = int(nmax)
    h = t.empty(rows, dtype=t.float64, device=prof.device)
    m = t.empty(rows, dtype=t.int32, device=prof.device)
    zs = t.empty((rows, max(nmax, 1)), dtype=t.float64, device=prof.device) if want_zs else None
    ws, wp, wsb = _hip.workspace(lib.pu_h_test_workspace_bytes(rows, n, nmax), prof.device)
    _hip.check(lib.pu_h_test(_hip.ptr(prof), rows, n, _hip.row_stride(prof), nmax, _hip.ptr(h), _hip.ptr(m), _hip.ptr(zs),
                             zs.stride(0) if zs is not None else 0, wp, wsb, _hip.stream_ptr()), "pu_h_test")
    return h, m, zs


def _profiles(profiles):
    """(float64 2-D device tensor, the input was 1-D, the input was numpy)."""
    return _hip.as_rows(profiles, "profiles must be 1-D or (rows, n)", (_hip.PU_F64,))


def z_n_all(profiles, nmax=20):
    """``Z^2_1 .. Z^2_nmax`` of each profile: float64 ``(rows, nmax)`` (a 1-D input is one
    row).  ``2 <= n <= 8192`` bins and ``1 <= nmax <= n - 1`` (``ValueError`` otherwise)."""
    x, _, as_numpy = _profiles(profiles)
    _, _, zs = _h_test_device(x, nmax, True)
    return zs.cpu().numpy() if as_numpy else zs


def h_test(profiles, nmax=20):
    """``(H, M)`` of each profile: scalars for a 1-D input, arrays (float64, int32) for a 2-D
    one."""
    x, one_d, as_numpy = _profiles(profiles)
    h, m, _ = _h_test_device(x, nmax, False)
    if as_numpy:
        h, m = h.cpu().numpy(), m.cpu().numpy()
        if one_d:
            return float(h[0]), int(m[0])
        return h, m
    return (h[0], m[0]) if one_d else (h, m)


def h_curve(plane, nmax=None):
    """The H-versus-DM panel of the reference's ``plot_diagnostics`` (clean.py:252-253) as
    arrays: ``h_test(row, nmax = n // 10)`` of every row of ``clean.digitize(plane)``
    (``plane``: the dedispersed plane of ``clean.dedispersion_search``, (ndm, n)).  The
    reference plots ``-H``; this returns ``(H, M)``.  ``digitize`` runs on the host (a folded
    plane is small); the statistics run on the GPU."""
    from .clean import digitize
    plane = np.asarray(plane)
    if plane.ndim != 2:
        raise ValueError("h_curve: a (ndm, n) plane")
    n = plane.shape[1]
    if nmax is None:
        nmax = n // 10
    if n // 10 < 1 or int(nmax) < 1:
        raise ValueError(f"h_curve: {n} bins give nmax = n // 10 < 1")
    with np.errstate(divide="ignore", invalid="ignore"):
        dig = digitize(plane.astype(np.float64))
    return h_test(dig.astype(np.float64), nmax=int(nmax))


def profile_stats(info, dm=None):
    """Fill ``info``'s profile fields from ``info.allprofs`` and return ``info``.

    ``disp_profile``: the sum over channels in channel order; ``dedisp_profile``:
    ``dedispersion.dedisperse(allprofs, shifts)`` at ``dm`` (default ``info.dm``) with
    ``sample_time = 1 / pulse_freq / nbin``.  ``disp_z2 / z6 / z12 / z20`` and ``dedisp_*``:
    ``Z^2_m`` of the digitized profiles (``clean.digitize``), each requested at ``nmax = m``;
    ``*_H, *_M``: :func:`h_test` at ``nmax = 20``."""
    from .clean import digitize
    from .dedispersion import dedisperse, dedispersion_shifts
    if dm is None:
        dm = info.dm
    if dm is None:
        raise ValueError("profile_stats: no dm given and info.dm is None")
    allprofs = np.asarray(info.allprofs)
    nchan, nbin = allprofs.shape
    sample_time = 1 / info.pulse_freq / nbin
    info.dm = float(dm)
    info.disp_profile = np.add.reduce(allprofs.astype(np.float64), axis=0)
    shifts = dedispersion_shifts(nchan, dm, info.start_freq, info.bandwidth, sample_time)
    info.dedisp_profile = dedisperse(allprofs, shifts)
    for name, prof in (("disp", info.disp_profile), ("dedisp", info.dedisp_profile)):
        with np.errstate(divide="ignore", invalid="ignore"):
            dig = np.asarray(digitize(np.array(prof, dtype=np.float64)), dtype=np.float64)
        for m in (2, 6, 12, 20):
            setattr(info, f"{name}_z{m}", float(z_n_all(dig, nmax=m)[0, -1]))
        h, mm = h_test(dig, nmax=20)
        setattr(info, f"{name}_H", h)
        setattr(info, f"{name}_M", mm)
    return info


# ------------------------------------------------------------------ the pulse-frequency search

def frequency_grid(fmin, fmax, tobs, oversample=8):
    """Trial frequencies ``fmin + k df``, ``df = 1 / (oversample tobs)``, for ``k = 0 ..
    ceil((fmax - fmin) / df)``: ``oversample`` trials per independent frequency ``1 / tobs`` of
    an observation of ``tobs`` seconds; the last one is at or just beyond ``fmax``.  Pure numpy."""
    fmin, fmax, tobs, oversample = float(fmin), float(fmax), float(tobs), float(oversample)
    if not fmax >= fmin:
        raise ValueError("frequency_grid: fmax < fmin")
    if not tobs > 0 or not oversample > 0:
        raise ValueError("frequency_grid: tobs and oversample must be positive")
    df = 1.0 / (oversample * tobs)
    nk = int(np.ceil((fmax - fmin) / df))
    return fmin + np.arange(nk + 1, dtype=np.float64) * df


_TRIALS_WS_BYTES = 1 << 30  # pu_fold_trials' partials per call: longer trial lists go in batches


def _series(series, what):
    """(float32 / float64 2-D device tensor, the input was 1-D, the input was numpy)."""
    return _hip.as_rows(series, f"{what}: series must be (rows, nsamples) or 1-D", (_hip.PU_F32, _hip.PU_F64))


def _fold_trials_device(x, dphase, phase0, nbin, first_sample, sums, counts):
    """pu_fold_trials of a 2-D row-major device tensor into device ``sums`` (rows, F, nbin) /
    ``counts`` (F, nbin); ``dphase``, ``phase0``: float64 device tensors (F,).  The trial list
    goes in batches whose partials stay under ``_TRIALS_WS_BYTES`` (a trial's bits do not
    depend on the batch it is in)."""
    lib = _hip.lib()
    rows, n = x.shape
    ntrials = dphase.numel()
    if rows == 0 or n == 0 or ntrials == 0:
        return
    ld = _hip.row_stride(x)
    per_trial = max(1, lib.pu_fold_trials_workspace_bytes(rows, n, 1, nbin))
    batch = max(1, min(ntrials, _TRIALS_WS_BYTES // per_trial))
    ws, wp, wsb = _hip.workspace(lib.pu_fold_trials_workspace_bytes(rows, n, batch, nbin), x.device)
    for k0 in range(0, ntrials, batch):
        nk = min(batch, ntrials - k0)
        _hip.check(lib.pu_fold_trials(_hip.ptr(x), _hip.dtype_code(x.dtype), rows, n, ld, int(first_sample),
                                      _hip.ptr(phase0[k0:]), _hip.ptr(dphase[k0:]), nk, int(nbin),
                                      _hip.ptr(sums[:, k0:]), sums.stride(1), sums.stride(0), _hip.ptr(counts[k0:]),
                                      wp, wsb, _hip.stream_ptr()), "pu_fold_trials")


def _trial_phases(freqs, sample_time, ph0, device):
    """``dphase[k] = float(sample_time) * float(freqs[k])`` (one float64 product) and ``ph0``
    broadcast to the trials, as float64 device tensors, and the frequencies as a numpy array."""
    t = _hip.torch()
    if isinstance(freqs, t.Tensor):
        freqs = freqs.detach().cpu().numpy()
    f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    if f.ndim != 1:
        raise ValueError("freqs must be a scalar or 1-D")
    if isinstance(ph0, t.Tensor):
        ph0 = ph0.detach().cpu().numpy()
    p = np.array(np.broadcast_to(np.asarray(ph0, dtype=np.float64), f.shape))  # (a writable copy for torch)
    dphase = float(sample_time) * f
    return t.from_numpy(np.ascontiguousarray(dphase)).to(device), t.from_numpy(np.ascontiguousarray(p)).to(device), f


def fold_trials(series, freqs, sample_time, nbin, ph0=0.0, first_sample=0, out=None):
    """Fold ``series`` (rows, nsamples; a 1-D array is one row) at every trial frequency of
    ``freqs`` (Hz): the bin rule is :func:`fold_bins`' for each trial (``ph0``: a scalar or one
    value per trial).

    Returns ``(sums, counts)``: float64 ``(rows, F, nbin)`` (``(F, nbin)`` for a 1-D series) and
    int64 ``(F, nbin)``, the same for every row.  ``first_sample`` places the chunk in the
    series the phase counts from; ``out=(sums, counts)``: existing device tensors (float64
    ``(rows, F, nbin)``, int64 ``(F, nbin)``, both contiguous) to accumulate into; they are
    returned.  float32 and float64 series are folded as they are, other types as float64.
    ``2 <= nbin <= 256``.  A trial whose phase is not finite or reaches 2^52 in the chunk gets
    NaN sums and no counts.  Exact for integer-valued input below 2^53; reproducible bit for bit
    otherwise, and a trial's result does not depend on the other trials of the call."""
    t = _hip.require_gpu()
    x, one_d, as_numpy = _series(series, "fold_trials")
    nbin = int(nbin)
    if nbin < 2:
        raise ValueError("fold_trials: nbin must be >= 2")
    dphase, phase0, _ = _trial_phases(freqs, sample_time, ph0, x.device)
    rows, nf = x.shape[0], dphase.numel()
    if out is None:
        sums = t.zeros((rows, nf, nbin), dtype=t.float64, device=x.device)
        counts = t.zeros((nf, nbin), dtype=t.int64, device=x.device)
    else:
        sums, counts = out
        ok = (isinstance(sums, t.Tensor) and isinstance(counts, t.Tensor) and sums.dtype == t.float64
              and counts.dtype == t.int64 and tuple(sums.shape) == (rows, nf, nbin)
              and tuple(counts.shape) == (nf, nbin) and sums.is_contiguous() and counts.is_contiguous()
              and sums.device == x.device and counts.device == x.device)
        if not ok:
            raise ValueError(f"fold_trials: out must be contiguous float64 ({rows}, {nf}, {nbin}) and int64 "
                             f"({nf}, {nbin}) tensors on {x.device}")
    _fold_trials_device(x, dphase, phase0, nbin, first_sample, sums, counts)
    if out is not None:
        return sums, counts
    if one_d:
        sums = sums[0]
    if as_numpy:
        return sums.cpu().numpy(), counts.cpu().numpy()
    return sums, counts


def _profile_chi2_device(sums, counts, mean, var):
    """pu_profile_chi2 of contiguous device ``sums`` (rows, F, nbin) / ``counts`` (F, nbin) ->
    (chi2 (rows, F) float64, dof (F,) int32) tensors."""
    t = _hip.torch()
    rows, nf, nbin = sums.shape
    chi2 = t.empty((rows, nf), dtype=t.float64, device=sums.device)
    dof = t.empty(nf, dtype=t.int32, device=sums.device)
    _hip.check(_hip.lib().pu_profile_chi2(_hip.ptr(sums), sums.stride(1), sums.stride(0), _hip.ptr(counts), rows, nf,
                                          nbin, _hip.ptr(mean), _hip.ptr(var), _hip.ptr(chi2), _hip.ptr(dof),
                                          _hip.stream_ptr()), "pu_profile_chi2")
    return chi2, dof


def frequency_search(series, sample_time, freqs=None, fmin=None, fmax=None, nbin=32, oversample=8, chunksize=None):
    """Epoch-folding search for a pulse frequency: fold ``series`` at every trial frequency and
    score each profile with the chi^2 against a constant (Leahy et al. 1983; ``pu_profile_chi2``).

    ``series``: one dedispersed series (1-D) or a plane of them (ndm, n), e.g. the plane of
    ``dedispersion_search(show=True)``.  ``freqs``: the trials in Hz, or ``fmin`` and ``fmax``
    for ``frequency_grid(fmin, fmax, n * sample_time, oversample)``.  Each row's mean and
    variance are the population ones, ``var = E[x^2] - E[x]^2`` from float64 row sums, as
    ``get_spectral_stats`` computes them.  ``chunksize``: fold the series that many samples at
    a time (the partial sums of a call grow with its length).

    Returns a table with one row per frequency: ``freq``, ``chi2``, ``dof`` for a 1-D series;
    for a plane ``chi2`` is (F, ndm) and ``best_row``, ``best_chi2`` give the row with the
    largest chi^2 at each frequency (a NaN chi^2 never wins).  The peak is
    ``table['freq'][np.nanargmax(table['chi2'])]`` (``best_chi2`` for a plane)."""
    from .stats import _chunk_row_sums
    from .table import make_table
    t = _hip.require_gpu()
    x, one_d, _ = _series(series, "frequency_search")
    rows, n = x.shape
    nbin = int(nbin)
    if nbin < 2:
        raise ValueError("frequency_search: nbin must be >= 2")
    if n < 1:
        raise ValueError("frequency_search: an empty series")
    if freqs is None:
        if fmin is None or fmax is None:
            raise ValueError("frequency_search: give freqs, or fmin and fmax")
        freqs = frequency_grid(fmin, fmax, n * float(sample_time), oversample)
    if chunksize is None:
        chunksize = n
    chunksize = int(chunksize)
    if chunksize < 1:
        raise ValueError("frequency_search: chunksize must be positive")
    dphase, phase0, freq = _trial_phases(freqs, sample_time, 0.0, x.device)
    nf = dphase.numel()
    sums = t.zeros((rows, nf, nbin), dtype=t.float64, device=x.device)
    counts = t.zeros((nf, nbin), dtype=t.int64, device=x.device)
    for i in range(0, n, chunksize):
        _fold_trials_device(x[:, i:i + chunksize], dphase, phase0, nbin, i, sums, counts)
    mean = _chunk_row_sums(x, 3) / float(n)
    var = _chunk_row_sums(x, 4) / float(n) - mean * mean
    chi2, dof = _profile_chi2_device(sums, counts, mean, var)
    chi2, dof = chi2.cpu().numpy(), dof.cpu().numpy()
    if one_d:
        return make_table({"freq": freq, "chi2": chi2[0], "dof": dof})
    by_freq = np.ascontiguousarray(chi2.T)
    filled = np.where(np.isnan(by_freq), -np.inf, by_freq)
    best = np.argmax(filled, axis=1) if rows else np.zeros(nf, np.int64)
    return make_table({"freq": freq, "chi2": by_freq, "dof": dof, "best_row": best,
                       "best_chi2": by_freq[np.arange(nf), best] if rows else np.full(nf, np.nan)})


__all__ = ["fold_bins", "fold", "fold_file", "z_n_all", "h_test", "h_curve", "profile_stats", "frequency_grid",
           "fold_trials", "frequency_search"]
