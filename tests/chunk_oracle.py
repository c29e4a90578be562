"""Host restatement of the file path (reference stats.py:35-90 and clean.py:276-351): the
spectra and the channel mask of a SIGPROC file, the chunk list of search_by_chunks and, per
chunk, the cleaned plane and its search table from the numpy / C oracle.

Test infrastructure only.  Nothing here imports ``pulsarutils.clean`` or ``pulsarutils.stats``
(the code under test): the file is read with the host ``FilReader.readBlock``, the trial grid
comes from the host planner, every array step from ``oracle``.  tests/test_chunk_oracle.py
pins these functions against the goldens."""
import numpy as np
from scipy.signal import medfilt

import oracle
from oracle import clean_oracle as co
from pulsarutils import _planner, sigproc


NCH, TSAMP = 64, 2e-4
MAIN = dict(ns=20000, fch1=1500.0, foff=-300.0 / NCH)   # step 3610: 11 chunks, a 1950-sample tail
UP = dict(ns=2000, fch1=1200.0, foff=300.0 / NCH)       # foff > 0: the 128-sample minimum step
PULSE_DM, PULSE_T = 300.0, 9000


def write_pulse_file(fname, kind="u8", ns=20000, fch1=1500.0, foff=-300.0 / NCH):
    """The file of test_gpu_files.test_search_by_chunks_finds_pulse: ``rint(N(60, 6))`` noise
    (seed 21) in 64 channels at ``tsamp = 2e-4`` with, when the file holds t = 9000, a pulse of
    +40 counts per channel at DM 300 there.  ``kind``: ``u8``; ``u16``: the same samples x 200
    (so they exceed 255); ``f32``: the same samples as float32."""
    rng = np.random.default_rng(21)
    x = np.clip(np.rint(rng.standard_normal((ns, NCH)) * 6 + 60), 0, 255)
    if ns > PULSE_T:
        ftop = fch1 - 0.5 * foff
        fbottom = ftop + foff * NCH
        sh = _planner.dedispersion_shifts(NCH, PULSE_DM, fbottom, abs(foff) * NCH, TSAMP).astype(int)
        for c in range(NCH):
            x[(PULSE_T + sh[c]) % ns, NCH - 1 - c if foff < 0 else c] += 40
    x = np.clip(x, 0, 255).astype(np.uint8)
    x = {"u8": x, "u16": x.astype(np.uint16) * np.uint16(200), "f32": x.astype(np.float32)}[kind]
    sigproc.write_filterbank(fname, x, fch1=fch1, foff=foff, tsamp=TSAMP)
    return x


def count_ties(width_snr, rtol):
    """The tie rule of test_gpu_dedisperse.test_search_full_size_all_trials: the trials whose
    best and second-best width S/N are within ``rtol`` of each other (boolean mask)."""
    srt = np.sort(width_snr, axis=1)
    return (srt[:, -1] - srt[:, -2]) <= rtol * np.abs(srt[:, -1])


def spectral_stats(fname, chunksize=10000):
    """stats.py:35-60: per-channel mean and std, summed chunk by chunk from ``0.``."""
    fil = sigproc.FilReader(fname)
    nsamples = fil.header["nsamples"]
    spectrum = 0.
    spectrsq = 0.
    for istart in range(0, nsamples, chunksize):
        size = min(chunksize, nsamples - istart)
        array = fil.readBlock(istart, size)
        spectrum += array.astype(float).sum(1)
        spectrsq += (array.astype(float) ** 2).sum(1)
    mean_spec = spectrum / nsamples
    mean_spectrsq = spectrsq / nsamples
    return mean_spec, np.sqrt(mean_spectrsq - mean_spec ** 2)


def bad_chans(fname, chunksize=10000):
    """stats.py:63-90 without the cache file: medfilt(11) + 4 ref_mad on both spectra."""
    mean_spec, std_spec = spectral_stats(fname, chunksize)
    badchans = np.zeros(mean_spec.size, dtype=bool)
    for spec in (mean_spec, std_spec):
        badchans = badchans | (spec > medfilt(spec, 11) + 4 * co.ref_mad(spec))
    return badchans


def chunk_list(nsamples, tsamp, fbottom, ftop, dmmax, chunk_length=None, tmin=0):
    """The loop of clean.py:296-326: ``(step, [(istart, iend), ...])`` of the searched chunks."""
    if chunk_length is None:
        chunk_length = _planner.delta_delay(dmmax, fbottom, ftop)
    step = max(int(chunk_length / tsamp) * 2, 128)
    chunks = []
    for istart in range(0, nsamples, step // 2):
        chunk_size = min(step, nsamples - istart)
        if istart * tsamp < tmin:
            continue
        if chunk_size < step // 2:
            continue
        chunks.append((istart, istart + chunk_size))
    return step, chunks


def resample_factor(header, dmmin, new_sample_time=None):
    """clean.py:303-315: ``(N, new_sample_time)``; the default sample time is a tenth of the
    smearing of ``dmmin`` in the lowest channel (clean.py:272-273), at least ``tsamp``."""
    tsamp = header["tsamp"]
    dm_dt = 8300 * dmmin * np.abs(header["foff"]) / header["fbottom"] ** 3
    if new_sample_time is None:
        new_sample_time = max(dm_dt / 10, tsamp)
    sampl_ratio = new_sample_time / tsamp
    N = 1
    if sampl_ratio >= 2:
        N = int(np.rint(sampl_ratio))
        new_sample_time = N * tsamp
    return N, new_sample_time


def expected_chunks(fname, dmmin, dmmax, new_sample_time=None, tmin=0, surelybad=(), zero_dm=False,
                    chunk_length=None, search_dtype="f64"):
    """Per searched chunk ``(istart, iend, plane64, dms, (max, std, snr, rebin), width_snr)``:
    the plane is clean_oracle.renormalize of readBlock, flipped when ``foff < 0`` and resampled
    when ``N >= 2`` (clean.py:327-336); the table is oracle.search of it (of its float32 cast
    for ``search_dtype='f32'``) on the planner's grid at ``N * tsamp``."""
    fil = sigproc.FilReader(fname)
    h = fil.header
    mask = bad_chans(fname)
    for c in surelybad:
        mask[c] = True
    _, chunks = chunk_list(h["nsamples"], h["tsamp"], h["fbottom"], h["ftop"], dmmax, chunk_length, tmin)
    N, new_sample_time = resample_factor(h, dmmin, new_sample_time)
    dms = _planner.dedispersion_plan(h["nchans"], dmmin, dmmax, h["fbottom"], h["bandwidth"], new_sample_time)
    out = []
    for istart, iend in chunks:
        plane = co.renormalize(fil.readBlock(istart, iend - istart), badchans_mask=mask, zero_dm=zero_dm)
        if h["foff"] < 0:
            plane = plane[::-1]
        if N >= 2:
            plane = co.quick_resample(plane, N)
        plane = np.ascontiguousarray(plane)
        searched = plane.astype(np.float32) if search_dtype == "f32" else plane
        mx, sd, snr, win, wsnr = oracle.search(searched, dms, h["fbottom"], h["bandwidth"], new_sample_time,
                                               return_width_snr=True)
        out.append((istart, iend, plane, dms, (mx, sd, snr, win), wsnr))
    return out
