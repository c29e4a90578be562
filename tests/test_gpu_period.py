"""pu_fold_trials and pu_profile_chi2 on the GPU against the host restatement
(tests/period_oracle.py, pinned by tests/test_period_oracle.py), and folding.fold_trials /
frequency_search end to end on a synthetic pulsar."""
import functools
import math

import numpy as np
import pytest

import period_oracle as po

pytestmark = pytest.mark.gpu

# the tiling of csrc/fold_trials.hip: the segment of one partial, the sub-block staged in LDS, the
# largest nbin; a trial tile is 256 trials up to nbin 64, 128 up to 128, 64 up to 256
S, SUB, MAX_NBIN = 16384, 2048, 256
U = 2.0 ** -53
DTYPES = {"f32": np.float32, "f64": np.float64}


def trial_list(nbin, ntrials):
    """(dphase, phase0) of ``ntrials`` trials: the fixed mix first (dphase 0, on the bin edges,
    whole and one-and-a-half turns per sample, the search regime, backwards, dphase nbin just
    below and just above 1, a non-zero phase0, two identical trials), then search-regime trials
    of ever longer runs with phases all over the turn."""
    edge = 1.0 / nbin
    mix = [(1e-4, 0.0), (0.0, 0.3), (0.125, 0.0), (1.0, 0.25), (1.5, -0.37), (-0.013, 0.0),
           (edge * (1 - 2.0 ** -30), 0.0), (edge * (1 + 2.0 ** -30), 0.6), (1e-4, 0.0), (0.125, 0.0)]
    more = [(1.0 / (nbin * (1.7 + 0.61 * j)), (0.137 * j) % 1.0 - 0.5) for j in range(max(0, ntrials - len(mix)))]
    tr = (mix + more)[:ntrials]
    return np.array([t[0] for t in tr]), np.array([t[1] for t in tr])


# (rows, n, ntrials, nbin, first_sample): every n, ntrials, nbin, rows and first_sample of the list
# at least once, each tile class (4, 2, 1 waves) on both sides of its nbin threshold, and a
# trial list longer than the widest tile
CASES = [
    (1, 1, 1, 2, 0),
    (3, 63, 64, 16, 12345),
    (1, S - 1, 70, 33, 0),
    (3, S + 1, 70, 16, 12345),
    (1, 2 * S + 777, 70, MAX_NBIN, 12345),
    (3, 2 * S + 777, 64, 2, 0),
    (1, S + 1, 1, MAX_NBIN, 0),
    (3, 63, 70, MAX_NBIN, 0),
    (1, 2 * S + 777, 64, 33, 0),
    (3, S - 1, 1, 16, 12345),
    (1, SUB + 1, 70, 64, 0), (1, SUB + 1, 70, 65, 0),
    (1, SUB - 1, 130, 128, 12345), (1, SUB + 1, 70, 129, 0),
    (2, 1000, 300, 16, 0),
    (1, 1000, 70, 16, 2 ** 53 - 500),   # sample indices up to 2^53: the index is converted, not incremented
    # nbin 72: the widest 256-trial tile, so both kernels' dynamic LDS is above 64 KiB (fold 160 KiB,
    # counts 72 KiB: nbin 65 above does that for the incrementing instances, this for the converting ones)
    (1, 1000, 70, 72, 2 ** 53 - 500),
]


def case_id(c):
    return "r%d-n%d-k%d-b%d-%s" % (c[0], c[1], c[2], c[3], "0" if not c[4] else "far" if c[4] > 2 ** 40 else "off")


@functools.lru_cache(maxsize=None)
def series(rows, n, kind):
    """float32-representable rows (so float32 and float64 input share one oracle): small integers,
    or Gaussian 8 N + 3."""
    rng = np.random.default_rng(1000 * rows + n)
    if kind == "int":
        x = rng.integers(-200, 200, (rows, n)).astype(np.float64)
    else:
        x = (rng.standard_normal((rows, n)) * 8 + 3).astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want(case, kind):
    rows, n, ntrials, nbin, first = case
    dph, ph0 = trial_list(nbin, ntrials)
    return po.fold_trials(series(rows, n, kind), dph, nbin, ph0, first, exact=kind == "int")


def device_rows(gpu, x, dtype, pad=5, lead=3):
    """``x`` as a view of a wider device tensor: rows ``n + pad`` apart, the first one ``lead``
    elements into the buffer (an odd address); the padding is NaN that must not reach a sum."""
    import torch
    rows, n = x.shape
    wide = torch.full((rows * (n + pad) + lead,), float("nan"), dtype=getattr(torch, np.dtype(dtype).name), device=gpu)
    view = wide[lead:].view(rows, n + pad)[:, :n]
    view.copy_(torch.from_numpy(np.array(x, dtype=dtype)).to(gpu))
    return view


def raw_trials(x, dph, ph0, nbin, first, out=None):
    """pu_fold_trials called directly on a 2-D device view -> (sums (rows, F, nbin), counts (F,
    nbin)) numpy, and the device tensors.  ``ph0`` None passes a NULL phase0.  The outputs are
    padded (ld_trial = nbin + 3, ld_row = F ld_trial + 5): the padding must stay untouched."""
    import torch
    from pulsarutils import _hip
    lib = _hip.lib()
    rows, n = x.shape
    dev = x.device
    nf = len(dph)
    ldt, ldr = nbin + 3, nf * (nbin + 3) + 5
    if out is None:
        out = (torch.zeros(rows * ldr, dtype=torch.float64, device=dev), torch.zeros((nf, nbin), dtype=torch.int64, device=dev))
    sums, counts = out
    d = torch.from_numpy(np.ascontiguousarray(dph, dtype=np.float64)).to(dev)
    p = None if ph0 is None else torch.from_numpy(np.ascontiguousarray(ph0, dtype=np.float64)).to(dev)
    wsb = lib.pu_fold_trials_workspace_bytes(rows, n, nf, nbin)
    ws = torch.empty(max(16, wsb), dtype=torch.uint8, device=dev)
    ld = x.stride(0) if rows > 1 else max(x.stride(0), n)
    rc = lib.pu_fold_trials(_hip.ptr(x), _hip.dtype_code(x.dtype), rows, n, ld, first, _hip.ptr(p), _hip.ptr(d), nf, nbin,
                            _hip.ptr(sums), ldt, ldr, _hip.ptr(counts), _hip.ptr(ws), wsb, _hip.stream_ptr())
    assert rc == 0, lib.pu_last_error().decode()
    s = sums.cpu().numpy().reshape(rows, ldr)
    assert not s[:, nf * ldt:].any()
    s = s[:, :nf * ldt].reshape(rows, nf, ldt)
    assert not s[:, :, nbin:].any()
    return np.ascontiguousarray(s[:, :, :nbin]), counts.cpu().numpy(), out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_float(got, want_sums, counts, abs_sums, extra_terms=0):
    """Each entry within 2 (m + extra) 2^-53 sum|x| of the exactly rounded sum: the bound of any
    summation order of m terms, doubled for the oracle's final rounding."""
    bound = 2.0 * (counts[None] + extra_terms) * U * abs_sums
    err = np.abs(got - want_sums)
    assert (err <= bound).all(), (float(err.max()), float(bound[err > bound].min()))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fold_trials_matches_the_oracle(gpu, case, kind, dtype):
    rows, n, ntrials, nbin, first = case
    dph, ph0 = trial_list(nbin, ntrials)
    x = device_rows(gpu, series(rows, n, kind), DTYPES[dtype])
    wsums, wcounts, wabs = want(case, kind)
    got, counts, _ = raw_trials(x, dph, ph0, nbin, first)
    assert np.array_equal(counts, wcounts)
    # (far from 0 the faster trials reach a phase of 2^52: NaN, no counts)
    good = np.array([not po.trial_is_bad(n, dph[k], ph0[k], first) for k in range(ntrials)])
    assert good.all() or first > 2 ** 40
    assert counts.sum(axis=1).tolist() == [n if g else 0 for g in good]
    assert np.isnan(got[:, ~good]).all()
    if kind == "int":
        assert np.array_equal(got[:, good], wsums[:, good])
    else:
        check_float(got[:, good], wsums[:, good], wcounts[good], wabs[:, good])


def test_a_null_phase0_is_zero_for_every_trial(gpu):
    x = device_rows(gpu, series(3, S + 1, "gauss"), np.float32)
    dph, _ = trial_list(16, 70)
    a, ca, _ = raw_trials(x, dph, None, 16, 12345)
    b, cb, _ = raw_trials(x, dph, np.zeros(70), 16, 12345)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(ca, cb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_trial_does_not_depend_on_the_rest_of_the_call(gpu, dtype):
    rows, n, ntrials, nbin, first = 3, S + 1, 70, 16, 12345
    dph, ph0 = trial_list(nbin, ntrials)
    x = device_rows(gpu, series(rows, n, "gauss"), DTYPES[dtype])
    full, cfull, _ = raw_trials(x, dph, ph0, nbin, first)
    again, cagain, _ = raw_trials(x, dph, ph0, nbin, first)
    assert np.array_equal(bits(full), bits(again)) and np.array_equal(cfull, cagain)
    for k in (0, 4, 7, 69):  # alone
        one, cone, _ = raw_trials(x, dph[k:k + 1], ph0[k:k + 1], nbin, first)
        assert np.array_equal(bits(one[:, 0]), bits(full[:, k])) and np.array_equal(cone[0], cfull[k])
    rev, crev, _ = raw_trials(x, dph[::-1], ph0[::-1], nbin, first)  # at another position
    assert np.array_equal(bits(rev[:, ::-1]), bits(full)) and np.array_equal(crev[::-1], cfull)
    x1 = device_rows(gpu, series(rows, n, "gauss")[:1], DTYPES[dtype])  # rows = 1 against rows = 3
    row0, c0, _ = raw_trials(x1, dph, ph0, nbin, first)
    assert np.array_equal(bits(row0[0]), bits(full[0])) and np.array_equal(c0, cfull)
    # the two identical trials of the list
    assert np.array_equal(bits(full[:, 0]), bits(full[:, 8])) and np.array_equal(bits(full[:, 2]), bits(full[:, 9]))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_fold_trials_accumulates_over_chunks(gpu, kind, dtype):
    case = (1, 2 * S + 777, 64, 33, 0)
    rows, n, ntrials, nbin, _ = case
    first = 12345
    dph, ph0 = trial_list(nbin, ntrials)
    xh = series(rows, n, kind)
    wsums, wcounts, wabs = po.fold_trials(xh, dph, nbin, ph0, first, exact=kind == "int")
    cuts = [0, 5000, 5000 + S + 3, n]
    out = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        got, counts, out = raw_trials(device_rows(gpu, xh[:, a:b], DTYPES[dtype]), dph, ph0, nbin, first + a, out=out)
    assert np.array_equal(counts, wcounts)
    if kind == "int":
        one, _, _ = raw_trials(device_rows(gpu, xh, DTYPES[dtype]), dph, ph0, nbin, first)
        assert np.array_equal(got, wsums) and np.array_equal(got, one)
    else:
        # three calls, each within its own m_i u S_i, and the adds of the second and the third
        # into sums: two more roundings of at most u S each
        check_float(got, wsums, wcounts, wabs, extra_terms=2)


def test_a_trial_that_cannot_be_binned_is_nan_and_counts_nothing(gpu):
    import torch
    rows, n, nbin, first = 2, SUB + 5, 16, 12345
    xh = series(rows, n, "int")
    # trial 4 reaches 2^52 at the chunk's end only, trial 5 starts there
    dph = np.array([0.013, math.inf, 0.013, math.nan, 2.0 ** 52 / 14000, 0.02, 1e-3, 1e-3])
    ph0 = np.array([0.0, 0.0, 0.2, 0.0, 0.0, 2.0 ** 52, math.nan, 0.5])
    bad = [1, 3, 4, 5, 6]
    assert [k for k in range(8) if po.trial_is_bad(n, dph[k], ph0[k], first)] == bad
    wsums, wcounts, _ = po.fold_trials(xh, dph, nbin, ph0, first, exact=True)
    ldr = 8 * (nbin + 3) + 5
    out = (torch.zeros(rows * ldr, dtype=torch.float64, device=gpu), torch.full((8, nbin), 7, dtype=torch.int64, device=gpu))
    got, counts, _ = raw_trials(device_rows(gpu, xh, np.float64), dph, ph0, nbin, first, out=out)
    for k in range(8):
        if k in bad:
            assert np.isnan(got[:, k]).all() and (counts[k] == 7).all()
        else:
            assert np.array_equal(got[:, k], wsums[:, k]) and np.array_equal(counts[k], wcounts[k] + 7)


# ------------------------------------------------------------------ pu_profile_chi2

def raw_chi2(gpu, sums, counts, mean, var):
    import torch
    from pulsarutils import _hip
    lib = _hip.lib()
    rows, nf, nbin = sums.shape
    s = torch.from_numpy(np.ascontiguousarray(sums)).to(gpu)
    c = torch.from_numpy(np.ascontiguousarray(counts)).to(gpu)
    m = torch.from_numpy(np.asarray(mean, dtype=np.float64)).to(gpu)
    v = torch.from_numpy(np.asarray(var, dtype=np.float64)).to(gpu)
    chi2 = torch.full((rows * nf + 2,), -7.0, dtype=torch.float64, device=gpu)
    dof = torch.full((nf + 2,), -7, dtype=torch.int32, device=gpu)
    rc = lib.pu_profile_chi2(_hip.ptr(s), nbin, nf * nbin, _hip.ptr(c), rows, nf, nbin, _hip.ptr(m), _hip.ptr(v),
                             _hip.ptr(chi2), _hip.ptr(dof), _hip.stream_ptr())
    assert rc == 0, lib.pu_last_error().decode()
    chi2, dof = chi2.cpu().numpy(), dof.cpu().numpy()
    assert (chi2[rows * nf:] == -7.0).all() and (dof[nf:] == -7).all()
    return chi2[:rows * nf].reshape(rows, nf), dof[:nf]


@pytest.mark.parametrize("case", [CASES[3], CASES[7], CASES[8]], ids=case_id)
def test_profile_chi2_matches_the_oracle(gpu, case):
    """On the device's own sums (read back), so device and oracle score the same profiles; the
    trial list has dphase = 0 (one bin hit: dof 0) and, at nbin 256 over 63 samples, many empty
    bins.  Row 0 gets var = 0: NaN."""
    rows, n, ntrials, nbin, first = case
    dph, ph0 = trial_list(nbin, ntrials)
    xh = series(rows, n, "gauss")
    sums, counts, _ = raw_trials(device_rows(gpu, xh, np.float64), dph, ph0, nbin, first)
    mean = xh.mean(axis=1)
    var = xh.var(axis=1)
    if rows > 1:
        var[0] = 0.0
    got, dof = raw_chi2(gpu, sums, counts, mean, var)
    wchi2, wdof = po.chi2_all(sums, counts, mean, var)
    assert np.array_equal(dof, wdof) and dof[1] == 0 and dof.max() <= nbin - 1
    for r in range(rows):
        if not var[r] > 0:
            assert np.isnan(got[r]).all() and np.isnan(wchi2[r]).all()
            continue
        for k in range(ntrials):
            tol = po.chi2_tolerance(nbin, sums[r, k], counts[k], mean[r], var[r])
            assert abs(got[r, k] - wchi2[r, k]) <= tol, (r, k, got[r, k], wchi2[r, k], tol)


def test_profile_chi2_of_nan_sums_is_nan(gpu):
    sums = np.ones((1, 3, 4))
    sums[0, 1, 2] = np.inf
    sums[0, 2] = np.nan
    counts = np.array([[2, 2, 2, 2], [2, 2, 2, 2], [0, 0, 0, 0]], np.int64)
    got, dof = raw_chi2(gpu, sums, counts, [0.5], [1.0])
    assert got[0, 0] == 0.0 and math.isnan(got[0, 1]) and math.isnan(got[0, 2]) and dof.tolist() == [3, 3, -1]


# ------------------------------------------------------------------ end to end

N, TSAMP, F0, NBIN, AMP = 40000, 1e-3, 7.3, 32, 2.0


@functools.lru_cache(maxsize=None)
def pulsar_plane():
    """Two rows of seeded unit Gaussian noise; row 1 carries a 5-sample pulse of amplitude AMP
    every 1 / F0 s."""
    rng = np.random.default_rng(73)
    x = rng.standard_normal((2, N))
    starts = np.rint(np.arange(int(N * TSAMP * F0)) / (F0 * TSAMP)).astype(np.int64)
    for j in range(5):
        idx = starts + j
        x[1, idx[idx < N]] += AMP
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pulsar_want():
    """The oracle's chi2 (2, F) over frequency_grid(6.8, 7.8, tobs), written out here so that the
    oracle does not lean on the code under test, and the grid."""
    df = 1.0 / (8 * N * TSAMP)
    freqs = 6.8 + np.arange(int(np.ceil((7.8 - 6.8) / df)) + 1) * df
    x = pulsar_plane()
    sums, counts, _ = po.fold_trials(x, TSAMP * freqs, NBIN)
    mean = x.mean(axis=1)
    var = (x * x).mean(axis=1) - mean * mean
    return freqs, po.chi2_all(sums, counts, mean, var)[0]


def test_frequency_search_finds_the_pulsar(gpu):
    from pulsarutils import folding
    freqs, wchi2 = pulsar_want()
    peak = int(np.argmin(np.abs(freqs - F0)))
    # the input is valid whatever the device does: the oracle's peak is the grid point nearest F0,
    # a fifth clear of the runner-up and far above the noise rows
    assert int(np.argmax(wchi2[1])) == peak
    assert np.sort(wchi2[1])[-2] < 0.8 * wchi2[1, peak] and wchi2[0].max() < 0.1 * wchi2[1, peak]
    grid = folding.frequency_grid(6.8, 7.8, N * TSAMP)
    assert np.array_equal(grid, freqs)
    x = np.array(pulsar_plane())  # (a writable copy: the cached plane is read-only)
    tab = folding.frequency_search(x[1], TSAMP, fmin=6.8, fmax=7.8, nbin=NBIN)
    assert list(tab.keys()) == ["freq", "chi2", "dof"] and np.array_equal(tab["freq"], freqs)
    assert int(np.argmax(tab["chi2"])) == peak and (np.asarray(tab["dof"]) == NBIN - 1).all()
    assert np.allclose(tab["chi2"], wchi2[1], rtol=1e-9, atol=0)
    tab = folding.frequency_search(x, TSAMP, freqs=freqs, nbin=NBIN)
    assert list(tab.keys()) == ["freq", "chi2", "dof", "best_row", "best_chi2"]
    chi2 = np.asarray(tab["chi2"])
    assert chi2.shape == (freqs.size, 2) and np.allclose(chi2, wchi2.T, rtol=1e-9, atol=0)
    best = np.asarray(tab["best_chi2"])
    assert int(np.argmax(best)) == peak and int(tab["best_row"][peak]) == 1
    assert np.array_equal(best, chi2.max(axis=1)) and np.array_equal(tab["best_row"], chi2.argmax(axis=1))


# ------------------------------------------------------------------ API

def test_fold_trials_api_numpy_and_tensor(gpu):
    import torch
    from pulsarutils import folding
    x = np.array(series(2, 1000, "int"))
    freqs = np.array([15.625, 3.0, 125.0])
    wsums, wcounts, _ = po.fold_trials(x, 1e-3 * freqs, 64, [0.25] * 3, 7, exact=True)
    s, c = folding.fold_trials(x, freqs, 1e-3, 64, ph0=0.25, first_sample=7)
    assert isinstance(s, np.ndarray) and s.shape == (2, 3, 64) and np.array_equal(s, wsums)
    assert c.dtype == np.int64 and np.array_equal(c, wcounts)
    s1, c1 = folding.fold_trials(x[0].astype(np.float32), freqs, 1e-3, 64, ph0=0.25, first_sample=7)
    assert s1.shape == (3, 64) and np.array_equal(s1, wsums[0]) and np.array_equal(c1, wcounts)
    s2, _ = folding.fold_trials(x[0].astype(np.int16), freqs[1], 1e-3, 64, ph0=0.25, first_sample=7)  # folded as float64
    assert s2.shape == (1, 64) and np.array_equal(s2[0], wsums[0, 1])
    sp, _ = folding.fold_trials(x, freqs, 1e-3, 64, ph0=[0.25, 0.25, 0.25], first_sample=7)  # a phase per trial
    assert np.array_equal(sp, wsums)
    xd = torch.from_numpy(np.array(x)).to(gpu)
    sd, cd = folding.fold_trials(xd, torch.from_numpy(freqs).to(gpu), 1e-3, 64, ph0=0.25, first_sample=7)
    assert sd.is_cuda and cd.is_cuda and cd.dtype == torch.int64 and np.array_equal(sd.cpu().numpy(), wsums)
    out = folding.fold_trials(xd, freqs, 1e-3, 64, ph0=0.25, first_sample=7, out=(sd, cd))
    assert out[0] is sd and out[1] is cd
    assert np.array_equal(sd.cpu().numpy(), 2 * wsums) and np.array_equal(cd.cpu().numpy(), 2 * wcounts)
    for bad in ((sd[:1], cd), (sd, cd[:2]), (sd.to(torch.float32), cd), (sd, cd.to(torch.int32)), (sd.cpu(), cd.cpu()),
                (sd.transpose(0, 1).contiguous().transpose(0, 1), cd), (sd.cpu().numpy(), cd.cpu().numpy())):
        with pytest.raises(ValueError):
            folding.fold_trials(xd, freqs, 1e-3, 64, out=bad)
    for kw in (dict(nbin=1), dict(nbin=257)):
        with pytest.raises(ValueError):
            folding.fold_trials(x, freqs, 1e-3, **kw)
    with pytest.raises(ValueError):
        folding.fold_trials(np.zeros((2, 3, 4)), freqs, 1e-3, 8)


def test_frequency_search_in_chunks_is_the_one_call_search(gpu):
    import torch
    from pulsarutils import folding
    x = np.array(series(2, 2 * S + 777, "int"))
    freqs = folding.frequency_grid(3.0, 3.5, 40.0)
    one = folding.frequency_search(x, 1e-3, freqs=freqs, nbin=16)
    for chunksize in (5000, S, 2 * S + 776):
        part = folding.frequency_search(x, 1e-3, freqs=freqs, nbin=16, chunksize=chunksize)
        for col in ("freq", "chi2", "dof", "best_row", "best_chi2"):
            assert np.array_equal(bits(np.asarray(one[col], dtype=np.float64)), bits(np.asarray(part[col], dtype=np.float64))), col
    dev = folding.frequency_search(torch.from_numpy(np.array(x[0])).to(gpu), 1e-3, freqs=freqs, nbin=16)
    assert np.array_equal(np.asarray(dev["chi2"]), np.asarray(one["chi2"])[:, 0])
    with pytest.raises(ValueError):
        folding.frequency_search(x, 1e-3, nbin=16)            # neither freqs nor fmin / fmax
    with pytest.raises(ValueError):
        folding.frequency_search(x, 1e-3, freqs=freqs, nbin=16, chunksize=0)
