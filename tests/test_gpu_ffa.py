"""pu_ffa on the GPU against tests/ffa_oracle.py: the transform bit for bit on both sides of the
LDS / global split, padded layouts, batch independence, the S/N within the header's bound, and the
search drivers end to end."""
import ctypes
import functools

import numpy as np
import pytest

import ffa_oracle as fo
from pulsarutils import _hip, ffa

pytestmark = pytest.mark.gpu

NAN32 = np.float32(np.nan)


def run_ffa(dev, x, m, p, want_out=True, widths=None, sigma=None, want_peak=True, pad_in=7, pad_out=5, nan_rows=()):
    """pu_ffa through the C ABI on rows ``x`` (rows, m p) with ld > m p, ld_out_row > m p and NaN in
    the input padding, the out padding and the whole workspace; checks that the padding survives.
    ``nan_rows``: rows whose samples hold a non-finite value, exempt from the "no NaN" asserts.
    Returns (out (rows, m, p) or None, snr, peak (rows, m, nw) or None)."""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, mp = x.shape
    assert mp == m * p
    clean = np.setdiff1d(np.arange(rows), np.asarray(nan_rows, dtype=np.int64))
    nw = 0 if widths is None else len(widths)
    xin = np.full((rows, mp + pad_in), NAN32, np.float32)
    xin[:, :mp] = x
    xd = torch.from_numpy(xin).to(dev)
    out = torch.full((rows, mp + pad_out), float("nan"), dtype=torch.float32, device=dev) if want_out else None
    snr = torch.full((rows, m, nw), float("nan"), dtype=torch.float32, device=dev) if nw else None
    peak = torch.full((rows, m, nw), -1, dtype=torch.int32, device=dev) if nw and want_peak else None
    need = ffa.describe(rows, m, p, nw, want_out)["workspace_bytes"]
    buf, wp, wsb = _hip.workspace(need, dev)
    buf.fill_(255)  # every float32 of it a NaN
    w = np.ascontiguousarray(widths if nw else [0], dtype=np.int32)
    sg = torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64)).to(dev) if sigma is not None else None
    _hip.check(_hip.lib().pu_ffa(_hip.ptr(xd), rows, mp + pad_in, m, p, _hip.ptr(out), mp + pad_out,
                                 w.ctypes.data_as(ctypes.c_void_p) if nw else None, nw, _hip.ptr(sg), _hip.ptr(snr),
                                 _hip.ptr(peak), wp, need, _hip.stream_ptr()), "pu_ffa")
    torch.cuda.synchronize()
    res = None
    if want_out:
        o = out.cpu().numpy()
        assert np.isnan(o[:, mp:]).all(), "out padding written"
        res = o[:, :mp].reshape(rows, m, p)
        assert not np.isnan(res[clean]).any(), "a NaN of the padding or the workspace reached out"
    assert np.isnan(xd.cpu().numpy()[:, mp:]).all()
    s = snr.cpu().numpy() if nw else None
    k = peak.cpu().numpy() if peak is not None else None
    if nw:
        assert not np.isnan(s[clean]).any(), "a NaN of the padding or the workspace reached snr"
        assert k is None or ((k >= 0) & (k < p)).all()
    return res, s, k


@functools.lru_cache(maxsize=None)
def gaussian_case(rows, m, p):
    """(rows of Gaussian float32, the oracle's transform of each), computed once per shape."""
    x = np.random.default_rng(1000 * m + p).standard_normal((rows, m * p)).astype(np.float32)
    want = np.stack([fo.ffa(r.reshape(m, p)) for r in x])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@functools.lru_cache(maxsize=None)
def integer_case(rows, m, p):
    x = np.random.default_rng(77 * m + p).integers(-200, 201, (rows, m * p)).astype(np.float32)
    want = np.stack([fo.ffa(r.reshape(m, p)) for r in x])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


B256 = 64  # the LDS block rows at p = 256 (asserted against pu_ffa_describe below)
CASES = [(1, 1, 2), (1, 2, 3), (3, 3, 4), (1, 5, 7), (2, 13, 33), (1, 64, 17),
         (1, B256 - 1, 256), (1, B256, 256), (1, B256 + 1, 256), (2, 2 * B256 + 1, 256),
         (1, 1000, 64), (1, 33, ffa.MAX_BINS), (1, 33, 1023), (3, 419, 250)]


def test_block_rows_of_the_cases():
    assert ffa.describe(1, 1, 256)["block_rows"] == B256
    assert ffa.describe(1, 33, ffa.MAX_BINS)["p_max"] == ffa.MAX_BINS
    assert ffa.describe(1, 1000, 64)["global_levels"] >= 2  # several global levels
    assert ffa.describe(1, 33, ffa.MAX_BINS)["global_levels"] >= 1 and ffa.describe(1, 33, 1023)["global_levels"] >= 1


@pytest.mark.parametrize("rows, m, p", CASES)
def test_transform_bits(gpu, rows, m, p):
    x, want = gaussian_case(rows, m, p)
    got, _, _ = run_ffa(gpu, x, m, p)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_signed_zero_and_single_row_copy(gpu):
    x = np.array([[-0.0, 0.0, 1.0, -2.0, -0.0, 3.0]], np.float32)  # m = 3, p = 2: row 0 is copied at the bottom level
    got, _, _ = run_ffa(gpu, x, 3, 2)
    assert np.array_equal(got[0].view(np.uint32), fo.ffa(x.reshape(3, 2)).view(np.uint32))
    got, _, _ = run_ffa(gpu, x[:, :2], 1, 2)
    assert np.array_equal(got[0].view(np.uint32), x[:, :2].view(np.uint32))


@pytest.mark.parametrize("rows, m, p", [(3, 2 * B256 + 1, 256), (3, 13, 33)])
def test_batch_independence_and_repeatability(gpu, rows, m, p):
    x, want = gaussian_case(rows, m, p)
    w = [1, 5, p - 1]
    out, snr, peak = run_ffa(gpu, x, m, p, widths=w)
    out2, snr2, peak2 = run_ffa(gpu, x, m, p, widths=w)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    assert np.array_equal(snr.view(np.uint32), snr2.view(np.uint32)) and np.array_equal(peak, peak2)
    _, fsnr, fpeak = run_ffa(gpu, x, m, p, want_out=False, widths=w)
    for r in range(rows):
        o1, s1, k1 = run_ffa(gpu, x[r:r + 1], m, p, widths=w)
        assert np.array_equal(o1[0].view(np.uint32), out[r].view(np.uint32))
        assert np.array_equal(s1[0].view(np.uint32), snr[r].view(np.uint32)) and np.array_equal(k1[0], peak[r])
        _, s1, k1 = run_ffa(gpu, x[r:r + 1], m, p, want_out=False, widths=w)
        assert np.array_equal(s1[0].view(np.uint32), fsnr[r].view(np.uint32)) and np.array_equal(k1[0], fpeak[r])


W16 = [1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 63, 100, 128, 200, 254, 255]


# all levels in LDS; one level above them (fused with the S/N); two (one pass, then the fused one)
@pytest.mark.parametrize("rows, m, p, widths", [(2, 37, 50, [1, 2, 7, 25, 49]), (1, B256 + 1, 256, W16),
                                                (2, 2 * B256 + 1, 256, W16)])
def test_snr_exact_on_integers(gpu, rows, m, p, widths):
    x, want = integer_case(rows, m, p)
    out, snr, peak = run_ffa(gpu, x, m, p, widths=widths)
    _, fsnr, fpeak = run_ffa(gpu, x, m, p, want_out=False, widths=widths)
    assert np.array_equal(out, want)
    assert np.array_equal(snr.view(np.uint32), fsnr.view(np.uint32)) and np.array_equal(peak, fpeak)
    _, nsnr, npeak = run_ffa(gpu, x, m, p, want_out=False, widths=widths, want_peak=False)
    assert npeak is None and np.array_equal(nsnr.view(np.uint32), fsnr.view(np.uint32))
    worst = 0.0
    for r in range(rows):
        for s in range(m):
            for k, w in enumerate(widths):
                exact, pk, _ = fo.snr_exact(want[r, s], w, m)
                ref = np.float32(exact)
                worst = max(worst, abs(float(fsnr[r, s, k]) - float(ref)) / float(np.spacing(np.abs(ref))))
                assert abs(np.float32(fsnr[r, s, k]) - ref) <= np.spacing(np.abs(ref)), (r, s, w)
                assert fpeak[r, s, k] == pk, (r, s, w)
    print("worst |snr - oracle| in float32 ulps:", worst)


def snr_bound(v, w, m, sigma, exact):
    """The header's bound on |snr - exact| and on the numerator, for profile v."""
    p = v.size
    num = 8.0 * p * 2.0 ** -53 * float(np.abs(v.astype(np.float64)).sum())
    return num / (np.sqrt(m * w * (1.0 - w / p)) * sigma) + 2.0 ** -23 * abs(exact), num


@pytest.mark.parametrize("rows, m, p, widths", [(1, 70, 100, [1, 3, 25, 99]), (1, B256 + 1, 256, [1, 4, 64, 255])])
def test_snr_within_the_bound_on_gaussian_rows(gpu, rows, m, p, widths):
    x, want = gaussian_case(rows, m, p)
    sigma = [1.25]
    for want_out in (True, False):
        _, snr, peak = run_ffa(gpu, x, m, p, want_out=want_out, widths=widths, sigma=sigma)
        worst = 0.0
        for s in range(m):
            for k, w in enumerate(widths):
                exact, _, sums = fo.snr_exact(want[0, s], w, m, sigma[0])
                tol, num = snr_bound(want[0, s], w, m, sigma[0], exact)
                worst = max(worst, abs(float(snr[0, s, k]) - exact) / tol)
                assert abs(float(snr[0, s, k]) - exact) <= tol, (s, w)
                assert sums.max() - sums[peak[0, s, k]] <= num, (s, w)
        print("worst |snr - exact| / bound:", worst)


def test_sigma_scales_the_snr(gpu):
    x, _ = gaussian_case(2, 13, 33)
    w = [1, 8, 32]
    _, one, pk1 = run_ffa(gpu, x, 13, 33, want_out=False, widths=w)
    _, sc, pk2 = run_ffa(gpu, x, 13, 33, want_out=False, widths=w, sigma=[2.0, 0.5])
    # a power of two scales the float64 quotient exactly, so the rounded float32 too
    assert np.array_equal(sc[0] * np.float32(2.0), one[0]) and np.array_equal(sc[1] * np.float32(0.5), one[1])
    assert np.array_equal(pk1, pk2)


def test_python_layer_shapes(gpu):
    import torch
    x, want = gaussian_case(2, 13, 33)
    series = np.concatenate((x, np.zeros((2, 5), np.float32)), axis=1)  # n = 13 * 33 + 5: the tail is not read
    out = ffa.ffa_transform(series, 33)
    assert isinstance(out, np.ndarray) and out.shape == (2, 13, 33) and np.array_equal(out, want)
    assert np.array_equal(ffa.ffa_transform(series[0], 33), want[0])
    snr, peak = ffa.ffa_snr(torch.from_numpy(series).to(gpu), 33, widths=[1, 4], sigma=[1.0, 2.0])
    assert snr.is_cuda and snr.shape == (2, 13, 2) and peak.dtype == torch.int32
    s1, _ = ffa.ffa_snr(series[1].astype(np.float64), 33, widths=[1, 4], sigma=2.0)
    assert s1.shape == (13, 2) and np.array_equal(s1, snr[1].cpu().numpy())
    assert ffa.ffa_snr(series[0], 33)[0].shape == (13, ffa.default_widths(33).size)
    with pytest.raises(ValueError):
        ffa.ffa_snr(series, 33, widths=[33])
    with pytest.raises(ValueError):
        ffa.ffa_transform(series, 4096)


N_SEARCH = 2 ** 17
P1, P2 = 250 + 137 / 418, 1300.4


@functools.lru_cache(maxsize=None)
def search_plane():
    plane = np.stack([fo.pulsar_series(N_SEARCH, P1, 0.02, 0.0, 20), fo.pulsar_series(N_SEARCH, P1, 0.02, 0.35, 21),
                      fo.pulsar_series(N_SEARCH, P2, 0.01, 0.8, 22)])
    plane.setflags(write=False)
    return plane


def test_search_end_to_end(gpu):
    tab = ffa.ffa_search(search_plane(), 1.0, 240.0, 1500.0, sigma=7.0)
    cols = {c: np.asarray(tab[c]) for c in ("period", "freq", "row", "snr", "width", "peak_phase", "dsfactor", "nabsorbed")}
    assert np.all(np.diff(cols["snr"]) <= 0) and np.all(cols["snr"] > 7.0)
    assert not np.any(cols["row"] == 0)  # nothing above 7 in the noise-only row
    for row, period, d in ((1, P1, 1), (2, P2, 5)):
        i = int(np.flatnonzero(cols["row"] == row)[0])  # the row's top candidate
        m = (N_SEARCH // d) // int(period / d)
        print("row", row, {c: v[i] for c, v in cols.items()}, "spacing", d / (m - 1))
        assert abs(cols["period"][i] - period) <= d / (m - 1)
        assert cols["dsfactor"][i] == d and cols["nabsorbed"][i] > 0
        assert cols["freq"][i] == 1.0 / cols["period"][i] and 0.0 <= cols["peak_phase"][i] < 1.0
        assert cols["snr"][i] > 12


def test_periodogram_is_ffa_snr_per_step(gpu):
    import torch
    from pulsarutils.dedispersion import quick_resample
    n = 2 ** 14
    row = fo.pulsar_series(n, 301.3, 0.02, 1.0, 5)
    per = ffa.ffa_periodogram(row, 0.5, 120.0, 250.0)
    plan = ffa.ffa_plan(n, 0.5, 120.0, 250.0)
    assert [d for d, _, _ in plan] == [1, 2]
    periods, snrs, wids, dsf = [], [], [], []
    for d, p0, p1 in plan:
        one = row.reshape(1, -1).copy()
        y = torch.from_numpy(quick_resample(one, d) if d > 1 else one.astype(np.float64)).to(gpu)
        y = y - y.mean(dim=1, keepdim=True)
        sd = y.std(dim=1, unbiased=False)
        z = y.to(torch.float32)
        for p in range(p0, p1):
            snr, _ = ffa.ffa_snr(z, p, sigma=sd)
            snr = snr[0, :-1].cpu().numpy()
            w = ffa.default_widths(p)
            periods.append(ffa.trial_periods(p, (n // d) // p, d * 0.5)[:-1])
            snrs.append(snr.max(axis=1))
            wids.append(w[snr.argmax(axis=1)] * d * 0.5)
            dsf.append(np.full(snr.shape[0], d))
    assert np.array_equal(per["period"], np.concatenate(periods))
    assert np.array_equal(per["snr"], np.concatenate(snrs)) and per["snr"].dtype == np.float32
    assert np.array_equal(per["width"], np.concatenate(wids))
    assert np.array_equal(per["dsfactor"], np.concatenate(dsf))
    best = int(np.argmax(per["snr"]))
    assert abs(per["period"][best] - 301.3 * 0.5) < 0.1 and per["snr"][best] > 12
