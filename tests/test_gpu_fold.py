"""pu_fold and pu_h_test on the GPU against the host restatement (tests/fold_oracle.py, pinned by
tests/test_fold_oracle.py), and the file path end to end: fold_file -> clean.dedispersion_search
-> h_curve / profile_stats on a synthetic 8-bit pulsar."""
import functools
import math

import numpy as np
import pytest

import fold_oracle as fo

pytestmark = pytest.mark.gpu

# the tiling of csrc/fold.hip: a lane's piece (8-bit path), a wave's group (float path), the
# sub-block whose bins are staged in LDS, the segment of one partial
PIECE, GROUP, SUB, SEG = 16, 64, 2048, 16384
U = 2.0 ** -53
DTYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}

# (nchan, n, nbin, dphase, phase0, first_sample)
FOLD_CASES = [
    (1, 1, 1, 0.013, -0.37, 0),
    (3, 63, 2, 0.013, -0.37, 2 ** 40),
    (3, 1000, 64, 1.0 / 1000, -0.37, 2 ** 40),         # dphase nbin = 0.064: 15 samples per bin
    (65, 1000, 64, 1.0 / 64.3, -0.37, 0),              # about one sample per bin
    (3, 1000, 1024, 2.2 / 1024, -0.37, 2 ** 40),       # bins narrower than a sample, nbin > n
    (3, 4099, 17, 2.75, -0.37, 0),                     # dphase > 1
    (3, 4099, 1024, 1.0 / 8, 0.0, 0),                  # every sample exactly on a bin edge
    (65, 4099, 64, 1.0 / 8, 0.0, 2 ** 40),             # ... and a period of 8 samples
    (1, 4099, 2, 0.5, 0.0, 0),                         # alternating bins: 32 runs per bin and group
    (3, 1000, 64, -0.0137, -0.37, 0),                  # phase running backwards
    (3, 4099, 4096, 1.0 / 4099.5, -0.37, 0),           # accumulators beyond 64 KiB of LDS
    (1, PIECE - 1, 17, 0.013, -0.37, 0), (1, PIECE, 17, 0.013, -0.37, 0), (1, PIECE + 1, 17, 0.013, -0.37, 0),
    (3, GROUP - 1, 17, 1.0 / 17.3, -0.37, 0), (3, GROUP, 17, 1.0 / 17.3, -0.37, 0),
    (3, GROUP + 1, 17, 1.0 / 17.3, -0.37, 0),
    (3, SUB - 1, 256, 1.0 / (61 * 256), -0.37, 0), (3, SUB, 256, 1.0 / (61 * 256), -0.37, 0),
    (3, SUB + 1, 256, 1.0 / (61 * 256), -0.37, 2 ** 40),
    (3, SEG - 1, 64, 0.00037, -0.37, 2 ** 40), (3, SEG, 64, 0.00037, -0.37, 0),
    (3, SEG + 1, 64, 0.00037, -0.37, 2 ** 40),
    (65, 2 * SEG + 77, 17, 1.0 / 700, -0.37, 0),       # three segments, five channel tiles
]


def case_id(c):
    return "c%d-n%d-b%d-%.3g-%s" % (c[0], c[1], c[2], c[3] * c[2], "far" if c[5] else "0")


@functools.lru_cache(maxsize=None)
def fold_input(nchan, n, kind):
    rng = np.random.default_rng(1000 * nchan + n)
    if kind == "u8":
        x = rng.integers(0, 256, (nchan, n)).astype(np.uint8)
    else:
        x = (rng.standard_normal((nchan, n)) * 8 + 3).astype(DTYPES[kind])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def fold_want(case, kind):
    nchan, n, nbin, dphase, phase0, first = case
    x = fold_input(nchan, n, kind)
    if kind == "u8":
        return fo.fold_exact(x, dphase, nbin, phase0, first) + (None,)
    return fo.fold_fsum(x, dphase, nbin, phase0, first)


def device_rows(gpu, x, pad=5, lead=0):
    """``x`` as a view of a wider device tensor: rows ``ld = n + pad`` apart, the first one
    ``lead`` elements into the buffer; the padding is garbage that must not be read into a sum."""
    import torch
    nchan, n = x.shape
    fill = 255 if x.dtype == np.uint8 else float("nan")
    wide = torch.full((nchan * (n + pad) + lead,), fill, dtype=getattr(torch, str(x.dtype)), device=gpu)
    view = wide[lead:].view(nchan, n + pad)[:, :n]
    view.copy_(torch.from_numpy(np.array(x)).to(gpu))
    return view


def raw_fold(x, dphase, nbin, phase0, first, out=None):
    """pu_fold called directly on a 2-D device view -> (sums, counts) numpy, and the tensors."""
    import torch
    from pulsarutils import _hip
    lib = _hip.lib()
    nchan, n = x.shape
    dev = x.device
    if out is None:
        # sums rows 3 elements wider than nbin: the padding must stay untouched
        out = (torch.zeros((nchan, nbin + 3), dtype=torch.float64, device=dev),
               torch.zeros(nbin, dtype=torch.int64, device=dev))
    sums, counts = out
    wsb = lib.pu_fold_workspace_bytes(nchan, n, nbin)
    ws = torch.empty(max(16, wsb), dtype=torch.uint8, device=dev)
    ld = x.stride(0) if nchan > 1 else max(x.stride(0), n)
    rc = lib.pu_fold(_hip.ptr(x), _hip.dtype_code(x.dtype), nchan, n, ld, first, phase0, dphase, nbin, _hip.ptr(sums),
                     sums.stride(0), _hip.ptr(counts), _hip.ptr(ws), ws.numel(), _hip.stream_ptr())
    assert rc == 0, lib.pu_last_error().decode()
    s = sums.cpu().numpy()
    assert not s[:, nbin:].any()
    return s[:, :nbin], counts.cpu().numpy(), out


def check_float(got, want, counts, abs_sums, extra_terms=0):
    """Each entry within 2 (m + extra) 2^-53 sum|x| of the exactly rounded sum: the bound of any
    summation order of m terms, doubled for the oracle's final rounding."""
    bound = 2.0 * (counts[None, :] + extra_terms) * U * abs_sums
    err = np.abs(got - want)
    assert (err <= bound).all(), (float(err.max()), float(bound[err > bound].min()))


@pytest.mark.parametrize("kind", ["u8", "f32", "f64"])
@pytest.mark.parametrize("case", FOLD_CASES, ids=case_id)
def test_fold_matches_the_oracle(gpu, case, kind):
    nchan, n, nbin, dphase, phase0, first = case
    x = device_rows(gpu, fold_input(nchan, n, kind))
    want, wcounts, wabs = fold_want(case, kind)
    got, counts, _ = raw_fold(x, dphase, nbin, phase0, first)
    assert np.array_equal(counts, wcounts)
    if kind == "u8":
        assert np.array_equal(got, want)
    else:
        check_float(got, want, wcounts, wabs)
        again, _, _ = raw_fold(x, dphase, nbin, phase0, first)
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("kind", ["u8", "f32", "f64"])
@pytest.mark.parametrize("case", [FOLD_CASES[2], FOLD_CASES[7], FOLD_CASES[-1]], ids=case_id)
def test_fold_accumulates_over_chunks(gpu, case, kind):
    nchan, n, nbin, dphase, phase0, first = case
    xh = fold_input(nchan, n, kind)
    want, wcounts, wabs = fold_want(case, kind)
    cut = n // 2 + 3
    a = device_rows(gpu, xh[:, :cut])
    b = device_rows(gpu, xh[:, cut:])
    _, _, out = raw_fold(a, dphase, nbin, phase0, first)
    got, counts, _ = raw_fold(b, dphase, nbin, phase0, first + cut, out=out)
    assert np.array_equal(counts, wcounts)
    if kind == "u8":
        assert np.array_equal(got, want)
    else:
        # two calls, each within its own m_i u S_i, and the add of the second into sums: one
        # more rounding of at most u S
        check_float(got, want, wcounts, wabs, extra_terms=1)


@pytest.mark.parametrize("kind", ["u8", "f32", "f64"])
@pytest.mark.parametrize("pad, lead", [(12, 0), (12, 16), (5, 3), (0, 1)])
def test_fold_reads_rows_at_any_alignment(gpu, kind, pad, lead):
    """(12, 0), (12, 16): 8-bit rows on 16-byte boundaries (n + pad = 4112), the vector-load path
    with a ragged last piece; the others start rows at odd addresses."""
    case = (3, 4100, 64, 1.0 / 1000, -0.37, 2 ** 40)
    nchan, n, nbin, dphase, phase0, first = case
    x = device_rows(gpu, fold_input(nchan, n, kind), pad=pad, lead=lead)
    want, wcounts, wabs = fold_want(case, kind)
    got, counts, _ = raw_fold(x, dphase, nbin, phase0, first)
    assert np.array_equal(counts, wcounts)
    if kind == "u8":
        assert np.array_equal(got, want)
    else:
        check_float(got, want, wcounts, wabs)


def test_fold_api_numpy_and_tensor(gpu):
    import torch
    from pulsarutils import folding
    x = fold_input(3, 1000, "u8")
    want, wcounts = fo.fold_exact(x, 1e-3 * 15.625, 64, 0.25, 7)
    s, c = folding.fold(x, 15.625, 1e-3, 64, ph0=0.25, first_sample=7)
    assert isinstance(s, np.ndarray) and np.array_equal(s, want) and np.array_equal(c, wcounts)
    xd = torch.from_numpy(np.array(x)).to(gpu)
    sd, cd = folding.fold(xd, 15.625, 1e-3, 64, ph0=0.25, first_sample=7)
    assert sd.is_cuda and cd.dtype == torch.int64 and np.array_equal(sd.cpu().numpy(), want)
    out = folding.fold(xd, 15.625, 1e-3, 64, ph0=0.25, first_sample=7, out=(sd, cd))
    assert out[0] is sd and np.array_equal(sd.cpu().numpy(), 2 * want) and np.array_equal(cd.cpu().numpy(), 2 * wcounts)
    s1, _ = folding.fold(x[0], 15.625, 1e-3, 64, ph0=0.25, first_sample=7)
    assert s1.shape == (64,) and np.array_equal(s1, want[0])
    with pytest.raises(ValueError):
        folding.fold(x, 15.625, 1e-3, 9000)


# ------------------------------------------------------------------ H-test

H_SIZES = (2, 10, 32, 100, 1021, 4096, 8192)
BIG = 4096  # from here on, five-row cases stop at nmax = n // 10 (the oracle is O(n nmax) fsum terms per row)


def h_rows(n):
    """Poisson(20) background plus a 10-bin pulse, a delta, a flat row, zeros, a row with a NaN."""
    rng = np.random.default_rng(n)
    p = rng.poisson(20, n).astype(np.float64)
    w = min(10, max(1, n // 3))
    p[n // 3:n // 3 + w] += 30
    delta = np.zeros(n)
    delta[n // 2] = 37.0
    nan = p.copy()
    nan[1] = np.nan
    return np.stack([p, delta, np.full(n, 20.0), np.zeros(n), nan])


@functools.lru_cache(maxsize=None)
def h_want(n, row, nmax):
    """Z^2_1 .. Z^2_nmax of row ``row`` of h_rows(n) (a prefix of a longer list serves a smaller nmax)."""
    return tuple(fo.z2_all_fast(h_rows(n)[row], nmax))


def nmax_values(n):
    return sorted({v for v in (1, 20, n // 10, n - 1) if 1 <= v <= n - 1})


H_CASES = [(rows, n, nmax) for n in H_SIZES for rows in (1, 5) for nmax in nmax_values(n)
           if not (rows == 5 and n >= BIG and nmax > n // 10)]


@pytest.mark.parametrize("with_zs", [True, False], ids=["zs", "nozs"])
@pytest.mark.parametrize("rows, n, nmax", H_CASES)
def test_h_test_matches_the_oracle(gpu, rows, n, nmax, with_zs):
    import torch
    from pulsarutils import _hip
    lib = _hip.lib()
    prof = h_rows(n)[:rows]
    full = n - 1 if (rows == 1 or n < BIG) else n // 10
    x = device_rows(gpu, prof, pad=7)
    h = torch.empty(rows, dtype=torch.float64, device=gpu)
    m = torch.empty(rows, dtype=torch.int32, device=gpu)
    zs = torch.full((rows, nmax + 2), -7.0, dtype=torch.float64, device=gpu) if with_zs else None
    wsb = lib.pu_h_test_workspace_bytes(rows, n, nmax)
    ws = torch.empty(wsb + 16, dtype=torch.uint8, device=gpu)
    off = (-ws.data_ptr()) % 16
    import ctypes
    rc = lib.pu_h_test(_hip.ptr(x), rows, n, x.stride(0), nmax, _hip.ptr(h), _hip.ptr(m), _hip.ptr(zs),
                       zs.stride(0) if with_zs else 0, ctypes.c_void_p(ws.data_ptr() + off), wsb, _hip.stream_ptr())
    assert rc == 0, lib.pu_last_error().decode()
    h, m = h.cpu().numpy(), m.cpu().numpy()
    zs = zs.cpu().numpy() if with_zs else None
    if with_zs:
        assert (zs[:, nmax:] == -7.0).all()
    for r in range(rows):
        want = list(h_want(n, r, full)[:nmax])
        wh, wm, hm = fo.h_from_z2(want)
        if r >= 3:  # the all-zero row and the row with a NaN
            assert math.isnan(wh) and wm == 0
            assert math.isnan(h[r]) and m[r] == 0
            if with_zs:
                assert np.isnan(zs[r, :nmax]).all()
            continue
        tot = math.fsum(prof[r])
        tols = [fo.z2_tolerance(n, k, tot) for k in range(1, nmax + 1)]
        if nmax > 1:  # the oracle alone: its maximum is clear of the runner-up
            second = max(v for k, v in enumerate(hm, start=1) if k != wm)
            assert wh - second > 2 * tols[-1], (wh - second, tols[-1])
        if with_zs:
            err = np.abs(zs[r, :nmax] - np.array(want))
            assert (err <= np.array(tols)).all(), (r, float(err.max()))
        assert m[r] == wm
        assert abs(h[r] - wh) <= tols[wm - 1]


def test_h_test_api(gpu):
    import torch
    from pulsarutils import folding
    rows = h_rows(100)
    z = folding.z_n_all(rows, nmax=10)
    assert z.shape == (5, 10)
    want = np.array(h_want(100, 0, 99)[:10])
    assert np.allclose(z[0], want, rtol=0, atol=fo.z2_tolerance(100, 10, rows[0].sum()))
    h, m = folding.h_test(rows[0], nmax=20)
    wh, wm, _ = fo.h_from_z2(list(h_want(100, 0, 99)[:20]))
    assert isinstance(h, float) and isinstance(m, int) and m == wm and abs(h - wh) <= fo.z2_tolerance(100, 20, rows[0].sum())
    hs, ms = folding.h_test(torch.from_numpy(rows).to(gpu), nmax=20)
    assert hs.is_cuda and ms.dtype == torch.int32 and int(ms[0]) == wm and math.isnan(float(hs[3]))
    with pytest.raises(ValueError):
        folding.h_test(np.ones(9000))
    with pytest.raises(ValueError):
        folding.h_test(np.ones(16), nmax=16)


# ------------------------------------------------------------------ end to end

PERIOD, DM, NCH, NS, TSAMP, NBIN = 0.064, 50.0, 32, 2 ** 14, 1e-3, 64
FBOT, FTOP = 1200.0, 1400.0


@pytest.fixture(scope="module")
def pulsar_file(tmp_path_factory):
    """A u8 filterbank (file channel 0 = the highest frequency): noise rint(64 + 8 N) and a pulsar of
    period 0.064 s at DM 50, +16 in the two bins around phase 0.5 of each turn, channel c (ascending
    frequency) delayed by the reference's dedispersion_shifts(DM) samples."""
    from pulsarutils import sigproc
    from pulsarutils._planner import dedispersion_shifts
    rng = np.random.default_rng(2024)
    data = np.rint(64 + 8 * rng.standard_normal((NS, NCH)))
    delay = np.rint(dedispersion_shifts(NCH, DM, FBOT, FTOP - FBOT, TSAMP)).astype(np.int64)
    i = np.arange(NS, dtype=np.int64)
    for c in range(NCH):
        phase = np.mod((i - delay[c]) * TSAMP / PERIOD, 1.0)
        b = np.floor(phase * NBIN).astype(np.int64)
        data[(b == NBIN // 2 - 1) | (b == NBIN // 2), c] += 16
    data = np.clip(data, 0, 255).astype(np.uint8)[:, ::-1]  # file order: descending frequency
    data = np.ascontiguousarray(data)
    foff = -(FTOP - FBOT) / NCH
    fname = str(tmp_path_factory.mktemp("fold") / "pulsar.fil")
    sigproc.write_filterbank(fname, data, fch1=FTOP + 0.5 * foff, foff=foff, tsamp=TSAMP)
    return fname, data


@pytest.fixture(scope="module")
def folded(gpu, pulsar_file):
    """fold_file(clean=False) in chunks of 5000 and in one chunk, and the oracle fold of the bytes."""
    from pulsarutils import folding
    from pulsarutils.stats import get_bad_chans
    fname, data = pulsar_file
    a = folding.fold_file(fname, 1 / PERIOD, nbin=NBIN, chunksize=5000, clean=False)
    b = folding.fold_file(fname, 1 / PERIOD, nbin=NBIN, chunksize=2 ** 14, clean=False)
    sums, counts = fo.fold_exact(data.T, TSAMP * (1 / PERIOD), NBIN)
    want = sums / counts.astype(np.float64)
    want[np.array(get_bad_chans(fname), dtype=bool)] = 0.0
    return a, b, np.ascontiguousarray(want[::-1]), counts


def test_fold_file_is_the_oracle_fold_of_the_bytes(folded):
    a, b, want, counts = folded
    for info in (a, b):
        assert np.array_equal(info.counts, counts) and counts.min() > 0
        assert info.allprofs.dtype == np.float64 and np.array_equal(info.allprofs, want)
        assert (info.nbin, info.nchan, info.ph0) == (NBIN, NCH, 0.0)
        assert info.pulse_freq == 1 / PERIOD and info.start_freq == FBOT and info.bandwidth == FTOP - FBOT
        assert info.date == 60000.0


def test_h_curve_of_the_folded_search(folded):
    from pulsarutils import clean, folding
    info = folded[0]
    plane, table = clean.dedispersion_search(info, 0, 80)
    assert plane.shape[1] == NBIN and plane.shape[0] == len(table["DM"])
    h, m = folding.h_curve(plane)
    nmax = NBIN // 10
    with np.errstate(divide="ignore", invalid="ignore"):
        dig = clean.digitize(np.array(plane, dtype=np.float64))
    want_h, want_m = [], []
    for r, row in enumerate(dig):
        zs = fo.z2_all(row, nmax)
        wh, wm, hm = fo.h_from_z2(zs)
        want_h.append(wh)
        want_m.append(wm)
        if math.isnan(wh):
            assert math.isnan(h[r]) and m[r] == 0
            continue
        tol = fo.z2_tolerance(NBIN, nmax, float(row.sum()))
        assert abs(h[r] - wh) <= tol
        second = max(v for k, v in enumerate(hm, start=1) if k != wm)
        if wh - second > 2 * tol:
            assert m[r] == wm
    best = int(np.nanargmax(want_h))
    assert int(np.nanargmax(h)) == best


def test_fold_file_cleaned_zeroes_masked_channels(gpu, pulsar_file):
    from pulsarutils import folding
    fname, _ = pulsar_file
    info = folding.fold_file(fname, 1 / PERIOD, nbin=NBIN, chunksize=5000, clean=True, surelybad=(3,))
    assert info.allprofs.shape == (NCH, NBIN) and np.isfinite(info.allprofs).all()
    assert not info.allprofs[NCH - 1 - 3].any()  # file channel 3, after the band flip
    assert info.allprofs[0].any() and info.counts.sum() == NS


def test_profile_stats_fills_every_field(folded):
    from pulsarutils import folding
    info = folding.profile_stats(folded[0], dm=DM)
    for side in ("disp", "dedisp"):
        assert getattr(info, side + "_profile").shape == (NBIN,)
        for f in ("z2", "z6", "z12", "z20", "H"):
            assert np.isfinite(getattr(info, f"{side}_{f}")), (side, f)
        assert 1 <= getattr(info, side + "_M") <= 20
        assert info.__dict__[side + "_z2"] <= info.__dict__[side + "_z20"]
    assert info.dm == DM and info.dedisp_H > info.disp_H
