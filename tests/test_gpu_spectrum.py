"""pu_rfft, pu_spectrum_normalize, pu_harmonic_search and pulsarutils.periodicity on the GPU.

The FFT is held to the Cooley-Tukey bound ||spec - ref||_2 <= 8 log2(nfft) 2^-24 ||ref||_2 per row
(Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: about 6.7 eps per stage with
correctly rounded twiddles, rounded up to 8 for the split step) against the float64 DFT of the
same float32-rounded samples; the float32 stages after it are compared bit for bit with
tests/spectrum_oracle.py fed the GPU's own spectrum."""
import math

import numpy as np
import pytest

import spectrum_oracle as so

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def hip(gpu):
    from pulsarutils import _hip
    _hip.require_gpu()
    return _hip


def _device_rows(hip, x, ld):
    """(rows, n) numpy -> a device view with leading dimension ``ld`` (the gap filled with NaN, which
    nothing may read)."""
    import torch
    rows, n = x.shape
    buf = torch.full((rows, ld), float("nan"), dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    buf[:, :n] = torch.from_numpy(x).cuda()
    return buf[:, :n]


def gpu_rfft(hip, x, nfft, mean=None, ld=None, ld_spec=None):
    """pu_rfft through the C ABI: complex64 numpy (rows, nfft / 2 + 1)."""
    import torch
    from pulsarutils import periodicity as pe
    x = np.atleast_2d(x)
    rows, n = x.shape
    xd = _device_rows(hip, x, n + 7 if ld is None else ld)
    ld_spec = nfft // 2 + 1 if ld_spec is None else ld_spec
    spec = torch.full((rows, ld_spec), float("nan"), dtype=torch.complex64, device="cuda")
    md = None if mean is None else torch.from_numpy(np.asarray(mean, dtype=np.float64)).cuda()
    lib = hip.lib()
    ws, wp, wsb = hip.workspace(lib.pu_rfft_workspace_bytes(rows, nfft), xd.device)
    hip.check(lib.pu_rfft(hip.ptr(xd), hip.dtype_code(xd.dtype), rows, n, xd.stride(0), hip.ptr(md), nfft, hip.ptr(spec),
                          ld_spec, wp, wsb, hip.stream_ptr()), "pu_rfft")
    torch.cuda.synchronize()
    return spec[:, :nfft // 2 + 1].cpu().numpy()


def _inputs(kind, n, dtype, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        x = rng.standard_normal(n)
    elif kind == "tone":
        x = np.cos(2 * np.pi * 0.1234567 * np.arange(n) + 0.3)  # off-bin at every nfft here
    elif kind == "spike":
        x = np.zeros(n)
        x[n // 3] = 5.0
    else:
        x = rng.standard_normal(n) + 100.0
    return x.astype(dtype)


def _ratios(spec, ref, nfft):
    err = np.linalg.norm(spec.astype(np.complex128) - ref, axis=1)
    return err / (math.log2(nfft) * EPS * np.linalg.norm(ref, axis=1))


KINDS = ("gauss", "tone", "spike", "offset")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfft", [2 ** 8, 2 ** 11, 2 ** 16])
def test_fft_accuracy(hip, nfft, dtype):
    worst = 0.0
    for n in (nfft, nfft - 24, nfft // 2 + 1):
        rows = [_inputs(k, n, dtype, 11 + i) for i, k in enumerate(KINDS)]
        # the offset row has its float64 mean taken out; the others go in as they are
        means = [0.0, 0.0, 0.0, float(rows[3].astype(np.float64).sum() / n)]
        # one row at a time, then batches of three (with another leading dimension)
        for i in range(4):
            mean = None if means[i] == 0.0 else [means[i]]
            spec = gpu_rfft(hip, rows[i][None], nfft, mean=mean)
            ratio = _ratios(spec, so.rfft(rows[i][None], nfft, mean), nfft)
            print(f"nfft 2^{int(math.log2(nfft))} {np.dtype(dtype).name} n {n} rows 1 {KINDS[i]}: ratio {ratio[0]:.3f}")
            worst = max(worst, ratio.max())
            assert ratio.max() <= 8.0, (KINDS[i], n, ratio)
        for pick in ((0, 1, 2), (3, 0, 1)):
            x = np.stack([rows[i] for i in pick])
            mean = [means[i] for i in pick]
            spec = gpu_rfft(hip, x, nfft, mean=mean, ld=n + 33)
            ratio = _ratios(spec, so.rfft(x, nfft, mean), nfft)
            print(f"nfft 2^{int(math.log2(nfft))} {np.dtype(dtype).name} n {n} rows 3 {[KINDS[i] for i in pick]}: "
                  f"ratio {np.round(ratio, 3).tolist()}")
            worst = max(worst, ratio.max())
            assert ratio.max() <= 8.0, (pick, n, ratio)
    print(f"nfft 2^{int(math.log2(nfft))} {np.dtype(dtype).name}: worst ratio {worst:.3f} of log2(nfft) 2^-24")


def test_fft_accuracy_one_long_row(hip):
    nfft = 2 ** 20
    x = _inputs("gauss", nfft - 24, np.float32, 3)[None]
    spec = gpu_rfft(hip, x, nfft)
    ratio = _ratios(spec, so.rfft(x, nfft), nfft)
    print(f"nfft 2^20 float32 n {nfft - 24} rows 1 gauss: ratio {ratio[0]:.3f}")
    assert ratio.max() <= 8.0


@pytest.mark.parametrize("nfft", [2 ** 8, 2 ** 11, 2 ** 16])
def test_fft_reproducible_and_independent_of_the_batch(hip, nfft):
    n = nfft - 24
    x = np.stack([_inputs(k, n, np.float32, 5 + i) for i, k in enumerate(("gauss", "offset", "tone"))])
    mean = x.astype(np.float64).sum(axis=1) / n
    a = gpu_rfft(hip, x, nfft, mean=mean, ld=n + 1)
    b = gpu_rfft(hip, x, nfft, mean=mean, ld=n + 1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for r in range(3):
        alone = gpu_rfft(hip, x[r:r + 1], nfft, mean=mean[r:r + 1], ld=n + 64, ld_spec=nfft // 2 + 9)
        assert np.array_equal(alone.view(np.uint32), a[r:r + 1].view(np.uint32)), r


# ------------------------------------------------------------------ normalise, sums, candidates

def _special_rows(n):
    rng = np.random.default_rng(21)
    t = np.arange(n)
    x = rng.standard_normal((4, n)).astype(np.float32)
    x[0] += (1.5 * (np.modf(t * 0.0431)[0] < 0.08)).astype(np.float32)  # a pulse train
    x[2, n // 2] = np.nan                                                # every block NaN
    x[3] = 3.0                                                           # constant: all 0
    mean = np.array([x[0].astype(np.float64).sum() / n, 0.0, 0.0, 3.0])
    return x, mean


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _search(hip, norm_d, nlev, thr, kmin, kmax, sums=None, cap=0):
    from pulsarutils import periodicity as pe
    return pe._harmonic_search_device(norm_d, nlev, thr, kmin, kmax, sums=sums, cap=cap)


@pytest.fixture(scope="module")
def staged(hip):
    """Per nfft: the GPU's spectrum of the special rows (computed once, shared, never changed)."""
    import torch
    out = {}
    for nfft in (2 ** 8, 2 ** 12):
        x, mean = _special_rows(nfft - 10)
        spec = gpu_rfft(hip, x, nfft, mean=mean)
        spec_d = torch.from_numpy(spec).cuda()
        spec.setflags(write=False)
        out[nfft] = (spec, spec_d)
    return out


@pytest.mark.parametrize("nfft, block", [(2 ** 8, 16), (2 ** 8, 128), (2 ** 12, 128), (2 ** 12, 1024)])
def test_normalize_bit_for_bit(hip, staged, nfft, block):
    from pulsarutils import periodicity as pe
    spec, spec_d = staged[nfft]
    nb = nfft // 2
    got = pe._normalize_device(spec_d, nb, block).cpu().numpy()
    want = so.normalize(spec, nb, block)
    assert _eq(got, want)
    assert got[2, 0] == 0 and np.all(np.isnan(got[2, 1:]))
    assert np.all(got[3] == 0) and np.all(got[:, 0] == 0)
    assert 0.5 < got[1, 1:].mean() < 2.0  # noise sits near 1


@pytest.mark.parametrize("nlev", [1, 6])
@pytest.mark.parametrize("nfft, block", [(2 ** 8, 16), (2 ** 8, 128), (2 ** 12, 128), (2 ** 12, 1024)])
def test_harmonic_sums_and_candidates_bit_for_bit(hip, staged, nfft, block, nlev):
    import torch
    from pulsarutils import periodicity as pe
    spec, spec_d = staged[nfft]
    nb = nfft // 2
    norm_d = pe._normalize_device(spec_d, nb, block)
    norm = norm_d.cpu().numpy()
    sums_d = torch.full((nlev, 4, nb), float("nan"), dtype=torch.float32, device="cuda")
    want_sums = so.harmonic_sums(norm, nlev)
    full0, full1 = np.zeros(nlev, np.int64), np.full(nlev, nb, np.int64)
    # (thresholds, kmin, kmax): a flood from bin 0 to nb (negative threshold: the edges at 0 and
    # nb - 1 take part), a 2-sigma cut, and ranges that cut inside
    cases = [(np.full(nlev, -1.0, np.float32), full0, full1),
             (np.array([pe.power_threshold(pe.logp_from_sigma(2.0), 1 << lv) for lv in range(nlev)], np.float32), full0,
              full1),
             (np.full(nlev, 1.0, np.float32), np.arange(nlev) + 5, np.full(nlev, nb - 3) - np.arange(nlev))]
    for thr, kmin, kmax in cases:
        sums_d.fill_(float("nan"))
        rec, count = _search(hip, norm_d, nlev, thr, kmin, kmax, sums=sums_d, cap=4 * nlev * nb)
        assert _eq(sums_d.cpu().numpy(), want_sums)
        want = so.candidates(sums_d.cpu().numpy(), thr, kmin, kmax)
        assert count == want.size and rec.size == want.size
        assert rec.tobytes() == want.tobytes()
        assert not np.any(rec["row"] == 2)                       # the NaN row
        assert thr.min() < 0 or not np.any(rec["row"] == 3)      # the zero row
        # the fused path (no sums written) delivers the same list
        rec2, count2 = _search(hip, norm_d, nlev, thr, kmin, kmax, cap=4 * nlev * nb)
        assert count2 == count and rec2.tobytes() == rec.tobytes()
        # cap = 0 counts; cap = 3 returns the first three in (row, level, bin) order
        rec0, count0 = _search(hip, norm_d, nlev, thr, kmin, kmax, cap=0)
        assert rec0.size == 0 and count0 == count
        rec3, count3 = _search(hip, norm_d, nlev, thr, kmin, kmax, cap=3)
        assert count3 == count and rec3.tobytes() == want[:3].tobytes()
    assert count > 3  # (the last case is not vacuous)
    # the public function returns the same sums
    assert _eq(pe.harmonic_sums(norm, nharm=1 << (nlev - 1)), want_sums)


# ------------------------------------------------------------------ end to end, API

def _pulsar_rows():
    rng = np.random.default_rng(5)
    n, dt = 2 ** 14, 1e-3
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    t = np.arange(n) * dt
    a[(t * 7.3) % 1 < 0.05] += np.float32(1.2)
    return np.stack([a, b]), dt


def test_end_to_end_pulse_train(hip):
    from pulsarutils import periodicity as pe
    x, dt = _pulsar_rows()
    tobs = x.shape[1] * dt
    raw = pe.periodicity_search(x, dt, nharm=16, sigma=8, block=128, sift=False)
    assert len(raw) > 1 and np.all(np.diff(raw["logp"]) >= 0)
    assert raw["nharm"][0] == 16 and abs(raw["freq"][0] - 7.3) <= 1 / (16 * 16.384)
    assert not np.any(raw["row"] == 1)                      # nothing from the noise row
    assert np.all(raw["sigma"] >= 8.0 - 1e-4)
    print(f"best: nharm {raw['nharm'][0]} bin {raw['bin'][0]} freq {raw['freq'][0]:.4f} logp {raw['logp'][0]:.1f}")
    tab = pe.periodicity_search(x, dt, nharm=16, sigma=8, block=128)
    assert tab["nharm"][0] == 16 and abs(tab["freq"][0] - 7.3) <= 1 / (16 * 16.384)
    assert not np.any(tab["row"] == 1)
    # exactly one candidate is left within 1.5 / T of a multiple or a fraction of 7.3 Hz
    j = np.arange(1, 17)
    f = np.asarray(tab["freq"])[:, None]
    related = ((np.abs(f - 7.3 * j) <= 1.5 / tobs) | (np.abs(f - 7.3 / j) <= 1.5 / tobs)).any(axis=1)
    assert related.sum() == 1 and related[0]
    assert tab["nabsorbed"][0] > 0 and int(np.sum(tab["nabsorbed"])) + len(tab) == len(raw)
    # a small first buffer changes nothing: the count comes first, then the room
    small = pe.periodicity_search(x, dt, nharm=16, sigma=8, block=128, sift=False, max_candidates=1)
    assert all(np.array_equal(small[c], raw[c]) for c in raw.colnames)


def test_api_conventions_and_errors(hip):
    import torch
    from pulsarutils import periodicity as pe
    x, dt = _pulsar_rows()
    nfft = x.shape[1]
    spec = pe.rfft(x)
    assert isinstance(spec, np.ndarray) and spec.dtype == np.complex64 and spec.shape == (2, nfft // 2 + 1)
    ref = so.rfft(x, nfft, x.astype(np.float64).sum(axis=1) / nfft)
    assert _ratios(spec, ref, nfft).max() <= 8.0
    xd = torch.from_numpy(x).cuda()
    spec_d = pe.rfft(xd)
    assert isinstance(spec_d, torch.Tensor) and spec_d.is_cuda and np.array_equal(spec_d.cpu().numpy(), spec)
    one = pe.rfft(x[0], nfft=2 * nfft)
    assert one.shape == (nfft + 1,)
    norm = pe.power_spectrum(x, block=128)
    assert isinstance(norm, np.ndarray) and norm.dtype == np.float32 and norm.shape == (2, nfft // 2)
    assert _eq(norm, so.normalize(spec, nfft // 2, 128))
    assert isinstance(pe.power_spectrum(xd), torch.Tensor) and pe.power_spectrum(x[0]).shape == (nfft // 2,)
    sums = pe.harmonic_sums(norm, nharm=4)
    assert isinstance(sums, np.ndarray) and sums.shape == (3, 2, nfft // 2) and _eq(sums, so.harmonic_sums(norm, 3))
    assert pe.harmonic_sums(norm[0], nharm=2).shape == (2, nfft // 2)
    assert isinstance(pe.harmonic_sums(torch.from_numpy(norm).cuda(), nharm=2), torch.Tensor)
    # float64 and 1-D series go through as they are
    tab = pe.periodicity_search(x[0].astype(np.float64), dt, sigma=8)
    assert tab.colnames == ["freq", "row", "nharm", "bin", "power", "logp", "sigma", "nabsorbed"]
    assert np.all(tab["row"] == 0) and tab["nharm"][0] == 16
    for bad in (dict(nfft=3000), dict(nfft=2 ** 13), dict(nfft=2 ** 25)):
        with pytest.raises(ValueError):
            pe.rfft(x, **bad)
    for bad in (dict(block=8), dict(block=100), dict(block=2048)):
        with pytest.raises(ValueError):
            pe.power_spectrum(x, **bad)
    for bad in (3, 0, 64, 12):
        with pytest.raises(ValueError):
            pe.harmonic_sums(norm, nharm=bad)
        with pytest.raises(ValueError):
            pe.periodicity_search(x, dt, nharm=bad)
