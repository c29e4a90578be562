"""The pure-numpy half of pulsarutils.periodicity, and the argument checks pu_rfft,
pu_spectrum_normalize and pu_harmonic_search make before any HIP call (CPU only)."""
import ctypes
import math

import numpy as np
import pytest

from pulsarutils import periodicity as pe

EINVAL, EUNSUPPORTED = -1, -4
U8, F32, F64 = 0, 1, 2
P = 4096  # never dereferenced: every case below returns before any HIP call


def test_next_nfft():
    assert pe.next_nfft(1) == 256 and pe.next_nfft(256) == 256 and pe.next_nfft(257) == 512
    assert pe.next_nfft(1000, pad=2) == 2048 and pe.next_nfft(2 ** 24) == 2 ** 24
    with pytest.raises(ValueError):
        pe.next_nfft(2 ** 24 + 1)
    with pytest.raises(ValueError):
        pe.next_nfft(0)


def test_harmonic_bins_are_the_sum_order():
    assert pe.harmonic_bins(10, 0).tolist() == [10]
    assert pe.harmonic_bins(10, 1).tolist() == [10, 5]
    assert pe.harmonic_bins(10, 2).tolist() == [10, 5, 3, 8]
    b = pe.harmonic_bins(np.arange(1000), 5)
    assert b.shape == (1000, 32) and b.min() == 0 and np.all(b.max(axis=1) == np.arange(1000))
    # the 16 bins of level 4 are the harmonics j k / 16 rounded to the nearest bin (half up)
    k = 1913
    assert sorted(pe.harmonic_bins(k, 4).tolist()) == [(k * j + 8) // 16 for j in range(1, 17)]


def test_erlang_logsf_one_harmonic_is_minus_s():
    s = np.array([0.0, 0.3, 1.0, 17.5, 800.0, 1e5])
    assert np.array_equal(pe.erlang_logsf(s, 1), -s)
    assert pe.erlang_logsf(0.0, 8) == 0.0


def test_erlang_logsf_agrees_with_scipy():
    from scipy import stats
    s = np.concatenate(([1e-3, 0.1, 0.5], np.linspace(1.0, 60.0, 60), [100.0, 300.0, 700.0, 3000.0]))
    for h in pe.NHARMS:
        want = stats.gamma.logsf(s, a=h)
        got = pe.erlang_logsf(s, h)
        assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want)), (h, np.abs(got / want - 1).max())


def test_power_threshold_round_trip():
    for h in pe.NHARMS:
        for logp in (-1.0, -20.7, -378.0, -5000.0):
            s = pe.power_threshold(logp, h)
            assert abs(float(pe.erlang_logsf(s, h)) - logp) <= 1e-10 * abs(logp)
    assert pe.power_threshold(-20.7, 1) == pytest.approx(20.7, rel=1e-12)
    with pytest.raises(ValueError):
        pe.power_threshold(0.5, 4)


def test_sigma_round_trip_through_the_asymptotic_form():
    for sigma in range(1, 41):
        logp = pe.logp_from_sigma(sigma)
        assert math.isfinite(logp) and logp < 0
        assert pe.sigma_from_logp(logp) == pytest.approx(sigma, rel=1e-10)
    assert pe.logp_from_sigma(0.0) == pytest.approx(math.log(0.5))
    assert pe.logp_from_sigma(6.0) == pytest.approx(math.log(9.865876450377e-10), rel=1e-9)
    # the two forms meet: the series' first neglected term is 105 / sigma^8
    a, b = pe.logp_from_sigma(37.0), pe.logp_from_sigma(37.0 + 1e-9)
    assert abs(a - b) < 1e-6
    assert pe.sigma_from_logp(-0.1) == 0.0


def test_bin_ranges_edges():
    nfft, dt = 1024, 2.0 ** -10  # T = 1 s exactly, nb = 512
    kmin, kmax = pe.bin_ranges(None, None, nfft, dt, 3)
    assert kmin.tolist() == [1, 2, 4] and kmax.tolist() == [512, 512, 512]
    # a fundamental exactly on a bin is inside at both ends
    kmin, kmax = pe.bin_ranges(10.0, 20.0, nfft, dt, 3)
    assert kmin.tolist() == [10, 20, 40] and kmax.tolist() == [21, 41, 81]
    # clipped to [0, nb]; an empty range stays empty
    kmin, kmax = pe.bin_ranges(0.0, 1e9, nfft, dt, 2)
    assert kmin.tolist() == [0, 0] and kmax.tolist() == [512, 512]
    kmin, kmax = pe.bin_ranges(400.0, 450.0, nfft, dt, 3)
    assert kmin.tolist() == [400, 512, 512] and kmax.tolist() == [451, 512, 512]
    kmin, kmax = pe.bin_ranges(10.25, 10.75, nfft, dt, 2)
    assert kmin.tolist() == [11, 21] and kmax.tolist() == [11, 22]  # level 0: no bin inside
    with pytest.raises(ValueError):
        pe.bin_ranges(5.0, 1.0, nfft, dt, 2)


def test_sift_candidates_hand_made_list():
    tobs, f0 = 100.0, 7.3
    cands = {
        "freq": np.array([2 * f0 + 0.004, f0, 5 * f0 - 0.01, f0 / 2 + 0.002, 11.1, f0 + 0.02, 3 * f0 + 0.016]),
        "row": np.array([0, 0, 0, 3, 1, 0, 0]),
        "logp": np.array([-50.0, -300.0, -40.0, -30.0, -25.0, -20.0, -10.0]),
    }
    out = pe.sift_candidates(cands, tobs)
    # the fundamental wins and absorbs its 2nd and 5th harmonic and the half-frequency of row 3;
    # 11.1 Hz is unrelated; f0 + 0.02 is 0.02 > 1.5 / T = 0.015 away: kept; 3 f0 + 0.016 is 0.016
    # from 3 f0 and 0.044 from 3 (f0 + 0.02): kept
    assert out["freq"].tolist() == [f0, 11.1, f0 + 0.02, 3 * f0 + 0.016]
    assert out["nabsorbed"].tolist() == [3, 0, 0, 0]
    assert out["row"].tolist() == [0, 1, 0, 0] and out["logp"].tolist() == [-300.0, -25.0, -20.0, -10.0]
    # max_ratio bounds the harmonics looked at
    out = pe.sift_candidates(cands, tobs, max_ratio=4)
    assert (5 * f0 - 0.01) in out["freq"].tolist() and out["nabsorbed"][0] == 2
    empty = pe.sift_candidates({"freq": np.zeros(0), "logp": np.zeros(0)}, tobs)
    assert empty["freq"].size == 0 and empty["nabsorbed"].size == 0


def test_module_imports_without_a_gpu_and_rejects_bad_nharm():
    with pytest.raises(ValueError):
        pe._nlev(3)
    with pytest.raises(ValueError):
        pe._nlev(64)
    assert [pe._nlev(h) for h in pe.NHARMS] == [1, 2, 3, 4, 5, 6]
    with pytest.raises(ValueError):
        pe._check_nfft(1000, 100)
    with pytest.raises(ValueError):
        pe._check_nfft(256, 300)
    with pytest.raises(ValueError):
        pe._check_block(48, 512)
    with pytest.raises(ValueError):
        pe._check_block(256, 128)


# ------------------------------------------------------------------ the C ABI's checks

@pytest.fixture(scope="module")
def lib():
    from pulsarutils import _hip
    return _hip.lib()


def _msg(lib):
    return lib.pu_last_error().decode()


def _rfft(lib, dtype=F32, rows=2, n=300, ld=300, nfft=512, ld_spec=257, ws=P, ws_bytes=1 << 20, x=P, spec=P):
    return lib.pu_rfft(x, dtype, rows, n, ld, None, nfft, spec, ld_spec, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, word", [
    (dict(nfft=128, ld_spec=65, n=100, ld=100), "power of two"),
    (dict(nfft=768, ld_spec=385), "power of two"),
    (dict(nfft=2 ** 25, ld_spec=2 ** 24 + 1), "power of two"),
    (dict(n=513, ld=513), "bad size"),
    (dict(n=-1), "bad size"),
    (dict(rows=-1), "bad size"),
    (dict(ld=299), "leading dimension"),
    (dict(ld_spec=256), "leading dimension"),
    (dict(ws_bytes=100), "workspace"),
    (dict(ws=None), "workspace"),
    (dict(ws=P + 8), "workspace"),
    (dict(x=None), "null"),
    (dict(spec=None), "null"),
    (dict(x=P + 2), "aligned"),
])
def test_rfft_rejects_before_any_hip_call(lib, kw, word):
    assert _rfft(lib, **kw) == EINVAL
    assert word in _msg(lib)


def test_rfft_dtype_and_empty_and_workspace_size(lib):
    assert _rfft(lib, dtype=U8) == EUNSUPPORTED and "dtype" in _msg(lib)
    assert _rfft(lib, rows=0, x=None, spec=None, ws=None, ws_bytes=0) == 0
    # the twiddle table alone up to 2^13, plus rows x nfft / 2 complex64 above
    assert lib.pu_rfft_workspace_bytes(3, 256) == 128 * 8
    assert lib.pu_rfft_workspace_bytes(3, 2 ** 13) == 2 ** 12 * 8
    assert lib.pu_rfft_workspace_bytes(3, 2 ** 14) == 2 ** 13 * 8 * 4
    assert lib.pu_rfft_workspace_bytes(3, 1000) == 0 and lib.pu_rfft_workspace_bytes(0, 256) == 0


@pytest.mark.parametrize("kw, word", [
    (dict(nb=64, block=16), "nb"),
    (dict(nb=384), "nb"),
    (dict(block=8), "block"),
    (dict(block=48), "block"),
    (dict(block=2048, nb=4096, ld_spec=4097, ld_out=4096), "block"),
    (dict(block=256, nb=128, ld_spec=129, ld_out=128), "block"),
    (dict(rows=-1), "rows"),
    (dict(ld_spec=255), "leading dimension"),
    (dict(ld_out=255), "leading dimension"),
    (dict(spec=None), "null"),
    (dict(out=None), "null"),
])
def test_normalize_rejects_before_any_hip_call(lib, kw, word):
    a = dict(spec=P, rows=2, nb=256, ld_spec=257, block=128, out=P, ld_out=256)
    a.update(kw)
    assert lib.pu_spectrum_normalize(a["spec"], a["rows"], a["nb"], a["ld_spec"], a["block"], a["out"], a["ld_out"],
                                     None) == EINVAL
    assert word in _msg(lib)


@pytest.mark.parametrize("kw, word", [
    (dict(nlev=0), "nlev"),
    (dict(nlev=7), "nlev"),
    (dict(rows=-1), "rows"),
    (dict(rows=70000), "rows"),
    (dict(nb=0), "bad shape"),
    (dict(ld=255), "bad shape"),
    (dict(sums=P, ld_row=100, ld_level=1000), "strides"),
    (dict(sums=P, ld_row=256, ld_level=256), "strides"),
    (dict(cap=-1), "cap"),
    (dict(cap=5, cands=None), "cap"),
    (dict(thr=None), "null"),
    (dict(norm=None), "null"),
    (dict(ws_bytes=8), "workspace"),
    (dict(ws=P + 8), "workspace"),
])
def test_harmonic_search_rejects_before_any_hip_call(lib, kw, word):
    thr = (ctypes.c_float * 6)()
    k0, k1 = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 6)()
    count = ctypes.c_int64(-5)
    a = dict(norm=P, rows=2, nb=256, ld=256, nlev=3, sums=None, ld_level=0, ld_row=0, thr=thr, cands=P, cap=4, ws=P,
             ws_bytes=1 << 20)
    a.update(kw)
    rc = lib.pu_harmonic_search(a["norm"], a["rows"], a["nb"], a["ld"], a["nlev"], a["sums"], a["ld_level"], a["ld_row"],
                                a["thr"], k0, k1, a["cands"], a["cap"], ctypes.byref(count), a["ws"], a["ws_bytes"], None)
    assert rc == EINVAL
    assert word in _msg(lib)


def test_spec_cand_record_is_24_bytes():
    from pulsarutils import _hip
    assert _hip.SPEC_CAND_DTYPE.itemsize == 24
    assert [_hip.SPEC_CAND_DTYPE.fields[n][1] for n in ("row", "level", "bin", "power", "pad")] == [0, 4, 8, 16, 20]
