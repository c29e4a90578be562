"""pu_fold / pu_h_test validate their arguments before any HIP call, pulsarutils.folding imports
without a GPU and its fold_bins is the oracle's bin rule (CPU only)."""
import numpy as np
import pytest

import fold_oracle as fo

EINVAL, EUNSUPPORTED = -1, -4
# pu_fold never dereferences these on the paths below: every case fails validation first
P = 4096


def _fold(lib, dtype=0, nchan=2, n=100, ld=100, first=0, phase0=0.0, dphase=0.01, nbin=16, ld_sums=None,
          ws_bytes=1 << 20):
    return lib.pu_fold(P, dtype, nchan, n, ld, first, phase0, dphase, nbin, P, nbin if ld_sums is None else ld_sums,
                       P, P, ws_bytes, None)


def _msg(lib):
    return lib.pu_last_error().decode()


@pytest.fixture(scope="module")
def lib():
    from pulsarutils import _hip
    return _hip.lib()


@pytest.mark.parametrize("kw, word", [
    (dict(nbin=0), "nbin"),
    (dict(nbin=-3), "nbin"),
    (dict(n=-1, ld=0), "negative"),
    (dict(ld=99), "leading dimension"),
    (dict(ld_sums=15), "leading dimension"),
    (dict(dphase=float("nan")), "finite"),
    (dict(dphase=float("inf")), "finite"),
    (dict(phase0=float("nan")), "finite"),
    (dict(first=2 ** 52, dphase=1.0), "2^52"),            # the phase overflows at the chunk's start
    (dict(first=2 ** 52 - 50, dphase=1.0), "2^52"),       # ... at its end only
    (dict(phase0=-2.0 ** 52), "2^52"),
    (dict(ws_bytes=8), "workspace"),
])
def test_fold_rejects_bad_arguments_without_a_gpu(lib, kw, word):
    assert _fold(lib, **kw) == EINVAL
    assert word in _msg(lib) and "pu_fold" in _msg(lib)


def test_fold_unsupported_without_a_gpu(lib):
    assert _fold(lib, nbin=8193) == EUNSUPPORTED and "8192" in _msg(lib)
    assert _fold(lib, dtype=3) == EUNSUPPORTED and "dtype" in _msg(lib)


def test_fold_of_nothing_is_ok_without_a_launch(lib):
    assert _fold(lib, n=0) == 0
    assert _fold(lib, nchan=0) == 0
    assert lib.pu_fold_workspace_bytes(0, 100, 16) == 0
    assert lib.pu_fold_workspace_bytes(3, 16385, 17) == 2 * 3 * 17 * 8


def _h(lib, rows=1, n=32, ld=None, nmax=3, zs=0, ld_zs=0, ws_bytes=1 << 20):
    return lib.pu_h_test(P, rows, n, n if ld is None else ld, nmax, P, P, zs, ld_zs, P, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(n=1, nmax=1), EINVAL, "at least 2"),
    (dict(n=32, nmax=32), EINVAL, "nmax"),
    (dict(n=32, nmax=0), EINVAL, "nmax"),
    (dict(n=8193, nmax=20), EUNSUPPORTED, "FFT"),
    (dict(n=32, ld=31), EINVAL, "leading dimension"),
    (dict(n=32, nmax=5, zs=P, ld_zs=4), EINVAL, "leading dimension"),
    (dict(rows=-1), EINVAL, "rows"),
    (dict(ws_bytes=16), EINVAL, "workspace"),
])
def test_h_test_rejects_bad_arguments_without_a_gpu(lib, kw, code, word):
    assert _h(lib, **kw) == code
    assert word in _msg(lib) and "pu_h_test" in _msg(lib)


def test_h_test_of_no_rows_is_ok(lib):
    assert _h(lib, rows=0) == 0
    assert lib.pu_h_test_workspace_bytes(5, 100, 10) >= 100 * 16 + 5 * 10 * 8


def test_folding_imports_without_a_gpu():
    from pulsarutils import folding
    for name in ("fold_bins", "fold", "fold_file", "z_n_all", "h_test", "h_curve", "profile_stats"):
        assert callable(getattr(folding, name))


def test_h_curve_and_profile_stats_reject_before_the_gpu():
    from pulsarutils import folding
    from pulsarutils.clean import PulseInfo
    with pytest.raises(ValueError):
        folding.h_curve(np.ones((3, 9)))
    info = PulseInfo()
    info.allprofs = np.ones((4, 32))
    with pytest.raises(ValueError):
        folding.profile_stats(info)


@pytest.mark.parametrize("nsamples, pulse_freq, tsamp, nbin, ph0, first", [
    (4099, 1 / 0.064, 1e-3, 64, 0.0, 0),
    (1000, 1 / 0.064, 1e-3, 17, -0.37, 2 ** 40),
    (64, 125.0, 1e-3, 8, 0.0, 0),          # dphase = 1/8: every sample on a bin edge
    (1000, 2750.0, 1e-3, 1024, 0.25, 7),   # dphase > 1
    (10, 3.0, 1e-3, 1, 0.9, 0),
])
def test_fold_bins_is_the_oracle_rule(nsamples, pulse_freq, tsamp, nbin, ph0, first):
    from pulsarutils import folding
    got = folding.fold_bins(nsamples, pulse_freq, tsamp, nbin, ph0=ph0, first_sample=first)
    want = fo.bins(nsamples, tsamp * pulse_freq, nbin, ph0, first)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < nbin
