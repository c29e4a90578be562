"""pu_fold_trials / pu_profile_chi2 validate their arguments before any HIP call, and
folding.frequency_grid is pure numpy (CPU only)."""
import math

import numpy as np
import pytest

EINVAL, EUNSUPPORTED = -1, -4
F32, F64 = 1, 2
# never dereferenced on the paths below: every case returns before any HIP call
P = 4096


def _msg(lib):
    return lib.pu_last_error().decode()


@pytest.fixture(scope="module")
def lib():
    from pulsarutils import _hip
    return _hip.lib()


def _trials(lib, dtype=F32, rows=2, n=100, ld=100, first=0, ntrials=5, nbin=16, ld_trial=None, ld_row=None,
            ws=P, ws_bytes=1 << 20, x=P, phase0=P, dphase=P):
    ld_trial = nbin if ld_trial is None else ld_trial
    ld_row = ntrials * ld_trial if ld_row is None else ld_row
    return lib.pu_fold_trials(x, dtype, rows, n, ld, first, phase0, dphase, ntrials, nbin, P, ld_trial, ld_row, P, ws,
                              ws_bytes, None)


@pytest.mark.parametrize("kw, word", [
    (dict(nbin=1), "nbin"),
    (dict(nbin=0), "nbin"),
    (dict(nbin=-3), "nbin"),
    (dict(n=-1, ld=0), "negative"),
    (dict(rows=-1), "negative"),
    (dict(ntrials=-1, ld_row=0), "negative"),
    (dict(ld=99), "leading dimension"),
    (dict(ld_trial=15), "leading dimension"),
    (dict(ld_row=5 * 16 - 1), "leading dimension"),
    (dict(ws_bytes=2 * 5 * 16 * 8 - 1), "workspace"),    # one byte short of rows x 1 segment x trials x bins x 8
    (dict(ws=P + 4), "workspace"),                       # not 8-byte aligned
    (dict(ws=None), "workspace"),
    (dict(x=None), "null"),
    (dict(dphase=None), "null"),
])
def test_fold_trials_rejects_bad_arguments_without_a_gpu(lib, kw, word):
    assert _trials(lib, **kw) == EINVAL
    assert word in _msg(lib) and "pu_fold_trials" in _msg(lib)


def test_fold_trials_unsupported_without_a_gpu(lib):
    assert _trials(lib, dtype=0) == EUNSUPPORTED and "dtype" in _msg(lib)   # PU_U8
    assert _trials(lib, dtype=3) == EUNSUPPORTED and "dtype" in _msg(lib)
    assert _trials(lib, nbin=257) == EUNSUPPORTED and "256" in _msg(lib)
    assert _trials(lib, nbin=100000) == EUNSUPPORTED


def test_fold_trials_of_nothing_is_ok_without_a_launch(lib):
    for kw in (dict(n=0), dict(rows=0), dict(ntrials=0), dict(n=0, x=None, ws=None, ws_bytes=0)):
        assert _trials(lib, **kw) == 0, kw
    assert lib.pu_fold_trials_workspace_bytes(0, 100, 5, 16) == 0
    assert lib.pu_fold_trials_workspace_bytes(3, 16385, 5, 17) == 3 * 2 * 5 * 17 * 8
    assert lib.pu_fold_trials_workspace_bytes(2, 100, 5, 16) == 2 * 5 * 16 * 8


def _chi2(lib, rows=2, ntrials=5, nbin=16, ld_trial=None, ld_row=None, sums=P, counts=P, mean=P, var=P, chi2=P, dof=P):
    ld_trial = nbin if ld_trial is None else ld_trial
    ld_row = ntrials * ld_trial if ld_row is None else ld_row
    return lib.pu_profile_chi2(sums, ld_trial, ld_row, counts, rows, ntrials, nbin, mean, var, chi2, dof, None)


@pytest.mark.parametrize("kw, word", [
    (dict(nbin=1), "nbin"),
    (dict(rows=-1), "negative"),
    (dict(ntrials=-2, ld_row=0), "negative"),
    (dict(ld_trial=15), "leading dimension"),
    (dict(ld_row=79), "leading dimension"),
    (dict(sums=None), "null"),
    (dict(dof=None), "null"),
])
def test_profile_chi2_rejects_bad_arguments_without_a_gpu(lib, kw, word):
    assert _chi2(lib, **kw) == EINVAL
    assert word in _msg(lib) and "pu_profile_chi2" in _msg(lib)


def test_profile_chi2_of_nothing_is_ok_without_a_launch(lib):
    assert _chi2(lib, rows=0) == 0
    assert _chi2(lib, ntrials=0, sums=None) == 0


def test_period_functions_import_without_a_gpu():
    from pulsarutils import folding
    for name in ("frequency_grid", "fold_trials", "frequency_search"):
        assert callable(getattr(folding, name)) and name in folding.__all__


def test_frequency_grid_end_points_and_count():
    from pulsarutils import folding
    g = folding.frequency_grid(6.8, 7.8, 40.0)
    df = 1.0 / (8 * 40.0)
    nk = math.ceil((7.8 - 6.8) / df)
    assert g.dtype == np.float64 and g.shape == (nk + 1,) and nk == 320
    assert g[0] == 6.8 and g[-1] >= 7.8 and g[-2] < 7.8
    assert np.array_equal(g, 6.8 + np.arange(nk + 1) * df)
    # a span that is no multiple of df: the last trial is the first one beyond fmax
    g = folding.frequency_grid(1.0, 1.01, 10.0, oversample=3)
    assert g.size == math.ceil(0.01 * 30) + 1 == 2 and g[0] == 1.0 and g[1] == 1.0 + 1 / 30.0 > 1.01
    assert folding.frequency_grid(5.0, 5.0, 10.0).tolist() == [5.0]
    assert folding.frequency_grid(0.0, 1.0, 2.0, oversample=0.5).tolist() == [0.0, 1.0]


@pytest.mark.parametrize("args", [(2.0, 1.0, 10.0), (1.0, 2.0, 0.0), (1.0, 2.0, -1.0), (1.0, 2.0, 10.0, 0),
                                  (1.0, 2.0, 10.0, -2), (math.nan, 2.0, 10.0)])
def test_frequency_grid_errors(args):
    from pulsarutils import folding
    with pytest.raises(ValueError):
        folding.frequency_grid(*args)
