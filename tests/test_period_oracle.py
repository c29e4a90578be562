"""tests/period_oracle.py pinned against facts (CPU only): a constant series has chi^2 = 0, a
series that is 1 on exactly one phase bin has a chi^2 worked out by hand, empty bins lower the
degrees of freedom, a trial whose phase cannot be binned is NaN, and the tolerance is what its
docstring derives."""
import math

import numpy as np

import fold_oracle as fo
import period_oracle as po


def test_a_constant_series_has_chi2_zero():
    x = np.full((1, 1000), 3.0)
    sums, counts, _ = po.fold_trials(x, [0.125, 1e-3, 0.0137], 8, exact=True)
    got, dof = po.chi2_all(sums, counts, [3.0], [2.0])
    assert np.array_equal(got, np.zeros((1, 3)))
    # dphase = 1e-3 over 1000 samples covers the turn once: all 8 bins hit
    assert dof.tolist() == [7, 7, 7]


def test_one_lit_phase_bin_gives_the_hand_computed_chi2():
    """n = 64, dphase = 1/8, nbin = 8: sample t is in bin t mod 8 exactly, 8 samples per bin.
    x = 1 on bin 3 and 0 elsewhere: mean = 1/8, var = 1/8 - 1/64 = 7/64.  Bin 3: (8 - 1)^2 /
    (8 * 7/64) = 49 / (7/8) = 56; each of the 7 others: (0 - 1)^2 / (7/8) = 8/7; chi^2 = 56 + 8 =
    64 = n: all of the variance is in the profile."""
    n, nbin = 64, 8
    x = np.zeros((1, n))
    x[0, 3::8] = 1.0
    sums, counts, _ = po.fold_trials(x, [0.125], nbin, exact=True)
    assert counts.tolist() == [[8] * 8]
    assert sums[0, 0].tolist() == [0, 0, 0, 8, 0, 0, 0, 0]
    mean, var = x.mean(), (x ** 2).mean() - x.mean() ** 2
    assert (mean, var) == (0.125, 7 / 64)
    got, dof = po.chi2(sums[0, 0], counts[0], mean, var)
    assert dof == 7 and abs(got - 64.0) <= 64 * 2 ** -50
    # at dphase = 1/4 the lit samples alternate between bins 3 * 2 = 6 and 14 mod 8 = 6: one bin
    # holds them all, bins 0, 2, 4, 6 are hit (16 samples each), the odd ones are empty
    sums, counts, _ = po.fold_trials(x, [0.25], nbin, exact=True)
    assert counts.tolist() == [[16, 0, 16, 0, 16, 0, 16, 0]]
    got, dof = po.chi2(sums[0, 0], counts[0], mean, var)
    # bin 6: (8 - 2)^2 / (16 * 7/64) = 36 / 1.75; three others: (0 - 2)^2 / 1.75 each
    assert dof == 3 and abs(got - (36 + 12) / 1.75) <= 2 ** -45


def test_dof_counts_only_the_bins_that_were_hit():
    # dphase = 0: every sample in bin floor(0.3 * 5) = 1
    x = np.arange(20, dtype=np.float64)[None]
    sums, counts, _ = po.fold_trials(x, [0.0], 5, phase0s=[0.3], exact=True)
    assert counts.tolist() == [[0, 20, 0, 0, 0]] and sums[0, 0, 1] == 190
    got, dof = po.chi2(sums[0, 0], counts[0], 9.5, 33.25)
    assert dof == 0 and got == 0.0


def test_chi2_is_nan_without_a_variance_or_with_a_non_finite_sum():
    c = np.array([4, 4])
    assert math.isnan(po.chi2([1.0, 2.0], c, 0.5, 0.0)[0])
    assert math.isnan(po.chi2([1.0, 2.0], c, 0.5, -1.0)[0])
    assert math.isnan(po.chi2([1.0, 2.0], c, 0.5, math.nan)[0])
    assert math.isnan(po.chi2([math.inf, 2.0], c, 0.5, 1.0)[0])
    # in an empty bin too: a trial the fold filled with NaN scores NaN (dof -1), not 0
    assert math.isnan(po.chi2([math.inf, 2.0], np.array([0, 4]), 0.5, 1.0)[0])
    got, dof = po.chi2([math.nan, math.nan], np.array([0, 0]), 0.5, 1.0)
    assert math.isnan(got) and dof == -1


def test_bad_trials_are_nan_with_no_counts_and_leave_the_others_alone():
    x = np.arange(12, dtype=np.float64)[None]
    dph = [0.125, math.inf, 0.125, math.nan, 2.0 ** 52]
    sums, counts, _ = po.fold_trials(x, dph, 4, exact=True)
    for k in (1, 3, 4):
        assert np.isnan(sums[:, k]).all() and not counts[k].any()
    want, wc = fo.fold_exact(x, 0.125, 4)
    for k in (0, 2):
        assert np.array_equal(sums[:, k], want) and np.array_equal(counts[k], wc)
    assert po.trial_is_bad(10, 1.0, 0.0, 2 ** 52 - 5) and not po.trial_is_bad(5, 1.0, 0.0, 2 ** 52 - 5)
    assert po.trial_is_bad(10, 0.1, -2.0 ** 52) and po.trial_is_bad(10, 0.1, math.inf)


def test_float_fold_returns_the_abs_sums_of_fold_fsum():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 300))
    sums, counts, abs_sums = po.fold_trials(x, [0.013, 0.5], 7, phase0s=[0.1, -0.2], first_sample=9)
    w = fo.fold_fsum(x, 0.5, 7, -0.2, 9)
    assert np.array_equal(sums[:, 1], w[0]) and np.array_equal(counts[1], w[1]) and np.array_equal(abs_sums[:, 1], w[2])


def test_tolerance_follows_its_derivation():
    """One bin, d = 3, c = 4, mean = 0.5, var = 2: T = 9 / 8, e_d = u (2 + 3); tol = 2 (6 e_d +
    e_d^2) / 8 + 8 u T + (nbin + 1) u T, and an error in the sums enters through e_d."""
    u = 2.0 ** -53
    ed = 5 * u
    want = 2 * (6 * ed + ed * ed) / 8 + 8 * u * 1.125 + 3 * u * 1.125
    got = po.chi2_tolerance(2, [5.0, 0.0], [4, 0], 0.5, 2.0)
    assert abs(got - want) <= 1e-12 * want
    ed = 5 * u + 1e-9
    want = 2 * (6 * ed + ed * ed) / 8 + 11 * u * 1.125
    assert abs(po.chi2_tolerance(2, [5.0, 0.0], [4, 0], 0.5, 2.0, sums_err=[1e-9, 0.0]) - want) <= 1e-12 * want
    # and it covers the rounding of a plain float64 evaluation of a long profile
    rng = np.random.default_rng(1)
    s, c = rng.standard_normal(256) * 30, rng.integers(1, 200, 256)
    exact = po.chi2(s, c, 0.01, 1.3)[0]
    plain = 0.0
    for b in range(256):
        d = s[b] - float(c[b]) * 0.01
        plain += d * d / (float(c[b]) * 1.3)
    assert abs(plain - exact) <= po.chi2_tolerance(256, s, c, 0.01, 1.3)
