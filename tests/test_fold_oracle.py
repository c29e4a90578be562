"""tests/fold_oracle.py checked against facts, not against the code under test (CPU only)."""
import math

import numpy as np

import fold_oracle as fo


def test_fractions_below_one_and_bins_in_range_far_into_a_file():
    for dphase, nbin, phase0 in ((1e-3 / 0.064, 64, 0.0), (0.3711, 17, -0.37), (1.0 / 8, 8, 0.0), (2.75, 1024, 0.5)):
        b, f = fo.bins(5000, dphase, nbin, phase0, first_sample=2 ** 40, return_frac=True)
        assert (f >= 0).all() and (f < 1).all()
        assert b.dtype == np.int64 and (b >= 0).all() and (b < nbin).all()


def test_samples_on_bin_edges_open_the_next_bin():
    # phase0 = 0, dphase = 1/8, 8 bins: sample t sits exactly on the lower edge of bin t mod 8
    b = fo.bins(64, 1.0 / 8, 8)
    assert np.array_equal(b, np.arange(64) % 8)


def test_constant_array_folds_to_constant_times_counts():
    x = np.full((3, 4099), 7, np.uint8)
    sums, counts = fo.fold_exact(x, 0.0137, 17, -0.37)
    assert counts.sum() == 4099
    assert np.array_equal(sums, 7.0 * np.broadcast_to(counts, (3, 17)))
    fs, fc, fa = fo.fold_fsum(x.astype(np.float64), 0.0137, 17, -0.37)
    assert np.array_equal(fs, sums) and np.array_equal(fc, counts) and np.array_equal(fa, sums)


def test_fold_of_two_halves_sums_to_the_fold_of_the_whole():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (3, 1000)).astype(np.uint8)
    whole, cw = fo.fold_exact(x, 0.0371, 64, -0.37, first_sample=2 ** 40)
    a, ca = fo.fold_exact(x[:, :437], 0.0371, 64, -0.37, first_sample=2 ** 40)
    b, cb = fo.fold_exact(x[:, 437:], 0.0371, 64, -0.37, first_sample=2 ** 40 + 437)
    assert np.array_equal(a + b, whole) and np.array_equal(ca + cb, cw)
    assert whole.sum() == x.astype(np.int64).sum()


def test_fsum_fold_agrees_with_the_integer_fold_on_integers():
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (2, 777))
    want, counts = fo.fold_exact(x, 0.11, 17)
    got, c, _ = fo.fold_fsum(x.astype(np.float64), 0.11, 17)
    assert np.array_equal(got, want) and np.array_equal(c, counts)


def test_delta_profile_has_z2_of_two_m_a():
    for n, a, at in ((32, 5.0, 0), (100, 37.0, 41), (1021, 3.0, 1020)):
        p = np.zeros(n)
        p[at] = a
        nmax = min(20, n - 1)
        for zs in (fo.z2_all(p, nmax), fo.z2_all_fast(p, nmax)):
            for m, z in enumerate(zs, start=1):
                assert abs(z - 2.0 * m * a) <= fo.z2_tolerance(n, m, a)


def test_flat_profile_has_h_zero_at_m_one():
    for n in (10, 32, 100):
        p = np.full(n, 20.0)
        zs = fo.z2_all(p, n // 2)
        assert max(abs(z) for z in zs) < 1e-20 * n * 20 + 1e-9
        h, m, _ = fo.h_from_z2(zs)
        assert m == 1 and abs(h) < 1e-9


def test_zero_and_nan_profiles_are_nan():
    for p in (np.zeros(16), np.array([1.0, np.nan, 2.0, 3.0]), np.array([1.0, np.inf, 2.0]), -np.ones(8)):
        zs = fo.z2_all_fast(p, 2)
        assert all(math.isnan(z) for z in zs)
        h, m, _ = fo.h_from_z2(zs)
        assert math.isnan(h) and m == 0


def test_fast_and_plain_z2_agree():
    rng = np.random.default_rng(7)
    p = rng.poisson(20, 100).astype(np.float64)
    p[40:50] += 30
    a, b = fo.z2_all(p, 20), fo.z2_all_fast(p, 20)
    for m, (u, v) in enumerate(zip(a, b), start=1):
        assert abs(u - v) <= fo.z2_tolerance(100, m, p.sum())
    assert fo.h_from_z2(a)[1] == fo.h_from_z2(b)[1]
    # beyond n / 2 the fast form mirrors the harmonics: still the plain sums
    for q in (p[:32], p[:33]):
        a, b = fo.z2_all(q, q.size - 1), fo.z2_all_fast(q, q.size - 1)
        for m, (u, v) in enumerate(zip(a, b), start=1):
            assert abs(u - v) <= fo.z2_tolerance(q.size, m, q.sum())
