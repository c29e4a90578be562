"""tests/accel_oracle.py pinned: the index map against exact rational arithmetic, and the
detection scenario of tests/test_gpu_accel.py searched on the host alone (CPU only)."""
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy import special, stats

import accel_oracle as ao

SPECIAL_AF = (1e-3, -1e-3, 1.0, -1.0, float("nan"), float("inf"), float("-inf"))


@pytest.mark.parametrize("n", [257, 4096])
def test_identity_end_points_and_range(n):
    assert np.array_equal(ao.resample_indices(n, 0.0), np.arange(n))
    assert np.array_equal(ao.resample_indices(n, -0.0), np.arange(n))
    for af in SPECIAL_AF + (1.0 / n, -1.0 / n, 0.3 / n):
        src = ao.resample_indices(n, af)
        assert src.dtype == np.int64 and src.shape == (n,)
        assert src[0] == 0, af
        assert src.min() >= 0 and src.max() <= n - 1, af
    for af in (1.0 / n, -1.0 / n, 0.3 / n, -0.71 / n, 1e-9):
        src = ao.resample_indices(n, af)
        assert np.all(np.diff(src) >= 0), af          # monotone while |af| n <= 1
        # the map's fixed points are 0 and n: the last sample moves by less than |af| n
        assert n - 2 <= src[-1] <= n - 1, af
    assert ao.resample_indices(n, 0.3 / n)[-1] == n - 1 and ao.resample_indices(n, -0.3 / n)[-1] == n - 1


def _rint_half_even(q):
    """rint of a Fraction, ties to even."""
    f = math.floor(q)
    d = q - f
    if d > Fraction(1, 2) or (d == Fraction(1, 2) and f % 2):
        return f + 1
    return f


def test_rounding_against_exact_rationals():
    """A few hundred (i, n, af) with af a short binary fraction: af i (i - n) is then exact in
    float64, exact ties occur, and Python's rationals say what rint and the clamp must give."""
    rng = np.random.default_rng(2)
    afs = [Fraction(s * num, 2 ** m) for num, m in ((1, 1), (1, 2), (3, 4), (1, 10), (5, 13), (1, 20), (3, 22))
           for s in (1, -1)]
    checked = ties = clamped = 0
    for n in (257, 4096, 65536):
        picks = np.unique(np.concatenate(([0, 1, 2, n // 2, n - 2, n - 1], rng.integers(0, n, 12))))
        for af in afs:
            src = ao.resample_indices(n, float(af))
            for i in picks.tolist():
                q = af * i * (i - n)
                assert Fraction(float(af) * float(i * (i - n))) == q   # the product is exact here
                ties += (q - math.floor(q)) == Fraction(1, 2)
                s = _rint_half_even(q)
                clamped += not -i <= s <= n - 1 - i
                want = i + min(max(s, -i), n - 1 - i)
                assert src[i] == want, (i, n, af)
                checked += 1
    assert checked >= 300 and ties >= 10 and clamped >= 10, (checked, ties, clamped)


def test_resample_is_the_gather_and_the_inverse_is_exact():
    x = np.arange(2 * 300, dtype=np.float32).reshape(2, 300)
    af = 0.8 / 300
    src = ao.resample_indices(300, af)
    assert np.array_equal(ao.resample(x, af), x[:, src]) and np.array_equal(ao.resample(x[1], af), x[1, src])
    assert np.array_equal(ao.resample(x, 0.0), x)
    for af in (0.0, 2e-7, -2e-7, 6.3e-7):
        n = 2 ** 14
        i = np.arange(n, dtype=np.float64)
        u = i + af * i * (i - n)
        assert np.abs(ao.emitted_index(u, n, af) - i).max() <= 1e-6


def _sigma(power, nharm):
    """The Gaussian equivalent of the single-trial tail probability of an Erlang(nharm) sum."""
    return float(-special.ndtri_exp(stats.gamma.logsf(power, a=nharm)))


def test_detection_scenario_on_the_host():
    """The pulse train drifts about 8 bins at the fundamental: searched as it is, no harmonic sum
    reaches 6 sigma; resampled at the true acceleration the 16-harmonic sum is far above 12 sigma
    at 23.7 Hz.  Measured: 4.9 and 19.1 sigma."""
    x = ao.drifting_rows()
    assert x.shape == (2, ao.N) and x.dtype == np.float32
    tobs = ao.N * ao.DT
    drift = ao.F0 * ao.ACCEL * tobs ** 2 / ao.C
    assert 7.5 < drift < 8.5
    raw = [_sigma(p, 1 << lv) for lv, (p, _) in enumerate(ao.best_sums(x[0]))]
    print("as is: sigma per level", np.round(raw, 2).tolist())
    assert max(raw) < 6.0
    fixed = ao.best_sums(ao.resample(x[0], ao.accel_factor(ao.ACCEL, ao.DT)))
    sig = [_sigma(p, 1 << lv) for lv, (p, _) in enumerate(fixed)]
    print("resampled: sigma per level", np.round(sig, 2).tolist(), "bins", [k for _, k in fixed])
    assert sig[4] > 12.0
    assert abs(fixed[4][1] / 16 / tobs - ao.F0) <= 1 / (16 * tobs)
    noise = [_sigma(p, 1 << lv) for lv, (p, _) in enumerate(ao.best_sums(x[1]))]
    assert max(noise) < 6.0
