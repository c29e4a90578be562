"""tests/spectrum_oracle.py pinned against hand-computed facts (CPU only)."""
import numpy as np

import spectrum_oracle as so

F32 = np.float32


def test_pure_tone_on_a_bin():
    nfft, k0 = 256, 19
    t = np.arange(nfft)
    x = np.cos(2 * np.pi * k0 * t / nfft).astype(F32)
    spec = so.rfft(x, nfft)
    mag = np.abs(spec[0])
    assert np.argmax(mag) == k0 and abs(mag[k0] - nfft / 2) < 1e-4
    assert np.delete(mag, k0).max() < 1e-4  # float32 rounding of the samples only
    # zero padding and the mean: half the samples of a constant 3 minus its mean are zeros all through
    assert np.all(so.padded_samples(np.full(100, 3.0), 256, mean=[3.0]) == 0)
    y = so.padded_samples(np.array([1.0, 2.0, 4.0]), 256, mean=[0.5])
    assert y.dtype == F32 and y[0, :4].tolist() == [0.5, 1.5, 3.5, 0.0]


def test_harmonic_index_rule_written_out():
    nb = 64
    norm = np.arange(nb, dtype=F32).reshape(1, nb) * F32(0.25) + F32(1)
    s = so.harmonic_sums(norm, 3)
    n = norm[0]
    for k in (0, 1, 7, 10, 63):
        # H = 2: the top harmonic k and bin (k + 1) // 2
        assert s[1, 0, k] == n[k] + n[(k + 1) // 2]
        # H = 4: then m = 1, 3 over 4: (k + 2) // 4 and (3 k + 2) // 4, in that order
        assert s[2, 0, k] == F32(F32(n[k] + n[(k + 1) // 2]) + n[(k + 2) // 4]) + n[(3 * k + 2) // 4]
    assert [(10 * m + 2) // 4 for m in (1, 3)] == [3, 8] and (10 + 1) // 2 == 5


def _spec_from_power(p):
    """A complex64 spectrum whose float32 power is exactly ``p`` (perfect squares)."""
    return np.sqrt(np.asarray(p, dtype=np.float64)).astype(np.complex64)


def test_block_zero_median_and_scaling():
    block, nb = 16, 32
    p = np.zeros(nb)
    p[:16] = np.arange(16) ** 2          # block 0: 0 (DC, left out), 1, 4 .. 225
    p[16:] = (np.arange(16) + 1) ** 2    # block 1: 1, 4 .. 256
    out = so.normalize(_spec_from_power(p).reshape(1, -1), nb, block)
    # block 0: the median of the 15 real bins 1 .. 225 is the 8th: 64; DC is 0 whatever it held
    med0 = F32(64)
    assert out[0, 0] == 0
    assert np.array_equal(out[0, 1:16], p[1:16].astype(F32) * (so.LN2 / med0))
    # block 1: 0.5 (64 + 81)
    med1 = F32(0.5) * F32(64 + 81)
    assert np.array_equal(out[0, 16:], p[16:].astype(F32) * (so.LN2 / med1))
    # a huge DC power does not reach block 0's median
    p[0] = 1e30
    assert np.array_equal(so.normalize(_spec_from_power(p).reshape(1, -1), nb, block), out)


def test_nan_block_and_zero_block():
    block, nb = 16, 48
    spec = np.ones((1, nb), np.complex64)
    spec[0, 20] = np.nan                 # block 1
    spec[0, 32:] = 0                     # block 2: median 0
    spec[0, 40] = 3                      # (one bin above a zero median)
    out = so.normalize(spec, nb, block)
    assert np.all(np.isnan(out[0, 16:32])) and np.all(out[0, 32:] == 0)
    assert out[0, 0] == 0 and np.all(out[0, 1:16] == so.LN2)
    # a NaN DC bin alone does not poison block 0
    spec[0, 0] = np.nan
    assert np.all(so.normalize(spec, nb, block)[0, 1:16] == so.LN2)
    # an infinite power does
    spec[0, 3] = np.inf
    assert np.all(np.isnan(so.normalize(spec, nb, block)[0, 1:16])) and so.normalize(spec, nb, block)[0, 0] == 0


def test_peak_and_tie_rule():
    s = np.zeros((1, 1, 12), F32)
    s[0, 0] = [5, 1, 3, 3, 1, 4, 2, 2, 2, 0, np.nan, 6]
    none, full = [0], [12]
    got = so.candidates(s, [0.5], none, full)
    # bin 0: left is -inf, 5 >= 1; bins 2, 3 tie: only the first (3 > 1 and 3 >= 3; then 3 > 3 fails);
    # bin 5; the plateau 2 2 2 has no bin above its left neighbour; bin 11 sits next to a NaN: 6 > NaN
    # is false
    assert got["bin"].tolist() == [0, 2, 5]
    assert got["power"].tolist() == [5, 3, 4] and got["row"].tolist() == [0, 0, 0] and got["level"].tolist() == [0, 0, 0]
    s[0, 0, 10] = 0
    assert so.candidates(s, [0.5], none, full)["bin"].tolist() == [0, 2, 5, 11]  # right of bin 11 is -inf
    assert so.candidates(s, [4.0], none, full)["bin"].tolist() == [0, 11]       # strictly above the threshold
    assert so.candidates(s, [0.5], [1], [11])["bin"].tolist() == [2, 5]          # kmin <= k < kmax
    # the order is (row, level, bin)
    two = np.zeros((2, 2, 4), F32)
    two[:, :, 1] = 9
    got = so.candidates(two, [1, 1], [0, 0], [4, 4])
    assert [(c["row"], c["level"], c["bin"]) for c in got] == [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
