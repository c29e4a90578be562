"""The FFA's definition on the CPU: the level tables the kernels walk against the recursion, the
shifts the tree applies, the radix-2 special case, and a synthetic pulsar through the oracle."""
import numpy as np
import pytest

import ffa_oracle as fo
from pulsarutils import ffa

MS = list(range(1, 71)) + [100, 257, 419, 1000]


@pytest.mark.parametrize("p", [5, 16])
def test_tables_reproduce_the_recursion(p):
    rng = np.random.default_rng(p)
    for m in MS:
        x = rng.standard_normal((m, p)).astype(np.float32)
        x[0, 0] = -0.0  # a copied row keeps its sign of zero
        tables = ffa.ffa_tables(m)
        assert len(tables) == (m - 1).bit_length()
        want, got = fo.ffa(x), fo.apply_tables(x, tables)
        assert got.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32)), m


def test_tables_layout():
    for m in MS:
        tables = ffa.ffa_tables(m)
        for lv, (head, tail, rot) in enumerate(tables):
            assert head.shape == tail.shape == rot.shape == (m,)
            copies = tail < 0
            assert lv == 0 or not copies.any()  # one-row blocks exist at the bottom level only
            assert np.all(head[copies] == np.flatnonzero(copies)) and np.all(rot[copies] == 0)
            assert np.all((head >= 0) & (head < m) & (tail < m) & (rot >= 0) & (rot < m))
    with pytest.raises(ValueError):
        ffa.ffa_tables(0)


def test_shift_properties():
    for m in MS:
        sh = fo.shifts(m)
        assert sh.shape == (m, m)
        assert np.all(np.diff(sh, axis=1) >= 0), m          # non-decreasing in the input row
        assert np.all(sh[0] == 0), m                        # trial 0: the plain fold
        assert np.all(sh[m - 1] == np.arange(m)), m         # the last trial shifts row i by i
        if m > 1:
            ideal = np.arange(m)[:, None] * np.arange(m)[None, :] / (m - 1)
            assert np.abs(sh - ideal).max() < 3, m


def test_transform_is_the_fold_at_those_shifts():
    rng = np.random.default_rng(7)
    for m, p in ((1, 4), (3, 4), (13, 33), (70, 9)):
        x = rng.integers(-50, 50, (m, p)).astype(np.float32)  # integer sums: exact in any order
        assert np.array_equal(fo.ffa(x).astype(np.float64), fo.brute_fold(x, fo.shifts(m)))
        assert np.array_equal(fo.ffa(x)[0].astype(np.float64), x.astype(np.float64).sum(axis=0))


@pytest.mark.parametrize("m", [2, 4, 8, 64, 512])
def test_powers_of_two_are_the_radix2_ffa(m):
    tables = ffa.ffa_tables(m)
    for lv, (head, tail, rot) in enumerate(tables):
        size = 2 << lv  # the blocks of this level
        g = np.arange(m)
        start, s = g - g % size, g % size
        assert np.array_equal(head, start + s // 2)
        assert np.array_equal(tail, start + size // 2 + s // 2)
        assert np.array_equal(rot, s - s // 2)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_synthetic_pulsar_is_detected(seed):
    p, m, trial = 250, 419, 137
    period = p + trial / (m - 1)
    series = fo.pulsar_series(m * p, period, 0.02, 0.35, seed)
    widths = ffa.default_widths(p)
    snr, _ = fo.snr_table(fo.ffa_series(series, p), widths, sigma=float(series.std()))
    s, k = np.unravel_index(np.argmax(snr), snr.shape)
    print("seed", seed, "row", s, "width", widths[k], "snr", snr[s, k])
    assert abs(int(s) - trial) <= 2
    assert widths[k] in (4, 6)
    assert snr[s, k] > 12
