"""tests/detrend_oracle.py against scipy and its own definition, the red-noise scenario the GPU
test's thresholds rest on, and the argument checks of the three entry points (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import detrend_oracle as do
import ffa_oracle as fo
from pulsarutils import _hip, detrend

EINVAL, EUNSUPPORTED = -1, -4


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n, w", [(1, 1), (1, 7), (2, 5), (5, 11), (50, 1), (50, 3), (200, 21), (333, 101)])
def test_running_median_matches_scipy(dtype, n, w):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(n * 1000 + w)
    for x in (rng.standard_normal((3, n)).astype(dtype), rng.integers(-3, 4, (3, n)).astype(dtype)):
        want = ndimage.median_filter(x, size=(1, w), mode="nearest")
        assert np.array_equal(do.running_median(x, w), want)
        assert np.array_equal(do.running_median(x[0], w), want[0])


def test_running_median_order_and_nan():
    x = np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0, 0.0], np.float32)
    got = do.running_median(x, 3)
    # windows (clamped): [+0 +0 -0] [+0 -0 +0] [-0 +0 -0] [+0 -0 -0] [-0 -0 +0] [-0 +0 +0] [+0 +0 +0]
    assert np.array_equal(np.signbit(got), [False, False, True, True, True, False, False])
    y = np.array([1.0, np.inf, 3.0, -np.inf, np.nan, 2.0, 5.0, 4.0, 6.0], np.float64)
    got = do.running_median(y, 3)
    assert np.array_equal(np.isnan(got), [False, False, False, True, True, True, False, False, False])
    assert do.same_bits(got[3:6], np.full(3, np.nan))
    assert np.array_equal(got[:3], [1.0, 3.0, 3.0]) and np.array_equal(got[6:], [4.0, 5.0, 6.0])
    assert np.array_equal(do.running_median(-y, 3)[:3], [-1.0, -3.0, -3.0])
    assert do.same_bits(do.running_median(-y, 3)[3:6], np.full(3, np.nan))  # canonical: not -nan
    assert do.same_bits(do.from_keys(do.to_keys(y[:4]), np.float64), y[:4])


def test_detrend_plan_values():
    for plan in (do.detrend_plan, detrend.detrend_plan):
        assert plan(1200) == (11, 109)
        assert plan(31250) == (309, 101)
        assert plan(100) == (1, 101) and plan(50) == (1, 51) and plan(1) == (1, 1) and plan(2) == (1, 3)
        assert plan(101) == (1, 101) and plan(201) == (1, 201) and plan(202) == (2, 101)
        assert plan(1200, min_points=11) == (109, 11)
        for W in list(range(101, 3000, 7)) + [10 ** 6, 10 ** 9 + 7]:
            d, w = plan(W)
            assert d == max(1, W // 101) and w % 2 == 1 and 101 <= w <= 203
        with pytest.raises(ValueError):
            plan(0)
    with pytest.raises(ValueError):
        detrend.detrend_plan(10 ** 6, min_points=5000)  # a median over more blocks than the kernel takes


def test_interpolation_properties():
    rng = np.random.default_rng(3)
    med = rng.standard_normal((2, 40))
    assert do.same_bits(do.interpolate(med, 40, 1), med)  # d = 1: the block centres are the samples
    # a constant series: zero residual, whatever the plan
    for n, W in ((1000, 300), (1000, 7), (37, 1200)):
        x = np.full((2, n), 3.25, np.float32)
        assert np.array_equal(do.baseline(x, W), np.full((2, n), 3.25))
        assert np.array_equal(do.detrend(x, W), np.zeros((2, n), np.float32))
    # the head before the first block centre and the tail beyond the last one
    d, n = 7, 7 * 9 + 5
    med = rng.standard_normal((1, 9))
    base = do.interpolate(med, n, d)
    assert np.array_equal(base[0, :4], np.full(4, med[0, 0]))          # centre of block 0: sample 3
    assert np.array_equal(base[0, 8 * d + 3:], np.full(n - 8 * d - 3, med[0, 8]))
    assert base[0, 8 * d + 2] != med[0, 8]
    for b in range(9):
        assert base[0, b * d + 3] == med[0, b]                         # odd d: a sample on every centre
    assert do.same_bits(do.interpolate(med[:, :1], 11, 7), np.full((1, 11), med[0, 0]))  # one block
    # a NaN median reaches the samples that interpolate from it, and no other
    med[0, 4] = np.nan
    bad = np.isnan(do.interpolate(med, n, d)[0])
    assert np.array_equal(np.flatnonzero(bad), np.arange(3 * d + 4, 5 * d + 3))  # weight > 0: between centres 3 and 5


def best_snr(x, p=250):
    """The best S/N over the trials and default widths of base period p, normalised as the search
    normalises (mean and standard deviation of the row), and its period."""
    x = np.asarray(x, np.float64)
    sd = (x - x.mean()).std()
    F = fo.ffa_series((x - x.mean()).astype(np.float32), p)
    m = F.shape[0]
    snr, _ = fo.snr_table(F, [1, 2, 3, 4, 6, 9, 13, 19, 28, 42], sd)
    s = int(np.argmax(snr.max(axis=1)))
    return float(snr.max()), p + s / (m - 1)


def test_red_noise_scenario_on_the_oracle():
    """65536 samples, a 2 % duty top-hat of amplitude 0.8 every 250.37 samples, two slow sinusoids
    and a random walk: 26.4 on the white series, 3.0 on the red one, 21.6 after the detrend at a
    width of 1200 samples."""
    white, red = do.red_noise_series(0.8)
    assert do.detrend_plan(1200) == (11, 109)
    s_white, p_white = best_snr(white)
    s_red, _ = best_snr(red)
    s_det, p_det = best_snr(do.detrend(red, 1200))
    print(f"best S/N at base period 250: white {s_white:.2f}, red {s_red:.2f}, detrended {s_det:.2f}")
    assert s_white > 20 and abs(p_white - 250.37) < 0.01
    assert s_red < 7
    assert s_det > 10 and abs(p_det - 250.37) < 0.01


# ------------------------------------------------------------------ the C ABI without a GPU

def _err():
    return _hip.lib().pu_last_error().decode()


def test_running_median_describe():
    for dtype, es in ((np.float32, 4), (np.float64, 8)):
        for w in (1, 3, 101, 2047):
            info = detrend.describe(dtype, w)
            assert info["w_max"] == 2047 == detrend.MAX_WIDTH
            assert info["tile"] >= 64 and info["tile"] % 64 == 0
            assert info["lds_bytes"] == (info["tile"] + w - 1) * es <= 64 * 1024
    lib = _hip.lib()
    info = np.full(3, -7, np.int64)
    ip = info.ctypes.data_as(ctypes.c_void_p)
    assert lib.pu_running_median_describe(_hip.PU_F32, 5, ip, 1) == 0 and info[0] > 0 and info[1] == -7
    assert lib.pu_running_median_describe(_hip.PU_U8, 5, ip, 3) == EUNSUPPORTED and "dtype" in _err()
    assert lib.pu_running_median_describe(_hip.PU_F32, 4, ip, 3) == EINVAL and "odd" in _err()
    assert lib.pu_running_median_describe(_hip.PU_F32, 0, ip, 3) == EINVAL
    assert lib.pu_running_median_describe(_hip.PU_F32, 2049, ip, 3) == EUNSUPPORTED and "2047" in _err()
    assert lib.pu_running_median_describe(_hip.PU_F32, 5, None, 3) == EINVAL
    with pytest.raises(ValueError):
        detrend.describe(np.float32, 2)


def test_running_median_argument_checks_without_gpu():
    """Every check comes before any HIP call: the pointers are never dereferenced."""
    lib = _hip.lib()
    x, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x80000)
    call = lib.pu_running_median
    assert call(x, _hip.PU_F32, 0, 100, 100, 5, out, 100, None) == 0          # rows == 0: no launch
    assert call(x, _hip.PU_I64, 1, 100, 100, 5, out, 100, None) == EUNSUPPORTED and "dtype" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, 4, out, 100, None) == EINVAL and "odd" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, -1, out, 100, None) == EINVAL
    assert call(x, _hip.PU_F64, 1, 100, 100, 2049, out, 100, None) == EUNSUPPORTED
    assert call(x, _hip.PU_F32, -1, 100, 100, 5, out, 100, None) == EINVAL
    assert call(x, _hip.PU_F32, 1, 0, 100, 5, out, 100, None) == EINVAL
    assert call(x, _hip.PU_F32, 1, 100, 99, 5, out, 100, None) == EINVAL and "ld" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, 5, out, 99, None) == EINVAL and "ld" in _err()
    assert call(None, _hip.PU_F32, 1, 100, 100, 5, out, 100, None) == EINVAL and "NULL" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, 5, None, 100, None) == EINVAL and "NULL" in _err()
    assert call(ctypes.c_void_p(0x10004), _hip.PU_F64, 1, 100, 100, 5, out, 100, None) == EINVAL and "aligned" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, 5, x, 100, None) == EINVAL and "overlap" in _err()
    assert call(x, _hip.PU_F32, 2, 100, 100, 5, ctypes.c_void_p(0x10000 + 4 * 199), 100, None) == EINVAL
    assert call(x, _hip.PU_F32, 1 << 40, 1 << 40, 1 << 40, 5, out, 1 << 40, None) == EUNSUPPORTED
    assert call(x, _hip.PU_F32, 2, 100, 1 << 62, 5, out, 100, None) == EINVAL and "address space" in _err()
    assert call(x, _hip.PU_F32, 2, 100, 100, 5, out, (1 << 62) + 1, None) == EINVAL and "address space" in _err()


def test_detrend_apply_argument_checks_without_gpu():
    lib = _hip.lib()
    x, med, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x40000), ctypes.c_void_p(0x80000)
    call = lib.pu_detrend_apply
    assert call(x, _hip.PU_F32, 0, 100, 100, med, 14, 14, 7, out, 100, None) == 0   # rows == 0: no launch
    assert call(x, _hip.PU_U8, 1, 100, 100, med, 14, 14, 7, out, 100, None) == EUNSUPPORTED and "dtype" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, med, 14, 14, 0, out, 100, None) == EINVAL and "d " in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, med, 15, 15, 7, out, 100, None) == EINVAL and "nblk" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, med, 13, 13, 7, out, 100, None) == EINVAL and "nblk" in _err()
    assert call(x, _hip.PU_F32, 1, 5, 5, med, 0, 0, 7, out, 5, None) == EINVAL and "nblk" in _err()   # n // d < 1
    assert call(x, _hip.PU_F32, 1, 100, 99, med, 14, 14, 7, out, 100, None) == EINVAL and "ld" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, med, 14, 14, 7, out, 99, None) == EINVAL
    assert call(x, _hip.PU_F32, 1, 100, 100, med, 13, 14, 7, out, 100, None) == EINVAL
    assert call(x, _hip.PU_F32, -1, 100, 100, med, 14, 14, 7, out, 100, None) == EINVAL
    assert call(x, _hip.PU_F32, 1, 0, 100, med, 0, 0, 7, out, 100, None) == EINVAL
    for args in ((None, med, out), (x, None, out), (x, med, None)):
        assert call(args[0], _hip.PU_F64, 1, 100, 100, args[1], 14, 14, 7, args[2], 100, None) == EINVAL and "NULL" in _err()
    assert call(x, _hip.PU_F32, 1, 100, 100, ctypes.c_void_p(0x40004), 14, 14, 7, out, 100, None) == EINVAL
    assert "aligned" in _err()
    assert call(ctypes.c_void_p(0x10002), _hip.PU_F32, 1, 100, 100, med, 14, 14, 7, out, 100, None) == EINVAL
    # out is x itself (same pointer, same stride) or apart from it
    for o, ldo in ((ctypes.c_void_p(0x10000 + 4 * 8), 100), (x, 104), (ctypes.c_void_p(0x10000 + 4 * 199), 100)):
        assert call(x, _hip.PU_F32, 2, 100, 100, med, 14, 14, 7, o, ldo, None) == EINVAL and "overlaps" in _err()
    assert call(x, _hip.PU_F32, 2, 100, 1 << 62, med, 14, 14, 7, out, 100, None) == EINVAL and "address space" in _err()


def test_python_layer_rejects_bad_widths_before_the_gpu():
    for w in (0, 2, 100, 2049, -3):
        with pytest.raises(ValueError):
            detrend._check_width(w)
    assert detrend._check_width(2047) == 2047
    with pytest.raises(ValueError):
        detrend._plan_for("detrend", 10, 1200, 101)  # d = 11 > n
    assert detrend._plan_for("detrend", 11, 1200, 101) == (11, 109)
