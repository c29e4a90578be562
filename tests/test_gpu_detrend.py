"""pu_running_median and pu_detrend_apply on the GPU against tests/detrend_oracle.py, bit for bit:
every width class at the tile edges, padded layouts, ties, signed zeros, NaN and inf, batch
independence; the Python layer; and the FFA search on a red-noise series end to end."""
import functools

import numpy as np
import pytest

import detrend_oracle as do
from pulsarutils import _hip, detrend, ffa

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 5, 101, 109, 2047)
DTYPES = (np.float32, np.float64)
KINDS = ("gaussian", "integers", "constant", "zeros", "nonfinite_a", "nonfinite_b")


# n of a case from the width, its half and the tile pu_running_median_describe reports
SIZES = {"1": lambda w, h, tile: 1, "2": lambda w, h, tile: 2, "h": lambda w, h, tile: h, "h+1": lambda w, h, tile: h + 1,
         "w-1": lambda w, h, tile: w - 1, "w": lambda w, h, tile: w, "w+1": lambda w, h, tile: w + 1,
         "tile-1": lambda w, h, tile: tile - 1, "tile": lambda w, h, tile: tile, "tile+1": lambda w, h, tile: tile + 1,
         "2tile+1": lambda w, h, tile: 2 * tile + 1, "3tile-h": lambda w, h, tile: 3 * tile - h}


def size_of(dtype, w, case):
    info = detrend.describe(dtype, w)
    assert info["w_max"] == 2047 and 64 <= info["tile"] <= 4096  # (the oracle's cost is n x w)
    return SIZES[case](w, (w - 1) // 2, info["tile"])


@functools.lru_cache(maxsize=None)
def rows_for(dtype, n):
    """One row of every kind of KINDS, (6, n); read-only."""
    rng = np.random.default_rng(12345 + n)
    g = rng.standard_normal((6, n))
    g[1] = rng.integers(-3, 4, n)                    # heavy ties
    g[2] = 1.75                                      # constant
    g[3] = np.where(rng.random(n) < 0.5, -0.0, 0.0)  # -0 and +0 alone
    g[4, 0], g[4, n - 1], g[4, n // 2] = np.inf, -np.inf, np.nan   # (a later one wins where n is tiny)
    g[5, min(1, n - 1)], g[5, max(0, n - 2)], g[5, n // 3] = np.nan, np.nan, np.inf
    if n > 40:
        g[5, n // 2 + 3], g[5, n // 2 + 4] = -np.inf, -np.inf
    x = g.astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want_for(dtype, n, w):
    out = do.running_median(rows_for(dtype, n), w)
    out.setflags(write=False)
    return out


def sentinel(dtype):
    """A NaN no kernel makes: what padding and unwritten outputs must still hold."""
    return np.array([0x7fc12345], np.uint32).view(np.float32)[0] if dtype == np.float32 else \
        np.array([0x7ff8000012345678], np.uint64).view(np.float64)[0]


def padded(dev, x, pad):
    """(device tensor (rows, n + pad) with the sentinel in the padding, its host image)."""
    import torch
    rows, n = x.shape
    host = np.full((rows, n + pad), sentinel(x.dtype.type), x.dtype)
    host[:, :n] = x
    return torch.from_numpy(host).to(dev), host


def run_rmed(dev, x, w, pad_in=7, pad_out=5):
    """pu_running_median through the C ABI on rows ``x`` with ld > n, ld_out > n and a sentinel NaN
    in the input padding, the output padding and the whole output; checks that the padding and
    the input survive.  Returns out (rows, n)."""
    import torch
    x = np.ascontiguousarray(x)
    rows, n = x.shape
    xd, xin = padded(dev, x, pad_in)
    od, oin = padded(dev, np.full((rows, n), sentinel(x.dtype.type), x.dtype), pad_out)
    _hip.check(_hip.lib().pu_running_median(_hip.ptr(xd), _hip.dtype_code(xd.dtype), rows, n, n + pad_in, w, _hip.ptr(od),
                                            n + pad_out, _hip.stream_ptr()), "pu_running_median")
    torch.cuda.synchronize()
    o = od.cpu().numpy()
    assert do.same_bits(o[:, n:], oin[:, n:]), "out padding written"
    assert do.same_bits(xd.cpu().numpy(), xin), "input written"
    return o[:, :n]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SIZES))
@pytest.mark.parametrize("w", WIDTHS)
def test_running_median_bits(gpu, dtype, w, case):
    n = size_of(dtype, w, case)
    if n < 1:
        return  # h or w - 1 of w = 1: no such series
    x = rows_for(dtype, n)
    got = run_rmed(gpu, x, w)
    want = want_for(dtype, n, w)
    for r, kind in enumerate(KINDS):
        assert do.same_bits(got[r], want[r]), kind
    assert not np.isnan(got[:4]).any()  # no sentinel left, no NaN of the padding read


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w, case", [(101, "2tile+1"), (5, "tile+1")])
def test_running_median_batch_independence(gpu, dtype, w, case):
    n = size_of(dtype, w, case)
    x = rows_for(dtype, n)[:5]
    got = run_rmed(gpu, x, w)
    assert do.same_bits(got, want_for(dtype, n, w)[:5])
    assert do.same_bits(run_rmed(gpu, x, w), got)  # and repeatable
    for r in range(5):
        assert do.same_bits(run_rmed(gpu, x[r:r + 1], w, pad_in=0, pad_out=0)[0], got[r]), r


# ------------------------------------------------------------------ pu_detrend_apply

def run_apply(dev, x, med, d, in_place, pad, pad_med=3):
    """pu_detrend_apply through the C ABI with padded rows of x, med and out (the sentinel NaN in
    the padding); returns out (rows, n)."""
    import torch
    x = np.ascontiguousarray(x)
    rows, n = x.shape
    nblk = med.shape[1]
    xd, xin = padded(dev, x, pad)
    md, _ = padded(dev, np.ascontiguousarray(med, dtype=np.float64), pad_med)
    if in_place:
        od, oin = xd, xin
    else:
        od, oin = padded(dev, np.full((rows, n), sentinel(x.dtype.type), x.dtype), pad)
    _hip.check(_hip.lib().pu_detrend_apply(_hip.ptr(xd), _hip.dtype_code(xd.dtype), rows, n, n + pad, _hip.ptr(md),
                                           nblk + pad_med, nblk, d, _hip.ptr(od), n + pad, _hip.stream_ptr()),
               "pu_detrend_apply")
    torch.cuda.synchronize()
    o = od.cpu().numpy()
    assert do.same_bits(o[:, n:], oin[:, n:]), "out padding written"
    if not in_place:
        assert do.same_bits(xd.cpu().numpy(), xin), "input written"
    return o[:, :n]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 7, 11])
def test_detrend_apply_bits(gpu, dtype, d):
    rng = np.random.default_rng(100 + d)
    for nblk in (1, 2, 3, 300):
        for tail in sorted({0, d - 1, d // 2}):
            n = nblk * d + tail
            x = (10.0 * rng.standard_normal((3, n))).astype(dtype)
            med = rng.standard_normal((3, nblk)) * 5.0
            want = do.apply(x, med, d)
            # rows a multiple of 16 bytes apart (16-byte pieces) and not (element by element)
            for pad in ((-n) % 4 + 4, (-n) % 4 + 5):
                for in_place in (False, True):
                    got = run_apply(gpu, x, med, d, in_place, pad)
                    assert do.same_bits(got, want), (nblk, tail, pad, in_place)


def test_detrend_apply_nan_median_reaches_its_neighbours_only(gpu):
    d, nblk = 7, 9
    n = nblk * d + 5
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, n)).astype(np.float32)
    med = rng.standard_normal((2, nblk))
    med[0, 4] = np.nan
    med[1, 0], med[1, nblk - 1] = np.nan, np.inf
    want = do.apply(x, med, d)
    for pad in (4 + (-n) % 4, 5):
        got = run_apply(gpu, x, med, d, False, pad)
        assert do.same_bits_or_nan(got, want)
        assert np.array_equal(np.flatnonzero(np.isnan(got[0])), np.arange(3 * d + 4, 5 * d + 3))
        assert np.array_equal(np.flatnonzero(np.isnan(got[1])), np.arange(0, d + 3))  # up to the second centre
        assert np.isinf(got[1, 8 * d + 3:]).all() and np.isinf(got[1, 7 * d + 4:]).all() and np.isfinite(got[1, 7 * d + 3])


# ------------------------------------------------------------------ the Python layer

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1200, 50])
def test_python_layer_matches_the_oracle(gpu, dtype, W):
    import torch
    rng = np.random.default_rng(W)
    n = 5003
    x = (rng.standard_normal((3, n)) + 4.0 * np.sin(np.arange(n) / 700.0)).astype(dtype)
    x[1, 17] = -0.0
    d, w = detrend.detrend_plan(W)
    want_med = do.running_median(x, w)
    want_base, want_det = do.baseline(x, W), do.detrend(x, W)
    assert want_base.dtype == np.float64 and want_det.dtype == dtype
    # numpy in, numpy out
    assert do.same_bits(detrend.running_median(x, w), want_med)
    assert do.same_bits(detrend.baseline(x, W), want_base)
    assert do.same_bits(detrend.detrend(x, W), want_det)
    # tensor in, tensor out
    xt = torch.from_numpy(x).to(gpu)
    for fn, arg, want in ((detrend.running_median, w, want_med), (detrend.baseline, W, want_base),
                          (detrend.detrend, W, want_det)):
        got = fn(xt, arg)
        assert isinstance(got, torch.Tensor) and got.is_cuda and do.same_bits(got.cpu().numpy(), want)
    assert do.same_bits(xt.cpu().numpy(), x)  # the input is left alone
    # 1-D in, 1-D out
    assert do.same_bits(detrend.running_median(x[2], w), want_med[2])
    assert do.same_bits(detrend.baseline(x[2], W), want_base[2])
    assert do.same_bits(detrend.detrend(x[2], W), want_det[2])
    assert detrend.detrend(xt[2], W).shape == (n,)


def test_python_layer_errors(gpu):
    x = np.zeros((2, 100), np.float32)
    for w in (0, 2, 2049):
        with pytest.raises(ValueError):
            detrend.running_median(x, w)
    with pytest.raises(ValueError):
        detrend.detrend(x, 0)
    with pytest.raises(ValueError):
        detrend.baseline(x, 101 * 101)  # d = 101 > n
    with pytest.raises(ValueError):
        detrend.detrend(np.zeros((2, 3, 4), np.float32), 5)


# ------------------------------------------------------------------ the search on a red series

def test_ffa_finds_the_pulsar_under_red_noise(gpu):
    """tests/test_detrend_oracle.py pins the scenario on the CPU: best S/N 3.0 on the red series
    and 21.6 after the detrend, against thresholds of 7 and 10."""
    _, red = do.red_noise_series(0.8)
    plain = ffa.ffa_periodogram(red, 1.0, 250.0, 251.0)
    k = int(np.argmin(np.abs(plain["period"] - 250.37)))
    print(f"trial {plain['period'][k]:.4f}: S/N {plain['snr'][k]:.2f} without detrending")
    assert plain["snr"][k] < 7
    det = ffa.ffa_periodogram(red, 1.0, 250.0, 251.0, detrend_width=1200.0)
    assert np.array_equal(det["period"], plain["period"])
    print(f"trial {det['period'][k]:.4f}: S/N {det['snr'][k]:.2f} with detrend_width=1200")
    assert det["snr"][k] > 10
    # the periodogram of the detrended series is the periodogram with detrend_width
    alone = ffa.ffa_periodogram(detrend.detrend(red.astype(np.float64), 1200), 1.0, 250.0, 251.0)
    assert np.abs(alone["snr"] - det["snr"]).max() < 1e-3
    cands = ffa.ffa_search(red, 1.0, 250.0, 251.0, detrend_width=1200.0)
    assert len(cands["period"]) >= 1
    assert abs(cands["period"][0] - 250.37) < 1e-3 * 250.37 and cands["snr"][0] > 10
    # None is today's path, bit for bit
    again = ffa.ffa_periodogram(red, 1.0, 250.0, 251.0, detrend_width=None)
    assert do.same_bits(again["snr"], plain["snr"]) and np.array_equal(again["width"], plain["width"])
    t_plain = ffa.ffa_search(red, 1.0, 250.0, 251.0, sigma=3.0)
    t_none = ffa.ffa_search(red, 1.0, 250.0, 251.0, sigma=3.0, detrend_width=None)
    for c in ("period", "row", "snr", "width", "peak_phase", "dsfactor", "nabsorbed"):
        assert np.array_equal(np.asarray(t_plain[c]), np.asarray(t_none[c])), c
    with pytest.raises(ValueError):
        ffa.ffa_periodogram(red, 1.0, 250.0, 251.0, detrend_width=0.0)
