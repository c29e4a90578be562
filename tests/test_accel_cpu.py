"""The pure-numpy half of the acceleration search in pulsarutils.periodicity, and the argument
checks pu_resample_accel and pu_rfft_accel make before any HIP call (CPU only)."""
import numpy as np
import pytest

import accel_oracle as ao
from pulsarutils import periodicity as pe

EINVAL, EUNSUPPORTED = -1, -4
U8, F32, F64 = 0, 1, 2
P = 4096  # never dereferenced: every case below returns before any HIP call


def test_new_names_are_public():
    for name in ("accel_factor", "resample_indices", "acceleration_grid", "resample", "rfft_accel",
                 "acceleration_search"):
        assert name in pe.__all__ and callable(getattr(pe, name))


def test_accel_factor():
    assert pe.accel_factor(0.0, 1e-3) == 0.0
    assert pe.accel_factor(2 * 299792458.0, 0.5) == 0.5
    a = np.array([-3.8e5, 0.0, 12.5, 3.8e5])
    assert np.array_equal(pe.accel_factor(a, 1e-3), [ao.accel_factor(v, 1e-3) for v in a])
    assert pe.accel_factor(a, 64e-6).dtype == np.float64
    with pytest.raises(ValueError):
        pe.accel_factor(1.0, 0.0)


@pytest.mark.parametrize("n", [1, 2, 257, 4096])
def test_resample_indices_basics_and_oracle(n):
    assert np.array_equal(pe.resample_indices(n, 0.0), np.arange(n))
    for af in (1e-3, -1e-3, 1.0, -1.0, float("nan"), float("inf"), float("-inf"), 1.0 / n, -1.0 / n, 0.37 / n, 3e-5):
        src = pe.resample_indices(n, af)
        assert src.dtype == np.int64 and src.shape == (n,)
        assert src[0] == 0 and src.min() >= 0 and src.max() <= n - 1, af
        assert np.array_equal(src, ao.resample_indices(n, af)), af
        if abs(af) * n <= 1:
            assert np.all(np.diff(src) >= 0), af
    with pytest.raises(ValueError):
        pe.resample_indices(2 ** 24 + 1, 0.0)
    with pytest.raises(ValueError):
        pe.resample_indices(-1, 0.0)


def test_acceleration_grid():
    tobs, ftop = 16.384, 16 * 23.7
    g = pe.acceleration_grid(4e5, tobs, ftop)
    step = 299792458.0 / (ftop * tobs ** 2)
    assert g.dtype == np.float64 and g.size % 2 == 1 and g[g.size // 2] == 0.0
    assert np.array_equal(g, -g[::-1])
    assert np.allclose(np.diff(g), step, rtol=1e-12, atol=0)
    assert g[0] <= -4e5 and g[-1] >= 4e5 and g[-2] < 4e5
    # a signal at ftop between two trials drifts half a bin at most
    assert ftop * (step / 2) * tobs ** 2 / 299792458.0 == pytest.approx(0.5)
    g2 = pe.acceleration_grid(4e5, tobs, ftop, drift_bins=2.0)
    assert np.allclose(np.diff(g2), 2 * step, rtol=1e-12, atol=0) and g2[g2.size // 2] == 0.0
    # the last point is the first at or beyond amax; a tiny amax still gives -step, 0, step
    assert pe.acceleration_grid(1.5 * step, tobs, ftop).size == 5
    assert pe.acceleration_grid(1e-9, tobs, ftop).size == 3
    for bad in ((0.0, tobs, ftop), (-1.0, tobs, ftop), (1.0, 0.0, ftop), (1.0, tobs, 0.0), (1.0, tobs, -2.0),
                (float("nan"), tobs, ftop), (float("inf"), tobs, ftop)):
        with pytest.raises(ValueError):
            pe.acceleration_grid(*bad)
    with pytest.raises(ValueError):
        pe.acceleration_grid(1.0, tobs, ftop, drift_bins=0.0)
    assert pe.acceleration_grid(32766.5 * step, tobs, ftop).size == 65535
    with pytest.raises(ValueError):
        pe.acceleration_grid(32767.5 * step, tobs, ftop)   # 65537 trials


def test_argument_errors_come_before_the_gpu():
    x = np.zeros((2, 300), np.float32)
    with pytest.raises(ValueError, match="exactly one"):
        pe.acceleration_search(x, 1e-3)
    with pytest.raises(ValueError, match="exactly one"):
        pe.acceleration_search(x, 1e-3, accels=[0.0], amax=1.0)
    with pytest.raises(ValueError):
        pe.acceleration_search(x, 1e-3, accels=[0.0], nharm=3)


# ------------------------------------------------------------------ the C ABI's checks

@pytest.fixture(scope="module")
def lib():
    from pulsarutils import _hip
    return _hip.lib()


# (rows, nacc, nfft, _FFT_WS_BYTES, _MAX_ROWS; None: the module's own).  A row of a four-step
# length takes nfft / 2 x 8 bytes of workspace, a row of a one-pass length none.
BATCH_CASES = [
    (5, 5, 2 ** 14, None, None),                 # one call
    (5, 5, 2 ** 14, 2 * 2 ** 16, None),          # room for 2 pairs < rows: one acceleration, rows 2 + 2 + 1
    (5, 5, 2 ** 14, 10 * 2 ** 16, None),         # room for 10 pairs: whole accelerations, 2 per call
    (5, 5, 2 ** 14, 7 * 2 ** 16 + 100, None),    # room for 7: one acceleration per call, 2 pairs of room unused
    (5, 5, 2 ** 14, 5 * 2 ** 16, None),          # room for exactly the rows
    (5, 5, 2 ** 14, 2 ** 16, None),              # one pair per call
    (5, 5, 2 ** 14, None, 2),                    # the same shapes from the row limit
    (5, 5, 2 ** 14, None, 12),
    (3, 7, 256, None, 4),                        # a one-pass length: the row limit alone
    (1, 9, 2 ** 20, 4 * 2 ** 22, None),          # one row: 4 accelerations per call
    (256, 300, 2 ** 20, None, None),             # the unpatched limits: 1 GiB is 256 rows of 2^20
    (300, 3, 2 ** 20, None, None),               # ... and rows 256 + 44 per acceleration beyond
    (3, 65535, 256, None, None),                 # the most trials: 10922 accelerations per call
    (40000, 2, 2 ** 8, None, None),              # more rows than a call takes
    (32768, 2, 2 ** 8, None, None),              # exactly as many
    (32769, 1, 2 ** 8, None, None),
]


@pytest.mark.parametrize("rows, nacc, nfft, ws_bytes, max_rows", BATCH_CASES)
def test_accel_batches_cover_every_pair_once_in_order(lib, monkeypatch, rows, nacc, nfft, ws_bytes, max_rows):
    if ws_bytes is not None:
        monkeypatch.setattr(pe, "_FFT_WS_BYTES", ws_bytes)
    if max_rows is not None:
        monkeypatch.setattr(pe, "_MAX_ROWS", max_rows)
    per_row = lib.pu_rfft_workspace_bytes(2, nfft) - lib.pu_rfft_workspace_bytes(1, nfft)
    assert per_row == (nfft // 2 * 8 if nfft > 2 ** 13 else 0) and per_row <= pe._FFT_WS_BYTES
    batches = pe._accel_batches(rows, nacc, nfft)
    pairs = []
    for a0, a1, r0, r1 in batches:
        assert 0 <= a0 < a1 <= nacc and 0 <= r0 < r1 <= rows
        # whole rows at several accelerations, or rows of one
        assert (r0, r1) == (0, rows) or a1 == a0 + 1
        m = (a1 - a0) * (r1 - r0)
        # what one call takes: the grid, the row limit of the stages after the transform, and the
        # workspace the rows' columns may fill (the twiddle table of nfft / 2 entries comes on top)
        assert m <= 65535 and m <= pe._MAX_ROWS and m * per_row <= pe._FFT_WS_BYTES
        assert lib.pu_rfft_accel_workspace_bytes(r1 - r0, a1 - a0, nfft) <= pe._FFT_WS_BYTES + nfft // 2 * 8 + 256
        pairs.append(np.add.outer(np.arange(a0, a1) * rows, np.arange(r0, r1)).ravel())
    # every (a, r) once, in (a, r) order: the order of the candidate list
    assert np.array_equal(np.concatenate(pairs), np.arange(nacc * rows))
    # both branches are what they say
    per = pe._rows_per_call(rows * nacc, nfft)
    if rows <= per:
        assert all(b[2:] == (0, rows) for b in batches) and len(batches) == -(-nacc // (per // rows))
    else:
        assert len(batches) == nacc * -(-rows // per)
    # the row batches of periodicity_search under the same limits
    per = pe._rows_per_call(rows, nfft)
    assert 1 <= per <= min(rows, pe._MAX_ROWS) and per * per_row <= pe._FFT_WS_BYTES
    assert per == rows or per == pe._MAX_ROWS or (per + 1) * per_row > pe._FFT_WS_BYTES


def _msg(lib):
    return lib.pu_last_error().decode()


def _rfft_accel(lib, dtype=F32, rows=2, n=300, ld=300, afac=P, nacc=3, nfft=512, ld_spec=257, ws=P, ws_bytes=1 << 20, x=P,
                spec=P):
    return lib.pu_rfft_accel(x, dtype, rows, n, ld, None, afac, nacc, nfft, spec, ld_spec, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, word", [
    (dict(rows=256, nacc=256), "grid limit"),
    (dict(rows=1, nacc=65536), "grid limit"),
    (dict(rows=65536, nacc=1), "grid limit"),
    (dict(rows=-1), "bad size"),
    (dict(nacc=-1), "bad size"),
    (dict(nacc=2 ** 31), "bad size"),
    (dict(afac=None), "null"),
    (dict(afac=P + 4), "aligned"),
    (dict(nfft=768, ld_spec=385), "power of two"),
    (dict(n=513, ld=513), "bad size"),
    (dict(ld=299), "leading dimension"),
    (dict(ld_spec=256), "leading dimension"),
    (dict(ws_bytes=100), "workspace"),
    (dict(ws=None), "workspace"),
    (dict(ws=P + 8), "workspace"),
    (dict(x=None), "null"),
    (dict(spec=None), "null"),
    (dict(x=P + 2), "aligned"),
])
def test_rfft_accel_rejects_before_any_hip_call(lib, kw, word):
    assert _rfft_accel(lib, **kw) == EINVAL
    assert word in _msg(lib) and "pu_rfft_accel" in _msg(lib)


def test_rfft_accel_dtype_empty_and_workspace_size(lib):
    assert _rfft_accel(lib, dtype=U8) == EUNSUPPORTED and "dtype" in _msg(lib)
    assert _rfft_accel(lib, rows=0, x=None, spec=None, ws=None, ws_bytes=0) == 0
    assert _rfft_accel(lib, nacc=0, afac=None, x=None, spec=None, ws=None, ws_bytes=0) == 0
    # pu_rfft's for nacc x rows rows; the four-step's rows of the workspace count the pairs
    for rows, nacc, nfft in ((3, 5, 256), (3, 5, 2 ** 13), (3, 5, 2 ** 14), (1, 1, 2 ** 20)):
        assert lib.pu_rfft_accel_workspace_bytes(rows, nacc, nfft) == lib.pu_rfft_workspace_bytes(rows * nacc, nfft)
    assert lib.pu_rfft_accel_workspace_bytes(3, 5, 2 ** 14) == 2 ** 13 * 8 * 16
    assert lib.pu_rfft_accel_workspace_bytes(3, 0, 256) == 0 and lib.pu_rfft_accel_workspace_bytes(-1, 2, 256) == 0
    # a workspace that holds pu_rfft's rows but not nacc x rows is too small
    small = lib.pu_rfft_workspace_bytes(2, 2 ** 14)
    assert _rfft_accel(lib, n=2 ** 14, ld=2 ** 14, nfft=2 ** 14, ld_spec=2 ** 13 + 1, ws_bytes=small) == EINVAL
    assert "workspace" in _msg(lib)
    # the words of pu_rfft's own messages are unchanged
    assert lib.pu_rfft(P, F32, 70000, 300, 300, None, 512, P, 257, P, 1 << 20, None) == EINVAL
    assert "pu_rfft:" in _msg(lib) and "grid limit" in _msg(lib)


@pytest.mark.parametrize("kw, word", [
    (dict(n=-1), "bad size"),
    (dict(rows=-1), "bad size"),
    (dict(nacc=-1), "bad size"),
    (dict(rows=2 ** 31), "bad size"),
    (dict(n=2 ** 24 + 1, ld=2 ** 25, ld_out=2 ** 25), "bad size"),
    (dict(ld=299), "leading dimension"),
    (dict(ld_out=299), "leading dimension"),
    (dict(x=None), "null"),
    (dict(out=None), "null"),
    (dict(afac=None), "null"),
    (dict(out=P), "not in place"),
    (dict(x=P + 2), "aligned"),
    (dict(out=2 * P + 2), "aligned"),
    (dict(afac=P + 4), "aligned"),
])
def test_resample_accel_rejects_before_any_hip_call(lib, kw, word):
    a = dict(x=P, dtype=F32, rows=2, n=300, ld=300, afac=P, nacc=3, out=2 * P, ld_out=300)
    a.update(kw)
    rc = lib.pu_resample_accel(a["x"], a["dtype"], a["rows"], a["n"], a["ld"], a["afac"], a["nacc"], a["out"], a["ld_out"],
                               None)
    assert rc == EINVAL
    assert word in _msg(lib)


def test_resample_accel_dtype_and_empty(lib):
    assert lib.pu_resample_accel(P, U8, 2, 300, 300, P, 3, 2 * P, 300, None) == EUNSUPPORTED and "dtype" in _msg(lib)
    assert lib.pu_resample_accel(None, F32, 0, 300, 300, None, 3, None, 300, None) == 0
    assert lib.pu_resample_accel(None, F64, 2, 300, 300, None, 0, None, 300, None) == 0
    assert lib.pu_resample_accel(None, F64, 2, 0, 0, None, 3, None, 0, None) == 0
