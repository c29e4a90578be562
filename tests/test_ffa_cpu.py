"""The FFA's host side without a GPU: the search plan, trial periods and widths, what
pu_ffa_describe reports, the rows the drivers give one call, and every argument error of pu_ffa
before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

from pulsarutils import _hip, ffa


def _covered(plan, sample_time):
    return [(d * p0 * sample_time, d * p1 * sample_time) for d, p0, p1 in plan]


def test_plan_of_the_documented_search():
    for ts in (1.0, 64e-6):
        plan = ffa.ffa_plan(2 ** 20, ts, 240 * ts, 15360 * ts)
        assert plan[:3] == [(1, 240, 480), (2, 240, 360), (3, 240, 320)]
        assert plan[-1] == (60, 240, 260)


@pytest.mark.parametrize("args", [(2 ** 20, 1.0, 240.0, 15360.0, 240, 260), (2 ** 18, 1e-3, 0.7, 9.0, 200, 230),
                                  (2 ** 17, 1.0, 300.0, 5000.0, 128, 136)])
def test_plan_tiles_the_period_axis(args):
    n, ts, pmin, pmax, bmin, bmax = args
    plan = ffa.ffa_plan(n, ts, pmin, pmax, bins_min=bmin, bins_max=bmax)
    assert plan[0][0] == max(1, math.floor(pmin / (bmin * ts)))
    for (d, p0, p1), (dn, q0, _) in zip(plan, plan[1:]):
        assert dn == max(d + 1, d * bmax // bmin)
        assert p0 == q0 == bmin and p1 == -(-bmin * dn // d)
        # the next factor starts inside [the last base period of this one, one bin past it]: no gap
        assert d * (p1 - 1) < dn * q0 <= d * p1
    assert all(p0 >= bmin and p1 > p0 for _, p0, p1 in plan)
    lo, hi = _covered(plan, ts)[0][0], _covered(plan, ts)[-1][1]
    assert lo <= max(pmin, bmin * ts) and hi > pmax


def test_plan_min_rows_and_errors():
    n = 2 ** 14
    full = ffa.ffa_plan(n, 1.0, 240, 4000, min_rows=1)
    cut = ffa.ffa_plan(n, 1.0, 240, 4000, min_rows=40)
    assert all((n // d) // (p1 - 1) >= 40 for d, _, p1 in cut)
    assert cut[0] == (1, 240, n // 40 + 1) and len(cut) < len(full)
    # every dropped base period indeed has too few rows
    kept = {(d, p) for d, p0, p1 in cut for p in range(p0, p1)}
    for d, p0, p1 in full:
        for p in range(p0, p1):
            assert ((d, p) in kept) == ((n // d) // p >= 40)
    assert ffa.ffa_plan(1000, 1.0, 240, 400, min_rows=8) == []
    with pytest.raises(ValueError, match="limit"):
        ffa.ffa_plan(2 ** 20, 1.0, 1100, 4000, bins_min=1100, bins_max=1200)
    for bad in ((0, 1.0, 240, 480), (1000, 0.0, 240, 480), (1000, 1.0, 0.0, 480), (1000, 1.0, 480, 240)):
        with pytest.raises(ValueError):
            ffa.ffa_plan(*bad)
    with pytest.raises(ValueError):
        ffa.ffa_plan(1000, 1.0, 240, 480, bins_min=240, bins_max=240)


def test_trial_periods_and_widths():
    assert np.array_equal(ffa.trial_periods(250, 1, 2.0), [500.0])
    per = ffa.trial_periods(250, 419, 0.5)
    assert per.shape == (419,) and per[0] == 125.0 and per[-1] == 125.5
    assert np.array_equal(per, (250 + np.arange(419) / 418) * 0.5)
    assert ffa.default_widths(256).tolist() == [1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 63]
    assert ffa.default_widths(250).tolist() == [1, 2, 3, 4, 6, 9, 13, 19, 28, 42]
    assert ffa.default_widths(52).tolist() == [1, 2, 3, 4, 6, 9, 13]
    assert ffa.default_widths(2).tolist() == [1] and ffa.default_widths(3).tolist() == [1]
    assert ffa.default_widths(2048).size <= 16 and ffa.default_widths(2048).dtype == np.int32
    for p in (2, 7, 64, 2048):
        w = ffa.default_widths(p)
        assert np.all(w >= 1) and np.all(w < p) and np.all(np.diff(w) > 0)


def test_describe_is_consistent():
    for p in (2, 3, 64, 250, 256, 1023, 1024, 2048):
        b = ffa.describe(1, 1, p)["block_rows"]
        assert b & (b - 1) == 0 and 8 <= b <= 256 and b * p <= 16384 and (b == 256 or 2 * b * p > 16384)
        for m in (1, 2, 3, b - 1, b, b + 1, 2 * b + 1, 1000, 4096):
            last = -1
            for rows in (0, 1, 2, 3, 64):
                for want_out, nw in ((True, 0), (True, 5), (False, 5)):
                    info = ffa.describe(rows, m, p, nw, want_out)
                    assert info["depth"] == (m - 1).bit_length() == math.ceil(math.log2(m))
                    assert info["block_rows"] == b and info["p_max"] == 2048
                    assert info["lds_levels"] == min(info["depth"], b.bit_length() - 1)
                    assert info["global_levels"] == info["depth"] - info["lds_levels"]
                    assert info["lds_bytes"] <= 160 * 1024
                    plane = rows * m * p * 4
                    if want_out:
                        assert info["workspace_bytes"] == (plane if info["global_levels"] >= 1 else 0)
                    else:
                        assert plane <= info["workspace_bytes"] <= 2 * plane + 255
                    assert info["traffic_bytes"] >= 2 * rows * m * p * 4
                info = ffa.describe(rows, m, p, 10, False)
                assert info["workspace_bytes"] >= last  # monotone in rows
                last = info["workspace_bytes"]


# all levels in LDS (no workspace with out); rows far below, just below and above 256 bytes; one, two
# and three levels above the LDS ones
@pytest.mark.parametrize("m, p", [(1, 2), (5, 2), (7, 3), (13, 5), (37, 50), (81, 100), (129, 256), (300, 5), (9, 2047),
                                  (33, 2048)])
@pytest.mark.parametrize("nw, want_out", [(0, True), (4, True), (4, False)])
def test_rows_per_call_keeps_the_limits_and_is_maximal(monkeypatch, m, p, nw, want_out):
    def ws(r):
        return ffa.describe(r, m, p, nw, want_out)["workspace_bytes"]
    glob = ffa.describe(1, m, p, nw, want_out)["global_levels"]
    nbuf = (1 if glob >= 1 else 0) if want_out else (2 if glob >= 2 else 1)  # the planes a call carves (ffa.hip)
    assert nbuf * m * p * 4 <= ws(1) <= nbuf * (m * p * 4 + 255)
    if want_out and glob == 0:
        assert ws(1) == ws(1000) == 0
    for ws_limit in sorted({ws(1), ws(2), ws(3) + 100, ws(10) + 1, ws(300), 4 << 30}):  # (a row always fits)
        for rows_m_limit in (m, 2 * m, 3 * m + 1, 100 * m + m // 2, (1 << 31) - 1):
            monkeypatch.setattr(ffa, "_WS_BYTES", ws_limit)
            monkeypatch.setattr(ffa, "_MAX_ROWS_M", rows_m_limit)
            for rows in (1, 2, 3, 5, 64, 1000):
                per = ffa._rows_per_call(rows, m, p, nw, want_out)
                case = (rows, ws_limit, rows_m_limit, per)
                assert 1 <= per <= rows, case
                assert per * m <= rows_m_limit, case
                assert ws(per) <= ws_limit + 256 * nbuf, case  # (one round-up per buffer)
                assert per == rows or (per + 1) * m > rows_m_limit or ws(per + 1) > ws_limit, case


def _call(x=4096, rows=1, ld=64, m=4, p=16, out=8192, ld_out=64, widths=(1, 2), nw=None, sigma=0, snr=12288, peak=0,
          ws=256 * 64, wsb=1 << 20):
    """pu_ffa with fake (never dereferenced) device addresses: every check is on the host."""
    w = (ctypes.c_int32 * max(1, len(widths or ())))(*(widths or ()))
    return _hip.lib().pu_ffa(x, rows, ld, m, p, out, ld_out, ctypes.cast(w, ctypes.c_void_p) if widths is not None else None,
                             len(widths or ()) if nw is None else nw, sigma, snr, peak, ws, wsb, None)


@pytest.mark.parametrize("kw, code, text", [
    (dict(p=1), -1, "p 1 < 2"),
    (dict(m=0), -1, "m 0 < 1"),
    (dict(rows=-1), -1, "rows -1 < 0"),
    (dict(ld=63), -1, "ld 63 < m x p"),
    (dict(ld_out=63), -1, "ld_out_row 63 < m x p"),
    (dict(out=0, snr=0), -1, "both out and snr"),
    (dict(snr=0, peak=64), -1, "peak without snr"),
    (dict(widths=()), -1, "nwidths 0 outside"),
    (dict(widths=tuple(range(1, 16)) + (1, 2)), -1, "nwidths 17 outside"),
    (dict(widths=None, nw=2), -1, "widths is NULL"),
    (dict(widths=(1, 0)), -1, "widths[1] = 0 outside"),
    (dict(widths=(16,)), -1, "widths[0] = 16 outside"),
    (dict(x=0), -1, "x is NULL"),
    (dict(x=4098), -1, "not aligned"),
    (dict(m=4096, ld=65536, ld_out=65536, wsb=100), -1, "workspace of"),
    (dict(m=4096, ld=65536, ld_out=65536, ws=0), -1, "workspace of"),
    (dict(m=4096, ld=65536, ld_out=65536, ws=256 * 64 + 8), -1, "workspace of"),
    (dict(out=0, ws=0), -1, "workspace of"),
    (dict(p=2049, ld=1 << 20, ld_out=1 << 20), -4, "p 2049 above 2048"),
    (dict(rows=1 << 20, m=1 << 12, ld=1 << 20, ld_out=1 << 20), -4, "above 2^31 - 1"),
])
def test_error_paths_without_gpu(kw, code, text):
    assert _call(**kw) == code
    assert text in _hip.lib().pu_last_error().decode()


def test_empty_batch_and_describe_errors():
    assert _call(rows=0, x=0, out=0, ws=0, wsb=0) == 0  # PU_OK without a launch
    info = (ctypes.c_int64 * 8)()
    lib = _hip.lib()
    assert lib.pu_ffa_describe(1, 4, 1, 0, 1, info, 8) == -1 and "p 1 < 2" in lib.pu_last_error().decode()
    assert lib.pu_ffa_describe(1, 4, 4096, 0, 1, info, 8) == -4 and "above 2048" in lib.pu_last_error().decode()
    assert lib.pu_ffa_describe(1, 4, 16, 17, 1, info, 8) == -1 and "nwidths" in lib.pu_last_error().decode()
    assert lib.pu_ffa_describe(1, 4, 16, 0, 0, info, 8) == -1 and "neither" in lib.pu_last_error().decode()
    assert lib.pu_ffa_describe(1, 4, 16, 0, 1, None, 8) == -1
    with pytest.raises(ValueError):
        ffa.describe(1, 0, 16)
