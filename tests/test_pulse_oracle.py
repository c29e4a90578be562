"""The single-pulse helper (tests/pulse_oracle.py) pinned to the golden-pinned oracle, the host
clusterer of pulsarutils.pulses against the helper, and the argument checks of
pu_series_events (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import oracle
import pulse_oracle as po


def ev(*rows):
    """Hand-made events: (row, window, start, nbins, snr); the peak is the start."""
    return np.array([(r, w, s, nb, s, snr) for r, w, s, nb, snr in rows], dtype=po.EVENT_DTYPE)


@pytest.mark.parametrize("name,thresholds", [("a", (1.0, 2.0)), ("b", (3.0, 6.0, 20.0))])
def test_largest_event_snr_is_the_reference_snr(name, thresholds):
    d = {"a": po.series_a, "b": po.series_b}[name]()
    snr = oracle.trial_stats(d)[2]
    assert all(t < snr for t in thresholds)
    for t in thresholds:
        events = po.series_events(d, t)
        assert events.size and events["snr"].max() == snr  # exactly
    assert po.series_events(d, snr).size == 0  # strict: a bin at the threshold is not above
    assert po.series_events(d, snr * (1 + 1e-9)).size == 0


def test_events_of_the_stated_series():
    a = po.series_events(po.series_a(), 2.0)
    assert [tuple(int(v) for v in (e["window"], e["start"], e["nbins"], e["peak"])) for e in a] == [
        (1, 5000, 3000, 6694), (2, 2500, 1500, 3520), (4, 1250, 750, 1432), (8, 625, 375, 716)]
    b = po.series_b()
    assert len(po.series_events(b, 6.0)) == 26 and len(po.series_events(b, 3.0)) == 30
    b6 = po.series_events(b, 6.0)
    n = po.N_SERIES
    # a run at bin 0, a run ending at the last kept bin, the dropped tail, the four-sample tie
    assert (b6["start"] == 0).sum() == 4
    for w in (1, 2):
        assert any(e["window"] == w and e["start"] + e["nbins"] == n // w for e in b6)
    assert not any(e["window"] == 8 and e["start"] + e["nbins"] == n // 8 for e in b6)
    tie = b6[(b6["window"] == 1) & (b6["start"] == 12000)][0]
    assert tie["nbins"] == 4 and tie["peak"] == 12000
    nan = b.copy()
    nan[777] = np.nan
    assert po.series_events(nan, 6.0).size == 0 and po.series_events(np.zeros(n), 6.0).size == 0


def test_single_spike():
    e8 = po.series_events(po.spike(8), 1.5)
    assert [tuple(int(v) for v in (e["window"], e["start"], e["nbins"], e["peak"])) for e in e8] == [
        (1, 4, 1, 4), (2, 2, 1, 2)]  # window 8: one bin, std 0, nothing
    e17 = po.series_events(po.spike(17), 1.5)
    assert len(e17) == 3 and e17[0]["window"] == 1 and e17[0]["snr"] == 4.0


def both(events, dm_tol, time_tol):
    from pulsarutils.pulses import cluster_events
    want = po.cluster(events, dm_tol, time_tol)
    got = cluster_events(events, dm_tol, time_tol)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


def test_cluster_chain_through_a_middle_member():
    # trials 0 and 4 are 4 apart: friends of trial 2 only; samples likewise through [10, 20)
    events = ev((0, 1, 10, 3, 7.0), (4, 1, 11, 3, 8.0), (2, 1, 12, 3, 6.5),
                (9, 1, 0, 10, 7.0), (9, 1, 20, 10, 7.5), (9, 2, 5, 5, 6.1))
    labels, reps = both(events, 2, 0)
    assert labels.tolist() == [0, 0, 0, 1, 1, 1] and reps.tolist() == [1, 4]
    labels, _ = both(events[[0, 1, 3, 4]], 2, 0)  # without the middle members: four pulses
    assert labels.tolist() == [0, 1, 2, 3]


def test_cluster_dm_tol():
    events = ev((10, 1, 100, 2, 9.0), (12, 1, 100, 2, 7.0), (13, 1, 101, 2, 6.5))
    assert both(events, 1, 0)[0].tolist() == [0, 1, 1]
    assert both(events, 2, 0)[0].tolist() == [0, 0, 0]
    assert both(events, 0, 0)[0].tolist() == [0, 1, 2]


def test_cluster_time_tol():
    # [8, 12) touches [12, 16) (window 4 bins 3): gap 0; [17, 18) is one sample from 16
    events = ev((5, 4, 2, 1, 7.0), (5, 4, 3, 1, 6.5), (5, 1, 17, 1, 6.2), (5, 1, 20, 1, 6.1))
    assert both(events, 2, 0)[0].tolist() == [0, 0, 1, 2]
    assert both(events, 2, 1)[0].tolist() == [0, 0, 0, 1]
    assert both(events, 2, 2)[0].tolist() == [0, 0, 0, 0]


def test_cluster_tie_breaks():
    # equal snr: lowest trial; then smallest window; then earliest start
    assert both(ev((3, 1, 10, 4, 7.0), (2, 1, 10, 4, 7.0), (2, 1, 11, 1, 6.0)), 2, 0)[1].tolist() == [1]
    assert both(ev((2, 2, 5, 2, 7.0), (2, 1, 10, 4, 7.0)), 2, 0)[1].tolist() == [1]
    assert both(ev((2, 1, 12, 2, 7.0), (2, 1, 10, 2, 7.0)), 2, 0)[1].tolist() == [1]
    assert both(ev((2, 1, 12, 2, 7.0), (2, 1, 10, 2, 7.5), (1, 8, 1, 1, 7.25)), 2, 0)[1].tolist() == [1]


def test_cluster_random_and_large():
    from pulsarutils.pulses import cluster_events
    rng = np.random.default_rng(5)
    for _ in range(40):
        n = int(rng.integers(1, 40))
        events = np.zeros(n, po.EVENT_DTYPE)
        events["row"] = rng.integers(0, 8, n)
        events["window"] = 2 ** rng.integers(0, 4, n)
        events["start"] = rng.integers(0, 30, n) // events["window"]
        events["nbins"] = rng.integers(1, 4, n)
        events["snr"] = rng.integers(5, 8, n)
        for dm_tol, time_tol in ((0, 0), (1, 0), (2, 0), (2, 1), (1, 3)):
            both(events, dm_tol, time_tol)
    assert cluster_events(np.zeros(0, po.EVENT_DTYPE))[0].size == 0
    # 10^5 events: one chain through all of them, and scattered ones (no pairwise loop)
    n = 100000
    events = np.zeros(n, po.EVENT_DTYPE)
    events["row"], events["window"], events["start"], events["nbins"] = np.arange(n) % 3, 1, np.arange(n), 1
    events["snr"] = 6 + (np.arange(n) == 4321)
    labels, reps = cluster_events(events)
    assert not labels.any() and reps.tolist() == [4321]
    events["start"] *= 2
    assert np.array_equal(cluster_events(events)[0], np.arange(n))


def test_wrapped():
    e = ev((0, 2, 10, 3, 7.0))[0]  # samples [20, 26)
    assert not po.wrapped(e, np.array([-20, 0, 74]), 100)
    assert po.wrapped(e, np.array([-21, 0, 0]), 100) and po.wrapped(e, np.array([0, 75]), 100)


# ---- the many-row cases of tests/test_gpu_pulses_scale.py: what keeps a wrong scan from passing ----
# entries = rows x event_blocks(n) against one wave (512) and one trip (8192) of event_scan_kernel
SCALE_ENTRIES = {
    "two-waves": lambda m: po.SCAN_WAVE < m <= po.SCAN_TRIP,
    "full-trip": lambda m: m == po.SCAN_TRIP,
    "second-trip": lambda m: po.SCAN_TRIP < m <= po.SCAN_TRIP + po.SCAN_WAVE,
    "short-below-trip": lambda m: po.SCAN_TRIP - 3 < m < po.SCAN_TRIP,   # the last row ends inside trip 1
    "short-above-trip": lambda m: po.SCAN_TRIP < m <= po.SCAN_TRIP + 3,  # ... and straddles the boundary
    "three-trips": lambda m: 2 * po.SCAN_TRIP < m <= 3 * po.SCAN_TRIP,
    "long-rows": lambda m: po.SCAN_TRIP < m <= 2 * po.SCAN_TRIP,
    "grid-cap": lambda m: m > po.MAX_BATCH * 4,  # a first batch of 16 full trips, then 3 rows
}


def test_event_blocks():
    assert [po.event_blocks(n) for n in (1, 5, 7, 8, 16, 64, 2048, 2049, 4101, 20011)] == [1, 3, 3, 4, 4, 4, 4, 5, 7, 20]


@pytest.mark.parametrize("name", list(po.SCALE_CASES))
def test_many_row_cases_can_tell_a_wrong_scan(name):
    rows, n, threshold, _ = po.SCALE_CASES[name]
    x, events = po.scale_case(name)
    assert x.shape == (rows, n) and set(SCALE_ENTRIES) == set(po.SCALE_CASES)
    assert SCALE_ENTRIES[name](rows * po.event_blocks(n)), rows * po.event_blocks(n)
    if n < 8:
        assert po.event_blocks(n) == 3
    counts = po.window_counts(events, rows)
    assert counts.sum() == len(events) > 0
    # delivery order: row, window, start
    key = np.stack([events["start"], events["window"], events["row"]])
    assert np.array_equal(np.lexsort(key), np.arange(len(events)))
    empty = (counts.sum(axis=1) == 0).mean()
    assert 0.05 <= empty <= 0.40, empty          # offsets that do not advance, next to ones that do
    assert not counts[::17].any() and not counts[5::29].any()  # the zero rows and the NaN rows
    assert np.unique(counts).size >= 3, np.unique(counts)
    per_window = counts.sum(axis=0)
    assert per_window[0] > 0 and per_window[1] > 0
    if n >= 64:
        assert (per_window > 0).all(), per_window
    if name == "long-rows":
        assert po.event_blocks(n) == 7
        for w in (1, 2):  # runs that start in a later workgroup of the window than its first
            assert ((events["window"] == w) & (events["start"] >= po.EV_BLOCK)).any(), w
        assert ((events["window"] == 1) & (events["start"] >= 2 * po.EV_BLOCK)).any()
        assert len(events) > 8 * rows  # the wrapper's first capacity is too small
    if name in ("second-trip", "three-trips"):
        assert len(events) <= 8 * rows  # ... and here it is large enough


def test_many_rows_generator():
    x = po.many_rows(60, 64, 1)
    assert not x[0].any() and not x[17].any() and x[1].any()
    assert np.flatnonzero(np.isnan(x).any(axis=1)).tolist() == [5, 34]  # (row 34 is a zero row but for its NaN)
    assert np.isnan(x[5, 0]) and not np.isnan(x[5, 1:]).any()
    assert np.array_equal(x[1:5], po.many_rows(60, 64, 1)[1:5]) and not np.array_equal(x[1], po.many_rows(60, 64, 2)[1])
    frac = (po.many_rows(400, 64, 3)[1:17] > 6).mean()
    assert 0.06 < frac < 0.10, frac
    ev0 = po.events_of(x[:3], 2.0)
    assert np.array_equal(po.relabel(ev0, [9, 4, 7])["row"], np.array([9, 4, 7], np.int32)[ev0["row"]])


def test_batch_rows_of_the_halving_rule():
    """A workspace sized for 300, 7 or 1 of 2049 rows gives batches of 257, 5 and 1 rows; one
    sized for 32768 of 32771 rows gives 32768 (the grid cap, not the workspace)."""
    from pulsarutils import _hip
    wsb = _hip.lib().pu_series_events_workspace_bytes
    assert [po.batch_rows(wsb, 2049, 64, b) for b in (2049, 300, 7, 1)] == [2049, 257, 5, 1]
    assert po.batch_rows(wsb, 32771, 8, po.MAX_BATCH) == po.MAX_BATCH
    assert wsb(32771, 8) > wsb(po.MAX_BATCH, 8)


def call_events(lib, series=1, rows=1, n=16, ld=16, thr=6.0, events=None, cap=0, count=1, ws=256, wsb=1 << 20):
    c = ctypes.c_int64(-7)
    vp = ctypes.c_void_p
    rc = lib.pu_series_events(vp(4096) if series else None, rows, n, ld, None, thr, events, cap,
                              ctypes.byref(c) if count else None, vp(ws) if ws else None, wsb, None)
    return rc, lib.pu_last_error().decode()


def test_series_events_argument_checks_without_gpu():
    from pulsarutils import _hip
    lib = _hip.lib()
    bad = [dict(series=0), dict(count=0), dict(rows=0), dict(n=0), dict(ld=15), dict(cap=-1), dict(cap=4),
           dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(ws=0), dict(ws=257),
           dict(wsb=512)]
    for kw in bad:
        rc, msg = call_events(lib, **kw)
        assert rc == -1 and msg.startswith("pu_series_events:"), (kw, rc, msg)
    assert lib.pu_series_events_workspace_bytes(0, 4096) == 0
    assert lib.pu_series_events_workspace_bytes(5, 0) == 0
    one, two = (lib.pu_series_events_workspace_bytes(r, 20011) for r in (1, 2))
    assert 0 < one < two and one % 256 == 0
    assert one > lib.pu_series_stats_workspace_bytes(1, 20011)
    assert _hip.EVENT_DTYPE == po.EVENT_DTYPE and _hip.EVENT_DTYPE.itemsize == 40
