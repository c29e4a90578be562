"""pu_series_events where its bookkeeping changes shape, record by record and bit for bit against
tests/pulse_oracle.py: count tables beyond one wave and one trip of event_scan_kernel (8 entries
per thread, 512 per wave, 8192 per trip), rows with three entries (n < 8), seven workgroups per
row, batches forced by the workspace and by the 32768-row grid cap with and without an index,
series shorter than 8 samples, and a threshold equal to an event's own S/N.  The inputs are
pinned without a GPU in tests/test_pulse_oracle.py."""
import functools

import numpy as np
import pytest

import pulse_oracle as po
from test_gpu_pulses import assert_events_equal, padded, raw_events

pytestmark = pytest.mark.gpu


def check_raw(series, want, threshold, where, **kw):
    """One direct call with room for three records more than there are: the count, every
    record in order, nothing past the count.  Returns the bytes of the whole buffer."""
    count, got = raw_events(series, threshold, len(want) + 3, **kw)
    assert count == len(want), (where, count, len(want))
    assert_events_equal(got[:count], want, where)
    assert not got[count:].tobytes().strip(b"\0"), where  # nothing written past the count
    return got.tobytes()


@functools.lru_cache(maxsize=None)
def permutation(rows):
    return np.random.default_rng(rows).permutation(rows).astype(np.int32)


@pytest.mark.parametrize("name", [k for k in po.SCALE_CASES if k != "grid-cap"])
def test_events_over_many_rows(gpu, name):
    rows, n, threshold, _ = po.SCALE_CASES[name]
    x, want = po.scale_case(name)
    series = padded(gpu, x)
    assert series.shape == (rows, n) and series.stride(0) == n + 5
    check_raw(series, want, threshold, name)


@pytest.mark.parametrize("name", ["second-trip", "three-trips", "long-rows"])
def test_events_over_many_rows_through_the_wrapper(gpu, name):
    """The wrapper's first capacity max(256, 8 rows) holds the first two and not the third."""
    from pulsarutils import _hip
    rows, n, threshold, _ = po.SCALE_CASES[name]
    x, want = po.scale_case(name)
    assert (len(want) > max(256, 8 * rows)) == (name == "long-rows")
    assert_events_equal(_hip.series_events(padded(gpu, x), threshold), want, name)


def test_batches_without_an_index_label_rows_from_the_batch_start(gpu):
    from pulsarutils import _hip
    rows, n, threshold, _ = po.SCALE_CASES["second-trip"]
    x, want = po.scale_case("second-trip")
    assert want["row"].max() == rows - 1 and np.unique(want["row"]).size > rows // 2
    series = padded(gpu, x)
    full = check_raw(series, want, threshold, "one batch")
    wsb = _hip.lib().pu_series_events_workspace_bytes
    for sized_for, per in ((300, 257), (7, 5), (1, 1)):
        assert po.batch_rows(wsb, rows, n, sized_for) == per
        assert check_raw(series, want, threshold, f"batches of {per}", batch_rows=sized_for) == full
    index = permutation(rows)
    want_index = po.relabel(want, index)
    assert not np.array_equal(want_index["row"], want["row"])
    labelled = check_raw(series, want_index, threshold, "index, one batch", index=index)
    assert check_raw(series, want_index, threshold, "index, batches of 257", index=index, batch_rows=300) == labelled


@pytest.mark.parametrize("with_index", [False, True], ids=["rows", "index"])
def test_more_rows_than_one_launch_takes(gpu, with_index):
    """32771 rows, a workspace sized for 32768: the grid cap splits the call into 32768 + 3 rows."""
    from pulsarutils import _hip
    rows, n, threshold, _ = po.SCALE_CASES["grid-cap"]
    x, want = po.scale_case("grid-cap")
    assert rows > po.MAX_BATCH and po.batch_rows(_hip.lib().pu_series_events_workspace_bytes, rows, n,
                                                  po.MAX_BATCH) == po.MAX_BATCH
    assert (want["row"] >= po.MAX_BATCH).any()  # the second batch has something to deliver
    index = permutation(rows) if with_index else None
    if with_index:
        want = po.relabel(want, index)
    check_raw(padded(gpu, x), want, threshold, "grid cap", index=index, batch_rows=po.MAX_BATCH)


# ---- series shorter than 8 samples: fewer than four windows, tail windows without a workgroup ----
def short_rows(n):
    """A spike alone (its widest window has one bin: std 0), noise with spikes, zeros, a ramp;
    for n = 4 also a row whose window-2 bins are both 0 after the mean is taken out."""
    rows = [po.spike(n), po.many_rows(3, n, 40 + n)[1], np.zeros(n), np.arange(n, dtype=np.float64) ** 2,
            -po.spike(n)]
    if n == 4:
        rows.append(np.array([100.0, 0.0, 0.0, 100.0]))
    return np.stack(rows)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7])
def test_series_shorter_than_eight_samples(gpu, n):
    x = short_rows(n)
    threshold = 0.5
    want = po.events_of(x, threshold)
    if n == 1:
        assert len(want) == 0  # one bin: std 0 in its only window
    else:
        assert len(want) >= 3 and want["window"].max() <= n // 2
        assert (want["row"] == 0).any() and not (want["row"] == 2).any()
        spike_windows = set(want["window"][want["row"] == 0].tolist())
        assert 1 in spike_windows and max(w for w in po.WINDOWS if w <= n) not in spike_windows
    if n == 4:
        assert set(want["window"][want["row"] == 5].tolist()) == {1}  # window 2: [0, 0]; window 4: one bin
    check_raw(padded(gpu, x, pad=3), want, threshold, f"n = {n}")


# ---- a threshold equal to an event's own S/N: the rule is strict ----
def test_threshold_equal_to_an_events_snr(gpu):
    rows, n, low, _ = po.SCALE_CASES["two-waves"]
    x, at_low = po.scale_case("two-waves")
    best = np.full(rows, -np.inf)
    np.maximum.at(best, at_low["row"], at_low["snr"])
    with_events = np.flatnonzero(np.isfinite(best))
    row = int(with_events[np.argsort(best[with_events])[len(with_events) // 2]])  # the median row maximum
    threshold = float(best[row])
    want = po.events_of(x, threshold)
    # the oracle alone: the row's largest event is gone (and with it the row), rows above it stay
    assert threshold > low and (at_low["snr"] == threshold).any()
    assert not (want["row"] == row).any() and not (want["snr"] == threshold).any()
    assert 10 <= len(want) < len(at_low) and (want["snr"] > threshold).all()
    series = padded(gpu, x)
    check_raw(series, want, threshold, "threshold = an event's S/N")
    count, _ = raw_events(series, threshold, 0, null_events=True)
    assert count == len(want)
    # just below it the event is back, with the S/N that was the threshold
    below = np.nextafter(threshold, 0.0)
    want_below = po.events_of(x, below)
    assert ((want_below["row"] == row) & (want_below["snr"] == threshold)).sum() >= 1
    check_raw(series, want_below, below, "threshold one ulp below")
