"""Single-pulse candidates on the GPU against the host restatement (tests/pulse_oracle.py, pinned
by tests/test_pulse_oracle.py): pu_series_events record by record and bit for bit (runs across
workgroups, at both ends, ties, padded rows, capacity, batching), Plan.events / find_pulses /
single_pulse_search on a small chunk in three data types, and the file driver's 'pulses'."""
import ctypes
import functools

import numpy as np
import pytest

import chunk_oracle as ck
import oracle
import pulse_oracle as po

pytestmark = pytest.mark.gpu

N = po.N_SERIES
INDEX = np.array([7, 3, 0, 9, 1], np.int32)


@functools.lru_cache(maxsize=None)
def five_rows():
    b = po.series_b()
    nan = b.copy()
    nan[777] = np.nan
    rows = np.stack([b, po.series_a(), np.zeros(N), nan, -b])
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def want_five(threshold):
    return po.events_of(five_rows(), threshold, INDEX)


@functools.lru_cache(maxsize=None)
def want_b(threshold):
    return po.series_events(po.series_b(), threshold)


def padded(gpu, rows, pad=5):
    """The rows as a view of a wider device tensor (ld = n + pad, the padding NaN)."""
    import torch
    rows = np.atleast_2d(rows)
    wide = torch.full((rows.shape[0], rows.shape[1] + pad), float("nan"), dtype=torch.float64, device=gpu)
    wide[:, :rows.shape[1]] = torch.from_numpy(np.array(rows, dtype=np.float64)).to(gpu)
    return wide[:, :rows.shape[1]]


def raw_events(series, threshold, cap, index=None, batch_rows=None, null_events=False):
    """pu_series_events called directly: (count, the cap records as written)."""
    import torch
    from pulsarutils import _hip
    lib = _hip.lib()
    rows, n = series.shape
    wsb = lib.pu_series_events_workspace_bytes(batch_rows or rows, n)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=series.device)
    off = (-ws.data_ptr()) % 256
    buf = torch.zeros(max(1, cap) * 40, dtype=torch.uint8, device=series.device)
    idx = torch.from_numpy(np.asarray(index, np.int32)).to(series.device) if index is not None else None
    count = ctypes.c_int64(-1)
    _hip.check(lib.pu_series_events(_hip.ptr(series), rows, n, series.stride(0), _hip.ptr(idx), float(threshold),
                                    None if null_events else _hip.ptr(buf), cap, ctypes.byref(count),
                                    ctypes.c_void_p(ws.data_ptr() + off), wsb, _hip.stream_ptr()), "pu_series_events")
    return count.value, buf.cpu().numpy().view(po.EVENT_DTYPE)[:cap]


def assert_events_equal(got, want, where=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (where, f, bad[:5], got[bad[:5]], want[bad[:5]])
    assert got.tobytes() == want.tobytes(), where  # snr bit for bit, the order


@pytest.mark.parametrize("threshold", [6.0, 3.0, 2.0])
def test_series_events_exact(gpu, threshold):
    from pulsarutils import _hip
    want = want_five(threshold)
    assert len(want_five(6.0)) >= 20  # the helper itself must have something to say
    if threshold == 2.0:  # series A: one run per window, across many workgroups
        a = want[want["row"] == 3]
        assert [(int(e["window"]), int(e["start"]), int(e["nbins"])) for e in a] == [
            (1, 5000, 3000), (2, 2500, 1500), (4, 1250, 750), (8, 625, 375)]
    assert not np.isin(want["row"], (0, 9)).any()  # the zero row and the NaN row
    series = padded(gpu, five_rows())
    assert series.stride(0) == N + 5
    got = _hip.series_events(series, threshold, index=INDEX)
    assert_events_equal(got, want, f"threshold {threshold}")


def test_series_events_capacity(gpu):
    from pulsarutils import _hip
    want = want_b(3.0)
    assert len(want) == 30
    series = padded(gpu, po.series_b())
    count, first = raw_events(series, 3.0, 5)
    assert count == 30
    assert_events_equal(first, want[:5], "cap 5")
    count, _ = raw_events(series, 3.0, 0, null_events=True)
    assert count == 30
    assert_events_equal(_hip.series_events(series, 3.0), want, "wrapper")
    # the wrapper's second call when the first capacity is too small: threshold 1 gives thousands
    many = po.series_events(po.series_b(), 1.0)
    assert len(many) > 256
    assert_events_equal(_hip.series_events(series, 1.0), many, "wrapper, reallocated")


def test_series_events_batching_and_determinism(gpu):
    want = want_five(6.0)
    series = padded(gpu, five_rows())
    count, full = raw_events(series, 6.0, len(want) + 3, index=INDEX)
    assert count == len(want)
    assert_events_equal(full[:count], want, "one batch")
    assert not full[count:].tobytes().strip(b"\0")  # nothing written past the count
    for batch_rows in (2, 1):
        c2, small = raw_events(series, 6.0, len(want) + 3, index=INDEX, batch_rows=batch_rows)
        assert c2 == count and small.tobytes() == full.tobytes(), batch_rows
    c3, again = raw_events(series, 6.0, len(want) + 3, index=INDEX)
    assert c3 == count and again.tobytes() == full.tobytes()


@pytest.mark.parametrize("m", [8, 9, 15, 16, 17])
def test_series_events_short_series(gpu, m):
    from pulsarutils import _hip
    want = po.series_events(po.spike(m), 1.5)
    assert len(want) >= 2
    assert_events_equal(_hip.series_events(padded(gpu, po.spike(m), pad=3), 1.5), want, f"m = {m}")


# ---- through a plan ----
THRESHOLD = 6.0


@functools.lru_cache(maxsize=None)
def plan_expected(kind):
    """(array, band, dms, oracle snr, helper events of every trial, helper pulse table)."""
    from pulsarutils import _planner
    x, band = po.plan_case()
    arr = {"f32": x.astype(np.float32), "f64": x,
           "u8": np.clip(np.rint(x * 16 + 128), 0, 255).astype(np.uint8)}[kind]
    dms = _planner.dedispersion_plan(64, 100, 200, band["start_freq"], band["bandwidth"], band["sample_time"])
    assert dms.size == 154
    _, _, snr, _, dd = oracle.search(arr, dms, band["start_freq"], band["bandwidth"], band["sample_time"],
                                     return_dedisp=True)
    events = po.events_of(dd, THRESHOLD)
    table = po.pulse_table(events, dms, band["start_freq"], band["bandwidth"], band["sample_time"], 64, arr.shape[1])
    return arr, band, dms, snr, events, table


def assert_tables_equal(got, want, where=""):
    assert list(got.colnames) == list(want), (where, got.colnames)
    for c, w in want.items():
        g = np.asarray(got[c])
        assert g.dtype == w.dtype and g.shape == w.shape, (where, c, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (where, c, g, w)


@pytest.mark.parametrize("kind", ["f32", "f64", "u8"])
def test_pulses_through_a_plan(gpu, kind):
    from pulsarutils import dedispersion as dd, pulses
    arr, band, dms, osnr, want_events, want_table = plan_expected(kind)
    above = np.flatnonzero(osnr > THRESHOLD)
    # a trial has an event iff the reference's snr exceeds the threshold, and its largest is that snr
    assert np.array_equal(np.unique(want_events["row"]), above)
    for tr in above:
        assert want_events["snr"][want_events["row"] == tr].max() == osnr[tr]
    if kind == "f32":
        assert above.size == 39 and want_events.size == 148
        assert want_table["trial"].tolist() == [77, 77] and want_table["sample"].tolist() == [1000, 3000]
        assert want_table["width"].tolist() == [1, 2] and not want_table["wrapped"].any()
        assert abs(want_table["DM"][0] - 150.37) < 0.01
    x = dd._prepare_data(arr)
    outs, plan = dd.search_device(x, dms, 64, **band)
    selected = np.flatnonzero(outs[2].cpu().numpy() > THRESHOLD * (1 - 1e-4)).astype(np.int32)
    assert np.isin(above, selected).all()
    got = plan.events(x, selected, THRESHOLD)
    assert_events_equal(got, want_events, kind)
    assert_tables_equal(pulses.find_pulses(arr, dms, 64, threshold=THRESHOLD, **band), want_table, kind)
    assert_tables_equal(pulses.find_pulses(x, dms, 64, threshold=THRESHOLD, plan=plan, table=outs, **band),
                        want_table, kind + " (table passed)")
    # dm_tol 1 and a time tolerance: against the helper's clustering of the same events
    for dm_tol, time_tol in ((1, 0), (0, 3)):
        want = po.pulse_table(want_events, dms, band["start_freq"], band["bandwidth"], band["sample_time"], 64,
                              arr.shape[1], dm_tol, time_tol)
        assert_tables_equal(pulses.find_pulses(x, dms, 64, threshold=THRESHOLD, dm_tol=dm_tol, time_tol=time_tol,
                                               plan=plan, table=outs, **band), want, f"{kind} {dm_tol} {time_tol}")
    # single_pulse_search: the search's own table, and the same pulses
    table, found = dd.single_pulse_search(arr, 100, 200, threshold=THRESHOLD, **band)
    plain = dd.dedispersion_search(arr, 100, 200, band["start_freq"], band["bandwidth"], band["sample_time"])
    assert list(table.colnames) == list(plain.colnames)
    for c in plain.colnames:
        a, b = np.asarray(table[c]), np.asarray(plain[c])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), c
    assert_tables_equal(found, want_table, kind + " single_pulse_search")


def test_nonfinite_input_gives_no_pulses(gpu):
    from pulsarutils import pulses
    arr, band, dms, *_ = plan_expected("f32")
    bad = arr.copy()
    bad[5, 100] = np.inf
    got = pulses.find_pulses(bad, dms, 64, threshold=THRESHOLD, **band)
    assert len(got) == 0 and list(got.colnames) == list(po.COLUMNS)


# ---- the file driver ----
DMMIN, DMMAX = 250, 350


@pytest.fixture(scope="module")
def pulse_file(gpu, tmp_path_factory):
    fname = str(tmp_path_factory.mktemp("pulses") / "main_u8.fil")
    ck.write_pulse_file(fname, "u8", **ck.MAIN)
    return fname


def expected_pulses(fname, search_dtype, new_sample_time):
    """Per candidate chunk (oracle snr above 6 somewhere): (istart, iend, helper pulse table
    with the driver's time offset and file_sample)."""
    from pulsarutils import sigproc
    h = sigproc.read_header(fname)[0]
    N, tsamp = ck.resample_factor(h, DMMIN, new_sample_time)
    out = []
    for istart, iend, plane, dms, (_, _, osnr, _), _ in ck.expected_chunks(
            fname, DMMIN, DMMAX, new_sample_time=new_sample_time, search_dtype=search_dtype):
        if not np.any(osnr > 6):
            continue
        searched = plane.astype(np.float32) if search_dtype == "f32" else plane
        sel = np.flatnonzero(osnr > 6)
        dd = oracle.search(searched, dms[sel], h["fbottom"], h["bandwidth"], tsamp, return_dedisp=True)[4]
        events = po.events_of(dd, 6.0, sel)
        tab = po.pulse_table(events, dms, h["fbottom"], h["bandwidth"], tsamp, h["nchans"], plane.shape[1])
        tab["time"] = tab["time"] + istart * h["tsamp"]
        tab["file_sample"] = istart + N * tab["sample"]
        out.append((istart, iend, tab))
    return out


@pytest.mark.parametrize("N,search_dtype", [(1, "f64"), (3, "f32")])
def test_search_by_chunks_pulses(pulse_file, tmp_path, monkeypatch, N, search_dtype):
    from pulsarutils import clean
    monkeypatch.chdir(tmp_path)
    kw = dict(dmmin=DMMIN, dmmax=DMMAX, snr_threshold=6, search_dtype=search_dtype, new_sample_time=N * ck.TSAMP)
    want = expected_pulses(pulse_file, search_dtype, N * ck.TSAMP)
    with_pulses = clean.search_by_chunks(pulse_file, find_pulses=True, **kw)
    assert [(c["istart"], c["iend"]) for c in with_pulses] == [(w[0], w[1]) for w in want]
    assert len(want) == 3 and want[1][:2] == (7220, 10830)
    for c, (istart, _, tab) in zip(with_pulses, want):
        assert_tables_equal(c["pulses"], tab, f"chunk {istart}")
    # the middle chunk holds the pulse unwrapped (inside its peak bin of at most 8 resampled samples);
    # its neighbours see it (or its image) wrapped
    mid = want[1][2]
    assert len(mid["snr"]) == 1 and not mid["wrapped"][0] and abs(mid["file_sample"][0] - ck.PULSE_T) < 8 * N
    assert abs(mid["DM"][0] - ck.PULSE_DM) < 1
    assert want[0][2]["wrapped"].all() and want[2][2]["wrapped"].all()
    # find_pulses=False: the same candidates, bit-equal tables, no new key
    plain = clean.search_by_chunks(pulse_file, **kw)
    assert [(c["istart"], c["iend"]) for c in plain] == [(c["istart"], c["iend"]) for c in with_pulses]
    for a, b in zip(plain, with_pulses):
        assert "pulses" not in a and set(b) - set(a) == {"pulses"}
        for col in ("DM", "max", "std", "snr", "rebin"):
            assert np.asarray(a["table"][col]).tobytes() == np.asarray(b["table"][col]).tobytes(), col
        assert (a["dm"], a["snr"], a["rebin"], a["t0"]) == (b["dm"], b["snr"], b["rebin"], b["t0"])
