"""Host restatement of the single-pulse definitions (include/pulsarutils_hip.h, pu_series_events;
pulsarutils/pulses.py): the events of a float64 series, their clustering into pulses, the
``wrapped`` flag and the pulse table, in plain numpy loops.

Test infrastructure only.  Nothing here imports ``pulsarutils.pulses`` (the code under test);
series come from ``oracle.dedisperse`` / ``oracle.search(return_dedisp=True)``.
tests/test_pulse_oracle.py pins ``series_events`` against the golden-pinned
``oracle.trial_stats``."""
import functools

import numpy as np

import oracle

EVENT_DTYPE = np.dtype([("row", "<i4"), ("window", "<i4"), ("start", "<i8"), ("nbins", "<i8"), ("peak", "<i8"),
                        ("snr", "<f8")])
WINDOWS = (1, 2, 4, 8)


def quick_resample(s, w):
    """dedispersion.py:53-56 on a 1-D series: ``(0 + s[wi]) + s[wi + 1] + ...``."""
    nb = s.size // w
    acc = np.zeros(nb)
    for j in range(w):
        acc = acc + s[j:nb * w:w]
    return acc


def series_events(d, threshold, row=0):
    """Events of one float64 series ``d`` (the definition, window by window)."""
    d = np.asarray(d, dtype=np.float64)
    out = []
    with np.errstate(all="ignore"):
        s = d - np.mean(d)
        for w in WINDOWS:
            if s.size // w < 1:
                continue
            reb = quick_resample(s, w)
            sd = np.std(reb)
            if not (np.isfinite(sd) and sd > 0):
                continue
            above = reb / sd > threshold
            # maximal runs of above bins: where the flag changes, the series taken as linear
            pad = np.concatenate(([False], above, [False]))
            edges = np.flatnonzero(pad[1:] != pad[:-1])
            for i, j in zip(edges[::2].tolist(), edges[1::2].tolist()):
                peak = i + int(np.argmax(reb[i:j]))  # the first largest bin
                out.append((row, w, i, j - i, peak, reb[peak] / sd))
    return np.array(out, dtype=EVENT_DTYPE)


def events_of(series, threshold, index=None):
    """Events of every row of ``series`` in delivery order (row, window, start)."""
    parts = [series_events(s, threshold, r if index is None else int(index[r])) for r, s in enumerate(series)]
    return np.concatenate(parts) if parts else np.zeros(0, EVENT_DTYPE)


def interval(e):
    lo = int(e["start"]) * int(e["window"])
    return lo, lo + int(e["nbins"]) * int(e["window"])


def friends(a, b, dm_tol, time_tol):
    (alo, ahi), (blo, bhi) = interval(a), interval(b)
    gap = max(alo, blo) - min(ahi, bhi)  # <= 0: overlapping or touching
    return abs(int(a["row"]) - int(b["row"])) <= dm_tol and gap <= time_tol


def cluster(events, dm_tol=2, time_tol=0):
    """Connected components of ``friends`` by flood fill over all pairs.  ``(labels,
    representatives)``: pulses numbered by their first member in the given order."""
    n = len(events)
    labels = np.full(n, -1, np.int64)
    reps = []
    for seed in range(n):
        if labels[seed] >= 0:
            continue
        p = len(reps)
        labels[seed] = p
        todo = [seed]
        while todo:
            i = todo.pop()
            for j in range(n):
                if labels[j] < 0 and friends(events[i], events[j], dm_tol, time_tol):
                    labels[j] = p
                    todo.append(j)
        members = [i for i in range(n) if labels[i] == p]
        # highest snr; ties: lowest trial, smallest window, earliest start
        reps.append(min(members, key=lambda i: (-float(events[i]["snr"]), int(events[i]["row"]),
                                                int(events[i]["window"]), int(events[i]["start"]))))
    return labels, np.array(reps, np.int64)


def wrapped(e, shifts, n):
    """The event's samples read columns ``t + shift_c`` outside ``[0, n)`` for some channel."""
    lo, hi = interval(e)
    return bool(lo + int(np.min(shifts)) < 0 or hi - 1 + int(np.max(shifts)) >= n)


COLUMNS = ("trial", "DM", "snr", "width", "sample", "time", "members", "trial_lo", "trial_hi", "sample_lo",
           "sample_hi", "wrapped")


def pulse_table(events, dms, start_freq, bandwidth, sample_time, nchan, n, dm_tol=2, time_tol=0):
    """The pulse table as a dict of numpy columns, sorted by snr descending (ties: trial,
    width, sample); shifts from ``oracle.shifts``."""
    labels, reps = cluster(events, dm_tol, time_tol)
    rows = []
    for p, ri in enumerate(reps):
        e = events[ri]
        mem = events[labels == p]
        w, trial = int(e["window"]), int(e["row"])
        sample = int(e["peak"]) * w
        iv = [interval(m) for m in mem]
        sh = oracle.shifts(nchan, dms[trial], start_freq, bandwidth, sample_time)
        rows.append((trial, float(dms[trial]), float(e["snr"]), w, sample, (sample + w / 2) * sample_time, len(mem),
                     int(mem["row"].min()), int(mem["row"].max()), min(a for a, _ in iv), max(b for _, b in iv),
                     wrapped(e, sh, n)))
    rows.sort(key=lambda r: (-r[2], r[0], r[3], r[4]))
    kinds = {"DM": np.float64, "snr": np.float64, "time": np.float64, "wrapped": bool}
    return {c: np.array([r[k] for r in rows], dtype=kinds.get(c, np.int64)) for k, c in enumerate(COLUMNS)}


# ---- the series of the tests ----
N_SERIES = 20011  # odd: every window drops a different tail


def series_a():
    d = np.random.default_rng(7).standard_normal(N_SERIES)
    d[5000:8000] += 50
    return d


def series_b():
    n = N_SERIES
    d = np.random.default_rng(7).standard_normal(n)
    d[0:3] += 30
    d[n - 2:] += 30
    d[12000:12004] = 40
    for c in (256, 1024, 4096, 8192, 16384):
        d[c - 1:c + 1] += 25
    return d


def spike(m):
    d = np.zeros(m)
    d[m // 2] = 100.0
    return d


# ---- many rows: the count table of pu_series_events beyond one wave and one trip of its scan ----
EV_BLOCK = 2048        # bins of one workgroup of the event stage (csrc/exact.hip, kEvBlock)
SCAN_WAVE = 64 * 8     # entries one wave of event_scan_kernel takes per trip
SCAN_TRIP = 1024 * 8   # entries of one trip
MAX_BATCH = 32768      # rows of one batch at the most (the launches' grid.y)


def event_blocks(n):
    """Entries of the count table per row: one per EV_BLOCK bins of each window."""
    return sum(((n >> k) + EV_BLOCK - 1) // EV_BLOCK for k in range(4))


def many_rows(rows, n, seed):
    """``rows`` series of N(0, 1) noise with +12 on about 8 % of the samples; every 17th row all
    zero (std 0: no event) and a NaN in sample 0 of every 29th row from row 5 (no event)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, n))
    x[rng.random((rows, n)) < 0.08] += 12.0
    x[::17] = 0.0
    x[5::29, 0] = np.nan
    x.setflags(write=False)
    return x


# (rows, n, threshold, seed) by what the rows x event_blocks(n) entries reach in the scan
SCALE_CASES = {
    "two-waves": (129, 64, 2.0, 129),           # 516 entries: wave 1 of the first trip
    "full-trip": (2048, 64, 2.0, 2048),         # 8192: exactly one trip
    "second-trip": (2049, 64, 2.0, 2049),       # 8196: a second trip of 4 entries
    "short-below-trip": (2730, 5, 1.0, 2730),   # 8190: 3 entries per row (windows 1, 2, 4)
    "short-above-trip": (2731, 5, 1.0, 2731),   # 8193
    "three-trips": (4500, 16, 2.0, 4500),       # 18000
    "long-rows": (1200, 4101, 3.0, 1200),       # 8400: 7 workgroups per row (3 + 2 + 1 + 1)
    "grid-cap": (32771, 8, 1.5, 32771),         # two batches forced by MAX_BATCH
}


@functools.lru_cache(maxsize=None)
def scale_case(name):
    """(the rows, their events in delivery order) of a SCALE_CASES entry, computed once."""
    rows, n, threshold, seed = SCALE_CASES[name]
    x = many_rows(rows, n, seed)
    want = events_of(x, threshold)
    want.setflags(write=False)
    return x, want


def window_counts(events, rows):
    """Events per (row, window) as a rows x 4 int64 array (rows labelled 0 .. rows - 1)."""
    c = np.zeros((rows, 4), np.int64)
    np.add.at(c, (events["row"], np.log2(events["window"]).astype(np.int64)), 1)
    return c


def relabel(events, index):
    """The events of rows 0 .. with ``row`` replaced by ``index[row]`` (what an index does)."""
    out = events.copy()
    out["row"] = np.asarray(index, np.int32)[events["row"]]
    return out


def batch_rows(workspace_bytes_of, rows, n, sized_for):
    """Rows per batch pu_series_events picks with a workspace sized for ``sized_for`` rows: at
    most MAX_BATCH, halved (rounding up) until the batch fits."""
    per = min(rows, MAX_BATCH)
    while per > 1 and workspace_bytes_of(per, n) > workspace_bytes_of(sized_for, n):
        per = (per + 1) // 2
    return per


def plan_case():
    """The chunk of the plan-level tests: 64 x 4096 N(0, 1) noise (seed 3), band 1200 + 200
    MHz, tsamp 5e-4; a +3 impulse per channel dispersed at DM 150 at sample 1000 and a
    two-sample +2 pulse at samples 3000-3001.  Returns (float64 array, band dict)."""
    nchan, n = 64, 4096
    band = dict(start_freq=1200.0, bandwidth=200.0, sample_time=5e-4)
    np.random.seed(3)
    x = np.random.normal(0, 1, (nchan, n))
    sh = oracle.shifts(nchan, 150.0, band["start_freq"], band["bandwidth"], band["sample_time"])
    for c in range(nchan):
        x[c, (1000 + sh[c]) % n] += 3
        x[c, (3000 + sh[c]) % n] += 2
        x[c, (3001 + sh[c]) % n] += 2
    return x, band
