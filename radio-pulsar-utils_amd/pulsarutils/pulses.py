"""Single-pulse candidates: events of the dedispersed series, clustered into pulses.

The search (``dedispersion.search_device``) reduces every trial to (max, std, snr,
rebin).  This module answers what the reference leaves to a person looking at
``plot_diagnostics``: when in the chunk a pulse arrived, how wide it was, how many there
were, and whether a peak is a wrap-around of the circular shift-and-sum.

**Events** of one float64 series ``d`` at ``threshold`` (``pu_series_events``,
include/pulsarutils_hip.h; the quantities are the reference's, dedispersion.py:186-201):
``s = d - mean(d)``; for window ``w`` in 1, 2, 4, 8, ``reb = quick_resample(s, w)`` and
``sd = np.std(reb)``; bin ``i`` is above when ``reb[i] / sd > threshold``; an event is a
maximal run ``[start, start + nbins)`` of above bins, ``peak`` its first largest bin and
``snr = reb[peak] / sd``.  A trial has an event iff its table S/N exceeds ``threshold``, and
its largest event S/N is then that S/N bit for bit: so the fast search is the filter and the
exact float64 series are computed for the few trials that pass it (:func:`find_pulses`).

**Pulses**: two events are friends when their trials differ by at most ``dm_tol`` and their
sample intervals ``[start * w, (start + nbins) * w)`` overlap or lie at most ``time_tol``
samples apart (touching intervals: gap 0).  A pulse is a connected component of that
relation; its representative is the member of highest S/N (ties: lowest trial, smallest
window, earliest start).

Importable without a GPU (:func:`cluster_events` is pure numpy); the HIP library is only
touched by :func:`find_pulses`.
"""
import numpy as np

from . import _hip
from .table import make_table

EVENT_DTYPE = _hip.EVENT_DTYPE

COLUMNS = ("trial", "DM", "snr", "width", "sample", "time", "members", "trial_lo", "trial_hi", "sample_lo",
           "sample_hi", "wrapped")


def _components(n, a, b):
    """Connected components of the graph on ``n`` nodes with edges ``a[i] - b[i]``: every
    node's label is the smallest node of its component (hook the larger root under the
    smaller, then pointer jumping, until no edge joins two labels)."""
    labels = np.arange(n, dtype=np.int64)
    while a.size:
        la, lb = labels[a], labels[b]
        differ = la != lb
        if not differ.any():
            break
        la, lb = la[differ], lb[differ]
        a, b = a[differ], b[differ]
        low = np.minimum(la, lb)
        np.minimum.at(labels, la, low)
        np.minimum.at(labels, lb, low)
        while True:
            jumped = labels[labels]
            if np.array_equal(jumped, labels):
                break
            labels = jumped
    return labels


def cluster_events(events, dm_tol=2, time_tol=0):
    """Group events (``EVENT_DTYPE`` records; ``row`` is the trial) into pulses.

    Returns ``(labels, representatives)``: ``labels[i]`` is the pulse of event ``i``, pulses
    numbered by their first member in the given order; ``representatives[p]`` is the index
    of pulse ``p``'s representative event.  Sort by (trial, start sample), one running
    furthest end per trial, a binary search per trial offset and a vectorised union-find:
    O(E (dm_tol + log E)), no pairwise loop.
    """
    ev = np.asarray(events)
    n = ev.size
    dm_tol, time_tol = int(dm_tol), int(time_tol)
    if dm_tol < 0 or time_tol < 0:
        raise ValueError("dm_tol and time_tol must be >= 0")
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    row = ev["row"].astype(np.int64)
    row -= row.min()
    w = ev["window"].astype(np.int64)
    lo = ev["start"].astype(np.int64) * w
    hi = lo + ev["nbins"].astype(np.int64) * w  # one past the last sample
    base = lo.min()
    lo, hi = lo - base, hi - base
    big = int(hi.max()) + time_tol + 2
    if (int(row.max()) + dm_tol + 2) * big >= 2 ** 62:
        raise ValueError("cluster_events: trial x sample range too large for 64-bit keys")
    order = np.lexsort((lo, row))
    srow, slo, shi = row[order], lo[order], hi[order]
    key = srow * big + slo  # ascending
    # per trial, the furthest end among the events up to each one and who reaches it: an event
    # of a trial within dm_tol that starts no earlier than they do is a friend of one of them
    # iff it is a friend of that one, and they are all friends of each other
    reach = np.maximum.accumulate(srow * big + shi)
    holder = np.maximum.accumulate(np.where(srow * big + shi == reach, np.arange(n), -1))
    ea, eb = [], []
    for d in range(-dm_tol, dm_tol + 1):
        # the last event of trial + d that starts no later (of its own trial: the one before it)
        j = np.searchsorted(key, (srow + d) * big + slo, side="right") - 1 if d else np.arange(n) - 1
        ok = j >= 0
        jj = np.where(ok, j, 0)
        ok &= srow[jj] == srow + d
        ok &= reach[jj] - srow[jj] * big + time_tol >= slo
        ea.append(np.flatnonzero(ok))
        eb.append(holder[jj[ok]])
    a, b = order[np.concatenate(ea)], order[np.concatenate(eb)]
    roots = _components(n, a, b)
    _, labels = np.unique(roots, return_inverse=True)  # roots are first members: in their order
    labels = labels.astype(np.int64)
    # representative: highest snr, then lowest trial, smallest window, earliest start
    best = np.lexsort((ev["start"], ev["window"], ev["row"], -ev["snr"], labels))
    first = np.ones(n, bool)
    first[1:] = labels[best][1:] != labels[best][:-1]
    return labels, best[first].astype(np.int64)


def _empty_table():
    kinds = {"DM": np.float64, "snr": np.float64, "time": np.float64, "wrapped": bool}
    return make_table({c: np.zeros(0, kinds.get(c, np.int64)) for c in COLUMNS})


def pulse_table(events, trial_DMs, shifts_of, nsamples, sample_time, dm_tol=2, time_tol=0):
    """The pulse table of ``events`` (trial-labelled): one row per cluster, described by its
    representative.  ``shifts_of(trials)`` returns the integer shift table of those trials
    (``pu_shift_table``), from which ``wrapped`` is decided."""
    ev = np.asarray(events)
    if ev.size == 0:
        return _empty_table()
    labels, reps = cluster_events(ev, dm_tol, time_tol)
    npulse = reps.size
    rep = ev[reps]
    trial = rep["row"].astype(np.int64)
    w = rep["window"].astype(np.int64)
    sample = rep["peak"] * w
    allw = ev["window"].astype(np.int64)
    lo, hi = ev["start"] * allw, (ev["start"] + ev["nbins"]) * allw
    members = np.bincount(labels, minlength=npulse).astype(np.int64)
    trial_lo, trial_hi = np.full(npulse, np.iinfo(np.int64).max), np.full(npulse, -1, np.int64)
    sample_lo, sample_hi = trial_lo.copy(), trial_hi.copy()
    np.minimum.at(trial_lo, labels, ev["row"].astype(np.int64))
    np.maximum.at(trial_hi, labels, ev["row"].astype(np.int64))
    np.minimum.at(sample_lo, labels, lo)
    np.maximum.at(sample_hi, labels, hi)
    # the representative's samples [start w, (start + nbins) w) read column t + shift_c of
    # channel c: past either end of the chunk they come from the other end (circular sum)
    sh = np.asarray(shifts_of(trial)).reshape(npulse, -1)
    wrapped = (rep["start"] * w + sh.min(axis=1) < 0) | ((rep["start"] + rep["nbins"]) * w - 1 + sh.max(axis=1)
                                                         >= int(nsamples))
    cols = {"trial": trial, "DM": np.asarray(trial_DMs, np.float64)[trial], "snr": rep["snr"].astype(np.float64),
            "width": w, "sample": sample, "time": (sample + w / 2) * sample_time, "members": members,
            "trial_lo": trial_lo, "trial_hi": trial_hi, "sample_lo": sample_lo, "sample_hi": sample_hi,
            "wrapped": wrapped}
    order = np.lexsort((sample, w, trial, -cols["snr"]))
    return make_table({c: np.asarray(cols[c])[order] for c in COLUMNS})


def find_pulses(data, trial_DMs, nchan, start_freq, bandwidth, sample_time, threshold=6.0, acc=None, dm_tol=2,
                time_tol=0, plan=None, table=None):
    """Single pulses of a (nchan, nsamples) chunk over the trial grid ``trial_DMs``.

    Runs ``search_device`` (unless its outputs are passed as ``table`` together with its
    ``plan``), selects the trials with ``snr > threshold * (1 - 1e-4)`` (the slack covers the
    float32 path's 1e-5 bar; a trial selected in vain has no event, so the slack never
    changes the result), takes the events of their exact float64 series (``Plan.events``:
    ``pu_plan_exact_series`` + ``pu_series_events``) and clusters them.

    Returns a Table sorted by ``snr`` descending (ties: trial, width, sample), one row per
    pulse: ``trial``, ``DM`` and ``snr`` of the representative event; ``width`` = its window
    ``w`` (samples) and ``sample`` = ``peak * w``; ``time`` = ``(sample + w / 2) *
    sample_time``; ``members`` = events in the cluster, which span trials ``trial_lo ..
    trial_hi`` and samples ``[sample_lo, sample_hi)``; ``wrapped``: the representative's
    samples read columns across the circular seam of the chunk.  An input holding NaN or
    +-inf (the search's NaN rule: every S/N is 0) gives an empty table.
    """
    from . import dedispersion as dd
    threshold = float(threshold)
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError("threshold must be finite and > 0")
    x = dd._prepare_data(data)
    dms = np.ascontiguousarray(np.atleast_1d(np.asarray(trial_DMs, dtype=np.float64)))
    if table is None or plan is None:
        table, plan = dd.search_device(x, dms, nchan, start_freq, bandwidth, sample_time, acc=acc, plan=plan)
    snr = table[2]
    snr = snr.detach().cpu().numpy() if hasattr(snr, "detach") else np.asarray(snr)
    trials = np.flatnonzero(snr > threshold * (1 - 1e-4)).astype(np.int32)
    if trials.size == 0:
        return _empty_table()
    events = plan.events(x, trials, threshold)
    return pulse_table(events, dms, lambda tr: _hip.shift_table(nchan, dms[tr], start_freq, bandwidth, sample_time),
                       x.shape[1], sample_time, dm_tol, time_tol)
