"""The host side of pulsarutils.filestream: the chunk lists against literal values, the step
timer with and without a ``profile`` list, and the channel mask from a ``.badchans`` cache."""
import types

import numpy as np
import pytest

from pulsarutils import filestream
from pulsarutils.filestream import StepTimer, bad_channel_mask, overlapped_chunks, tiled_chunks


def test_tiled_chunks_literal():
    assert tiled_chunks(0, 20000, 8192) == [(0, 8192), (8192, 11808)]
    assert tiled_chunks(0, 20000, 4096) == [(0, 4096), (4096, 4096), (8192, 4096), (12288, 4096), (16384, 3616)]
    assert tiled_chunks(0, 5000, 2048) == [(0, 2048), (2048, 2952)]
    assert tiled_chunks(0, 5000, 1024) == [(0, 1024), (1024, 1024), (2048, 1024), (3072, 1024), (4096, 904)]


def test_tiled_chunks_edges():
    assert tiled_chunks(0, 700, 1024) == [(0, 700)]            # shorter than a chunk: one chunk
    assert tiled_chunks(0, 1, 1024) == [(0, 1)]                # (and never merged away)
    assert tiled_chunks(0, 0, 1024) == []                      # an empty range
    assert tiled_chunks(300, 300, 1024) == []
    assert tiled_chunks(300, 2800, 1024) == [(300, 1024), (1324, 1476)]   # first > 0, 452 < 512 merged
    assert tiled_chunks(300, 2860, 1024) == [(300, 1024), (1324, 1024), (2348, 512)]  # a tail of just half stays
    assert tiled_chunks(0, 2048, 1024) == [(0, 1024), (1024, 1024)]
    assert tiled_chunks(0, 5, 1) == [(i, 1) for i in range(5)]  # chunksize // 2 == 0: nothing is ever merged


@pytest.mark.parametrize("first,last,chunksize", [(0, 20000, 8192), (17, 5000, 1000), (5, 1234, 100), (0, 3, 2)])
def test_tiled_chunks_cover_the_range_once(first, last, chunksize):
    chunks = tiled_chunks(first, last, chunksize)
    assert chunks[0][0] == first and sum(size for _, size in chunks) == last - first
    assert all(a + n == b for (a, n), (b, _) in zip(chunks, chunks[1:]))
    assert all(chunksize // 2 <= n < chunksize + chunksize // 2 or len(chunks) == 1 for _, n in chunks)


def test_overlapped_chunks_literal():
    # the reference's rule: hop step // 2, skip before tmin, skip shorter than step // 2
    assert overlapped_chunks(1000, 400, 1.0) == [(0, 400), (200, 400), (400, 400), (600, 400), (800, 200)]
    assert overlapped_chunks(999, 400, 1.0) == [(0, 400), (200, 400), (400, 400), (600, 399)]
    assert overlapped_chunks(1000, 400, 0.5, tmin=150) == [(400, 400), (600, 400), (800, 200)]
    assert overlapped_chunks(100, 400, 1.0) == []
    assert overlapped_chunks(0, 128, 1.0) == []


def test_timer_without_profile_does_nothing(monkeypatch):
    import torch
    calls = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append(1))
    timer = StepTimer(None)
    timer.start()
    timer.mark("h2d")
    timer.record(0, 10, ndm=3)
    assert calls == [] and timer.profile is None and timer._marks == []


def test_timer_records_one_dict_per_chunk(monkeypatch):
    import torch
    calls = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append(1))
    ticks = iter(np.arange(100) * 0.5)       # the clock advances by half a second per stamp
    monkeypatch.setattr(filestream, "time", types.SimpleNamespace(perf_counter=lambda: float(next(ticks))))
    profile = []
    timer = StepTimer(profile)
    for istart in (0, 512):
        timer.start()
        for name in ("h2d", "transpose", "clean"):
            timer.mark(name)
        timer.record(istart, 512, ndm=7)
    assert len(calls) == 8                   # every stamp synchronises first ("start" too)
    assert [list(rec) for rec in profile] == [["istart", "nsamples", "ndm", "h2d", "transpose", "clean"]] * 2
    assert profile[0] == {"istart": 0, "nsamples": 512, "ndm": 7, "h2d": 500.0, "transpose": 500.0, "clean": 500.0}
    assert profile[1]["istart"] == 512 and profile[1]["h2d"] == 500.0   # the second chunk starts afresh
    timer.start()
    timer.mark("h2d")
    timer.record(1024, 100)
    assert list(profile[2]) == ["istart", "nsamples", "h2d"]


def test_bad_channel_mask(tmp_path):
    fname = str(tmp_path / "x.fil")          # never opened: the cache file answers
    cached = np.zeros(16, dtype=bool)
    cached[[3, 9]] = True
    np.savetxt(fname + ".badchans", [cached], fmt="%g")
    mask = bad_channel_mask(fname, surelybad=[0, 9, 15])
    assert mask.dtype == np.bool_ and mask.flags.writeable
    assert np.flatnonzero(mask).tolist() == [0, 3, 9, 15]
    mask[:] = True                           # a caller may change its mask ...
    again = bad_channel_mask(fname)
    assert again.dtype == np.bool_ and np.array_equal(again, cached)   # ... the next call is not affected
    assert again is not mask
