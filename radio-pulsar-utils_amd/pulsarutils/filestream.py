"""What ``clean.search_by_chunks``, ``clean.cleanup_data`` and ``folding.fold_file`` share: the channel
mask, the two chunk rules, the step timer and the stream of device blocks.  Importable without a GPU."""
import time

import numpy as np

from . import _hip


def bad_channel_mask(fname, surelybad=(), stats=None):
    """``get_bad_chans(fname, stats=stats)`` with ``surelybad`` set: a fresh ``bool`` array."""
    from .stats import get_bad_chans
    mask = np.array(get_bad_chans(fname, stats=stats), dtype=bool)
    for bad_chan in surelybad:
        mask[bad_chan] = True
    return mask


def tiled_chunks(first, last, chunksize):
    """``(istart, size)`` of the non-overlapping ``chunksize``-sample chunks over ``[first, last)``;
    a tail shorter than ``chunksize // 2`` is merged into the chunk before it."""
    chunks = [(i, min(chunksize, last - i)) for i in range(first, last, chunksize)]
    if len(chunks) > 1 and chunks[-1][1] < chunksize // 2:
        chunks[-2:] = [(chunks[-2][0], chunks[-2][1] + chunks[-1][1])]
    return chunks


def overlapped_chunks(nsamples, step, sample_time, tmin=0):
    """The reference's search chunks (clean.py:319-325): ``step`` samples at a hop of ``step // 2``
    (50 % overlap); chunks before ``tmin`` seconds or shorter than ``step // 2`` are skipped."""
    sizes = ((i, min(step, nsamples - i)) for i in range(0, nsamples, step // 2))
    return [(i, size) for i, size in sizes if not (i * sample_time < tmin or size < step // 2)]


class StepTimer:
    """Per-step timings of a chunk loop for a driver's ``profile`` list: ``start()`` opens a chunk,
    ``mark(name)`` synchronises the device and stamps a step's end, ``record`` appends the chunk's
    dict.  With ``profile=None`` every method does nothing and never synchronises."""

    def __init__(self, profile):
        self.profile, self._marks = profile, []

    def start(self):
        self._marks = []
        self.mark("start")

    def mark(self, name):
        if self.profile is not None:
            _hip.torch().cuda.synchronize()
            self._marks.append((name, time.perf_counter()))

    def record(self, istart, nsamples, **extra):
        if self.profile is not None:
            rec = {"istart": istart, "nsamples": nsamples, **extra}
            rec.update({name: (tt - self._marks[i][1]) * 1e3 for i, (name, tt) in enumerate(self._marks[1:])})
            self.profile.append(rec)


class ChunkStream:
    """Iterating yields ``(istart, size, block)`` per chunk of the ``FilReader`` ``fil``: ``block`` is
    ``fil.device_block`` of the uploaded chunk (1/2/4-bit files go up packed and are unpacked there),
    as float64 when the library has no code for its dtype (16-bit files), ordered on the consumer's
    current stream.  ``prefetch`` and more than one chunk: a loader thread copies chunk k + 1 from the
    memory map to the device (a pageable H2D on a copy stream: the runtime's own staging, no extra
    host copy) while the consumer works on chunk k; otherwise chunks go up on the current stream.
    Leaving the ``with`` (normal exit, ``break``, an exception) joins the loader thread and drops the
    block it had loaded ahead."""

    def __init__(self, fil, chunks, device, prefetch=True, timer=None):
        self._fil, self._chunks, self._dev, self._timer = fil, chunks, device, timer or StepTimer(None)
        self._pool = self._pending = self._copy_stream = None
        if prefetch and len(chunks) > 1:
            from concurrent.futures import ThreadPoolExecutor
            self._copy_stream = _hip.torch().cuda.Stream(device=device)
            self._pool = ThreadPoolExecutor(max_workers=1)
            self._pending = self._pool.submit(self._load, 0)

    def _load(self, k):
        with _hip.torch().cuda.device(self._dev):
            src = self._fil.upload_block(*self._chunks[k], device=self._dev, stream=self._copy_stream)
            return src, self._copy_stream.record_event()

    def _block(self, k):
        t = _hip.torch()
        self._timer.start()
        if self._pool is not None:
            src, ev = self._pending.result()
            self._pending = self._pool.submit(self._load, k + 1) if k + 1 < len(self._chunks) else None
            t.cuda.current_stream(self._dev).wait_event(ev)
            src.record_stream(t.cuda.current_stream(self._dev))
        else:
            src = self._fil.upload_block(*self._chunks[k], device=self._dev)
        self._timer.mark("h2d")
        block = self._fil.device_block(src)
        del src
        self._timer.mark("transpose")
        return block if _hip.dtype_code(block.dtype) is not None else block.to(t.float64)

    def __iter__(self):
        for k, (istart, size) in enumerate(self._chunks):
            yield istart, size, self._block(k)  # (no name bound here: the consumer owns the block)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
        self._pending = None
