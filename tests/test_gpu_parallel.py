"""The multi-GPU product path on one GPU: the HIP compute of ``parallel.sharded_search``
under a world-size-1 RCCL (nccl) process group, and the pipelined broadcast + search
(time-tile range launches, pu_plan_search_tiles + pu_plan_finalize) against the one-shot
search.  The multi-rank split / broadcast / gather plumbing is covered on CPU by
tests/test_parallel_gloo.py (gloo, world 2-4)."""
import ctypes
import functools
import socket

import numpy as np
import pytest

import oracle
from pulsarutils import _hip, parallel, synth
from pulsarutils import dedispersion as D
from pulsarutils.configs import CONFIGS

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("name,chunks", [("C5", 5), ("C2s", 8), ("C3s", 3)])
def test_pipelined_tiles_equal_full_search(gpu, name, chunks):
    """Searching time-tile ranges as chunks land, then finalising, gives the one-shot
    pu_plan_search outputs bit for bit (same kernels, same per-tile records, same
    deterministic finalize order); wrapping tiles wait for the last chunk."""
    import torch
    from dataclasses import replace
    c = {"C5": CONFIGS["C5"], "C2s": replace(CONFIGS["C2"], nchan=256, nsamples=1 << 18),
         "C3s": replace(CONFIGS["C3"], nchan=512, nsamples=1 << 18)}[name]
    xd = synth.pulsar_filterbank_device(c)
    dms = D.dedispersion_plan(c.nchan, c.dmmin, c.dmmax, c.start_freq, c.bandwidth, c.tsamp)[:300]
    sh = _hip.shift_table(c.nchan, dms, c.start_freq, c.bandwidth, c.tsamp)
    plan = _hip.Plan(_hip.dtype_code(xd.dtype), _hip.PU_ACC_NATIVE, c.nchan, c.nsamples, sh)
    full = [o.cpu().numpy() for o in plan.search(xd)]
    piped = [o.cpu().numpy() for o in parallel.pipelined_broadcast_search(xd, plan, chunks=chunks)]
    torch.cuda.synchronize()
    for a, b in zip(full, piped):
        np.testing.assert_array_equal(a, b)
    # tile-range launches with an empty and a partial range, finalised
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=xd.device)
    ntt = plan.info["time_tiles"]
    plan.search_tiles(xd, 0, 0, ws)
    plan.search_tiles(xd, ntt // 3, ntt, ws)
    plan.search_tiles(xd, 0, ntt // 3, ws)
    for a, b in zip(full, plan.finalize(ws, xd)):
        np.testing.assert_array_equal(a, b.cpu().numpy())
    with pytest.raises(ValueError):
        plan.search_tiles(xd, 0, ntt + 1, ws)


@pytest.mark.parametrize("search", ["pipelined", "tile_sharded"])
def test_world1_phase_events(gpu, search):
    """World 1, no process group, real PhaseEvents (the path bench.py --full takes): both
    pipelined searches give plan.search's bits and record one search span per chunk walked
    (column_chunks for the pipelined search, a single chunk for the tile-sharded one with
    src=None), one finalize span, and no exchange span - so no step span either."""
    import torch
    c = CONFIGS["C5"]
    xd = synth.pulsar_filterbank_device(c)
    dms = D.dedispersion_plan(c.nchan, c.dmmin, c.dmmax, c.start_freq, c.bandwidth, c.tsamp)[:300]
    sh = _hip.shift_table(c.nchan, dms, c.start_freq, c.bandwidth, c.tsamp)
    plan = _hip.Plan(_hip.dtype_code(xd.dtype), _hip.PU_ACC_NATIVE, c.nchan, c.nsamples, sh)
    full = [o.cpu().numpy() for o in plan.search(xd)]
    ph = parallel.PhaseEvents()
    if search == "pipelined":
        res, (lo, hi) = parallel.pipelined_broadcast_search(xd, plan, chunks=5, phases=ph), (0, dms.size)
        nchunks = len(parallel.column_chunks(c.nsamples, 5))
    else:
        res, (lo, hi) = parallel.tile_sharded_search(xd, plan, src=None, chunks=5, phases=ph)
        nchunks = 1
    torch.cuda.synchronize()
    assert (lo, hi) == (0, dms.size)
    for a, b in zip(full, res):
        np.testing.assert_array_equal(a[lo:hi], b[lo:hi].cpu().numpy())
    t = ph.times_ms()
    assert len(t["search_ms"]) == nchunks and len(t["finalize_ms"]) == 1, t
    assert "exchange_ms" not in t and "step_span_ms" not in t, t


@pytest.mark.parametrize("pipelined", [False, True])
def test_sharded_search_nccl_world1(gpu, pipelined):
    """parallel.sharded_search with the HIP compute (the product path) under a real
    RCCL process group of size 1: equals the single-process search, and the sampled
    trials equal the oracle within SURVEY §8a's 1e-5."""
    import torch
    import torch.distributed as dist
    from dataclasses import replace
    c = replace(CONFIGS["C2"], nchan=256, nsamples=1 << 17)
    xd = synth.pulsar_filterbank_device(c)
    dms = D.dedispersion_plan(c.nchan, c.dmmin, c.dmmax, c.start_freq, c.bandwidth, c.tsamp)[:257]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                            device_id=xd.device)
    try:
        mx, sd, snr, win = parallel.sharded_search(xd, dms, c.nchan, c.start_freq, c.bandwidth, c.tsamp,
                                                   pipelined=pipelined)
    finally:
        dist.destroy_process_group()
    ref = D._dedispersion_search(xd, dms, c.nchan, c.start_freq, c.bandwidth, c.tsamp)
    for a, b in zip((mx, sd, snr, win), ref):
        np.testing.assert_array_equal(a, b)
    assert win.dtype == np.int32
    idx = np.unique(np.r_[np.linspace(0, dms.size - 1, 8).astype(int), np.argmax(snr)])
    o = oracle.search(xd.cpu().numpy(), dms[idx], c.start_freq, c.bandwidth, c.tsamp, nthreads=16)
    np.testing.assert_allclose(snr[idx], o[2], rtol=1e-5)
    np.testing.assert_array_equal(win[idx], o[3])
    torch.cuda.synchronize()


@pytest.mark.parametrize("offset", [0, 5000])
@pytest.mark.parametrize("dt", ["f32", "u8dma", "u8", "f64"])
def test_ready_tiles_read_only_landed_columns(gpu, dt, offset):
    """the halo that gates early tile launches (Plan.tile_window) is checked
    against the kernels' real reads.  Every chunk's not-yet-landed columns are
    overwritten with garbage (NaN / 255) before the tiles ``ready_tiles`` marks are
    searched; the finalised result must equal the one-shot search bit for bit, so no
    ready tile may read past the landed prefix.  Plans: float32 (LDS-DMA rows), 8-bit
    with LDS-DMA rows (N % 4 == 0) and with global-memory rows (N % 4 != 0), float64
    (channel mode); shift tables with a negative (offset 0: the reference's delays
    around the band centre) and a positive smallest shift (offset 5000)."""
    import torch
    c = CONFIGS["C2"]
    nchan = 96
    n = 40962 if dt == "u8" else 40960
    rng = np.random.default_rng(17)
    xh = rng.random((nchan, n)) * 40
    x = torch.from_numpy({"f32": xh.astype(np.float32), "u8dma": xh.astype(np.uint8), "u8": xh.astype(np.uint8),
                          "f64": xh}[dt]).cuda()
    dms = np.linspace(0.0, 80.0, 150)
    sh = _hip.shift_table(nchan, dms, c.start_freq, c.bandwidth, c.tsamp) + offset
    assert (sh.min() < 0) == (offset == 0)
    plan = _hip.Plan(_hip.dtype_code(x.dtype), _hip.PU_ACC_NATIVE, nchan, n, sh)
    full = [o.cpu().numpy() for o in plan.search(x)]
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=x.device)
    done = np.zeros(plan.info["time_tiles"], dtype=bool)
    launched = 0
    for c0, c1 in parallel.column_chunks(n, 6):
        xg = x.clone()
        if c1 < n:
            xg[:, c1:] = 255 if x.dtype == torch.uint8 else float("nan")
        ready = parallel.ready_tiles(plan, c1) & ~done
        idx = np.flatnonzero(ready)
        for run in np.split(idx, np.flatnonzero(np.diff(idx) != 1) + 1) if idx.size else []:
            plan.search_tiles(xg, int(run[0]), int(run[-1]) + 1, ws)
            launched += 1
        done |= ready
        torch.cuda.synchronize()
        del xg
    assert done.all() and launched > 1
    got = [o.cpu().numpy() for o in plan.finalize(ws, x)]
    for a, b in zip(full, got):
        np.testing.assert_array_equal(a, b)


def test_cached_plan_two_threads(gpu):
    """one cached plan searched from two threads at once (ctypes releases the
    GIL), each thread on its own stream; one input is constant, so every one of its trials
    is certified by the exact recheck (resolve_flagged: the pinned CertState read-back and
    the recheck scratch), the other is noise.  Every result equals the single-threaded
    one: the library's per-plan lock keeps the calls' certification state apart."""
    import threading

    import torch
    c = CONFIGS["C5"]
    rng = np.random.default_rng(9)
    n = 1 << 15
    noise = torch.from_numpy((rng.random((c.nchan, n)) * 50).astype(np.uint8)).cuda()
    const = torch.full((c.nchan, n), 7, dtype=torch.uint8, device=noise.device)
    dms = np.linspace(c.dmmin, c.dmmax, 120)
    args = (c.nchan, c.start_freq, c.bandwidth, c.tsamp)
    want = {}
    for name, x in (("noise", noise), ("const", const)):
        (o, plan) = D.search_device(x, dms, *args)
        want[name] = [t.cpu().numpy() for t in o]
        if name == "const":
            assert plan.cert_info()["rechecked"] == dms.size
    _, p1 = D.search_device(noise, dms, *args)
    _, p2 = D.search_device(const, dms, *args)
    assert p1 is p2  # one cached plan serves both inputs
    errors = []

    def worker(name, x):
        try:
            s = torch.cuda.Stream(device=x.device)
            with torch.cuda.stream(s):
                for _ in range(6):
                    o, _ = D.search_device(x, dms, *args)
                    got = [t.cpu().numpy() for t in o]
                    for a, b in zip(want[name], got):
                        np.testing.assert_array_equal(a, b)
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(f"{name}: {e!r}")

    th = [threading.Thread(target=worker, args=a) for a in (("noise", noise), ("const", const))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "thread hung"
    assert not errors, errors


@pytest.mark.parametrize("name,acc", [("C5", "native"), ("C3s", "native"), ("C5", "f64")])
def test_finalize_range_pieces_equal_full_search(gpu, name, acc):
    """Round 6 (time-tile sharding): the records of a tile-range search, finalized
    in trial ranges (pu_plan_finalize_range), equal the one-shot search bit for bit; the
    deferred form (pu_plan_finalize_range_flagged) writes the same fast statistics and
    returns the trials the one-shot search's certification recomputed, whose exact series
    (pu_plan_exact_series) + pu_series_stats give the one-shot outputs; the records view
    has the documented layout."""
    import torch
    from dataclasses import replace
    c = {"C5": CONFIGS["C5"], "C3s": replace(CONFIGS["C3"], nchan=512, nsamples=1 << 18)}[name]
    xd = synth.pulsar_filterbank_device(c)
    dms = D.dedispersion_plan(c.nchan, c.dmmin, c.dmmax, c.start_freq, c.bandwidth, c.tsamp)[:300]
    sh = _hip.shift_table(c.nchan, dms, c.start_freq, c.bandwidth, c.tsamp)
    code = {"native": _hip.PU_ACC_NATIVE, "f64": _hip.PU_ACC_F64}[acc]
    plan = _hip.Plan(_hip.dtype_code(xd.dtype), code, c.nchan, c.nsamples, sh)
    full = [o.cpu().numpy() for o in plan.search(xd)]
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=xd.device)
    ntt = plan.info["time_tiles"]
    plan.search_tiles(xd, 0, ntt // 3, ws)
    plan.search_tiles(xd, ntt // 3, ntt, ws)
    rec = plan.records(ws)
    assert rec.shape == (dms.size, ntt, plan.info["rec_stride"])
    assert rec.element_size() == plan.info["rec_elem_bytes"]
    outs = None
    for lo, hi in [(0, 7), (7, 7), (7, 151), (151, dms.size)]:
        outs = plan.finalize_range(ws, xd, lo, hi, out=outs)
    for k in range(4):
        np.testing.assert_array_equal(outs[k].cpu().numpy(), full[k], err_msg=f"output {k}")
    # deferred certification: same fast statistics, flagged trials settled by the caller
    plan.search_tiles(xd, 0, ntt, ws)
    outs2, flagged, nnf = plan.finalize_range_flagged(ws, 0, dms.size)
    assert nnf == 0 and np.all(np.diff(flagged) > 0)
    if flagged.size:
        ser = plan.exact_series(xd, flagged)
        # a sample range is the same samples of the whole series (time-split ranks)
        n3 = c.nsamples // 3 + 5
        assert torch.equal(plan.exact_series(xd, flagged, t_begin=n3, t_end=2 * n3), ser[:, n3:2 * n3])
        st = _hip.series_stats(ser)
        for k in range(4):
            outs2[k][torch.as_tensor(flagged.astype(np.int64), device=xd.device)] = st[k]
    for k in range(4):
        np.testing.assert_array_equal(outs2[k].cpu().numpy(), full[k], err_msg=f"deferred output {k}")


def test_finalize_range_flagged_zero_input_and_nonfinite_scan(gpu):
    """All-zero input: every trial's std is zero, so every trial of the range is flagged and
    its exact series is all zeros; pu_nonfinite_any sees a NaN in a column range only when
    the range holds it."""
    import torch
    from dataclasses import replace
    c = replace(CONFIGS["C3"], nchan=256, nsamples=1 << 16)
    xd = torch.zeros((c.nchan, c.nsamples), dtype=torch.uint8, device="cuda")
    dms = D.dedispersion_plan(c.nchan, c.dmmin, c.dmmax, c.start_freq, c.bandwidth, c.tsamp)[:40]
    sh = _hip.shift_table(c.nchan, dms, c.start_freq, c.bandwidth, c.tsamp)
    plan = _hip.Plan(_hip.dtype_code(xd.dtype), _hip.PU_ACC_NATIVE, c.nchan, c.nsamples, sh)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=xd.device)
    plan.search_tiles(xd, 0, plan.info["time_tiles"], ws)
    _, flagged, nnf = plan.finalize_range_flagged(ws, 10, 30)
    assert list(flagged) == list(range(10, 30)) and nnf == 0
    assert torch.count_nonzero(plan.exact_series(xd, flagged[:3])) == 0
    assert plan.exact_series(xd, flagged[:3], t_begin=100, t_end=100).shape == (3, 0)
    xf = torch.ones((16, 1000), dtype=torch.float32, device="cuda")
    xf[5, 700] = float("nan")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert int(_hip.nonfinite_any(xf[:, 600:800], flag)[0]) == 1
    assert int(_hip.nonfinite_any(xf[:, :700], flag)[0]) == 0
    assert int(_hip.nonfinite_any(xd[:, :100], flag)[0]) == 0


@pytest.mark.parametrize("dt", ["u8", "f32", "f64"])
def test_exact_series_ranges_equal_oracle_rows(gpu, dt):
    """pu_plan_exact_series (the certification recompute; loads of 8/4/2 channels issued ahead
    of their adds, round 6) equals the oracle's float64 channel-order rows bit for bit, over
    the whole series and over sample ranges that start and end anywhere (ragged n, windows
    wrapping modulo n).  For u8 this length covers the element-by-element path of the generic
    kernel only: n = 70001 gives ld % 4 != 0, so pu::exact_series skips
    exact_series_u8_seg_kernel and the generic kernel's dword path is off too (rows4 false);
    the 8-bit production kernels are test_exact_series_u8_* below."""
    import torch
    n, nchan = 70001, 37
    rng = np.random.default_rng(7)
    x = {"u8": rng.integers(0, 256, (nchan, n)).astype(np.uint8), "f32": rng.random((nchan, n)).astype(np.float32),
         "f64": rng.random((nchan, n))}[dt]
    xd = torch.from_numpy(x).cuda()
    dms = np.linspace(0.0, 400.0, 9)
    sh = _hip.shift_table(nchan, dms, 1200.0, 300.0, 64e-6)
    plan = _hip.Plan(_hip.dtype_code(xd.dtype), _hip.PU_ACC_F64, nchan, n, sh)
    want = np.stack([oracle.dedisperse(x, sh[d]) for d in range(dms.size)])
    tr = np.arange(dms.size, dtype=np.int32)
    np.testing.assert_array_equal(plan.exact_series(xd, tr).cpu().numpy(), want)
    for a, b in [(0, 1), (5, 4100), (n - 700, n), (12345, 12346 + 8 * 513)]:
        np.testing.assert_array_equal(plan.exact_series(xd, tr, t_begin=a, t_end=b).cpu().numpy(), want[:, a:b])


# ------------------------------------------------------------------ exact series: production kernels

SEG_NCHAN, SEG_N = 300, 70000   # two 256-channel segments; the second 44 = 5 x 8 + 4 channels
SEG_RANGES = [(0, 1), (5, 4100), (SEG_N - 700, SEG_N), (12345, 12346 + 8 * 513), (3, 3 + 8 * 64 + 5)]


def _series_input(dt, nchan, n):
    rng = np.random.default_rng(7)
    return {"u8": lambda: rng.integers(0, 256, (nchan, n)).astype(np.uint8),
            "f32": lambda: rng.random((nchan, n)).astype(np.float32), "f64": lambda: rng.random((nchan, n))}[dt]()


@functools.lru_cache(maxsize=None)
def _series_case(dt, nchan, n):
    """(input, shift table, the oracle's rows of every trial), computed once and read-only."""
    x = _series_input(dt, nchan, n)
    sh = _hip.shift_table(nchan, np.linspace(0.0, 400.0, 9), 1200.0, 300.0, 64e-6)
    want = np.stack([oracle.dedisperse(x, sh[d]) for d in range(sh.shape[0])])
    for a in (x, sh, want):
        a.setflags(write=False)
    return x, sh, want


def _raw_exact_series(plan, data, a, b):
    """pu_plan_exact_series of every trial on the tensor as it is (no aligning copy)."""
    import torch
    tr = np.arange(plan.ndm, dtype=np.int32)
    out = torch.full((tr.size, b - a), -1.0, dtype=torch.float64, device=data.device)
    _hip.check(_hip.lib().pu_plan_exact_series(plan._h, _hip.ptr(data), data.stride(0),
                                               tr.ctypes.data_as(ctypes.c_void_p), tr.size, a, b, _hip.ptr(out),
                                               _hip.stream_ptr()), "pu_plan_exact_series")
    return out.cpu().numpy()


@pytest.mark.parametrize("dt", ["u8", "f32", "f64"])
def test_exact_series_channel_segments_equal_oracle_rows(gpu, dt):
    """nchan = 300, n = 70000 (ld % 4 == 0): 8-bit input runs exact_series_u8_seg_kernel, what
    every aligned 8-bit tensor gets - two channel segments, the second partial (unrolled
    groups of 8 and a four-channel tail), integer sums added by float64 atomics, the
    three-dword funnel-shift reads; float input the generic kernel over more than one
    unrolled group.  Whole series and ranges that start and end anywhere, ranges shorter than
    a thread's 8 samples and ending inside a wave's 512 included: bit-equal to the oracle."""
    import torch
    x, sh, want = _series_case(dt, SEG_NCHAN, SEG_N)
    xd = torch.from_numpy(x.copy()).cuda()
    assert xd.stride(0) % 4 == 0 and xd.data_ptr() % 4 == 0
    plan = _hip.Plan(_hip.dtype_code(xd.dtype), _hip.PU_ACC_F64, SEG_NCHAN, SEG_N, sh)
    tr = np.arange(sh.shape[0], dtype=np.int32)
    np.testing.assert_array_equal(plan.exact_series(xd, tr).cpu().numpy(), want)
    for a, b in SEG_RANGES:
        np.testing.assert_array_equal(plan.exact_series(xd, tr, t_begin=a, t_end=b).cpu().numpy(), want[:, a:b],
                                      err_msg=f"samples [{a}, {b})")


@pytest.mark.parametrize("off,pad", [(0, 4), (4, 0), (0, 3), (3, 0)])
def test_exact_series_u8_padded_rows(gpu, off, pad):
    """The same 8-bit data as a view of a wider tensor filled with 255.  Row stride n + 4 with
    the rows on 4-byte boundaries: the segment kernel with ld != n.  Row stride n + 3 (through
    the C call, on a plan that does not stage rows by LDS-DMA: the wrapper would copy such a
    view): the generic kernel, element by element.  A row pointer computed with n for ld, or a
    read past a row's n samples, adds a wrong byte to an integer sum."""
    import torch
    x, sh, want = _series_case("u8", SEG_NCHAN, SEG_N)
    big = torch.full((SEG_NCHAN, off + SEG_N + pad), 255, dtype=torch.uint8, device=gpu)
    view = big[:, off:off + SEG_N]
    view.copy_(torch.from_numpy(x.copy()))
    plan = _hip.Plan(_hip.PU_U8, _hip.PU_ACC_F64, SEG_NCHAN, SEG_N, sh, u8_dma=False)
    aligned = (off + pad) % 4 == 0
    assert view.stride(0) == SEG_N + off + pad and (view.data_ptr() % 4 == 0 and view.stride(0) % 4 == 0) == aligned
    if aligned:  # the wrapper passes the view itself
        assert plan._rows_aligned(view) is view
        tr = np.arange(sh.shape[0], dtype=np.int32)
        np.testing.assert_array_equal(plan.exact_series(view, tr).cpu().numpy(), want)
    np.testing.assert_array_equal(_raw_exact_series(plan, view, 0, SEG_N), want)
    for a, b in SEG_RANGES:
        np.testing.assert_array_equal(_raw_exact_series(plan, view, a, b), want[:, a:b], err_msg=f"samples [{a}, {b})")


@pytest.mark.parametrize("dt", ["u8", "f32", "f64"])
def test_exact_series_shorter_than_a_wave(gpu, dt):
    """nchan = 9, n = 40: the series is shorter than the 512 samples a wave owns, so a thread's
    window wraps modulo n more than once (8-bit: the segment kernel, ld = 40; one unrolled
    group of 8 channels and a tail of one)."""
    import torch
    nchan, n = 9, 40
    x, sh, want = _series_case(dt, nchan, n)
    assert sh.max() >= n  # shifts beyond the series: reduced modulo n
    xd = torch.from_numpy(x.copy()).cuda()
    plan = _hip.Plan(_hip.dtype_code(xd.dtype), _hip.PU_ACC_F64, nchan, n, sh)
    tr = np.arange(sh.shape[0], dtype=np.int32)
    np.testing.assert_array_equal(plan.exact_series(xd, tr).cpu().numpy(), want)
    np.testing.assert_array_equal(plan.exact_series(xd, tr, t_begin=7, t_end=33).cpu().numpy(), want[:, 7:33])


# ------------------------------------------------------------------ pu_nonfinite_any

def _flag_of(x, preset):
    """pu_nonfinite_any's flag for x, the flag tensor holding ``preset`` before the call."""
    import torch
    flag = torch.full((1,), preset, dtype=torch.int32, device=x.device)
    return int(_hip.nonfinite_any(x, flag)[0])


@pytest.mark.parametrize("shape", [(1, 1), (3, 1000), (17, 70001)])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_nonfinite_any_every_corner(gpu, dt, shape):
    """NaN, +inf and -inf at the first and last element of the first and last row each set the
    flag; clean data and the finite extremes (largest, smallest subnormal, -0.0) clear a flag
    left at 1.  (17, 70001) is more than 4096 x 256 elements: the grid-stride loop runs twice."""
    import torch
    tdt = {"f32": torch.float32, "f64": torch.float64}[dt]
    rows, n = shape
    rng = np.random.default_rng(rows * n)
    x = torch.from_numpy(rng.standard_normal(shape)).to(tdt).to(gpu)
    assert _flag_of(x, 1) == 0
    for r, c in sorted({(0, 0), (0, n - 1), (rows - 1, 0), (rows - 1, n - 1)}):
        keep = x[r, c].item()
        for bad in (float("nan"), float("inf"), float("-inf")):
            x[r, c] = bad
            assert _flag_of(x, 0) == 1, (r, c, bad)
        fi = torch.finfo(tdt)
        for ok in (fi.max, -fi.max, fi.smallest_normal * fi.eps, -0.0):
            x[r, c] = ok
            assert x[r, c].item() == ok and _flag_of(x, 1) == 0, (r, c, ok)
        x[r, c] = keep
    assert _flag_of(x, 1) == 0


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_nonfinite_any_padding_uint8_and_empty(gpu, dt):
    """Only the nrows x ncols elements count: NaN in the padding of a view (ld = n + 3) is not
    seen, a NaN in the view's last column is.  A uint8 tensor and an empty one (no rows, or no
    columns: the column range of a rank with no time tiles, whose torch pointer is NULL) give 0,
    resetting a flag left at 1."""
    import torch
    tdt = {"f32": torch.float32, "f64": torch.float64}[dt]
    rows, n = 5, 1001
    big = torch.full((rows, n + 3), float("nan"), dtype=tdt, device=gpu)
    view = big[:, :n]
    view.fill_(1.5)
    assert view.stride(0) == n + 3 and torch.isnan(big[:, n:]).all()
    assert _flag_of(view, 1) == 0
    for r in (0, 2, rows - 1):
        big[r, n - 1] = float("nan")
        assert _flag_of(view, 0) == 1, r
        big[r, n - 1] = 1.5
    assert _flag_of(view, 1) == 0
    assert _flag_of(torch.full((7, 300), 255, dtype=torch.uint8, device=gpu), 1) == 0
    big[1, 2] = float("inf")
    assert _flag_of(view, 0) == 1
    for empty in (view[:0], view[:, 2:2]):
        assert empty.numel() == 0
        assert _flag_of(empty, 1) == 0
    # the C call itself with a real pointer and no rows
    flag = torch.ones(1, dtype=torch.int32, device=gpu)
    _hip.check(_hip.lib().pu_nonfinite_any(_hip.ptr(view), _hip.dtype_code(tdt), 0, n, n + 3, _hip.ptr(flag),
                                           _hip.stream_ptr()), "pu_nonfinite_any")
    assert int(flag[0]) == 0
