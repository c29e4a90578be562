"""8-bit dedispersion up to its 65793-channel exactness limit (GPU).

The 8-bit paths rest on packed-integer arguments - a u16 half that never carries, float32
sums that stay below 2^24, 256-row column segments - whose bounds these inputs reach
(tests/test_u8_range_cpu.py asserts on the CPU that they do, under the stage partition the
planner gives each case).  Input: all-255 bytes with a few dozen seeded zeros and three rows
of random bytes, so that trials differ.  Reference: the oracle; plane rows bit for bit.

Tolerances: planes exact; search tables 1e-5 relative, rebin equal; trials
the certification recomputed equal the oracle bit for bit.
"""
import functools

import numpy as np
import pytest

import oracle
import u8_range_cases as R
from pulsarutils import _hip
from test_gpu_dedisperse import _slot16_pair, _tables_agree

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ a. flush periods

_FLUSH = [(g, ng, partial, table, budget)
          for g in R.GROUPS for ng, partial in R.flush_group_counts(g)
          for table, budget in (("physical", 0), ("physical", R.SMALL_BUDGET_KB), ("random", 0),
                                ("random", R.EVEN_BUDGET_KB[g]), ("random", R.SMALL_BUDGET_KB))]


@pytest.mark.parametrize("group,ngroups,partial,table,budget", _FLUSH)
def test_slot16_flush_periods(gpu, group, ngroups, partial, table, budget):
    """16-bit slots, tall shape, G = 2, 4, 8 with F16 - 1, F16, F16 + 1, 2 F16 and 2 F16 + 1
    groups (and 2 F16 + 1 with a partial last group) of full-scale input, n = 1000, 40
    trials of a physical and of an any-sign random shift table, at the default LDS budget,
    at the smallest one (one or two groups per stage: the flush counter runs across
    hundreds of stages) and, for the random table, at the budget whose stages hold an even
    number of groups - there a ``lo`` half reaches exactly 65535 before a flush from 2 F16
    groups on (test_flush_cases_reach_65535_in_a_lo_half).  Every plane row equals the
    oracle and the float32-slot plan; the tables equal the float32-slot plan's."""
    x, sh = R.flush_case(group, ngroups, partial, table)
    nchan = x.shape[0]
    assert nchan == ngroups * group - partial and (nchan % group != 0) == partial
    ref = np.stack([oracle.dedisperse(x, sh[k]) for k in range(sh.shape[0])])
    assert ref.max() == nchan * 255  # some sample of some trial sums full-scale bytes only
    p16, p32, r16, r32, i16, i32 = _slot16_pair(x, sh, group=group, shape="tall", lds_budget_kb=budget)
    assert (i16["kernel"], i16["group"], i16["time_tile"]) == (3, group, 256), i16
    assert (i32["kernel"], i32["group"], i32["time_tile"]) == (2, group, 256), i32
    np.testing.assert_array_equal(p16.astype(np.float64), ref)
    np.testing.assert_array_equal(p16, p32)
    _tables_agree(r16, r32)


# ------------------------------------------------------------------ b. top of the range

@functools.lru_cache(maxsize=2)
def _device_case(nchan, n):
    """top_case's input on the device (kept for the routes that follow: the parametrisation
    runs one (nchan, n) after the other)."""
    x, sh, ref = R.top_case(nchan, n)
    return _hip.to_device(np.array(x)), sh, ref


_TOP = [(R.NCHAN_MAX, 512), (R.NCHAN_MAX, 500), (R.NCHAN_MAX, 510), (65536, 512), (65792, 512)]


@pytest.mark.parametrize("route", list(R.ROUTES))
@pytest.mark.parametrize("nchan,n", _TOP)
def test_top_of_range_planes(gpu, nchan, n, route):
    """65793 channels - 65793 x 255 = 2^24 - 1, the last sum float32 holds exactly and the
    last whose count of 256s fits ``hi`` - on every 8-bit route: tall G = 2, 4, 8 with
    16-bit slots, tall G = 4 with float32 slots, wide G = 4, the automatic plan, the channel
    kernel, and the channel kernel with float64 accumulation; n = 512, 500 (a ragged last
    tile) and 510 (n % 4 != 0: rows read from global memory, float32 slots).  65536 and
    65792 channels: ``hi`` ends just below and at 65535.  The oracle's plane reaches
    nchan x 255 in every trial (asserted before the launch); every row equals it."""
    xd, sh, ref = _device_case(nchan, n)
    assert ref.max(axis=1).tolist() == [nchan * 255] * sh.shape[0]
    assert nchan != R.NCHAN_MAX or ref.max() == R.PLANE_MAX
    acc, opts = R.ROUTES[route]
    plan = _hip.Plan(_hip.PU_U8, acc, nchan, n, sh, **opts)
    info = plan.info
    assert (info["kernel"], info["group"], info["time_tile"], info["acc_is_f64"]) == R.route_plan(route, n), info
    plane = plan.dedisperse(xd).cpu().numpy()
    assert plane.dtype == (np.float64 if acc == R.ACC_F64 else np.float32)
    np.testing.assert_array_equal(plane.astype(np.float64), ref)


def test_f64_accumulation_has_no_channel_limit(gpu):
    """70000 channels: refused for float32 sums, exact with float64 accumulation
    (70000 x 255 > 2^24)."""
    xd, sh, ref = _device_case(70000, 512)
    assert ref.max() == 70000 * 255 > R.PLANE_MAX
    with pytest.raises(ValueError, match="65793"):
        _hip.Plan(_hip.PU_U8, _hip.PU_ACC_NATIVE, 70000, 512, sh)
    plan = _hip.Plan(_hip.PU_U8, _hip.PU_ACC_F64, 70000, 512, sh)
    assert plan.info["acc_is_f64"] == 1 and plan.info["group"] == 1
    np.testing.assert_array_equal(plan.dedisperse(xd).cpu().numpy(), ref)


def test_exact_series_at_the_channel_limit(gpu):
    """pu_plan_exact_series of every trial at 65793 channels: 257 whole 256-channel segments
    and a segment of one channel on an aligned tensor (exact_series_u8_seg_kernel, float64
    atomics), the channel-order kernel on a view whose row stride is no multiple of 4
    (n = 510, stride 511); the whole series and a sub-range.  Equal to the oracle's rows."""
    import torch
    trials = np.arange(8)
    xd, sh, ref = _device_case(R.NCHAN_MAX, 512)
    assert ref.max() == R.PLANE_MAX
    assert xd.data_ptr() % 4 == 0 and xd.stride(0) % 4 == 0  # the segment kernel's condition
    plan = _hip.Plan(_hip.PU_U8, _hip.PU_ACC_NATIVE, R.NCHAN_MAX, 512, sh)
    np.testing.assert_array_equal(plan.exact_series(xd, trials).cpu().numpy(), ref)
    np.testing.assert_array_equal(plan.exact_series(xd, trials[::-1], t_begin=37, t_end=451).cpu().numpy(),
                                  ref[::-1, 37:451])
    np.testing.assert_array_equal(plan.exact_series(xd, [5], t_begin=511, t_end=512).cpu().numpy(), ref[5:6, 511:])
    x, sh, ref = R.top_case(R.NCHAN_MAX, 510)
    big = torch.zeros((R.NCHAN_MAX, 511), dtype=torch.uint8, device=xd.device)
    view = big[:, :510].copy_(torch.from_numpy(np.array(x)))
    assert view.stride(0) == 511 and view.stride(0) % 4 != 0  # the channel-order kernel's
    plan = _hip.Plan(_hip.PU_U8, _hip.PU_ACC_NATIVE, R.NCHAN_MAX, 510, sh)
    np.testing.assert_array_equal(plan.exact_series(view, trials).cpu().numpy(), ref)
    np.testing.assert_array_equal(plan.exact_series(view, trials, t_begin=3, t_end=498).cpu().numpy(), ref[:, 3:498])


# ------------------------------------------------------------------ c. certification regimes

def _cert_search(x):
    """The default plan's search of ``x`` over the certification grid: (table as numpy,
    cert_info, flagged trials, plan.info)."""
    import torch
    nchan = x.shape[0]
    sh = np.stack([oracle.shifts(nchan, dm, *R.BAND) for dm in R.cert_dms()])
    xd = _hip.to_device(x)
    plan = _hip.Plan(_hip.PU_U8, _hip.PU_ACC_NATIVE, nchan, x.shape[1], sh)
    ws = torch.empty(max(plan.workspace_bytes, 16), dtype=torch.uint8, device=xd.device)
    res = [v.cpu().numpy() for v in plan.search(xd, workspace=ws)]
    cert = plan.cert_info()
    # which trials those were: the finalize step again on the records the search left
    _, flagged, _ = plan.finalize_range_flagged(ws, 0, sh.shape[0])
    assert cert["rechecked"] == flagged.size and not cert["nan_rule"]
    return res, cert, flagged, plan.info


def _check_table(res, ref, flagged):
    """Rechecked trials: the oracle's statistics bit for bit.  Every other trial: max, std
    and snr within 1e-5.  rebin: equal for every trial."""
    fast = np.setdiff1d(np.arange(ref[0].size), flagged)
    for a, b in zip(res[:3], ref[:3]):
        np.testing.assert_array_equal(a[flagged], b[flagged])
        np.testing.assert_allclose(a[fast], b[fast], rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(res[3], ref[3])


@pytest.mark.parametrize("nchan", R.CERT_NCHAN)
def test_cert_regimes_noise_with_pulse(gpu, nchan):
    """Uniform noise and one dispersed pulse 8 samples wide at both sides of the exact
    regime's end (8224 | 8225 channels: 8 x 255 x nchan against 2^24) and up to the channel
    limit, where the statistical float model certifies rebinned float32 sums above 2^24.
    No trial is left out: the oracle's best width beats its runner-up by more than 1e-4
    relative in every trial (asserted first), ten times the tolerance."""
    x = R.noise_pulse(nchan, seed=nchan % 97)
    ref = oracle.search(x, R.cert_dms(), *R.BAND, return_width_snr=True)
    assert ref[3][R.CERT_PULSE_TRIAL] == 8 and np.argmax(ref[2]) == R.CERT_PULSE_TRIAL
    assert R.width_margin(ref[4]).min() > 1e-4
    res, cert, flagged, info = _cert_search(x)
    print(f"cert pulse nchan {nchan}: kernel {info['kernel']} group {info['group']} rechecked "
          f"{cert['rechecked']} flagged_by {cert['flagged_by']}")
    _check_table(res, ref, flagged)


@pytest.mark.parametrize("nchan", R.CERT_NCHAN)
def test_cert_regimes_low_variance(gpu, nchan):
    """Bytes in {127, 128}: a mean of 127.5 nchan under a deviation of sqrt(nchan) / 2.  The
    exact regime (8224 channels) has no series error to weigh against that deviation and
    flags no trial for it; from 8225 channels on the float model's bound on the series
    error exceeds a quarter of the deviation and every trial is recomputed - through
    exact_series_u8_seg_kernel and pu_series_stats, bit for bit the oracle's."""
    x = R.low_variance(nchan, seed=nchan)
    ref = oracle.search(x, R.cert_dms(), *R.BAND)
    res, cert, flagged, info = _cert_search(x)
    print(f"cert low variance nchan {nchan}: kernel {info['kernel']} group {info['group']} rechecked "
          f"{cert['rechecked']} flagged_by {cert['flagged_by']}")
    if nchan == 8224:
        assert cert["flagged_by"]["std"] == 0, cert
    if nchan == 8225:
        assert cert["flagged_by"]["std"] == R.CERT_NDM and flagged.size == R.CERT_NDM, cert
    _check_table(res, ref, flagged)


# ------------------------------------------------------------------ d. column means

@pytest.mark.parametrize("ncols", [8, 64, 4104])
@pytest.mark.parametrize("nrows", [255, 256, 257, 512, 1023, 1024, 1025])
def test_col_means_u8_full_scale(gpu, nrows, ncols):
    """pu_col_means on full-scale 8-bit columns: a 256-row segment of 255s sums to 65280 in
    its u16 half, beside a partner half of zeros in each of a dword's four byte positions
    (columns 0/2 and 1/3 share a register), then 255 everywhere, then with one row skipped;
    1 to 4 whole segments, partial last ones, and 1025 rows (more than four segments: the
    row-sequential kernel).  Equal to the float64 mean bit for bit."""
    import torch
    lib = _hip.lib()
    out = torch.empty(ncols, dtype=torch.float64, device="cuda")

    def run(x, skip):
        xd = torch.from_numpy(x).cuda()
        sd = None if skip is None else torch.from_numpy(skip).cuda()
        out.fill_(-1.0)
        _hip.check(lib.pu_col_means(_hip.ptr(xd), _hip.PU_U8, nrows, ncols, ncols, None if sd is None else _hip.ptr(sd),
                                    _hip.ptr(out), _hip.stream_ptr()), "pu_col_means")
        good = np.ones(nrows, bool) if skip is None else skip == 0
        ref = x[good].astype(np.float64).sum(axis=0) / float(good.sum())
        np.testing.assert_array_equal(out.cpu().numpy(), ref)

    for pos in range(4):
        x = np.zeros((nrows, ncols), np.uint8)
        x[:, pos::4] = 255
        if nrows >= 256:
            assert x[:256].sum(axis=0, dtype=np.int64).max() == 65280
        run(x, None)
    x = np.full((nrows, ncols), 255, np.uint8)
    run(x, None)
    run(x, np.zeros(nrows, np.uint8))
    skip = np.zeros(nrows, np.uint8)
    skip[nrows // 2] = 1
    run(x, skip)
