"""The 8-bit paths' exactness bounds, on the CPU.

Two halves.  A numpy restatement of the 16-bit slots' packed accumulation
(tests/u8_range_cases.py: it does not import the library) proves that the inputs of
tests/test_gpu_u8_range.py touch the bounds the kernel's "this half never carries" arguments
rest on: 65535 in a ``lo`` half, 65535 in ``hi``, 2^24 - 1 in a plane.  The host planner
(``_hip.describe_plan``, and the stage partition from tests/u8_range_stages.cpp) pins the
plans those inputs run on.
"""
import os
import subprocess

import numpy as np
import pytest

import u8_range_cases as R
from pulsarutils import _hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "radio-pulsar-utils_amd", "csrc")


# ------------------------------------------------------------------ the packed accumulation

def _residue_then_full(group, ngroups, n=8):
    """Slot values of ``ngroups`` groups of all-255 channels, but one byte of the first group
    is 254 in sample 0 and 0 in sample 1: the first flush leaves 255 in sample 0's half
    (F16 G 255 - 1 = 255 mod 256) and 1 in sample 1's."""
    gs = np.full((ngroups, n), group * 255, np.uint32)
    gs[0, 0] -= 1
    gs[0, 1] -= 255
    return gs


@pytest.mark.parametrize("group", R.GROUPS)
def test_flush_period_is_tight(group):
    """F16 = 128, 64, 32 for G = 2, 4, 8: F16 all-255 groups on top of a flushed residue of
    255 put exactly 65535 into a half - the most it can hold - and the sum is still exact;
    one more group between two flushes (the counter steps by two: a period of F16 + 2)
    carries into the neighbouring half and the sum is wrong."""
    f = R.f16(group)
    assert f == {2: 128, 4: 64, 8: 32}[group]
    assert f * group * 255 + 255 == R.U16 and 255 + (f + 1) * group * 255 > R.U16
    gs = _residue_then_full(group, 2 * f)
    truth = gs.sum(axis=0).astype(np.int64)
    out, lo_max, hi_max, _ = R.packed_accumulate(gs, group)
    assert lo_max == R.U16
    np.testing.assert_array_equal(out, truth)
    # the kernel's counter is even, so F16 + 1 flushes where F16 does: the same sums
    out1, lo1, _, _ = R.packed_accumulate(gs, group, period=f + 1)
    assert lo1 == R.U16
    np.testing.assert_array_equal(out1, truth)
    # F16 + 2: one more pair of groups before the flush
    gs2 = _residue_then_full(group, 2 * f + 4)
    out2, lo2, _, _ = R.packed_accumulate(gs2, group, period=f + 2)
    assert lo2 > R.U16
    assert not np.array_equal(out2, gs2.sum(axis=0).astype(np.int64))
    # sample 0's half wrapped and its carry landed in sample 1's: both are wrong
    assert out2[0] != gs2[:, 0].sum() and out2[1] != gs2[:, 1].sum()


@pytest.mark.parametrize("group", R.GROUPS)
def test_hi_mask_is_needed(group):
    """Without the 0x00ff00ff mask on ``hi +=`` the low byte of the upper half lands in the
    lower half's count of 256s: wrong as soon as a flush meets a residue."""
    f = R.f16(group)
    gs = _residue_then_full(group, 2 * f)
    out, _, _, _ = R.packed_accumulate(gs, group, mask_hi=False)
    assert not np.array_equal(out, gs.sum(axis=0).astype(np.int64))


@pytest.mark.parametrize("group", R.GROUPS)
def test_hi_ends_at_65535_for_65793_channels(group):
    """65793 all-255 channels in one stage: 257 flush periods cover 65792 channels, whose
    sum is 65535 x 256, and the last group holds the one channel left - ``hi`` ends at
    65535, ``lo`` at 255, the sum is 2^24 - 1.  One channel more would need ``hi`` = 65536
    (the planner refuses 65794: test_planner_refuses_above_the_limit)."""
    ng = -(-R.NCHAN_MAX // group)
    y = np.full((R.NCHAN_MAX, 4), 255, np.uint8)
    gs = R.group_sums(y, group)
    assert gs.shape[0] == ng == 257 * R.f16(group) + 1
    out, lo_max, hi_max, hi_end = R.packed_accumulate(gs, group)
    assert np.all(out == R.PLANE_MAX) and R.NCHAN_MAX * 255 == R.PLANE_MAX
    assert np.all(hi_end == R.U16) and hi_max == R.U16 and lo_max == R.U16 - 255
    assert (R.NCHAN_MAX + 1) * 255 >> 8 > R.U16


@pytest.mark.parametrize("group", R.GROUPS)
def test_any_stage_partition_stays_in_range(group):
    """An odd stage makes the counter run ahead (it counts the missing second group of the
    stage's last iteration), so flushes only come earlier: whatever the stage partition, no
    half passes 65535 and the sum is exact."""
    rng = np.random.default_rng(group)
    f = R.f16(group)
    ng = 5 * f + 3
    gs = np.full((ng, 64), group * 255, np.uint32)
    gs[rng.integers(0, ng, 200), rng.integers(0, 64, 200)] -= rng.integers(0, 256, 200).astype(np.uint32)
    truth = gs.sum(axis=0).astype(np.int64)
    for _ in range(20):
        cuts = np.sort(rng.choice(np.arange(1, ng), size=int(rng.integers(0, 40)), replace=False))
        stages = np.diff(np.concatenate([[0], cuts, [ng]])).tolist()
        out, lo_max, hi_max, _ = R.packed_accumulate(gs, group, stages=stages)
        assert lo_max <= R.U16 and hi_max <= R.U16, stages
        np.testing.assert_array_equal(out, truth)


# ------------------------------------------------------------------ the plans the GPU tests run

@pytest.fixture(scope="module")
def stage_tool(tmp_path_factory):
    """tests/u8_range_stages.cpp built against the planner's own sources."""
    exe = str(tmp_path_factory.mktemp("u8_range") / "u8_range_stages")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
           "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "u8_range_stages.cpp"),
           os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "planner.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stderr

    def stages(nchan, n, shifts, group, lds_budget_kb=0, shape=2, slot16=1):
        path = exe + ".shifts"
        np.ascontiguousarray(shifts, np.int64).tofile(path)
        run = subprocess.run([exe, str(nchan), str(n), str(shifts.shape[0]), str(group), str(shape),
                              str(lds_budget_kb), str(slot16), path], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        lines = run.stdout.splitlines()
        head = dict(zip(lines[0].split()[0::2], map(int, lines[0].split()[1::2])))
        return head, [[int(v) for v in ln.split()] for ln in lines[1:]]
    return stages


def _model_over_trials(x, sh, group, partitions, trials):
    """The packed accumulation of ``trials`` under every distinct stage partition of the
    plan (which DM tile a trial falls in is the plan's business: each trial is run under all
    of them) - (largest lo, largest hi)."""
    lo_top = hi_top = 0
    parts = sorted({tuple(p) for p in partitions})
    for k in trials:
        gs = R.group_sums(R.gather(x, sh[k]), group)
        truth = gs.sum(axis=0).astype(np.int64)
        for p in parts:
            out, lo_max, hi_max, _ = R.packed_accumulate(gs, group, stages=p)
            np.testing.assert_array_equal(out, truth)
            lo_top, hi_top = max(lo_top, lo_max), max(hi_top, hi_max)
    return lo_top, hi_top


@pytest.mark.parametrize("group", R.GROUPS)
def test_flush_cases_reach_65535_in_a_lo_half(group, stage_tool):
    """The flush-period inputs of the GPU test, under the stage partition the planner gives
    them.  With the random shift table every trial is its own DM tile and the stages of a
    tile are equal; at R.EVEN_BUDGET_KB their group count is even, the counter does not run
    ahead, and from 2 F16 groups on a half reaches exactly 65535 before a flush.  Below
    2 F16 groups no period is full.  No case and no partition passes 65535."""
    f = R.f16(group)
    for ngroups, partial in R.flush_group_counts(group):
        x, sh = R.flush_case(group, ngroups, partial, "random")
        head, parts = stage_tool(x.shape[0], x.shape[1], sh, group, R.EVEN_BUDGET_KB[group])
        assert head == {"group": group, "slot16": 1, "ngroups": ngroups, "tiles": sh.shape[0]}
        assert all(c % 2 == 0 for p in parts for c in p[:-1]), parts[0]
        lo_top, hi_top = _model_over_trials(x, sh, group, parts, range(0, sh.shape[0], 4))
        if ngroups >= 2 * f:
            assert lo_top == R.U16, (ngroups, partial, lo_top)
        else:
            assert lo_top < R.U16
        assert hi_top <= R.U16


@pytest.mark.parametrize("group", R.GROUPS)
@pytest.mark.parametrize("table,budget", [("physical", 0), ("random", 0), ("physical", R.SMALL_BUDGET_KB),
                                          ("random", R.SMALL_BUDGET_KB)])
def test_flush_cases_other_partitions_stay_in_range(group, table, budget, stage_tool):
    """The same inputs under the default and the smallest LDS budget (stages of any parity,
    down to one or two groups): every half stays within 16 bits and the sums are exact."""
    ngroups, partial = R.flush_group_counts(group)[-1]
    x, sh = R.flush_case(group, ngroups, partial, table)
    head, parts = stage_tool(x.shape[0], x.shape[1], sh, group, budget)
    assert head["slot16"] == 1 and head["ngroups"] == ngroups
    if budget:
        assert max(max(p) for p in parts) <= 2, "the smallest budget: one or two groups per stage"
    lo_top, hi_top = _model_over_trials(x, sh, group, parts, (0, sh.shape[0] - 1))
    assert lo_top <= R.U16 and hi_top <= R.U16


def test_top_case_reaches_every_bound(stage_tool):
    """65793 channels, n = 512, under the planner's own stage partition: the oracle's plane
    reaches 2^24 - 1 in every trial; with G = 8 (343 stages, all but the last even) a ``lo``
    half reaches 65535 and ``hi`` ends at 65535; G = 4 reaches 65535 in ``lo``; G = 2 (odd
    stages) comes within a flush period of both.  One trial is modelled: all are alike."""
    x, sh, ref = R.top_case(R.NCHAN_MAX, 512)
    assert ref.max(axis=1).tolist() == [R.PLANE_MAX] * sh.shape[0]
    got = {}
    for group in R.GROUPS:
        head, parts = stage_tool(R.NCHAN_MAX, 512, sh, group)
        assert head["slot16"] == 1 and head["tiles"] == 1
        gs = R.group_sums(R.gather(x, sh[3]), group)
        out, lo_max, hi_max, hi_end = R.packed_accumulate(gs, group, stages=parts[0])
        np.testing.assert_array_equal(out, ref[3].astype(np.int64))
        got[group] = (lo_max, int(hi_end.max()))
        assert lo_max <= R.U16 and hi_max <= R.U16
    assert got[8] == (R.U16, R.U16), got
    assert got[4][0] == R.U16 and got[4][1] >= R.U16 - 255, got
    assert got[2][0] >= R.U16 - 2 * 255 * 2 and got[2][1] >= R.U16 - 255, got


@pytest.mark.parametrize("nchan", [65536, 65792])
def test_below_the_limit_hi_is_just_below(nchan):
    """65536 and 65792 channels: the planes top out at nchan x 255, so ``hi`` ends at 65280
    and 65535 (65792 x 255 = 65535 x 256: the last value before the limit)."""
    x, sh, ref = R.top_case(nchan, 512)
    assert ref.max() == nchan * 255
    assert (nchan * 255) >> 8 == {65536: 65280, 65792: 65535}[nchan]


@pytest.mark.parametrize("n", [512, 1024])
@pytest.mark.parametrize("nchan", [8224, 8225, 16384, R.NCHAN_MAX])
def test_planner_pins(nchan, n):
    """Every route of the GPU range test plans the kernel, group and time tile that test
    expects, at both sides of the certification threshold and at the channel limit; each
    plan is made in well under a second."""
    import time
    _hip.lib()  # loaded before the clock runs
    sh = R.physical_shifts(nchan, 8, 3.0)
    for name, (acc, opts) in R.ROUTES.items():
        t0 = time.perf_counter()
        info, _ = _hip.describe_plan(_hip.PU_U8, acc, nchan, n, sh, **opts)
        dt = time.perf_counter() - t0
        want = R.route_plan(name, n)
        assert (info["kernel"], info["group"], info["time_tile"], info["acc_is_f64"]) == want, (name, info)
        assert info["dm_tiles"] == 1 and info["time_tiles"] == n // info["time_tile"]
        assert dt < 1.0, (name, dt)


@pytest.mark.parametrize("n", [500, 510])
def test_planner_pins_ragged(n):
    """n = 500 (a ragged last tile) keeps the LDS-DMA rows and the 16-bit slots; n = 510
    (n % 4 != 0) reads rows from global memory: float32 slots on every subband route."""
    sh = R.physical_shifts(R.NCHAN_MAX, 8, 3.0)
    for name, (acc, opts) in R.ROUTES.items():
        info, _ = _hip.describe_plan(_hip.PU_U8, acc, R.NCHAN_MAX, n, sh, **opts)
        assert (info["kernel"], info["group"], info["time_tile"], info["acc_is_f64"]) == R.route_plan(name, n), (name, info)


def test_planner_refuses_above_the_limit():
    """65794 x 255 = 2^24 + 254: refused for native and float32 accumulation on every route,
    planned for float64 accumulation (as is 70000)."""
    sh = R.physical_shifts(R.NCHAN_MAX + 1, 8, 3.0)
    for acc in (_hip.PU_ACC_NATIVE, _hip.PU_ACC_F32):
        for opts in ({}, dict(group=1), dict(group=4, shape="tall"), dict(group=8, shape="tall", slot16=False)):
            with pytest.raises(ValueError, match="65793"):
                _hip.describe_plan(_hip.PU_U8, acc, R.NCHAN_MAX + 1, 512, sh, **opts)
    for nchan in (R.NCHAN_MAX + 1, 70000):
        sh = R.physical_shifts(nchan, 8, 3.0)
        info, _ = _hip.describe_plan(_hip.PU_U8, _hip.PU_ACC_F64, nchan, 512, sh)
        assert info["acc_is_f64"] == 1 and info["group"] == 1, info


def test_certification_threshold_arithmetic():
    """cert_model's exact regime ends where an 8-sample rebin of full-scale sums can pass
    2^24: 8 x 255 x 8224 < 2^24 <= 8 x 255 x 8225."""
    assert 8 * 255 * 8224 < 1 << 24 <= 8 * 255 * 8225


def test_column_half_bound():
    """colsum_u8_seg_kernel's halves: a segment of 256 rows of 255 sums to 65280; 257 rows
    would fill a half to the last bit and 258 would carry."""
    assert 256 * 255 == 65280 and 257 * 255 == 65535 and 258 * 255 > 65535
