"""The subband kernel's stage metadata across stage boundaries (GPU).

``sub_item`` carries a stage's first window record over from the previous stage's sum (the
record after a stage's last group, loaded into one of two ping-pong registers by the parity
of the stage's group count) and loads its first slot record and the stage record after next
a phase ahead ("Stage metadata off the critical path").  These tests choose
the stage structure - explicit ``group``, ``shape`` and ``lds_budget_kb``, with the stage
count the planner then reports asserted - so that the carry-over meets every case: tiles of
one stage (no carry, the clamp at the tile's last group), stages of 1, 2 and 3 groups (both
parities, and a stage that ends on the group loop's ``break``), stages of alternating odd and
even counts, two DM tiles with a partial second one (inactive waves, a wave with trials
missing, and in the last tile's last group the end of the record table), a partial last group
at G = 2 / 4 / 8, every workgroup shape, every input type, plane and search mode, and a
search over sub-ranges of the time tiles.  Every case also runs at the default LDS budget.

Shift tables are hand-made: trial d shifts every channel by b_d = 40 d / (ntrials - 1); to
give groups a second vector class (a second slot), ``uniform`` moves the second channel of
every group one sample later on odd trials (equal groups: g groups per stage throughout,
the last stage the remainder), ``mixed`` moves it d mod 3 samples later in every third group
only (unequal groups: stages of 1 and 2 groups alternate).

Tolerances (as tests/test_gpu_build_passes.py): 8-bit input bit-equal to the
oracle's float64 roll-and-sum (integer sums < 2^24); float32 accumulation of float input
within nchan * 2^-24 * sum_c |x_c| per sample; search statistics within 1e-5 relative, rebin
equal.
"""
import functools

import numpy as np
import pytest

import oracle
from pulsarutils import _hip

pytestmark = pytest.mark.gpu

N = 2404                                          # 9 time tiles of 256 + 100; 4 of 512 + 356
NTRIALS = {"tall": 300, "wide": 150, "pair": 150}  # two DM tiles: 256 + 44, 128 + 22
NCHAN = {2: 19, 4: 27, 8: 55}                     # 10 / 7 / 7 groups, the last one partial
SPAN = 40
CODE = {"u8": _hip.PU_U8, "f32": _hip.PU_F32, "f64": _hip.PU_F64}

# (table, shape, G, {lds_budget_kb: stages of the two DM tiles together}) per input kind,
# recorded from pu_plan_describe.  With 7 (G = 2: 10) equal groups per tile, 14 (20) stages
# are 1 group per stage; 8 (10) are 2 per stage - 2, 2, 2, 1: the last stage leaves the group
# loop by its break (G = 2: 2 x 5, every stage through the loop's end); 6 (8) are 3 per stage
# - 3, 3, 1 (3, 3, 3, 1); 2 are one stage per tile.  mixed: 10 stages of 7 groups (12 of 10)
# alternate 1 and 2 groups.
F32_CASES = [
    ("uniform", "tall", 4, {0: 2, 12: 14, 24: 8, 32: 6, 48: 4}),
    ("uniform", "tall", 2, {0: 2, 12: 20, 16: 18, 20: 10, 24: 8}),
    ("uniform", "tall", 8, {0: 2, 20: 14, 32: 8, 48: 6}),
    ("uniform", "wide", 4, {0: 2, 24: 14, 40: 8, 64: 6}),
    ("uniform", "wide", 2, {0: 2, 16: 20, 32: 10, 48: 8}),
    ("uniform", "wide", 8, {0: 4, 32: 14, 64: 8}),
    ("uniform", "pair", 4, {0: 2, 12: 14, 24: 8, 32: 6}),
    ("uniform", "pair", 8, {0: 4, 20: 14, 32: 8, 48: 6}),
    ("mixed", "tall", 4, {0: 2, 20: 10, 24: 8}),
    ("mixed", "tall", 2, {0: 2, 16: 12, 12: 18}),
]
# 8-bit rows staged by LDS-DMA (N % 4 == 0): 16-bit slots where the tile is 256 samples
# (slot16 None: kernel 3) and float32 slots (slot16 False: kernel 2)
U8_CASES = [
    ("uniform", "tall", 4, {0: 2, 8: 14, 16: 8, 24: 6}),
    ("uniform", "tall", 2, {0: 2, 8: 20, 10: 18, 16: 10, 20: 8}),
    ("uniform", "tall", 8, {0: 2, 10: 14, 20: 8, 28: 6}),
    ("uniform", "pair", 4, {0: 2, 8: 14, 16: 8, 24: 6}),
    ("uniform", "wide", 4, {0: 2, 16: 14, 28: 8, 40: 6}),
    ("mixed", "tall", 4, {0: 2, 12: 14, 16: 8, 20: 6}),
    ("mixed", "tall", 2, {0: 2, 12: 12, 16: 10}),
]
# float64 input summed in float32: rows read from global memory
F64_CASES = [
    ("uniform", "tall", 4, {0: 2, 8: 14, 10: 8, 16: 6}),
    ("uniform", "tall", 8, {0: 2, 8: 14, 10: 8, 16: 6}),
    ("uniform", "wide", 2, {0: 2, 10: 20, 20: 10, 28: 8}),
    ("mixed", "tall", 4, {0: 2, 8: 10, 10: 8}),
]


def _ids(cases):
    return [f"{t}-{s}-g{g}" for t, s, g, _ in cases]


@functools.lru_cache(maxsize=None)
def shift_table(table, shape, group):
    ntr, nchan = NTRIALS[shape], NCHAN[group]
    sh = np.zeros((ntr, nchan), np.int64)
    chan = np.arange(nchan)
    second = chan % group == 1
    third = (chan // group) % 3 == 0
    for d in range(ntr):
        sh[d, :] = (SPAN * d) // (ntr - 1)
        if table == "uniform":
            sh[d, second] += d % 2
        else:
            sh[d, second & third] += d % 3
    sh.setflags(write=False)
    return sh


@functools.lru_cache(maxsize=None)
def inputs(nchan):
    """(u8, f32, f64) inputs of one channel count, shared by every test (never written)."""
    rng = np.random.default_rng(77 + nchan)
    u = rng.integers(0, 256, (nchan, N)).astype(np.uint8)
    f = (rng.random((nchan, N)) * 40).astype(np.float32)
    d = rng.random((nchan, N)) * 40
    for a in (u, f, d):
        a.setflags(write=False)
    return {"u8": u, "f32": f, "f64": d}


@functools.lru_cache(maxsize=None)
def reference(kind, table, shape, group):
    """The oracle's plane (float64 roll-and-sum per trial) of one input and shift table."""
    x = inputs(NCHAN[group])[kind]
    sh = shift_table(table, shape, group)
    ref = np.stack([oracle.dedisperse(x, sh[k]) for k in range(sh.shape[0])])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference_stats(kind, table, shape, group):
    ref = reference(kind, table, shape, group)
    return [np.array(col) for col in zip(*(oracle.trial_stats(ref[k]) for k in range(ref.shape[0])))]


def f32_bound(kind, table, shape, group):
    """Per-sample first-order bound nchan * 2^-24 * sum_c |x_c[(t + s_c) mod N]| (the inputs
    are non-negative: the sum of absolute values is the reference itself)."""
    return NCHAN[group] * 2.0 ** -24 * reference(kind, table, shape, group) + 1e-30


def make_plan(kind, table, shape, group, kb, stages, slot16=None):
    acc = _hip.PU_ACC_F32 if kind == "f64" else _hip.PU_ACC_NATIVE
    plan = _hip.Plan(CODE[kind], acc, NCHAN[group], N, shift_table(table, shape, group), group=group, shape=shape,
                     lds_budget_kb=kb, slot16=slot16)
    s16 = kind == "u8" and slot16 is None and shape != "wide"
    want = {"group": group, "time_tile": 512 if shape == "wide" else 256, "dm_tiles": 2, "kernel": 3 if s16 else 2,
            "stages": stages}
    assert {k: plan.info[k] for k in want} == want, plan.info
    return plan


def check_plane(kind, table, shape, group, plane):
    ref = reference(kind, table, shape, group)
    if kind == "u8":
        np.testing.assert_array_equal(plane.astype(np.float64), ref)
    else:
        err = np.abs(plane - ref)
        assert np.all(err <= f32_bound(kind, table, shape, group)), err.max()


def check_stats(kind, table, shape, group, got):
    want = reference_stats(kind, table, shape, group)
    for a, b in zip(got[:3], want[:3]):
        np.testing.assert_allclose(a, b.astype(np.float64).ravel(), rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(got[3], want[3].ravel())


def run_both_modes(kind, table, shape, group, budgets, slot16=None):
    import torch
    x = _hip.to_device(inputs(NCHAN[group])[kind])
    for kb, stages in budgets.items():
        plan = make_plan(kind, table, shape, group, kb, stages, slot16)
        check_plane(kind, table, shape, group, plan.dedisperse(x).cpu().numpy())
        got = [v.cpu().numpy() for v in plan.search(x)]
        torch.cuda.synchronize()
        check_stats(kind, table, shape, group, got)


@pytest.mark.parametrize("table,shape,group,budgets", F32_CASES, ids=_ids(F32_CASES))
def test_f32_stage_structures(gpu, table, shape, group, budgets):
    """float32 rows (LDS-DMA): plane within the accumulation bound, search statistics."""
    run_both_modes("f32", table, shape, group, budgets)


@pytest.mark.parametrize("slot16", [None, False], ids=["slot16", "f32slots"])
@pytest.mark.parametrize("table,shape,group,budgets", U8_CASES, ids=_ids(U8_CASES))
def test_u8_stage_structures(gpu, table, shape, group, budgets, slot16):
    """8-bit rows by byte DMA, 16-bit and float32 slots: plane bit-equal to the oracle."""
    run_both_modes("u8", table, shape, group, budgets, slot16)


@pytest.mark.parametrize("table,shape,group,budgets", F64_CASES, ids=_ids(F64_CASES))
def test_f64_input_stage_structures(gpu, table, shape, group, budgets):
    """float64 input, float32 accumulation (rows read from global memory)."""
    run_both_modes("f64", table, shape, group, budgets)


@pytest.mark.parametrize("kind,kb,stages", [("f32", 24, 8), ("f32", 0, 2), ("u8", 16, 8)])
def test_search_tiles_sub_ranges(gpu, kind, kb, stages):
    """``search_tiles`` over sub-ranges of the 10 time tiles (launches whose first tile is not
    tile 0, the partial last tile in a range of its own), out of order, then ``finalize``."""
    import torch
    table, shape, group = "uniform", "tall", 4
    x = _hip.to_device(inputs(NCHAN[group])[kind])
    plan = make_plan(kind, table, shape, group, kb, stages)
    assert plan.info["time_tiles"] == 10, plan.info
    ws = torch.zeros(max(plan.workspace_bytes, 16), dtype=torch.uint8, device=x.device)
    for lo, hi in ((3, 7), (9, 10), (0, 3), (7, 9)):
        plan.search_tiles(x, lo, hi, ws)
    got = [v.cpu().numpy() for v in plan.finalize(ws, x)]
    torch.cuda.synchronize()
    check_stats(kind, table, shape, group, got)
