"""The float32 slot build's passes at their width boundaries (GPU).

``sub_item`` builds a slot of ``len = TT + span + 1`` elements in passes of 64-element
chunks: a first pass of U or, for a slot that needs no more, U - 1 chunks, picked per slot
and stored without guards, then full-width passes that guard the stores past the slot's
``ceil(len / 64)`` chunks.  These tests put slot lengths on both sides of
every such boundary with hand-made shift tables: every channel of
a group has the same shift b_d (one slot per group, its span the sweep of b_d), plus a
second vector class (the group's second channel one sample later, on the odd trials) that
sweeps another span - so one stage holds slots of different widths, next to each other.

Tolerances (as tests/test_gpu_dedisperse.py): 8-bit input bit-equal to the
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

NTRIALS = 40
# (nchan, n): 18 channels leave a partial last group (it reads the zero row), 4099 samples a
# partial last time tile (and, for 8-bit input, rows read from global memory: n % 4 != 0)
SHAPES = [(16, 4096), (18, 4096), (16, 4099), (18, 4099)]
TALL_SPANS = [63, 64, 127, 128, 191, 192]  # TT = 256: 5, 6, 6, 7, 7, 8 chunks
# (shape, G, span): tall G = 4 / 2 build U = 6 chunks per pass, tall G = 8 U = 5, wide G = 4
# (TT = 512) U = 10
PLANS = ([("tall", g, s) for g in (4, 2) for s in TALL_SPANS] + [("tall", 8, s) for s in (63, 64)]
         + [("wide", 4, s) for s in (63, 64, 127, 128)])


def other_span(span):
    """The second vector class's span: another chunk count than ``span``'s."""
    return 20 if span >= 64 else 130


def shift_table(nchan, group, span):
    """(NTRIALS, nchan): even trials sweep b_d over 0..span with every channel at b_d; odd
    trials sweep 0..other_span(span) with the second channel of every group at b_d + 1."""
    sh = np.zeros((NTRIALS, nchan), np.int64)
    half = NTRIALS // 2
    for d in range(NTRIALS):
        sp = span if d % 2 == 0 else other_span(span)
        sh[d, :] = (sp * (d // 2) + (half - 1) // 2) // (half - 1)
        if d % 2:
            sh[d, 1::group] += 1
    assert sh[0::2].max() == span and sh[0::2].min() == 0 and sh[1::2, 0].max() == other_span(span)
    return sh


@functools.lru_cache(maxsize=None)
def inputs(nchan, n):
    """(u8, f32, f64) inputs of one shape, shared by every test (never written)."""
    rng = np.random.default_rng(1000 * nchan + n)
    u = rng.integers(0, 256, (nchan, n)).astype(np.uint8)
    f = (rng.random((nchan, n)) * 40).astype(np.float32)
    d = rng.random((nchan, n)) * 40
    return u, f, d


@functools.lru_cache(maxsize=None)
def reference(kind, nchan, n, group, span):
    """The oracle's plane (float64 roll-and-sum per trial) of one input ("u8", "f32", "f64";
    "abs..." of its absolute values) and shift table."""
    x = inputs(nchan, n)[("u8", "f32", "f64").index(kind[3:] if kind.startswith("abs") else kind)]
    if kind.startswith("abs"):
        x = np.abs(x)
    sh = shift_table(nchan, group, span)
    ref = np.stack([oracle.dedisperse(x, sh[k]) for k in range(NTRIALS)])
    ref.setflags(write=False)
    return ref


def f32_bound(kind, nchan, n, group, span):
    """Per-sample first-order bound nchan * 2^-24 * sum_c |x_c[(t + s_c) mod N]|."""
    return nchan * 2.0 ** -24 * reference("abs" + kind, nchan, n, group, span) + 1e-30


def make_plan(x, acc, nchan, n, shape, group, span, **opts):
    code = {np.dtype(np.uint8): _hip.PU_U8, np.dtype(np.float32): _hip.PU_F32, np.dtype(np.float64): _hip.PU_F64}
    plan = _hip.Plan(code[x.dtype], acc, nchan, n, shift_table(nchan, group, span), group=group, shape=shape, **opts)
    assert plan.info["group"] == group and plan.info["time_tile"] == (256 if shape == "tall" else 512), plan.info
    # subband kernel with float32 slots, one DM tile: each full group holds both classes' slots
    assert plan.info["kernel"] == 2 and plan.info["dm_tiles"] == 1, plan.info
    assert plan.info["slots"] >= 2 * (nchan // group), plan.info
    return plan


@pytest.mark.parametrize("shape,group,span", PLANS)
def test_planes_at_pass_boundaries(gpu, shape, group, span):
    """8-bit input with float32 slots (slot16=False): the plane bit-equal to the oracle;
    float32 input: within the native-accumulation bound.  Every input shape."""
    for nchan, n in SHAPES:
        u, f, _ = inputs(nchan, n)
        plane = make_plan(u, _hip.PU_ACC_NATIVE, nchan, n, shape, group, span, slot16=False).dedisperse(
            _hip.to_device(u)).cpu().numpy()
        np.testing.assert_array_equal(plane.astype(np.float64), reference("u8", nchan, n, group, span),
                                      err_msg=f"u8 {nchan}x{n}")
        plane = make_plan(f, _hip.PU_ACC_NATIVE, nchan, n, shape, group, span).dedisperse(
            _hip.to_device(f)).cpu().numpy()
        err = np.abs(plane - reference("f32", nchan, n, group, span))
        assert np.all(err <= f32_bound("f32", nchan, n, group, span)), (nchan, n, err.max())


def test_plane_f64_input_f32_accumulation(gpu):
    """float64 input summed in float32 (U = 5 at G = 4: 7 chunks = a pass of 5 and a guarded one storing 2)."""
    nchan, n, shape, group, span = 18, 4099, "tall", 4, 128
    d = inputs(nchan, n)[2]
    plane = make_plan(d, _hip.PU_ACC_F32, nchan, n, shape, group, span).dedisperse(_hip.to_device(d)).cpu().numpy()
    assert plane.dtype == np.float32
    err = np.abs(plane - reference("f64", nchan, n, group, span))
    assert np.all(err <= f32_bound("f64", nchan, n, group, span)), err.max()


def test_planes_small_lds_budget_reuses_stale_slots(gpu):
    """An 8 KiB LDS budget: a group or two per stage, so every stage builds its slots over
    the previous stage's (chunks a narrower pass no longer writes hold stale values).  8-bit
    rows: float rows of these spans do not fit 8 KiB in one DM tile."""
    nchan, n, shape = 16, 4096, "tall"
    u = inputs(nchan, n)[0]
    for group, span in ((2, 63), (2, 64), (4, 64)):
        plan = make_plan(u, _hip.PU_ACC_NATIVE, nchan, n, shape, group, span, slot16=False, lds_budget_kb=8)
        assert plan.info["stages"] >= 4, plan.info
        np.testing.assert_array_equal(plan.dedisperse(_hip.to_device(u)).cpu().numpy().astype(np.float64),
                                      reference("u8", nchan, n, group, span), err_msg=f"G {group} span {span}")


@pytest.mark.parametrize("nchan,n", SHAPES)
def test_search_table_at_pass_boundaries(gpu, nchan, n):
    """The fused search (max, std, snr, rebin) on slots of 7 and 5 chunks: against the
    oracle's statistics of its own series."""
    import torch
    shape, group, span = "tall", 4, 128
    u = inputs(nchan, n)[0]
    plan = make_plan(u, _hip.PU_ACC_NATIVE, nchan, n, shape, group, span, slot16=False)
    got = [v.cpu().numpy() for v in plan.search(_hip.to_device(u))]
    torch.cuda.synchronize()
    ref = reference("u8", nchan, n, group, span)
    want = [np.array(col) for col in zip(*(oracle.trial_stats(ref[k]) for k in range(NTRIALS)))]
    for a, b in zip(got[:3], want[:3]):
        np.testing.assert_allclose(a, b.astype(np.float64).ravel(), rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(got[3], want[3].ravel())
