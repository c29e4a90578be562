"""pu_ffa and pulsarutils.ffa where tests/test_gpu_ffa.py does not reach: the scoring kernel at wide
and narrow profiles (its LDS on both sides of 64 KiB, 32 scan rounds, a ragged last round, p < 64
under a fused top level), the pass kernel's 256-row cap, designed ties at the maximum, the row
batching of the drivers, ffa_search's selection against a numpy restatement, non-finite samples and
the base-period convention against pu_fold_trials.

Every comparison is bit equality, or one float32 ulp on integer samples whose sums are exact (the
bound include/pulsarutils_hip.h gives for them).  Each numpy precondition a case rests on - exact
sums, a tie that really is one, the level split, the plan - is asserted before the device call."""
import math

import numpy as np
import pytest

import ffa_oracle as fo
from pulsarutils import _hip, ffa
from test_gpu_ffa import integer_case, run_ffa

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_split(rows, m, p, nw, block_rows, global_levels):
    """The case has the level split it was chosen for."""
    for want_out in (True, False):
        info = ffa.describe(rows, m, p, nw, want_out)
        assert info["block_rows"] == block_rows and info["global_levels"] == global_levels, info
        assert info["lds_bytes"] == 2 * block_rows * p * 4 + block_rows * 8 * 4
        assert info["lds_levels"] + info["global_levels"] == info["depth"] == (m - 1).bit_length()


def exact_case(gpu, x, want, m, p, widths, sigma=None):
    """Integer rows ``x`` with the oracle's transform ``want``: the transform bit for bit, the fused,
    unfused and no-peak calls equal bit for bit, every S/N within one float32 ulp of the exact one
    and every peak the oracle's.  Returns the fused (snr, peak)."""
    rows = x.shape[0]
    # integer samples, every prefix, window sum and total below 2^24: all sums exact in both formats
    assert np.array_equal(x, np.rint(x)) and float(np.abs(want.astype(np.float64)).sum(axis=2).max()) < 2.0 ** 24
    out, snr, peak = run_ffa(gpu, x, m, p, widths=widths, sigma=sigma)
    _, fsnr, fpeak = run_ffa(gpu, x, m, p, want_out=False, widths=widths, sigma=sigma)
    _, nsnr, npeak = run_ffa(gpu, x, m, p, want_out=False, widths=widths, sigma=sigma, want_peak=False)
    assert np.array_equal(bits(out), bits(want))
    assert np.array_equal(bits(snr), bits(fsnr)) and np.array_equal(peak, fpeak)
    assert npeak is None and np.array_equal(bits(nsnr), bits(fsnr))
    worst = 0.0
    for r in range(rows):
        for s in range(m):
            for k, w in enumerate(widths):
                exact, pk, _ = fo.snr_exact(want[r, s], w, m, 1.0 if sigma is None else sigma[r])
                ref = np.float32(exact)
                worst = max(worst, abs(float(fsnr[r, s, k]) - float(ref)) / float(np.spacing(np.abs(ref))))
                assert abs(np.float32(fsnr[r, s, k]) - ref) <= np.spacing(np.abs(ref)), (r, s, w)
                assert fpeak[r, s, k] == pk, (r, s, w)
    print("worst |snr - oracle| in float32 ulps:", worst)
    return fsnr, fpeak


# ------------------------------------------------------------------ 1. wide and narrow profiles

SCORE_WAVES = 4  # profiles in flight of a scoring workgroup, each with p + 1 float64 prefix sums


def test_score_lds_on_both_sides_of_64_kib():
    assert SCORE_WAVES * (2047 + 1) * 8 == 65536      # exactly the default limit: must not raise it
    assert SCORE_WAVES * (2048 + 1) * 8 == 65568 > 65536  # the one FFA launch that has to
    assert ffa.MAX_BINS == 2048
    for p in (2047, 2048):  # the LDS kernel's own workgroup is above 64 KiB at every p of this file
        assert ffa.describe(1, 9, p)["lds_bytes"] == 2 * 8 * p * 4 + 8 * 8 * 4 > 65536


# (rows, m, p, widths, block rows B, levels above the LDS ones)
PROFILE_CASES = [
    (1, 9, 2048, [1, 2, 1024, 2047], 8, 1),    # 32 full scan rounds, the score kernel's LDS above 64 KiB
    (1, 9, 2047, [1, 2, 1024, 2046], 8, 1),    # ... exactly 64 KiB, a last round of 63 bins
    (1, 33, 2048, [1, 7, 512, 2047], 8, 3),    # the fused kernel reads the plane two passes made
    (1, 20, 63, [1, 32, 62], 256, 0),          # one round, not full; two scoring chunks (16 profiles each)
    (1, 20, 64, [1, 32, 63], 256, 0),          # one full round
    (1, 20, 65, [1, 32, 64], 128, 0),          # a second round of one bin
    (3, 5, 2, [1], 256, 0),
    (2, 7, 3, [1, 2], 256, 0),
    (1, 300, 5, [1, 2, 4], 256, 1),            # p < 64 under a fused top level; the pass kernel's row cap
    (1, 257, 15, [1, 7, 14], 256, 1),          # the same, 4096 / 15 = 273 rows capped to 256
]


@pytest.mark.parametrize("rows, m, p, widths, block_rows, global_levels", PROFILE_CASES)
def test_snr_exact_at_wide_and_narrow_profiles(gpu, rows, m, p, widths, block_rows, global_levels):
    check_split(rows, m, p, len(widths), block_rows, global_levels)
    if m > 256:
        assert p < 16 and min(4096 // p, 256) == 256  # a workgroup of the pass kernel is capped, and there are two
    x, want = integer_case(rows, m, p)
    exact_case(gpu, x, want, m, p, widths)  # (the transform's bits among it)


def test_snr_exact_with_a_ragged_last_round_and_per_row_sigma(gpu):
    rows, m, p, widths = 2, 17, 1023, [1, 3, 511, 1022]
    check_split(rows, m, p, len(widths), 16, 1)
    assert p % 64 == 63 and (p + 63) // 64 == 16
    x, want = integer_case(rows, m, p)
    snr, peak = exact_case(gpu, x, want, m, p, widths, sigma=[2.0, 0.5])
    one, peak1 = exact_case(gpu, x, want, m, p, widths)
    # a power of two scales the float64 quotient exactly, so the rounded float32 too
    assert np.array_equal(bits(snr[0] * np.float32(2.0)), bits(one[0]))
    assert np.array_equal(bits(snr[1] * np.float32(0.5)), bits(one[1]))
    assert np.array_equal(peak, peak1)


# ------------------------------------------------------------------ 2. designed ties

TIE_P = 256
TIE_WIDTHS = [1, 3, 64, 255]
# bins of value 5.0 in the series' first row -> the peak of each width, worked out by hand:
#   {70, 133, 198}: 70 and 198 share lane 6 (the in-lane rule keeps the first), 133 is on lane 5 (the
#     cross-lane rule must prefer the lower bin of the higher lane).  w = 3: the windows from 68, 69,
#     70 hold bin 70.  w = 64: the window from 70 alone holds two of them.  w = 255: the window from 0
#     leaves out bin 255, a zero, as 252 others do.
#   {133, 134}: neighbouring lanes, the lower bin on the lower lane; w = 64 ties the 63 windows that
#     hold both.  {5, 69}: one lane; no window of 64 holds both, 128 hold one.
#   {63, 64}: the lower bin on the last lane, the higher on lane 0.
# The oracle confirms each below, and that all but ({70, 133, 198}, w = 64) are ties.
TIE_PATTERNS = [((70, 133, 198), [70, 68, 70, 0]),
                ((133, 134), [133, 132, 71, 0]),
                ((5, 69), [5, 3, 0, 0]),
                ((63, 64), [63, 62, 1, 0])]


@pytest.mark.parametrize("m", [65, 129])  # a fused top level over the LDS ones; one pass below it
def test_peak_is_the_lowest_bin_on_designed_ties(gpu, m):
    p = TIE_P
    check_split(len(TIE_PATTERNS), m, p, len(TIE_WIDTHS), 64, 1 if m == 65 else 2)
    x = np.zeros((len(TIE_PATTERNS), m * p), np.float32)
    for r, (hot, _) in enumerate(TIE_PATTERNS):
        x[r, list(hot)] = 5.0
    want = np.stack([fo.ffa(row.reshape(m, p)) for row in x])
    for r, (hot, peaks) in enumerate(TIE_PATTERNS):
        # only row 0 of the series is non-zero and the tree never rotates the head-most leaf:
        # every trial's profile is that row
        assert np.array_equal(bits(want[r]), bits(np.broadcast_to(x[r, :p], (m, p))))
        for w, pk in zip(TIE_WIDTHS, peaks):
            sums = fo.window_sums(x[r, :p], w)
            assert int(np.argmax(sums)) == pk and sums[pk] == sums.max()
            assert (np.count_nonzero(sums == sums.max()) >= 2) == ((r, w) != (0, 64))  # the tie is a tie
    snr, peak = exact_case(gpu, x, want, m, p, TIE_WIDTHS)
    for r, (_, peaks) in enumerate(TIE_PATTERNS):
        assert np.array_equal(peak[r], np.broadcast_to(np.asarray(peaks, np.int32), (m, len(peaks)))), r


@pytest.mark.parametrize("m", [65, 129])
def test_flat_series_score_plus_zero_at_bin_zero(gpu, m):
    p = TIE_P
    x = np.zeros((2, m * p), np.float32)
    x[1] = 3.0  # every profile is 3 m in every bin: w T / p = 3 m w exactly, the numerator +0.0
    want = np.stack([fo.ffa(row.reshape(m, p)) for row in x])
    assert np.all(want[0] == 0.0) and np.all(want[1] == 3.0 * m)
    for want_out in (True, False):
        _, snr, peak = run_ffa(gpu, x, m, p, want_out=want_out, widths=TIE_WIDTHS)
        assert not bits(snr).any()  # +0.0, not -0.0: x - x is +0.0 in round to nearest
        assert not peak.any()       # p equal sums: the lowest bin


# ------------------------------------------------------------------ 3. batched drivers

DRV_N, DRV_P, DRV_M = 2 ** 13, 100, 81
DRV_SIGMA = [1.0, 1.5, 2.0, 2.5, 3.0]
DRV_WIDTHS = [1, 3, 9, 25]
DRV_SEARCH = dict(sample_time=1.0, period_min=100.0, period_max=101.5, bins_min=100, bins_max=108, min_rows=80)
DRV_STEPS = [(100, 81), (101, 81), (102, 80)]  # (p, m) of the search's pu_ffa calls


def five_rows():
    """Noise in rows 0, 2, 4; pulse trains in rows 1 and 3."""
    return np.stack([fo.pulsar_series(DRV_N, 100.0, 0.03, 0.0, 31), fo.pulsar_series(DRV_N, 100.4, 0.03, 6.0, 32),
                     fo.pulsar_series(DRV_N, 100.0, 0.03, 0.0, 33), fo.pulsar_series(DRV_N, 101.7, 0.05, 5.0, 34),
                     fo.pulsar_series(DRV_N, 100.0, 0.03, 0.0, 35)])


def driver_results(x, gpu, calls):
    """Every driver once -> ({name: array or table}, {name: the rows of its pu_ffa calls})."""
    import torch
    res, batches = {}, {}

    def run(name, fn):
        del calls[:]
        out = fn()
        batches[name] = list(calls)
        return out

    res["transform"] = run("transform", lambda: ffa.ffa_transform(x, DRV_P))
    res["snr"], res["peak"] = run("snr", lambda: ffa.ffa_snr(x, DRV_P, widths=DRV_WIDTHS, sigma=DRV_SIGMA))
    s, k = run("snr_tensor", lambda: ffa.ffa_snr(torch.from_numpy(x).to(gpu), DRV_P, widths=DRV_WIDTHS, sigma=DRV_SIGMA))
    res["snr_tensor"], res["peak_tensor"] = s.cpu().numpy(), k.cpu().numpy()
    per = run("periodogram", lambda: ffa.ffa_periodogram(x, **DRV_SEARCH))
    for c, v in per.items():
        res["periodogram_" + c] = v
    for sift in (False, True):
        res["search", sift] = run(("search", sift), lambda: ffa.ffa_search(x, sigma=3.0, sift=sift, **DRV_SEARCH))
    return res, batches


@pytest.mark.parametrize("limit", ["_WS_BYTES", "_MAX_ROWS_M"])
def test_batch_drivers_label_rows(gpu, monkeypatch, limit):
    x = five_rows()
    assert ffa.ffa_plan(DRV_N, **DRV_SEARCH) == [(1, 100, 103)]
    assert [(p, DRV_N // p) for p in range(100, 103)] == DRV_STEPS and DRV_N // DRV_P == DRV_M
    lib = _hip.lib()
    real, calls = lib.pu_ffa, []

    def counted(xp, rows, *rest):
        calls.append(int(rows))
        return real(xp, rows, *rest)

    monkeypatch.setattr(lib, "pu_ffa", counted)
    want, one = driver_results(x, gpu, calls)
    assert one == {"transform": [5], "snr": [5], "snr_tensor": [5], "periodogram": [5] * 3, ("search", False): [5] * 3,
                   ("search", True): [5] * 3}
    # the unbatched answer has something to mislabel: candidates in the noise rows too, the two
    # pulse trains on top and in their rows
    ref = want["search", False]
    assert len(ref) > 5 and set(np.asarray(ref["row"]).tolist()) == set(range(5))
    assert sorted(np.asarray(ref["row"])[:2].tolist()) == [1, 3]
    assert want["search", True]["row"][0] in (1, 3) and want["search", True]["nabsorbed"][0] > 0
    assert not np.array_equal(want["peak"][0], want["peak"][4]) and not np.array_equal(want["peak"][1], want["peak"][3])
    if limit == "_WS_BYTES":
        # two rows' worth of the fused call's one plane, at the step that needs most
        per_row = [ffa.describe(2, m, p, 4, False)["workspace_bytes"] - ffa.describe(1, m, p, 4, False)["workspace_bytes"]
                   for p, m in DRV_STEPS]
        assert per_row == [m * p * 4 for p, m in DRV_STEPS] and max(per_row) == 81 * 101 * 4
        monkeypatch.setattr(ffa, "_WS_BYTES", 2 * max(per_row))
        for p, m in DRV_STEPS:
            for nw in (4, ffa.default_widths(p).size):
                assert ffa.describe(2, m, p, nw, False)["workspace_bytes"] <= 2 * max(per_row)
                assert ffa.describe(3, m, p, nw, False)["workspace_bytes"] > 2 * max(per_row)
        # m = 81 <= B = 128: the transform alone needs no workspace and has nothing to split
        assert ffa.describe(5, DRV_M, DRV_P, 0, True)["workspace_bytes"] == 0
        transform = [5]
    else:
        monkeypatch.setattr(ffa, "_MAX_ROWS_M", 2 * DRV_M)
        assert all((2 * DRV_M) // m == 2 for _, m in DRV_STEPS)
        transform = [2, 2, 1]
    got, split = driver_results(x, gpu, calls)
    assert split == {"transform": transform, "snr": [2, 2, 1], "snr_tensor": [2, 2, 1], "periodogram": [2, 2, 1] * 3,
                     ("search", False): [2, 2, 1] * 3, ("search", True): [2, 2, 1] * 3}
    for key, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[key].dtype == w.dtype and got[key].shape == w.shape, key
            assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), key
        else:
            assert got[key].colnames == w.colnames and len(got[key]) == len(w) > 0, key
            for c in w.colnames:
                assert np.array_equal(got[key][c], w[c]), (key, c)


# ------------------------------------------------------------------ 4. ffa_search's selection

SEL_N = 2 ** 14
SEL_ARGS = dict(sample_time=1.0, period_min=300.0, period_max=410.0, bins_min=100, bins_max=110)
SEL_PLAN = [(3, 100, 134), (4, 100, 125)]
SEL_COLS = ("period", "row", "snr", "width", "peak_phase", "dsfactor")


def search_by_numpy(gpu, plane, thr, sample_time, **plan_args):
    """ffa_search(sift=False) restated: ffa_snr per step on the rows normalised as ffa_periodogram
    normalises them (test_periodogram_is_ffa_snr_per_step pins that), the selection in numpy."""
    import torch
    from pulsarutils.dedispersion import quick_resample
    rows, n = plane.shape
    cols = {c: [] for c in SEL_COLS}
    for d, p0, p1 in ffa.ffa_plan(n, sample_time, **plan_args):
        y = torch.from_numpy(quick_resample(plane.copy(), d) if d > 1 else plane.astype(np.float64)).to(gpu)
        y = y - y.mean(dim=1, keepdim=True)
        sd = y.std(dim=1, unbiased=False)
        sd = torch.where(sd > 0, sd, torch.full_like(sd, math.inf))
        z = y.to(torch.float32)
        for p in range(p0, p1):
            w = ffa.default_widths(p)
            snr, peak = ffa.ffa_snr(z, p, sigma=sd)
            snr, peak = snr.cpu().numpy()[:, :-1], peak.cpu().numpy()[:, :-1]  # the last trial is the next step's first
            k = snr.argmax(axis=2)
            best = np.take_along_axis(snr, k[:, :, None], axis=2)[:, :, 0]
            pk = np.take_along_axis(peak, k[:, :, None], axis=2)[:, :, 0]
            edge = np.full((rows, 1), -np.inf, np.float32)
            left, right = np.concatenate((edge, best[:, :-1]), axis=1), np.concatenate((best[:, 1:], edge), axis=1)
            r, s = np.nonzero((best > np.float32(thr)) & (best > left) & (best >= right))  # row by row, trials ascending
            m = (n // d) // p
            cols["period"].append((p + s / (m - 1)) * (d * sample_time))
            cols["row"].append(r.astype(np.int64))
            cols["snr"].append(best[r, s].astype(np.float64))
            cols["width"].append(w[k[r, s]].astype(np.float64) * d * sample_time)
            cols["peak_phase"].append(((pk[r, s] + 0.5 * w[k[r, s]]) / p) % 1.0)
            cols["dsfactor"].append(np.full(r.size, d, np.int64))
    cols = {c: np.concatenate(v) for c, v in cols.items()}
    order = np.argsort(-cols["snr"], kind="stable")
    return {c: v[order] for c, v in cols.items()}


def check_table(tab, want):
    assert len(tab) == want["snr"].size
    for c in SEL_COLS:
        col = np.asarray(tab[c])
        assert col.dtype == want[c].dtype and np.array_equal(col, want[c]), c
    assert np.array_equal(np.asarray(tab["freq"]), 1.0 / want["period"])
    assert not np.asarray(tab["nabsorbed"]).any()


def test_search_selection_against_numpy(gpu):
    assert ffa.ffa_plan(SEL_N, **SEL_ARGS) == SEL_PLAN  # two downsampling factors
    plane = np.stack([fo.pulsar_series(SEL_N, 333.3, 0.03, 5.0, 41), fo.pulsar_series(SEL_N, 350.0, 0.03, 0.0, 42),
                      fo.pulsar_series(SEL_N, 405.7, 0.02, 6.0, 43)])
    want = search_by_numpy(gpu, plane, 3.0, **SEL_ARGS)
    # something of every kind to get wrong: many candidates, every row, both factors, several widths
    assert want["snr"].size > 5 and set(want["row"].tolist()) == {0, 1, 2} and set(want["dsfactor"].tolist()) == {3, 4}
    assert np.unique(want["width"]).size > 2 and np.unique(want["peak_phase"]).size > 5
    assert want["row"][0] in (0, 2)
    check_table(ffa.ffa_search(plane, sigma=3.0, sift=False, **SEL_ARGS), want)


def test_search_reports_a_plateau_once_and_no_constant_row(gpu):
    import torch
    plane = np.zeros((3, SEL_N), np.float32)
    plane[0, 7] = 40.0    # inside the first bin-row of every step: 7 // d < 100 <= p
    plane[1] = 3.0        # constant: mean 3.0 exactly, deviation 0, sigma = inf
    plane[2, 10:13] = 25.0
    # after the mean is taken off, every row of the (m, p) plane but the first is one constant, and a
    # rotation does not change a constant row: the profiles of a step's trials are all the same
    y = torch.from_numpy(plane[:, :SEL_N // 3 * 3].astype(np.float64)).to(gpu).reshape(3, -1, 3).sum(dim=2)
    z = (y - y.mean(dim=1, keepdim=True)).to(torch.float32)
    prof = ffa.ffa_transform(z, 101).cpu().numpy()
    assert prof.shape[1] == 54 and all(np.array_equal(bits(prof[:, s]), bits(prof[:, 0])) for s in range(54))
    assert not prof[1].any() and prof[0].any() and prof[2].any()
    tab = ffa.ffa_search(plane, sigma=3.0, sift=False, **SEL_ARGS)
    want = search_by_numpy(gpu, plane, 3.0, **SEL_ARGS)
    check_table(tab, want)
    # one candidate per step and row, the step's first trial (above its left edge, not below its
    # equal right neighbour); none in the constant row
    steps = [(d, p) for d, p0, p1 in SEL_PLAN for p in range(p0, p1)]
    for row in (0, 2):
        sel = np.asarray(tab["row"]) == row
        assert sorted(zip(np.asarray(tab["dsfactor"])[sel].tolist(), np.asarray(tab["period"])[sel].tolist())) == \
            sorted((d, float(p * d)) for d, p in steps)
        assert np.all(np.asarray(tab["snr"])[sel] > 3.0)
    assert len(tab) == 2 * len(steps) and not np.any(np.asarray(tab["row"]) == 1)
    per = ffa.ffa_periodogram(plane, **SEL_ARGS)
    assert not np.isnan(per["snr"]).any() and not np.isnan(per["width"]).any() and not np.isnan(per["period"]).any()
    assert not per["snr"][1].any() and np.all(per["snr"][0] > 3.0)


# ------------------------------------------------------------------ 5. non-finite samples

def test_a_non_finite_sample_stays_in_its_series(gpu):
    rows, m, p, widths = 3, 129, 256, [1, 4, 64]
    check_split(rows, m, p, len(widths), 64, 2)
    x, _ = integer_case(rows, m, p)
    bad = x.copy()
    at = 80 * p + 17  # series row 80: beyond the first LDS block of 64 rows
    assert at // p >= 64
    bad[1, at], bad[2, at + 5] = np.nan, np.inf
    for want_out in (True, False):
        out, snr, peak = run_ffa(gpu, x, m, p, want_out=want_out, widths=widths)
        bout, bsnr, bpeak = run_ffa(gpu, bad, m, p, want_out=want_out, widths=widths, nan_rows=(1, 2))
        if want_out:
            assert np.array_equal(bits(bout[0]), bits(out[0]))
            assert np.isnan(bout[1]).any() and np.isinf(bout[2]).any()  # the samples were read
        assert np.array_equal(bits(bsnr[0]), bits(snr[0])) and np.array_equal(bpeak[0], peak[0])
        # rows 1 and 2 are unspecified by the header; run_ffa has checked 0 <= peak < p for them too


# ------------------------------------------------------------------ 6. against the folding search

@pytest.mark.parametrize("p", [64, 256])
def test_first_trial_is_the_plain_fold_of_pu_fold_trials(gpu, p):
    import torch
    m = 40
    x, want = integer_case(1, m, p)
    out, _, _ = run_ffa(gpu, x, m, p)
    assert np.array_equal(bits(out), bits(want))
    # 1 / p is a power of two: t / p and its fraction are exact, so sample t falls in bin t mod p
    lib, n = _hip.lib(), m * p
    xd = torch.from_numpy(x.copy()).to(gpu)
    dph = torch.tensor([1.0 / p], dtype=torch.float64, device=gpu)
    sums = torch.zeros((1, 1, p), dtype=torch.float64, device=gpu)
    counts = torch.zeros((1, p), dtype=torch.int64, device=gpu)
    need = lib.pu_fold_trials_workspace_bytes(1, n, 1, p)
    buf, wp, wsb = _hip.workspace(need, gpu)
    _hip.check(lib.pu_fold_trials(_hip.ptr(xd), _hip.PU_F32, 1, n, n, 0, None, _hip.ptr(dph), 1, p, _hip.ptr(sums), p, p,
                                  _hip.ptr(counts), wp, wsb, _hip.stream_ptr()), "pu_fold_trials")
    torch.cuda.synchronize()
    assert np.all(counts.cpu().numpy() == m)
    fold = sums.cpu().numpy()[0, 0]
    assert np.array_equal(fold, x.reshape(m, p).astype(np.float64).sum(axis=0))  # both exact on integers
    assert np.array_equal(out[0, 0].astype(np.float64), fold)
