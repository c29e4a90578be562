"""Every dedispersion kernel variant, bit for bit, on float input and on padded / offset views.

Inputs on which float32 accumulation is exact in ANY order: dyadic rationals k / 8 with
integer k in [-256, 255], stored as float32 and (the same values) as float64.  With
nchan <= 300 every partial sum times 8 is an integer of magnitude <= 8 * nchan * 32 < 2^24, so
the float32 plane of any correct kernel equals the float64 oracle's rows bit for bit, whatever
its summation order (channel order, subband groups, slots).  8-bit input is exact the same way
(integer sums <= nchan * 255).  The summation-order bound of tests/test_gpu_dedisperse.py
(nchan * 2^-24 * sum|x|) cannot see one wrong sample; these comparisons can.

Shapes: nchan = 38 leaves a partial last group for G = 2, 4 and 8; n = 300 is shorter than a
time tile (the kernels' small_n mode: rows wrap more than once, per-lane modular DMA), 4096 has
full tiles and gives 8-bit rows by LDS-DMA, 4099 has a partial last tile and gives 8-bit rows
from global memory.  Every case names the planner options and the kernel, group and tile length
they must give (found with _hip.describe_plan, which needs no GPU): a variant that fell back to
another kernel fails.  Kernels by plan.info["kernel"]: 0 dedisp_kernel (channel order, float32
rows: u8, f32 and f64 input with float32 accumulation, and u8 with float64 accumulation), 1
dedisp_f64_kernel (f32 and f64 input, float64 accumulation), 2 dedisp_sub_kernel with float32
slots (f32; f64 with PU_ACC_F32; u8 by LDS-DMA rows or from global memory), 3 dedisp_sub_kernel
with 16-bit slots (u8 by LDS-DMA rows, 256-sample tiles; n % 4 == 0, so never n = 4099).

Views: the data sits at columns [off, off + n) of a wider tensor filled with poison (NaN, or
255 for 8-bit), so a row pointer computed with n where the row stride belongs, or any read
outside [0, n) of a row, reaches the plane, the statistics or the exact series.
"""
import collections
import functools

import numpy as np
import pytest

import oracle
from pulsarutils import _hip

pytestmark = pytest.mark.gpu

NCHAN = 38
NS = (300, 4096, 4099)
NDM = 40
BAND = (1200.0, 300.0, 64e-6)  # start_freq, bandwidth, tsamp
DMS = np.linspace(0.0, 25.0, NDM)
NPDT = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}
CODE = {"u8": _hip.PU_U8, "f32": _hip.PU_F32, "f64": _hip.PU_F64}
ACC = {"native": _hip.PU_ACC_NATIVE, "f32": _hip.PU_ACC_F32, "f64": _hip.PU_ACC_F64}

# the exactness argument of the module docstring: |8 x| <= 256 = 8 * 32 per sample
assert NCHAN <= 300 and 8 * 300 * 32 < 2 ** 24

Case = collections.namedtuple("Case", "dt acc group shape u8_dma slot16 n kernel time_tile")


def _cases():
    out = []
    # dedisp_kernel (channel order, float32 rows): 512-sample tiles, 256 with float64 accumulators
    for dt, acc in (("u8", "native"), ("f32", "native"), ("f64", "f32"), ("u8", "f64")):
        for n in NS:
            out.append(Case(dt, acc, 1, None, None, None, n, 0, 256 if acc == "f64" else 512))
    # dedisp_f64_kernel
    for dt, acc in (("f32", "f64"), ("f64", "native")):
        for n in NS:
            out.append(Case(dt, acc, 0, None, None, None, n, 1, 256))
    # dedisp_sub_kernel, float32 slots: every (G, shape) with f32 and with u8 input, the lengths
    # rotating; u8 at n = 4099 reads global memory (no choice), at 300 / 4096 LDS-DMA rows and
    # u8_dma=False alternate; f64 input (PU_ACC_F32) once per shape and group size
    pairs = [(g, s) for g in (2, 4, 8) for s in ("wide", "pair", "tall")]
    for i, (g, s) in enumerate(pairs):
        tt = 512 if s == "wide" else 256
        out.append(Case("f32", "native", g, s, None, None, NS[i % 3], 2, tt))
        n8 = NS[(i // 3 + i + 1) % 3]
        out.append(Case("u8", "native", g, s, None if n8 == 4099 else bool((i // 3 + i) % 2), False, n8, 2, tt))
    for k, (g, s) in enumerate(((2, "wide"), (4, "pair"), (8, "tall"), (8, "wide"))):
        out.append(Case("f64", "f32", g, s, None, None, NS[k % 3], 2, 512 if s == "wide" else 256))
    # dedisp_sub_kernel, 16-bit slots: every (G, shape) at n = 4096, and one short series
    for g in (2, 4, 8):
        for s in ("pair", "tall"):
            out.append(Case("u8", "native", g, s, None, True, 4096, 3, 256))
    out.append(Case("u8", "native", 4, "tall", None, True, 300, 3, 256))
    return out


CASES = _cases()


def _id(c):
    dma = {None: "", True: "-dma", False: "-nodma"}[c.u8_dma]
    return f"k{c.kernel}-{c.dt}-acc_{c.acc}-g{c.group}-{c.shape or 'auto'}{dma}-n{c.n}"


def test_case_list_covers_what_it_claims():
    """The parametrisation itself: every kernel with every input type it takes and every length
    it can run at, every (G, shape) of the subband kernels with float32 and with 8-bit input,
    8-bit float32 slots from LDS-DMA rows and from global memory (by choice and by n % 4)."""
    seen = {(c.kernel, c.dt, c.acc) for c in CASES}
    assert seen == {(0, "u8", "native"), (0, "f32", "native"), (0, "f64", "f32"), (0, "u8", "f64"),
                    (1, "f32", "f64"), (1, "f64", "native"),
                    (2, "f32", "native"), (2, "f64", "f32"), (2, "u8", "native"), (3, "u8", "native")}
    for k in range(4):
        assert {c.n for c in CASES if c.kernel == k} == set(NS) - ({4099} if k == 3 else set()), k
    gs = {(g, s) for g in (2, 4, 8) for s in ("wide", "pair", "tall")}
    assert {(c.group, c.shape) for c in CASES if c.kernel == 2 and c.dt == "f32"} == gs
    assert {(c.group, c.shape) for c in CASES if c.kernel == 2 and c.dt == "u8"} == gs
    assert {(c.group, c.shape) for c in CASES if c.kernel == 3} == {p for p in gs if p[1] != "wide"}
    u8 = [c for c in CASES if c.kernel == 2 and c.dt == "u8"]
    assert any(_dma8(c) for c in u8) and any(c.u8_dma is False for c in u8) and any(c.n % 4 for c in u8)


def _dma8(c):
    """8-bit rows staged by LDS-DMA: subband plans of 8-bit input with n % 4 == 0 unless refused."""
    return c.kernel >= 2 and c.dt == "u8" and c.n % 4 == 0 and c.u8_dma is not False


@functools.lru_cache(maxsize=None)
def _tables(n):
    """The two shift tables of a length: the reference's delays of 40 trials (both signs about
    the band centre; spread within one DM tile), and the same plus per-channel constants that
    leave some shifts negative and some larger than n (the header: "any sign")."""
    phys = _hip.shift_table(NCHAN, DMS, *BAND)
    assert phys.min() < 0 < phys.max() and (phys.max(0) - phys.min(0)).max() < 254
    anysign = phys - phys.max() // 2 + np.where(np.arange(NCHAN) % 3 == 0, 2 * n + 5, 0)[None, :]
    assert anysign.min() < 0 and anysign.max() > n
    for t in (phys, anysign):
        t.setflags(write=False)
    return {"phys": phys, "anysign": anysign}


@functools.lru_cache(maxsize=None)
def _input(dt, n):
    """k / 8 for float (the same values in float32 and float64), bytes for 8-bit; read-only."""
    rng = np.random.default_rng(1000 + n)
    if dt == "u8":
        x = rng.integers(0, 256, (NCHAN, n)).astype(np.uint8)
    else:
        x = (rng.integers(-256, 256, (NCHAN, n)) / 8.0).astype(NPDT[dt])
        assert np.array_equal(x * 8, np.rint(x * 8)) and np.abs(x).max() <= 32
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(dt, n, table):
    """The oracle's float64 rows of every trial, computed once per (input, table); read-only."""
    x, sh = _input(dt, n), _tables(n)[table]
    rows = np.stack([oracle.dedisperse(x, sh[k]) for k in range(NDM)])
    rows.setflags(write=False)
    return rows


def _plan(c, sh):
    """The case's plan, pinned: the host-only planner and the device plan both report the
    kernel, group and tile length the case names."""
    opts = dict(group=c.group, shape=c.shape, u8_dma=c.u8_dma, slot16=c.slot16)
    described, _ = _hip.describe_plan(CODE[c.dt], ACC[c.acc], NCHAN, c.n, sh, **opts)
    plan = _hip.Plan(CODE[c.dt], ACC[c.acc], NCHAN, c.n, sh, **opts)
    for info in (described, plan.info):
        assert (info["kernel"], info["time_tile"]) == (c.kernel, c.time_tile), (c, info)
        assert info["group"] == (c.group or 1), (c, info)
        assert info["acc_is_f64"] == (c.acc == "f64" or (c.dt, c.acc) == ("f64", "native")), (c, info)
        # a staged row longer than the series: the kernels' small_n mode (multiple wraps)
        assert (info["row_stride"] + 2 > c.n) == (c.n == 300), (c, info)
    assert plan.ndm == NDM
    return plan


def _np(t):
    return t.cpu().numpy()


def _dev(x, gpu):
    """A device copy of a (read-only, shared) host array."""
    import torch
    return torch.from_numpy(x.copy()).to(gpu)


@pytest.mark.parametrize("table", ["phys", "anysign"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_plane_equals_oracle_bit_for_bit(gpu, case, table):
    """Every trial's row of plan.dedisperse on the contiguous tensor equals the oracle's, bit for
    bit: 8-bit, float32 and float64 input, float32 and float64 accumulation."""
    import torch
    # |8 x| <= 8 * 32 per sample (255 for bytes): every partial sum is an integer below 2^24 in
    # units of 1 / 8 (of 1), so float32 accumulation rounds nothing, in any order
    assert 8 * NCHAN * 32 < 2 ** 24 and NCHAN * 255 < 2 ** 24
    sh = _tables(case.n)[table]
    plan = _plan(case, sh)
    plane = _np(plan.dedisperse(_dev(_input(case.dt, case.n), gpu)))
    assert plane.dtype == (np.float64 if plan.acc_is_f64 else np.float32) and plane.shape == (NDM, case.n)
    np.testing.assert_array_equal(plane.astype(np.float64), _want(case.dt, case.n, table))


def _raw_dedisperse(plan, data):
    """pu_plan_dedisperse on the tensor as it is (no aligning copy by the wrapper)."""
    import torch
    pdt = torch.float64 if plan.acc_is_f64 else torch.float32
    plane = torch.full((plan.ndm, plan.nsamples), -7.0, dtype=pdt, device=data.device)
    _hip.check(_hip.lib().pu_plan_dedisperse(plan._h, _hip.ptr(data), data.stride(0), _hip.ptr(plane),
                                             plane.stride(0), _hip.stream_ptr()), "pu_plan_dedisperse")
    return plane


@pytest.mark.parametrize("off,pad,table", [(1, 6, "phys"), (3, 0, "anysign"), (4, 4, "anysign")],
                         ids=["odd_stride", "misaligned_base", "aligned_padded"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_padded_and_offset_views(gpu, case, off, pad, table):
    """The data as columns [off, off + n) of a poisoned wider tensor (row stride n + off + pad):
    plane (also into a padded plane), search, tile-range search + finalize, one DM tile and
    the exact series all equal the contiguous tensor's, which test_plane_equals_oracle_bit_for_bit
    compares with the oracle."""
    import torch
    n = case.n
    sh = _tables(n)[table]
    plan = _plan(case, sh)
    xd = _dev(_input(case.dt, n), gpu)
    plane = _np(plan.dedisperse(xd))
    full = [_np(o) for o in plan.search(xd)]
    assert np.isfinite(plane).all() and all(np.isfinite(o).all() for o in full)

    poison = 255 if case.dt == "u8" else float("nan")
    big = torch.full((NCHAN, off + n + pad), poison, dtype=xd.dtype, device=gpu)
    big[:, off:off + n] = xd
    view = big[:, off:off + n]
    assert view.stride(0) == n + off + pad and not view.is_contiguous()
    passed = plan._rows_aligned(view)
    if (off, pad) == (4, 4):  # rows on 4-byte boundaries: the kernels get the view itself
        assert passed is view and passed.stride(0) == n + 8
    elif case.dt != "u8" or n % 4:  # only 8-bit views of LDS-DMA-able lengths are copied
        assert passed is view
    else:
        assert passed is not view and passed.is_contiguous()
        # past the wrapper's copy: an LDS-DMA plan refuses rows off 4-byte boundaries before any
        # launch; a global-memory build (u8_dma=False) reads them at any alignment
        if _dma8(case):
            with pytest.raises(ValueError):
                _raw_dedisperse(plan, view)
        else:
            np.testing.assert_array_equal(_np(_raw_dedisperse(plan, view)), plane)

    np.testing.assert_array_equal(_np(plan.dedisperse(view)), plane)
    # a plane with ld_plane > n: the same rows, nothing written past column n
    sentinel = -12345.0
    wide = torch.full((NDM, n + 5), sentinel, dtype=torch.float64 if plan.acc_is_f64 else torch.float32, device=gpu)
    assert plan.dedisperse(view, plane=wide[:, :n]).stride(0) == n + 5
    np.testing.assert_array_equal(_np(wide[:, :n]), plane)
    np.testing.assert_array_equal(_np(wide[:, n:]), np.full((NDM, 5), sentinel))
    # the search, one shot and as two tile ranges + finalize
    for k, o in enumerate(plan.search(view)):
        np.testing.assert_array_equal(_np(o), full[k], err_msg=f"search output {k}")
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=gpu)
    ntt = plan.info["time_tiles"]
    assert ntt == -(-n // case.time_tile)
    plan.search_tiles(view, 0, ntt // 2, ws)
    plan.search_tiles(view, ntt // 2, ntt, ws)
    for k, o in enumerate(plan.finalize(ws, view)):
        np.testing.assert_array_equal(_np(o), full[k], err_msg=f"finalize output {k}")
    # one DM tile
    first, count = plan.dm_tiles()
    rows = _np(plan.dedisperse_dm_tile(view, 0))
    np.testing.assert_array_equal(rows, plane[int(first[0]):int(first[0] + count[0])])
    # the exact recompute (float64, channel order): the oracle's rows
    series = _np(plan.exact_series(view, np.arange(NDM, dtype=np.int32)))
    np.testing.assert_array_equal(series, _want(case.dt, n, table))
