"""pu_fold at every channel-tile class of fold_tile (csrc/fold.hip) that tests/test_gpu_fold.py
does not reach, and in the upper half of the 13-bit bin field of the packed group table (bins
4096 .. 8191), against the same oracles and bounds as test_gpu_fold.py: ``fold_exact`` and equal
bits for 8-bit input, ``fold_fsum`` within 2 m 2^-53 sum|x| and equal bits on a second run for
float input.

The tile classes, from fold_tile and the constants of fold.hip: LDS = tc x pitch x acc_bytes +
FOLD_TABLE_BYTES, the tables 2048 x 4 + 32 x 4 = 8320 bytes, which leaves 12160 bytes of 20 KiB,
57216 of 64 KiB and 155520 of 160 KiB.

  float (pitch = nbin, 8 bytes):   20 KiB  tc 16: nbin <= 95    tc 8: <= 190    tc 4: <= 380
                                   64 KiB  tc 16: <= 447        tc 8: <= 894    tc 4: <= 1788
                                  160 KiB  tc 4:  <= 4860       tc 2: <= 8192 (FOLD_MAX_NBIN)
  8-bit (pitch = nbin + nbin // 32, 4 bytes):
                                   64 KiB  tc 16: nbin <= 867   tc 8: <= 1734   tc 4: <= 3468
                                  160 KiB  tc 4:  <= 8192

test_gpu_fold.py folds at nbin 1, 2, 17, 64 (float tc 16 @ 20 KiB, 8-bit tc 16), 256 (tc 4 @ 20
KiB, 8-bit tc 16), 1024 (tc 4 @ 64 KiB, 8-bit tc 8) and 4096 (tc 4 @ 160 KiB both)."""
import functools

import numpy as np
import pytest

import fold_oracle as fo
from test_gpu_fold import SEG, check_float, device_rows, fold_input, raw_fold

pytestmark = pytest.mark.gpu

TABLES = 2048 * 4 + 32 * 4
KIB = 1024
NBIN_MAX = 8192
PU_EUNSUPPORTED = -4  # include/pulsarutils_hip.h


def tile_of(nbin, kind):
    """(tc, LDS budget in KiB) by the rule stated in fold.hip, restated here from its text."""
    pitch, acc = (nbin + nbin // 32, 4) if kind == "u8" else (nbin, 8)
    budgets = [64, 64] if kind == "u8" else [20, 64]
    for kib in budgets:
        for tc in (16, 8, 4):
            if tc * pitch * acc + TABLES <= kib * KIB:
                return tc, kib
    for tc in (4, 2, 1):
        if tc * pitch * acc + TABLES <= 160 * KIB:
            return tc, 160
    raise AssertionError(nbin)


def test_tile_classes_as_derived():
    assert [tile_of(b, "f32") for b in (95, 96, 190, 191, 380, 381, 447, 448, 894, 895, 1788, 1789, 4860, 4861,
                                        8192)] == [
        (16, 20), (8, 20), (8, 20), (4, 20), (4, 20), (16, 64), (16, 64), (8, 64), (8, 64), (4, 64), (4, 64), (4, 160),
        (4, 160), (2, 160), (2, 160)]
    assert [tile_of(b, "u8") for b in (867, 868, 1734, 1735, 3468, 3469, 8192)] == [
        (16, 64), (8, 64), (8, 64), (4, 64), (4, 64), (4, 160), (4, 160)]
    # what test_gpu_fold.py reaches, and what it leaves
    old = {tile_of(b, k) + (k != "u8",) for b in (1, 2, 17, 64, 256, 1024, 4096) for k in ("u8", "f32")}
    new = {tile_of(c[2], k) + (k != "u8",) for c, kinds, _ in TILE_CASES for k in kinds}
    assert old == {(16, 20, True), (4, 20, True), (4, 64, True), (4, 160, True), (16, 64, False), (8, 64, False),
                   (4, 160, False)}
    assert new - old == {(8, 20, True), (16, 64, True), (8, 64, True), (2, 160, True), (4, 64, False)}


# 1 / 1000.3: 4.1 turns over 4099 samples whose phases interleave 0.1 to 0.3 samples apart, so
# every bin up to nbin 2048 is hit
TURNS = 1.0 / 1000.3
# ((nchan, n, nbin, dphase, phase0, first_sample), kinds, (tc, KiB) per kind): nchan no multiple of tc
TILE_CASES = [
    ((19, 4099, 120, TURNS, -0.37, 0), ("f32", "f64"), (8, 20)),
    ((19, 4099, 190, TURNS, -0.37, 0), ("f32",), (8, 20)),             # the last nbin of the class
    ((19, 4099, 400, TURNS, -0.37, 2 ** 40), ("f32", "f64"), (16, 64)),
    ((19, 4099, 700, TURNS, -0.37, 0), ("f32", "f64"), (8, 64)),
    ((5, 4099, 4860, TURNS, -0.37, 0), ("f32",), (4, 160)),            # tc 4 with exactly 160 KiB of LDS
    ((5, 4099, 4861, TURNS, -0.37, 0), ("f32", "f64"), (2, 160)),      # the first nbin of tc 2
    ((9, 4099, 2048, TURNS, -0.37, 0), ("u8",), (4, 64)),
]
# nbin 8192 (float tc 2, 8-bit tc 4, both @ 160 KiB), three phase laws
HALF = (4095.5 / NBIN_MAX)  # with dphase 0.5 the phase alternates between bins 4095 and 8191
HIGH_CASES = [
    (5, 4099, NBIN_MAX, 1.0 / 4099.5, -0.37, 0),         # one turn: a bin is used once or not at all
    (5, 4099, NBIN_MAX, 2.2 / NBIN_MAX, -0.37, 2 ** 40),  # 2.2 bins per sample, a wrap inside the chunk
    (5, 4099, NBIN_MAX, 0.5, HALF, 0),                   # 32 ranked runs per group in each of two bins
]


def case_id(c):
    return "c%d-n%d-b%d-%.3g-%s" % (c[0], c[1], c[2], c[3] * c[2], "far" if c[5] else "0")


@functools.lru_cache(maxsize=None)
def fold_want(case, kind):
    nchan, n, nbin, dphase, phase0, first = case
    x = fold_input(nchan, n, kind)
    if kind == "u8":
        return fo.fold_exact(x, dphase, nbin, phase0, first) + (None,)
    return fo.fold_fsum(x, dphase, nbin, phase0, first)


def check_fold(gpu, case, kind):
    nchan, n, nbin, dphase, phase0, first = case
    x = device_rows(gpu, fold_input(nchan, n, kind))
    want, wcounts, wabs = fold_want(case, kind)
    assert wcounts.sum() == n
    got, counts, _ = raw_fold(x, dphase, nbin, phase0, first)
    assert np.array_equal(counts, wcounts)
    if kind == "u8":
        assert np.array_equal(got, want)
    else:
        check_float(got, want, wcounts, wabs)
        again, _, _ = raw_fold(x, dphase, nbin, phase0, first)
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    return wcounts


@pytest.mark.parametrize("case, kind, tile", [(c, k, t) for c, kinds, t in TILE_CASES for k in kinds],
                         ids=lambda v: v if isinstance(v, str) else case_id(v) if len(v) == 6 else "tc%d-%dK" % v)
def test_fold_at_every_tile_class(gpu, case, kind, tile):
    nchan, nbin = case[0], case[2]
    assert tile_of(nbin, kind) == tile and nchan % tile[0] != 0 and nchan > tile[0]  # a partial last tile
    wcounts = check_fold(gpu, case, kind)
    if nbin <= 2048:
        assert wcounts.min() > 0  # every bin is hit


@pytest.mark.parametrize("kind", ["u8", "f32", "f64"])
@pytest.mark.parametrize("case", HIGH_CASES, ids=case_id)
def test_fold_in_the_upper_half_of_the_bin_field(gpu, case, kind):
    nchan, n, nbin, dphase, phase0, first = case
    assert tile_of(nbin, kind) == ((4, 160) if kind == "u8" else (2, 160)) and nchan % 4 and nchan % 2
    wcounts = fold_want(case, kind)[1]
    hit = np.flatnonzero(wcounts)
    if dphase == 0.5:
        assert hit.tolist() == [4095, 8191] and wcounts[4095] == 2050 and wcounts[8191] == 2049
    else:
        # a turn at the most: a bin is used once or not at all; 1.1 turns: the overlap may use one twice
        assert wcounts.max() == (1 if dphase * n < 1 else 2)
        assert 0.4 * n < wcounts[4096:].sum() < 0.6 * n  # half the hits in bins >= 4096
        assert hit.min() < 64 and hit.max() > nbin - 64
        b = fo.bins(n, dphase, nbin, phase0, first)
        assert (np.diff(b) < 0).sum() == 1  # one wrap inside the chunk
    check_fold(gpu, case, kind)


def test_fold_two_segments_of_high_bins(gpu):
    """n = 16384 + 77 at nbin 8192: the combine kernel adds two partials of bins >= 4096."""
    case = (3, SEG + 77, NBIN_MAX, 1.0 / 4099.5, 0.13, 2 ** 40)
    nchan, n, nbin, dphase, phase0, first = case
    b = fo.bins(n, dphase, nbin, phase0, first)
    both = np.intersect1d(b[:SEG], b[SEG:])
    assert both.size == 77 and both.min() >= 7680  # every bin of the second segment, bits 9 to 12 set
    check_fold(gpu, case, "f32")


@pytest.mark.parametrize("kind", ["u8", "f32", "f64"])
def test_fold_rejects_more_bins_than_the_field_holds(gpu, kind):
    import torch
    from pulsarutils import _hip
    lib = _hip.lib()
    nchan, n, nbin = 3, 100, NBIN_MAX + 1
    x = device_rows(gpu, fold_input(nchan, n, kind))
    sums = torch.full((nchan, nbin + 3), -7.0, dtype=torch.float64, device=gpu)
    counts = torch.full((nbin,), -7, dtype=torch.int64, device=gpu)
    ws = torch.empty(max(16, lib.pu_fold_workspace_bytes(nchan, n, nbin)), dtype=torch.uint8, device=gpu)
    rc = lib.pu_fold(_hip.ptr(x), _hip.dtype_code(x.dtype), nchan, n, x.stride(0), 0, -0.37, 0.013, nbin,
                     _hip.ptr(sums), sums.stride(0), _hip.ptr(counts), _hip.ptr(ws), ws.numel(), _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == PU_EUNSUPPORTED and lib.pu_last_error().decode().startswith("pu_fold:")
    assert (sums == -7.0).all().item() and (counts == -7).all().item()
