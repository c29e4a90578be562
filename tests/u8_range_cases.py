"""Inputs and a numpy restatement of the packed 8-bit accumulation for the range tests
(tests/test_u8_range_cpu.py proves on the CPU that these inputs touch every bound,
tests/test_gpu_u8_range.py runs them on the device).

Nothing here imports the library: the shift tables come from the oracle, the model of the
16-bit slots' accumulators is written out again from the kernel's description
(csrc/dedisperse.hip: ``lo16`` / ``hi16``, ``flush16``, the ``gc16 + 2 > F16`` rule).
"""
import functools

import numpy as np

import oracle

U16 = 65535
NCHAN_MAX = 65793            # 65793 x 255 = 2^24 - 1: the last channel count whose sums are exact in float32
PLANE_MAX = (1 << 24) - 1
GROUPS = (2, 4, 8)

# the band the physical shift tables use (C3-like: 1200 MHz, 300 MHz wide, 64 us samples)
BAND = (1200.0, 300.0, 64e-6)


# LDS budgets of the flush-period cases: at EVEN_BUDGET_KB the random table's stages hold an
# even number of groups (18, 14 and 14 for G = 2, 4, 8), so the flush counter, which counts
# two groups per iteration, does not run ahead at a stage's end and a period is F16 groups
# long; SMALL_BUDGET_KB is the smallest the planner takes (one or two groups per stage)
EVEN_BUDGET_KB = {2: 64, 4: 64, 8: 96}
SMALL_BUDGET_KB = 8

# pu_plan accumulation codes (include/pulsarutils_hip.h)
ACC_NATIVE, ACC_F32, ACC_F64 = 0, 1, 2

# the routes of the top-of-the-range test: name -> (accumulation, Plan / describe_plan options)
ROUTES = {
    "tall2": (ACC_NATIVE, dict(group=2, shape="tall")),
    "tall4": (ACC_NATIVE, dict(group=4, shape="tall")),
    "tall8": (ACC_NATIVE, dict(group=8, shape="tall")),
    "tall4_f32slots": (ACC_NATIVE, dict(group=4, shape="tall", slot16=False)),
    "wide4": (ACC_NATIVE, dict(group=4, shape="wide")),
    "auto": (ACC_NATIVE, dict()),
    "chan": (ACC_NATIVE, dict(group=1)),
    "chan_f64": (ACC_F64, dict(group=1)),
}


def route_plan(name, n):
    """(kernel, group, time_tile, acc_is_f64) a route plans at 8224 .. 65793 channels and 8
    trials: 16-bit slots (kernel 3) need LDS-DMA rows, that is n % 4 == 0; the automatic
    plan is the wide shape, G = 8 with DMA rows and G = 4 without."""
    dma = n % 4 == 0
    return {
        "tall2": (3 if dma else 2, 2, 256, 0),
        "tall4": (3 if dma else 2, 4, 256, 0),
        "tall8": (3 if dma else 2, 8, 256, 0),
        "tall4_f32slots": (2, 4, 256, 0),
        "wide4": (2, 4, 512, 0),
        "auto": (2, 8 if dma else 4, 512, 0),
        "chan": (0, 1, 512, 0),
        "chan_f64": (0, 1, 256, 1),
    }[name]


def f16(group):
    """Groups between two flushes: F16 G 255 + 255 <= 65535 (128, 64, 32 for G = 2, 4, 8)."""
    return (U16 - 255) // (group * 255)


# ---------------------------------------------------------------- inputs

def full_scale(nchan, n, seed, nrand=3, nzero=40):
    """All-255 bytes with ``nzero`` seeded zeros; the first ``nrand`` rows hold random bytes
    in their first half and 255 in their second, so that trials differ, every residue of a
    half mod 256 occurs, and some sample of every trial still sums nchan x 255."""
    rng = np.random.default_rng(seed)
    x = np.full((nchan, n), 255, np.uint8)
    k = min(nrand, nchan)
    x[:k, :n // 2] = rng.integers(0, 256, (k, n // 2), dtype=np.uint8)
    if nchan > k:
        x[rng.integers(k, nchan, nzero), rng.integers(0, n, nzero)] = 0
    return x


def physical_shifts(nchan, ndm, dm_max):
    """The reference's shift table of ``ndm`` trials from DM 0 to ``dm_max`` on BAND."""
    return np.stack([oracle.shifts(nchan, dm, *BAND) for dm in np.linspace(0.0, dm_max, ndm)])


def random_shifts(nchan, ndm, seed, span=20000):
    """Any-sign shifts far beyond the series length (every window wraps), sorted per channel
    over the trials as a trial grid is."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.integers(-span, span, (ndm, nchan)), axis=0)


def flush_case(group, ngroups, partial, table, n=1000, ndm=40):
    """(x, shifts) of one flush-period case: ``ngroups`` groups of ``group`` channels, the
    last one a channel short if ``partial``."""
    nchan = ngroups * group - (1 if partial else 0)
    x = full_scale(nchan, n, seed=1000 * group + ngroups + (500 if partial else 0))
    sh = physical_shifts(nchan, ndm, 30.0) if table == "physical" else random_shifts(nchan, ndm, 77 + group)
    return x, sh


def flush_group_counts(group):
    """(ngroups, partial last group) around the flush period: F16 - 1, F16, F16 + 1, 2 F16,
    2 F16 + 1 (three of them odd counts), and 2 F16 + 1 with nchan % G != 0."""
    f = f16(group)
    return [(f - 1, False), (f, False), (f + 1, False), (2 * f, False), (2 * f + 1, False), (2 * f + 1, True)]


@functools.lru_cache(maxsize=None)
def top_case(nchan, n):
    """(x, shifts, oracle plane rows as float64 (8, n)) of a top-of-the-range case: 8 trials
    with small physical shifts.  Computed once and shared (read-only)."""
    x = full_scale(nchan, n, seed=nchan + n)
    sh = physical_shifts(nchan, 8, 3.0)
    ref = np.stack([oracle.dedisperse(x, sh[k]) for k in range(sh.shape[0])])
    for a in (x, sh, ref):
        a.setflags(write=False)
    return x, sh, ref


# ---------------------------------------------------------------- the packed accumulation

def gather(x, shifts_k):
    """y[c, t] = x[c, (t + s_c) mod n]: the bytes one trial sums."""
    n = x.shape[1]
    idx = (np.arange(n)[None, :] + np.asarray(shifts_k)[:, None]) % n
    return np.take_along_axis(x, idx, axis=1)


def group_sums(y, group):
    """Slot values of one trial: per group of ``group`` channels (a partial last group reads
    zeros) the byte sums, uint32 (ngroups, n)."""
    nchan, n = y.shape
    ng = -(-nchan // group)
    pad = np.zeros((ng * group, n), np.uint32)
    pad[:nchan] = y
    return pad.reshape(ng, group, n).sum(axis=1, dtype=np.uint32)


def packed_accumulate(gs, group, stages=None, period=None, mask_hi=True):
    """The 16-bit slots' sum of one trial, as the kernel does it.

    ``gs``: (ngroups, n) slot values, n even.  Samples 2 i and 2 i + 1 share a 32-bit word
    as u16 halves (``lo``), added as plain 32-bit words; ``hi`` counts 256s.  The groups of
    a stage are taken two per iteration, and before an iteration ``gc + 2 > F16`` flushes
    (``hi += (lo >> 8) & 0x00ff00ff; lo &= 0x00ff00ff``) and clears ``gc``; ``gc`` grows by
    2 per iteration, also when an odd stage ends on the iteration's first group.  The result
    is ``hi x 256 + lo`` per half.  ``stages``: group counts of the stages (default: one).

    Returns (sums int64 (n,), largest ``lo`` half seen, largest ``hi`` half seen, ``hi``
    halves at the end (n,)): the maxima are taken on the exact integers, so a value above
    65535 means that the 32-bit word carried into its neighbour (``sums`` is then what the
    words give, carry and all).

    ``period`` and ``mask_hi`` restate faults (a longer flush period, the mask dropped from
    ``hi +=``)."""
    ng, n = gs.shape
    f = f16(group) if period is None else period
    stages = [ng] if stages is None else list(stages)
    assert sum(stages) == ng and n % 2 == 0
    word = (gs[:, 0::2].astype(np.uint64) | (gs[:, 1::2].astype(np.uint64) << np.uint64(16))).astype(np.uint32)
    lo = np.zeros(n // 2, np.uint32)
    hi = np.zeros(n // 2, np.uint32)
    # the same sums on exact integers per half: what a half would hold if it could not carry
    lo_true = np.zeros((2, n // 2), np.int64)
    hi_true = np.zeros((2, n // 2), np.int64)
    lo_max = hi_max = 0
    m = np.uint32(0x00ff00ff)

    def flush():
        nonlocal lo, hi, lo_true, hi_true, hi_max
        hi = hi + (((lo >> np.uint32(8)) & m) if mask_hi else (lo >> np.uint32(8)))
        lo = lo & m
        hi_true += lo_true >> 8
        lo_true &= 255
        hi_max = max(hi_max, int(hi_true.max()))

    def add(g):
        nonlocal lo, lo_true, lo_max
        lo = lo + word[g]  # uint32: wraps like v_add_u32
        lo_true[0] += gs[g, 0::2]
        lo_true[1] += gs[g, 1::2]
        lo_max = max(lo_max, int(lo_true.max()))

    gc = 0
    g0 = 0
    for count in stages:
        gl = g0 + count - 1
        for g in range(g0, g0 + count, 2):
            if gc + 2 > f:
                flush()
                gc = 0
            gc += 2
            add(g)
            if g + 1 > gl:
                break
            add(g + 1)
        g0 += count
    out = np.empty(n, np.int64)
    out[0::2] = (hi & np.uint32(0xffff)).astype(np.int64) * 256 + (lo & np.uint32(0xffff))
    out[1::2] = (hi >> np.uint32(16)).astype(np.int64) * 256 + (lo >> np.uint32(16))
    hi_end = np.empty(n, np.int64)
    hi_end[0::2] = hi & np.uint32(0xffff)
    hi_end[1::2] = hi >> np.uint32(16)
    return out, lo_max, max(hi_max, int(hi_end.max())), hi_end


# ---------------------------------------------------------------- certification inputs

CERT_NCHAN = (8224, 8225, 16384, 32768, 65793)
CERT_N = 2048
CERT_NDM = 12
CERT_DM_MAX = 6.0
CERT_PULSE_TRIAL = 7


def cert_dms():
    return np.linspace(0.0, CERT_DM_MAX, CERT_NDM)


def noise_pulse(nchan, seed):
    """Uniform random bytes in [0, 240] plus one pulse 8 samples wide, dispersed at trial
    CERT_PULSE_TRIAL's DM.  Its height per channel falls with sqrt(nchan) (6 counts at 8224
    channels, 2 at 65793), which keeps the dedispersed pulse near 8 sigma per sample: a much
    stronger one carries the variance of every rebinned series by itself, and the widths 4
    and 8 then tie."""
    rng = np.random.default_rng(seed)
    amp = max(1, int(round(6.0 * np.sqrt(8224.0 / nchan))))
    x = rng.integers(0, 241, (nchan, CERT_N), dtype=np.uint8)
    sh = oracle.shifts(nchan, cert_dms()[CERT_PULSE_TRIAL], *BAND)
    t0 = 1000  # a multiple of 8: the pulse fills one width-8 bin
    for j in range(8):
        cols = (t0 + j + sh) % CERT_N
        x[np.arange(nchan), cols] += amp
    return x


def low_variance(nchan, seed):
    """Large mean, small variance: bytes in {127, 128}."""
    rng = np.random.default_rng(seed)
    return rng.integers(127, 129, (nchan, CERT_N), dtype=np.uint8)


def width_margin(width_snr):
    """Relative margin of the reference's strict-first-best width over its runner-up, per
    trial, from the oracle's per-width S/N (ndm, 4)."""
    s = np.sort(np.asarray(width_snr), axis=1)
    return (s[:, -1] - s[:, -2]) / s[:, -1]
