"""The host planner on its own (no GPU): ``_hip.describe_plan`` plans exactly as ``_hip.Plan``
does and returns the plan's info fields and a digest of the tables it would upload.  Both are
pinned per case in ``tests/golden/plan_tables.json``, recorded from the commit before the
planner was separated from the device state - so a planner change that moves one byte of
one table, or picks another plan, shows here before any GPU time is spent.

A pull request that changes the planner on purpose re-records the file:
``python tests/test_plan_tables.py`` (then reviews the diff of the JSON).
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN_DIR

from pulsarutils import _hip, _planner
from pulsarutils.configs import CONFIGS

GOLDEN = os.path.join(GOLDEN_DIR, "plan_tables.json")
DTYPES = {"u8": _hip.PU_U8, "f32": _hip.PU_F32, "f64": _hip.PU_F64}
ACCS = {"native": _hip.PU_ACC_NATIVE, "f32": _hip.PU_ACC_F32, "f64": _hip.PU_ACC_F64}


def config_shifts(name, ntrials=None):
    c = CONFIGS[name]
    dms = _planner.dedispersion_plan(c.nchan, c.dmmin, c.dmmax, c.start_freq, c.bandwidth, c.tsamp)[:ntrials]
    return _hip.shift_table(c.nchan, dms, c.start_freq, c.bandwidth, c.tsamp)


def small_shifts(nchan, ntrials=40):
    """The grid of test_slot16_default_every_group (GPU suite)."""
    return _hip.shift_table(nchan, np.linspace(0, 50, ntrials), 400., 100., 1e-3)


def wrapping_shifts():
    """The grid of test_slot16_u8_wrapping_windows_and_small_budget (GPU suite)."""
    rng = np.random.default_rng(9)
    rng.integers(0, 256, (48, 1024))  # that test draws its data first
    return np.sort(rng.integers(-20000, 20000, (70, 48)), axis=0)


def _config(name, dtype=None, acc="native", ntrials=None):
    c = CONFIGS[name]
    return lambda: (dtype or c.dtype, acc, c.nchan, c.nsamples, config_shifts(name, ntrials), {})


def _small(dtype, nchan=64, n=4096, acc="native", **opts):
    return lambda: (dtype, acc, nchan, n, small_shifts(nchan), opts)


# name -> () -> (dtype, acc, nchan, nsamples, shifts, Plan keyword options)
CASES = {
    "C1": _config("C1"),
    "C1_f32_acc_f64": _config("C1", dtype="f32", acc="f64"),
    "C2": _config("C2"),
    "C2_acc_f64": _config("C2", acc="f64"),
    "C4": _config("C4"),
    "C5": _config("C5"),
    "C3_625": _config("C3", ntrials=625),
    "C3": _config("C3"),
    **{f"u8_tall_g{g}_slot16_{s16}": _small("u8", group=g, shape="tall", slot16=s16)
       for g in (2, 4, 8) for s16 in (None, False)},
    "u8_pair_g4": _small("u8", group=4, shape="pair"),
    "u8_pair_g4_slot16_False": _small("u8", group=4, shape="pair", slot16=False),
    "u8_n4099": _small("u8", n=4099),
    "u8_n4099_tall_g4": _small("u8", n=4099, group=4, shape="tall"),
    "u8_no_dma": _small("u8", u8_dma=False),
    "u8_no_dma_tall_g4": _small("u8", group=4, shape="tall", u8_dma=False),
    "f64_acc_f32_g4": _small("f64", acc="f32", group=4),
    "u8_nchan50_g4": _small("u8", nchan=50, group=4),
    "f32_nchan50_g4": _small("f32", nchan=50, group=4),
    "u8_tall_g4_lds64": _small("u8", group=4, shape="tall", lds_budget_kb=64),
    "u8_tall_g4_lds8": _small("u8", group=4, shape="tall", lds_budget_kb=8),
    "f32_lds64": _small("f32", lds_budget_kb=64),
    "f32_lds8": _small("f32", lds_budget_kb=8),
    "u8_wrapping": lambda: ("u8", "native", 48, 1024, wrapping_shifts(), dict(group=4, shape="tall")),
    "u8_wrapping_lds64": lambda: ("u8", "native", 48, 1024, wrapping_shifts(),
                                  dict(group=4, shape="tall", lds_budget_kb=64)),
    # item order on grids of several DM tiles of unequal cost (51 and 4): DM-tile major sorts them
    **{f"u8_wrapping_dt_major_{m}": (lambda m=m: ("u8", "native", 48, 1024, wrapping_shifts(),
                                                  dict(group=4, shape="tall", dt_major=m))) for m in (False, True)},
    **{f"f32_lds64_dt_major_{m}": _small("f32", lds_budget_kb=64, dt_major=m) for m in (False, True)},
    "f32_channel_mode": _small("f32", group=1),
    "u8_acc_f64": _small("u8", acc="f64"),
    "f32_nchan3": _small("f32", nchan=3),
    "u8_nchan3": _small("u8", nchan=3),
    "f32_nchan1": _small("f32", nchan=1),
    "u8_nchan1": _small("u8", nchan=1),
}


@functools.lru_cache(maxsize=None)
def outcome(case, describe=None):
    """What the planner makes of a case: {"info", "digest"}, or {"rc", "error"} where it
    refuses.  ``describe``: stands in for the library's pu_plan_describe (recording from a
    build that lacks it)."""
    dtype, acc, nchan, n, sh, opts = CASES[case]()
    sh, popts = _hip._plan_inputs(nchan, sh, opts.get("group", 0), opts.get("shape"), opts.get("lds_budget_kb", 0),
                                  opts.get("u8_dma"), opts.get("dt_major"), opts.get("slot16"))
    if describe is not None:
        return describe(DTYPES[dtype], ACCS[acc], nchan, n, sh, popts)
    try:
        info, digest = _hip.describe_plan(DTYPES[dtype], ACCS[acc], nchan, n, sh, **opts)
    except ValueError:
        import ctypes
        rc = _hip.lib().pu_plan_describe(DTYPES[dtype], ACCS[acc], nchan, n, sh.ctypes.data_as(ctypes.c_void_p),
                                         sh.shape[0], ctypes.byref(popts), None, 0, None)
        return {"rc": rc, "error": _hip.lib().pu_last_error().decode()}
    return {"info": info, "digest": f"{digest:#018x}"}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        rec = json.load(f)
    return {case: {**o, "info": dict(zip(rec["fields"], o["info"]))} if "info" in o else o
            for case, o in rec["cases"].items()}


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_plan_tables_pinned(recorded, case):
    got, want = outcome(case), recorded[case]
    assert sorted(got) == sorted(want), (got, want)
    if "info" in want:
        diff = {k: (got["info"][k], v) for k, v in want["info"].items() if got["info"][k] != v}
        assert not diff, f"info fields (got, recorded): {diff}"
    assert got == want


@pytest.mark.parametrize("pair", ["u8_wrapping_dt_major", "f32_lds64_dt_major"])
def test_item_order_option_reaches_the_tables(recorded, pair):
    """The dt_major cases pin the item order only if the option changes the tables: time-tile
    major and DM-tile major record different digests, and the same geometry."""
    off, on = recorded[pair + "_False"], recorded[pair + "_True"]
    assert off["digest"] != on["digest"]
    assert off["info"] == on["info"] and off["info"]["dm_tiles"] > 2


def test_slot16_default_every_group():
    """test_slot16_default_every_group of the GPU suite, on the planner alone."""
    sh = small_shifts(64)
    mk = lambda g, s16: _hip.describe_plan(_hip.PU_U8, _hip.PU_ACC_NATIVE, 64, 4096, sh, group=g, shape="tall",
                                           slot16=s16)[0]
    assert mk(8, None)["kernel"] == 3 and mk(4, None)["kernel"] == 3 and mk(2, None)["kernel"] == 3
    assert mk(8, True)["kernel"] == 3 and mk(4, False)["kernel"] == 2 and mk(8, False)["kernel"] == 2


def test_c3_plan_choice_shard_and_full():
    """test_c3_plan_choice_shard_and_full of the GPU suite, on the planner alone: the 625-trial
    shard takes tall G = 8, the whole 5000-trial grid tall G = 4, both with 16-bit slots."""
    for case, group, kernel in (("C3_625", 8, 3), ("C3", 4, 3)):
        info = outcome(case)["info"]  # default options (planned once for this module)
        assert (info["group"], info["kernel"], info["trials_per_tile"]) == (group, kernel, 256), (case, info)


def test_u8_native_channel_limit():
    """8-bit input with float32 sums is exact while nchan x 255 <= 2^24 - 1: the argument check
    accepts nchan = 65793 and refuses 65794.  (plan_sub repeats the bound for 16-bit slots;
    no entry point reaches that second check, so this test does not cover it.)"""
    rng = np.random.default_rng(3)
    for nchan, ok in ((65793, True), (65794, False)):
        sh = np.sort(rng.integers(0, 40, (4, nchan)), axis=0)
        if ok:
            info, _ = _hip.describe_plan(_hip.PU_U8, _hip.PU_ACC_NATIVE, nchan, 1024, sh)
            assert info["ndm"] == 4 and info["acc_is_f64"] == 0
        else:
            with pytest.raises(ValueError, match="exact only for nchan <= 65793"):
                _hip.describe_plan(_hip.PU_U8, _hip.PU_ACC_NATIVE, nchan, 1024, sh)


def record(describe=None, path=GOLDEN):
    """One line per case; ``info`` holds the values in the order of ``fields``."""
    out = {case: outcome(case, describe) for case in CASES}
    fields = list(_hip.INFO_FIELDS)
    lines = []
    for case, o in out.items():
        if "info" in o:
            o = {"info": [o["info"][k] for k in fields], "digest": o["digest"]}
        lines.append(f'  {json.dumps(case)}: {json.dumps(o)}')
    with open(path, "w") as f:
        f.write('{\n "fields": %s,\n "cases": {\n%s\n }\n}\n' % (json.dumps(fields), ",\n".join(lines)))
    return out


if __name__ == "__main__":
    record()
    print(f"recorded {len(CASES)} cases in {GOLDEN}")
