"""Host planner (product code) vs the reference's own plan / shift tables."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, PKG_DIR
from pulsarutils import _planner
from pulsarutils.configs import CONFIGS


def test_doctests(golden):
    arrays, _ = golden
    np.testing.assert_array_equal(_planner.normalize_shifts(np.array([-1, 0, 2, 4]), 3), [2, 0, 2, 1])
    np.testing.assert_array_equal(_planner.normalize_shifts(np.array([-1, 0, 2, 4]), 3),
                                  arrays["doctest_normalize"])
    assert _planner.normalize_shifts(np.array([-1.0]), 3).dtype == np.int32
    tdm = _planner.dedispersion_plan(10, 0, 10, 1400, 128, 0.0005)
    np.testing.assert_array_equal(tdm, arrays["doctest_plan"])
    assert np.isclose(tdm[0], 0) and np.isclose(tdm[-1], 10., atol=1)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_plan_bitexact(golden, name):
    arrays, _ = golden
    c = CONFIGS[name]
    p = _planner.dedispersion_plan(c.nchan, c.dmmin, c.dmmax, c.start_freq, c.bandwidth, c.tsamp)
    np.testing.assert_array_equal(p, arrays[f"plan_{name}"])
    assert p.size == c.ntrials


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_python_shifts_bitexact(golden, name):
    arrays, _ = golden
    c = CONFIGS[name]
    dms = arrays[f"plan_{name}"]
    idx = arrays[f"shiftidx_{name}"]
    if name == "C1":
        idx = idx[::7]
    for i in idx:
        got = _planner.dedispersion_shifts(c.nchan, dms[i], c.start_freq, c.bandwidth, c.tsamp)
        k = list(arrays[f"shiftidx_{name}"]).index(i)
        np.testing.assert_array_equal(got, arrays[f"shifts_{name}"][k])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cpp_shift_table_bitexact(golden, name):
    """pu_shift_table (C++ in the HIP library; host function, no GPU needed)."""
    from pulsarutils import _hip
    arrays, _ = golden
    c = CONFIGS[name]
    dms = arrays[f"plan_{name}"]
    idx = arrays[f"shiftidx_{name}"]
    got = _hip.shift_table(c.nchan, dms[idx], c.start_freq, c.bandwidth, c.tsamp)
    np.testing.assert_array_equal(got, arrays[f"shifts_{name}"].astype(np.int64))


def test_delta_delay():
    assert _planner.delta_delay(1.0, 1200., 1400.) == 4149. * 1200. ** -2 - 4149. * 1400. ** -2


# the cases of csrc/plan_check.cpp that tests/golden/plan_tables.json records too (same key,
# same linspace(0, 50, 40) shift grid, same options)
PLAN_CHECK_CASES = ([f"u8_tall_g{g}_slot16_{s16}" for g in (2, 4, 8) for s16 in (None, False)] +
                    ["u8_pair_g4", "u8_n4099", "u8_n4099_tall_g4", "u8_no_dma_tall_g4", "u8_acc_f64",
                     "f32_channel_mode", "f64_acc_f32_g4", "u8_nchan50_g4", "f32_nchan50_g4",
                     "u8_tall_g4_lds64", "u8_tall_g4_lds8", "f32_lds64", "f32_lds8",
                     "f32_lds64_dt_major_False", "f32_lds64_dt_major_True",
                     "f32_nchan3", "u8_nchan3", "f32_nchan1", "u8_nchan1"])


def test_plan_check_without_hip():
    """The library's planner objects link and run with no HIP header or library, and plan
    there what they plan inside the shared library: every case of plan_check that the golden
    file records prints the recorded table digest."""
    # the Makefile's compilers: $(CXX), and $(PLAN_CXX) for plan.cpp
    plan_cxx = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    for tool in ("make", os.environ.get("CXX", "g++"), os.environ.get("PLAN_CXX", plan_cxx)):
        if shutil.which(tool) is None:
            pytest.skip(f"no host C++ compiler ({tool})")
    csrc = os.path.join(PKG_DIR, "csrc")
    made = subprocess.run(["make", "-C", csrc, "plan_check"], capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    run = subprocess.run([os.path.join(csrc, "plan_check")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    digests = dict(re.findall(r"^(\S+) .* digest ([0-9a-f]{16})$", run.stdout, re.M))
    with open(os.path.join(GOLDEN_DIR, "plan_tables.json")) as f:
        recorded = json.load(f)["cases"]
    assert not set(PLAN_CHECK_CASES) - set(digests), "plan_check no longer runs these cases"
    compared = sorted(set(digests) & set(recorded))
    assert set(compared) >= set(PLAN_CHECK_CASES)
    diff = {k: (digests[k], recorded[k]["digest"]) for k in compared if "0x" + digests[k] != recorded[k]["digest"]}
    assert not diff, f"table digests (plan_check, recorded): {diff}"
