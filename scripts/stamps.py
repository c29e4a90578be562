"""Phase breakdown of the subband kernel from in-kernel shader-clock stamps.

Loads the diagnostic library (make -C radio-pulsar-utils_amd/csrc stamps; PU_STAMPS),
runs the C2 search a few times and prints each phase's share of the summed wave
cycles (stamps drain the LDS queue at every phase boundary: read the SHARES, not the
run time - cdna_hip_programming.md §7), in total and by role: the DMA-issuing waves and
the others.  Phases: barrier_A_wait runs from the end of a stage's sum through the wave's
own DMA wait and the barrier before the build (no stamp stands between the loop-top scalar
loads and that barrier); metadata_stall is the wait for the stage's scalar metadata after
that barrier (its floor is one scalar-cache round trip: the clock read of the stamp
itself); build; barrier_B_wait: the barrier after the build; dma_issue; sum; epilogue.

    python scripts/stamps.py [config] [launches]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PULSARUTILS_HIP_LIB", os.path.join(REPO, "radio-pulsar-utils_amd", "pulsarutils", "_lib",
                                                          "libpulsarutils_hip_stamps.so"))
sys.path[:0] = [os.path.join(REPO, "radio-pulsar-utils_amd"), REPO]
import ctypes  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
from pulsarutils import _hip, synth  # noqa: E402
from pulsarutils.configs import CONFIGS  # noqa: E402
from pulsarutils.dedispersion import dedispersion_plan  # noqa: E402

PHASES = ("metadata_stall", "barrier_A_wait", "build", "barrier_B_wait", "dma_issue", "sum", "epilogue", "unused")
ROLES = ("other_waves", "dma_waves")
NST = len(PHASES) * len(ROLES)


def main():
    cfg = CONFIGS[sys.argv[1] if len(sys.argv) > 1 else "C2"]
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    x = synth.pulsar_filterbank_device(cfg)
    dms = dedispersion_plan(cfg.nchan, cfg.dmmin, cfg.dmmax, cfg.start_freq, cfg.bandwidth, cfg.tsamp)
    ntr = int(os.environ.get("PU_TRIALS", "0"))
    if ntr:
        dms = dms[:ntr]
    sh = _hip.shift_table(cfg.nchan, dms, cfg.start_freq, cfg.bandwidth, cfg.tsamp)
    plan = _hip.Plan(_hip.dtype_code(x.dtype), _hip.PU_ACC_NATIVE, cfg.nchan, cfg.nsamples, sh)
    out = np.zeros(NST, np.int64)
    buf = out.ctypes.data_as(ctypes.c_void_p)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=x.device)
    plan.search(x, workspace=ws)
    _hip.lib().pu_plan_stamps(plan._h, buf, NST)  # arm
    for _ in range(launches):
        plan.search(x, workspace=ws)
    m = _hip.lib().pu_plan_stamps(plan._h, buf, NST)
    if m <= 0:
        print("not a stamps build", file=sys.stderr)
        return
    tot = float(out.sum())
    np_ = len(PHASES)
    by_role = out.reshape(len(ROLES), np_)
    rec = {"config": cfg.name, "plan": {k: plan.info[k] for k in ("group", "stages", "dm_tiles", "time_tiles")},
           "env": {k: os.environ.get(k) for k in ("PU_SUB_SHAPE", "PU_GROUP") if os.environ.get(k)},
           "share": {p: round(float(by_role[:, i].sum()) / tot, 4) for i, p in enumerate(PHASES[:7])},
           "wave_cycles_per_launch": tot / launches,
           # per role: each phase's share of that role's own wave cycles, and the role's cycles
           "roles": {r: {"wave_cycles_per_launch": float(by_role[j].sum()) / launches,
                         "share": {p: round(float(by_role[j, i]) / max(float(by_role[j].sum()), 1.0), 4)
                                   for i, p in enumerate(PHASES[:7])}}
                     for j, r in enumerate(ROLES)}}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
