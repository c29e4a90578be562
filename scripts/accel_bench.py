#!/usr/bin/env python
"""Time the acceleration trials on a float32 plane of 256 rows x n = 2^20 samples (tsamp 64 us, 67 s):

  (1) pu_rfft of the plane (the transform without an acceleration axis);
  (2) pu_resample_accel at one non-zero acceleration into a second plane, then pu_rfft of it;
  (3) pu_rfft_accel at the same acceleration (the resampling in the transform's first load);
  (4) the whole acceleration_search over a grid of about 100 trials (host work included).

One process.  (1) - (3) are warmed up, then timed with HIP events in rounds that alternate the three
(so that a drift of the machine falls on all alike); median with min - max, and the spread of (1),
max - min, is the yardstick for "(3) is not slower than (2)".  (4) is timed with the wall clock
around a synchronise.  What is timed is checked: (3) has the bits of (2); row 0 holds a pulse
train of 7.3 Hz that drifts at 2000 m/s^2, and the search's best candidate is that row at that
frequency within a bin and that acceleration within a bin of drift at its top harmonic, while
periodicity_search of the same plane ranks it lower.

    python scripts/accel_bench.py [--rounds 15] [--rows 256] [--out DIR]

Prints one JSON line; with --out also writes accel_bench.json there.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "radio-pulsar-utils_amd"))

N, TSAMP, NHARM, BLOCK = 2 ** 20, 64e-6, 16, 128
F0, DUTY, AMP, ACCEL = 7.3, 0.05, 0.3, 2000.0
FMAX, TRIALS = 50.0, 101  # the grid: ftop = FMAX * NHARM, TRIALS steps across
HBM_PEAK_GBS = 8000.0  # bench.py


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--search-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from pulsarutils import _hip
    from pulsarutils import periodicity as pe
    t = _hip.require_gpu()
    lib = _hip.lib()
    dev = torch.device("cuda", 0)
    rows, nfft, nb = args.rows, N, N // 2
    tobs = N * TSAMP
    x = torch.randn((rows, N), dtype=t.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    # the pulse train is periodic in the series resampled at ACCEL: received sample u shows the phase
    # of the root i of af i^2 + (1 - af n) i - u = 0
    af0 = float(pe.accel_factor(ACCEL, TSAMP))
    u = torch.arange(N, device=dev, dtype=t.float64)
    b = 1.0 - af0 * N
    emitted = 2.0 * u / (b + torch.sqrt(b * b + 4.0 * af0 * u))
    x[0] += AMP * ((emitted * (TSAMP * F0)) % 1.0 < DUTY).to(t.float32)
    mean = x.to(t.float64).sum(dim=1) / N
    af = torch.tensor([af0], dtype=t.float64, device=dev)
    moved = int(np.sum(pe.resample_indices(N, af0) != np.arange(N)))
    resampled = torch.empty((rows, N), dtype=t.float32, device=dev)
    spec = {k: torch.empty((rows, nb + 1), dtype=t.complex64, device=dev) for k in ("plain", "two_step", "fused")}
    ws, wp, wsb = pe._aligned(lib.pu_rfft_accel_workspace_bytes(rows, 1, nfft), dev)
    st = _hip.stream_ptr()

    def rfft(src, out):
        _hip.check(lib.pu_rfft(_hip.ptr(src), _hip.PU_F32, rows, N, N, _hip.ptr(mean), nfft, _hip.ptr(out), nb + 1, wp, wsb,
                               st), "pu_rfft")

    def plain():
        rfft(x, spec["plain"])

    def two_step():
        _hip.check(lib.pu_resample_accel(_hip.ptr(x), _hip.PU_F32, rows, N, N, _hip.ptr(af), 1, _hip.ptr(resampled), N, st),
                   "pu_resample_accel")
        rfft(resampled, spec["two_step"])

    def gather_only():
        _hip.check(lib.pu_resample_accel(_hip.ptr(x), _hip.PU_F32, rows, N, N, _hip.ptr(af), 1, _hip.ptr(resampled), N, st),
                   "pu_resample_accel")

    def fused():
        _hip.check(lib.pu_rfft_accel(_hip.ptr(x), _hip.PU_F32, rows, N, N, _hip.ptr(mean), _hip.ptr(af), 1, nfft,
                                     _hip.ptr(spec["fused"]), nb + 1, wp, wsb, st), "pu_rfft_accel")

    variants = {"pu_rfft": plain, "pu_resample_accel+pu_rfft": two_step, "pu_rfft_accel": fused,
                "pu_resample_accel": gather_only}
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):  # alternating: one of each per round
        for k, fn in variants.items():
            times[k].append(timed(fn))
    rec = {k: stats(v) for k, v in times.items()}
    spread = rec["pu_rfft"]["ms_max"] - rec["pu_rfft"]["ms_min"]
    excess = rec["pu_rfft_accel"]["ms_median"] - rec["pu_resample_accel+pu_rfft"]["ms_median"]
    # ---- what was timed is right
    assert torch.equal(spec["fused"].view(t.float32).view(t.int32), spec["two_step"].view(t.float32).view(t.int32))
    assert not torch.equal(spec["fused"].view(t.float32), spec["plain"].view(t.float32)) and moved > N // 2
    grid = pe.acceleration_grid((TRIALS // 2 - 0.5) * 299792458.0 / (FMAX * NHARM * tobs ** 2), tobs, FMAX * NHARM)
    table = [None]

    def whole():
        table[0] = pe.acceleration_search(x, TSAMP, accels=grid, fmax=FMAX, nharm=NHARM, sigma=6.0, block=BLOCK)

    whole()
    rec["acceleration_search"] = dict(stats([wall(whole) for _ in range(args.search_runs)]), trials=int(grid.size),
                                      pairs=int(grid.size) * rows)
    tab = table[0]
    step = float(grid[1] - grid[0])
    assert len(tab) > 0 and tab["row"][0] == 0 and abs(tab["freq"][0] - F0) <= 1.0 / tobs, (tab["freq"][:3], tab["row"][:3])
    # the 16 harmonics of 7.3 Hz end far below ftop: the trials within a bin of drift at the top harmonic
    # summed respond alike, and the noise picks among them
    tol = 299792458.0 / (float(tab["nharm"][0]) * F0 * tobs ** 2)
    assert abs(tab["accel"][0] - ACCEL) <= tol, (tab["accel"][:3], tol)
    flat = pe.periodicity_search(x, TSAMP, fmax=FMAX, nharm=NHARM, sigma=6.0, block=BLOCK)
    flat_logp = float(flat["logp"][0]) if len(flat) and flat["row"][0] == 0 else 0.0
    assert float(tab["logp"][0]) < flat_logp
    result = {"shape": [rows, N], "dtype": "float32", "tsamp": TSAMP, "nharm": NHARM, "block": BLOCK,
              "accel_timed_m_s2": ACCEL, "samples_moved": moved, "rounds": args.rounds, "times": rec,
              "criterion": {"pu_rfft_spread_ms": round(spread, 4), "fused_minus_two_step_ms": round(excess, 4),
                            "fused_not_slower": bool(excess <= spread)},
              "checks": {"fused_equals_two_step_bits": True, "grid_step_m_s2": round(step, 3), "accel_tolerance_m_s2": round(tol, 1),
                         "best_freq_hz": float(tab["freq"][0]), "best_accel_m_s2": float(tab["accel"][0]),
                         "best_nharm": int(tab["nharm"][0]), "best_logp": float(tab["logp"][0]),
                         "periodicity_search_best_logp": flat_logp, "candidates_sifted": len(tab)},
              # compulsory HBM bytes: the FFT reads the plane, writes the spectrum and makes one workspace
              # round trip; the two-step path adds the gather's read and write of the plane
              "hbm_bytes": {"pu_rfft": rows * (N * 4 + (nb + 1) * 8 + 2 * nb * 8),
                            "pu_resample_accel": rows * N * 8},
              "hbm_peak_GBs": HBM_PEAK_GBS}
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "accel_bench.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
