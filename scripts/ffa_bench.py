#!/usr/bin/env python
"""Time pu_ffa against the two yardsticks it has, and one whole ffa_search.

256 float32 rows of n = 2^20 samples at base period p = 256 (m = 4096 trial periods, of which the
last is the first of p = 257), ten boxcar widths (the first ten of default_widths(256)):

  fused      pu_ffa with snr and peak only: the top level is formed where it is scored
  unfused    pu_ffa with out, snr and peak: transform, then score the written plane
  transform  pu_ffa with out only

Yardstick 1, the only way the parent commit can do this work: pu_fold_trials + pu_profile_chi2 on the
same rows at the same 4095 trial periods with nbin = 256.  Its workspace is 512 MiB per row, so it
runs on ``--fold-rows`` rows (default 8) per call; the figure for 256 rows is that time x 256 /
fold-rows (the work is the same for every row) and is marked as scaled.
Yardstick 2, a traffic floor: pu_ffa_describe's traffic_bytes of the fused call over the 6.15 TB/s
read ceiling of DESIGN.md section 7.

Then one ffa_search of the plane from 240 to 15360 samples of period (sample_time 1).

HIP events around each call, ``--warmup`` calls first, the median (min - max) of ``--rounds``; the
three pu_ffa forms alternate inside a round.

    python scripts/ffa_bench.py [--rounds 15] [--fold-rows 8] [--search-rounds 3] [--out DIR]

Prints one JSON line; with --out also writes ffa_bench.json there.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "radio-pulsar-utils_amd"))

ROWS, N, P = 256, 2 ** 20, 256
HBM_READ_TBS = 6.15


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fold-rows", type=int, default=8)
    ap.add_argument("--fold-rounds", type=int, default=3)
    ap.add_argument("--search-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from pulsarutils import _hip, ffa
    t = _hip.require_gpu()
    lib = _hip.lib()
    dev = torch.device("cuda", 0)
    m = N // P
    x = torch.randn((ROWS, N), dtype=t.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    widths = np.ascontiguousarray(ffa.default_widths(P)[:10])
    nw = widths.size
    wptr = widths.ctypes.data_as(ctypes.c_void_p)
    out = torch.empty((ROWS, m, P), dtype=t.float32, device=dev)
    snr = torch.empty((ROWS, m, nw), dtype=t.float32, device=dev)
    peak = torch.empty((ROWS, m, nw), dtype=t.int32, device=dev)
    info = {k: ffa.describe(ROWS, m, P, n_, o) for k, (n_, o) in
            {"fused": (nw, False), "unfused": (nw, True), "transform": (0, True)}.items()}
    ws = _hip.workspace(max(i["workspace_bytes"] for i in info.values()), dev)

    def call(want_out, want_snr):
        _hip.check(lib.pu_ffa(_hip.ptr(x), ROWS, N, m, P, _hip.ptr(out) if want_out else None, m * P, wptr if want_snr else None,
                              nw if want_snr else 0, None, _hip.ptr(snr) if want_snr else None,
                              _hip.ptr(peak) if want_snr else None, ws[1], ws[2], _hip.stream_ptr()), "pu_ffa")
    forms = {"fused": lambda: call(False, True), "unfused": lambda: call(True, True), "transform": lambda: call(True, False)}
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    # the two S/N forms agree bit for bit
    forms["fused"]()
    a, b = snr.clone(), peak.clone()
    forms["unfused"]()
    torch.cuda.synchronize()
    assert torch.equal(a.view(t.int32), snr.view(t.int32)) and torch.equal(b, peak)
    del a, b
    result = {"shape": [ROWS, N], "p": P, "m": m, "widths": widths.tolist(), "describe": info,
              "pu_ffa": {k: stats(v) for k, v in times.items()}}
    fused = statistics.median(times["fused"])
    floor_ms = info["fused"]["traffic_bytes"] / (HBM_READ_TBS * 1e12) * 1e3
    result["traffic_floor"] = {"bytes": info["fused"]["traffic_bytes"], "TBps": HBM_READ_TBS, "ms": round(floor_ms, 4),
                               "fused_over_floor": round(fused / floor_ms, 3),
                               "fused_achieved_TBps": round(info["fused"]["traffic_bytes"] / fused / 1e9, 3)}
    del out, snr, peak, ws

    # yardstick 1: epoch folding at the same trial periods
    fr = max(1, min(ROWS, args.fold_rows))
    ntr = m - 1
    periods = ffa.trial_periods(P, m)[:ntr]
    dph = torch.from_numpy(1.0 / periods).to(dev)
    sums = torch.zeros((fr, ntr, P), dtype=t.float64, device=dev)
    counts = torch.zeros((ntr, P), dtype=t.int64, device=dev)
    fws = torch.empty(lib.pu_fold_trials_workspace_bytes(fr, N, ntr, P), dtype=t.uint8, device=dev)
    mean = x[:fr].to(t.float64).mean(dim=1)
    var = x[:fr].to(t.float64).var(dim=1, unbiased=False)
    chi2 = torch.empty((fr, ntr), dtype=t.float64, device=dev)
    dof = torch.empty(ntr, dtype=t.int32, device=dev)

    def fold():
        _hip.check(lib.pu_fold_trials(_hip.ptr(x), _hip.PU_F32, fr, N, N, 0, None, _hip.ptr(dph), ntr, P, _hip.ptr(sums), P,
                                      ntr * P, _hip.ptr(counts), _hip.ptr(fws), fws.numel(), _hip.stream_ptr()),
                   "pu_fold_trials")
        _hip.check(lib.pu_profile_chi2(_hip.ptr(sums), P, ntr * P, _hip.ptr(counts), fr, ntr, P, _hip.ptr(mean), _hip.ptr(var),
                                       _hip.ptr(chi2), _hip.ptr(dof), _hip.stream_ptr()), "pu_profile_chi2")
    fold()
    torch.cuda.synchronize()
    tf = [timed(fold) for _ in range(args.fold_rounds)]
    scaled = statistics.median(tf) * ROWS / fr
    result["fold_trials_chi2"] = {"rows_timed": fr, "ntrials": ntr, "nbin": P, **stats(tf),
                                  "ms_for_256_rows_scaled": round(scaled, 1), "over_fused": round(scaled / fused, 1)}
    del sums, counts, fws, chi2

    # one whole search of the plane
    def search():
        return ffa.ffa_search(x, 1.0, 240.0, 15360.0)
    tab = search()
    torch.cuda.synchronize()
    tsr = [timed(search) for _ in range(args.search_rounds)]
    plan = ffa.ffa_plan(N, 1.0, 240.0, 15360.0)
    result["ffa_search"] = {"period_samples": [240, 15360], "steps": sum(p1 - p0 for _, p0, p1 in plan), "factors": len(plan),
                            "candidates": len(tab["snr"]), **stats(tsr)}
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "ffa_bench.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
