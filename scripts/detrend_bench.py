#!/usr/bin/env python
"""Time the running-median detrend at the FFA's headline shape: 256 rows of n = 2^20 samples, a
width of 31250 samples (d = 309, w = 101, 3393 block means per row).

  apply      pu_detrend_apply, float32 out of place and float64 in place (what ffa_search runs),
             against the floor of its bytes (read x, write out) at the 6.15 TB/s read ceiling of
             DESIGN.md section 7
  median     pu_running_median on the (256, 3393) block means, float64 and float32, against the
             same result from torch on the same tensor: replicate-pad, unfold, sort, take the
             middle; and d = 1, w = 101 on one float32 row of 2^20 samples, the same way.  The
             two alternate inside a round and the results are compared bit for bit.
  detrend    the whole detrend of the float64 plane in place (rebin, divide, median, apply), as
             ffa_search calls it, and one ffa_search of the plane with and without detrend_width

HIP events around each call, ``--warmup`` calls first, the median (min - max) of ``--rounds``.

    python scripts/detrend_bench.py [--rounds 15] [--search-rounds 2] [--out DIR]

Prints one JSON line; with --out also writes detrend_bench.json there.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "radio-pulsar-utils_amd"))

ROWS, N, WIDTH = 256, 2 ** 20, 31250
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


def alternate(forms, warmup, rounds):
    import torch
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--search-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from pulsarutils import _hip, detrend, ffa
    from pulsarutils.dedispersion import _rebin_time_device
    t = _hip.require_gpu()
    dev = torch.device("cuda", 0)
    d, w = detrend.detrend_plan(WIDTH)
    h = (w - 1) // 2
    nblk = N // d
    x = torch.randn((ROWS, N), dtype=t.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    x64 = x.to(t.float64)
    result = {"shape": [ROWS, N], "width_samples": WIDTH, "d": d, "w": w, "nblk": nblk,
              "describe": {"float64": detrend.describe("float64", w), "float32": detrend.describe("float32", w)}}

    # ---- the running median against torch's unfold + sort
    mean64 = _rebin_time_device(x64, d) / torch.full((), float(d), dtype=t.float64, device=dev)
    mean32 = mean64.to(t.float32)
    row32 = x[0:1].contiguous()

    def by_torch(v):
        pad = F.pad(v[:, None, :], (h, h), mode="replicate")[:, 0]
        return pad.unfold(1, w, 1).sort(dim=-1).values[..., h].contiguous()
    result["median"] = {}
    for name, v in (("means_float64", mean64), ("means_float32", mean32), ("one_row_2^20_float32", row32)):
        got, want = detrend._running_median_device(v, w), by_torch(v)
        torch.cuda.synchronize()
        ivt = t.int64 if v.dtype == t.float64 else t.int32
        assert torch.equal(got.view(ivt), want.view(ivt)), name
        del got, want
        times = alternate({"pu_running_median": lambda: detrend._running_median_device(v, w), "torch_unfold_sort": lambda: by_torch(v)},
                          args.warmup, args.rounds)
        k, s = statistics.median(times["pu_running_median"]), statistics.median(times["torch_unfold_sort"])
        result["median"][name] = {"shape": list(v.shape), "w": w, **{n_: stats(tv) for n_, tv in times.items()},
                                  "torch_over_kernel": round(s / k, 2)}
    del mean32, row32

    # ---- pu_detrend_apply against the floor of its bytes
    med = detrend._running_median_device(mean64, w)
    out32 = torch.empty_like(x)
    work64 = x64.clone()
    times = alternate({"float32_out_of_place": lambda: detrend._apply_device(x, med, d, out32),
                       "float64_in_place": lambda: detrend._apply_device(work64, med, d, work64)}, args.warmup, args.rounds)
    result["apply"] = {}
    for name, es in (("float32_out_of_place", 4), ("float64_in_place", 8)):
        nbytes = 2 * ROWS * N * es
        floor_ms = nbytes / (HBM_READ_TBS * 1e12) * 1e3
        m = statistics.median(times[name])
        result["apply"][name] = {**stats(times[name]), "bytes": nbytes, "floor_ms": round(floor_ms, 4),
                                 "over_floor": round(m / floor_ms, 3), "achieved_TBps": round(nbytes / m / 1e9, 3)}
    del out32, work64, med, mean64

    # ---- the whole detrend, as ffa_search runs it, and its share of a search
    work64 = x64.clone()
    times = alternate({"detrend_float64_in_place": lambda: detrend._detrend_device(work64, WIDTH, in_place=True),
                       "detrend_float32_public": lambda: detrend.detrend(x, WIDTH)}, args.warmup, args.rounds)
    result["detrend"] = {n_: stats(tv) for n_, tv in times.items()}
    del work64, x64

    def search(width):
        return ffa.ffa_search(x, 1.0, 240.0, 15360.0, detrend_width=width)
    search(None)
    torch.cuda.synchronize()
    ts = {"none": [], "width": []}
    for _ in range(args.search_rounds):
        ts["none"].append(timed(lambda: search(None)))
        ts["width"].append(timed(lambda: search(float(WIDTH))))
    result["ffa_search"] = {"period_samples": [240, 15360], "without": stats(ts["none"]), "with_detrend_width": stats(ts["width"]),
                            "detrend_share_of_search": round(statistics.median(times["detrend_float64_in_place"])
                                                             / statistics.median(ts["none"]), 6)}
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "detrend_bench.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
