#!/usr/bin/env python
"""Time pu_fold against the library's one-pass read-bound yardstick, pu_row_sums mode 3.

On the C4 shape (1024 channels x 2^18 samples), uint8 and float32, in one process: pu_fold at
nbin 256 with about 61 samples per bin, pu_fold at nbin 1024 with about 0.5 samples per bin, and
pu_row_sums mode 3 (the float64 sum of every row) on the same array.  Every variant is warmed up,
then timed with HIP events in rounds that alternate the variants; the figure is the median call.
A pu_fold call is three launches (fold, combine, counts) and is timed whole.  The read rate is the
input's bytes over the call time (the fold's partials - nseg x nchan x nbin - travel on top and
are reported as ``partial_bytes``).

    python scripts/fold_bench.py [--rounds 15] [--out DIR]

Prints one JSON line; with --out also writes fold_bench.json and a markdown table there.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "radio-pulsar-utils_amd"))

NCHAN, N = 1024, 2 ** 18
READ_CEILING_TBS = 6.15  # the measured HBM read ceiling
SEG = 16384              # csrc/fold.hip FOLD_SEG


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pulsarutils import _hip
    t = _hip.require_gpu()
    lib = _hip.lib()
    dev = torch.device("cuda", 0)
    folds = {"fold_nbin256_61_per_bin": (256, 1.0 / (61.03 * 256)), "fold_nbin1024_0.5_per_bin": (1024, 1.0 / (0.4997 * 1024))}
    result = {"shape": [NCHAN, N], "rounds": args.rounds, "read_ceiling_TBs": READ_CEILING_TBS, "dtypes": {}}
    for name, dtype in (("uint8", t.uint8), ("float32", t.float32)):
        g = torch.Generator(device=dev).manual_seed(1)
        if dtype == t.uint8:
            x = torch.randint(0, 256, (NCHAN, N), dtype=dtype, device=dev, generator=g)
        else:
            x = torch.randn((NCHAN, N), dtype=dtype, device=dev, generator=g)
        code = _hip.dtype_code(x.dtype)
        nbytes = x.numel() * x.element_size()
        calls = {}
        keep, outs = [], {}
        for key, (nbin, dphase) in folds.items():
            sums = torch.zeros((NCHAN, nbin), dtype=t.float64, device=dev)
            counts = torch.zeros(nbin, dtype=t.int64, device=dev)
            ws = torch.empty(lib.pu_fold_workspace_bytes(NCHAN, N, nbin), dtype=t.uint8, device=dev)
            keep += [ws]
            outs[key] = (sums, counts)

            def call(nbin=nbin, dphase=dphase, sums=sums, counts=counts, ws=ws):
                _hip.check(lib.pu_fold(_hip.ptr(x), code, NCHAN, N, N, 0, 0.0, dphase, nbin, _hip.ptr(sums), nbin,
                                       _hip.ptr(counts), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), "pu_fold")
            calls[key] = call
        out = torch.empty(NCHAN, dtype=t.float64, device=dev)
        rws = torch.empty(max(16, lib.pu_row_sums_workspace_bytes(NCHAN, N)), dtype=t.uint8, device=dev)

        def rowsums():
            _hip.check(lib.pu_row_sums(_hip.ptr(x), code, NCHAN, N, N, 3, None, None, 0.0, _hip.ptr(out), _hip.ptr(rws),
                                       rws.numel(), _hip.stream_ptr()), "pu_row_sums")
        calls["row_sums_mode3"] = rowsums
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
        # the fold's result is checked where it is timed: every sample counted once, the sums' total
        # equal to the row sums' total (exact for uint8)
        torch.cuda.synchronize()
        ncalls = args.warmup + args.rounds
        total = int(x.sum(dtype=t.int64)) if name == "uint8" else None
        for key, (sums, counts) in outs.items():
            assert int(counts.sum()) == ncalls * N, key
            if total is not None:
                assert float(sums.sum()) == float(ncalls * total), key
        rec = {}
        yard = statistics.median(times["row_sums_mode3"])
        for k, v in times.items():
            med = statistics.median(v)
            rec[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                      "read_TBs": round(nbytes / med / 1e9, 3), "of_ceiling": round(nbytes / med / 1e9 / READ_CEILING_TBS, 3),
                      "vs_row_sums": round(med / yard, 3)}
            if k in folds:
                rec[k]["partial_bytes"] = (N // SEG) * NCHAN * folds[k][0] * (4 if name == "uint8" else 8)
        result["dtypes"][name] = {"input_bytes": nbytes, "calls": rec}
        del x, keep, outs
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "fold_bench.json"), "w") as f:
            json.dump(result, f, indent=1)
        with open(os.path.join(args.out, "fold_bench.md"), "w") as f:
            f.write("| dtype | call | median ms | min - max ms | read TB/s | of 6.15 TB/s | time / row_sums |\n|---|---|---|---|---|---|---|\n")
            for name, d in result["dtypes"].items():
                for k, r in d["calls"].items():
                    f.write(f"| {name} | {k} | {r['ms_median']} | {r['ms_min']} - {r['ms_max']} | {r['read_TBs']} | "
                            f"{r['of_ceiling']} | {r['vs_row_sums']} |\n")


if __name__ == "__main__":
    main()
