#!/usr/bin/env python
"""Time pu_fold_trials against the only other route to the same arrays: a loop of pu_fold over the
trials on the same row.

One float32 row of n = 2^20 samples (tsamp 64 us, 67 s), F = 4096 trial frequencies on
frequency_grid(5 Hz, ..., oversample 8) and nbin = 32, then once more at nbin = 256.  Both routes
are warmed up, then timed with HIP events in rounds that alternate them; a pu_fold_trials call is
three launches (fold, combine, counts) and is timed whole, and so is the loop (three launches per
trial).  The loop runs ``--loop-rounds`` times only (it is slow).  Where they are timed the two
results are compared: counts equal, sums within the folds' stated bound of each other.

The achieved float64 rate counts the fold kernel's FT_OPS = 8 float64 operations per sample and
trial (index + 1, multiply, add, floor, subtract, multiply, convert, accumulate) and the counts
kernel's 7 (the same without the accumulate), over the whole call's time, against bench.py's
VALU_F64_ADD_PEAK_TFLOPS.

    python scripts/period_bench.py [--rounds 15] [--loop-rounds 3] [--out DIR]

Prints one JSON line; with --out also writes period_bench.json there.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "radio-pulsar-utils_amd"))

N, F, TSAMP, FMIN = 2 ** 20, 4096, 64e-6, 5.0
FT_OPS, COUNT_OPS = 8, 7
VALU_F64_ADD_PEAK_TFLOPS = 39.3  # bench.py


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
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nbins", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pulsarutils import _hip, folding
    t = _hip.require_gpu()
    lib = _hip.lib()
    dev = torch.device("cuda", 0)
    x = torch.randn((1, N), dtype=t.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    freqs = folding.frequency_grid(FMIN, FMIN + (F - 1) / (8 * N * TSAMP), N * TSAMP)[:F]
    assert freqs.size == F
    dph_h = TSAMP * freqs
    dph = torch.from_numpy(dph_h).to(dev)
    code = _hip.dtype_code(x.dtype)
    result = {"shape": [1, N], "dtype": "float32", "ntrials": F, "tsamp": TSAMP, "freq_range_hz": [float(freqs[0]), float(freqs[-1])],
              "f64_ops_per_sample_and_trial": {"fold": FT_OPS, "counts": COUNT_OPS}, "peak_TFLOPs": VALU_F64_ADD_PEAK_TFLOPS, "nbin": {}}
    for nbin in args.nbins:
        sums = torch.zeros((1, F, nbin), dtype=t.float64, device=dev)
        counts = torch.zeros((F, nbin), dtype=t.int64, device=dev)
        ws = torch.empty(lib.pu_fold_trials_workspace_bytes(1, N, F, nbin), dtype=t.uint8, device=dev)

        def trials():
            _hip.check(lib.pu_fold_trials(_hip.ptr(x), code, 1, N, N, 0, None, _hip.ptr(dph), F, nbin, _hip.ptr(sums), nbin,
                                          F * nbin, _hip.ptr(counts), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()),
                       "pu_fold_trials")
        lsums = torch.zeros((F, nbin), dtype=t.float64, device=dev)
        lcounts = torch.zeros((F, nbin), dtype=t.int64, device=dev)
        lws = torch.empty(max(16, lib.pu_fold_workspace_bytes(1, N, nbin)), dtype=t.uint8, device=dev)
        sp, cp, step = lsums.data_ptr(), lcounts.data_ptr(), nbin * 8
        xs, wp, st = _hip.ptr(x), _hip.ptr(lws), _hip.stream_ptr()
        dlist = [float(d) for d in dph_h]

        def loop():
            for k, d in enumerate(dlist):
                rc = lib.pu_fold(xs, code, 1, N, N, 0, 0.0, d, nbin, sp + k * step, nbin, cp + k * step, wp, lws.numel(), st)
                if rc:
                    _hip.check(rc, "pu_fold")
        for _ in range(args.warmup):
            trials()
        loop()
        torch.cuda.synchronize()
        tt, tl = [], []
        for r in range(args.rounds):
            tt.append(timed(trials))
            if r < args.loop_rounds:
                tl.append(timed(loop))
        # the two routes fold the same bins: from zeroed outputs one call of each gives equal
        # counts and sums within 2 m u sum|x| of each other (each is within m u sum|x| of the
        # exact sum of the bin's m samples, and |x| < 6 for 2^20 normal deviates)
        for buf in (sums, counts, lsums, lcounts):
            buf.zero_()
        trials()
        loop()
        torch.cuda.synchronize()
        assert torch.equal(counts, lcounts) and int(counts.sum()) == F * N
        m = counts.to(t.float64)
        err = (sums[0] - lsums).abs()
        assert bool((err <= 2 * m * 2.0 ** -53 * 6.0 * m).all()), float(err.max())
        med = statistics.median(tt)
        ops = N * F * (FT_OPS + COUNT_OPS)
        rec = {"fold_trials": stats(tt), "pu_fold_loop": stats(tl),
               "speedup_median": round(statistics.median(tl) / med, 2),
               "f64_TFLOPs": round(ops / med / 1e9, 3), "of_f64_add_peak": round(ops / med / 1e9 / VALU_F64_ADD_PEAK_TFLOPS, 4),
               "workspace_bytes": ws.numel()}
        result["nbin"][str(nbin)] = rec
        del sums, counts, ws, lsums, lcounts, lws
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "period_bench.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
