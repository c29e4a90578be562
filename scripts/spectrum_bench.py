#!/usr/bin/env python
"""Time the FFT periodicity search stage by stage on float32 rows of n = 2^20 samples (tsamp 64 us,
67 s), at rows = 1 and 256, nharm = 16, block = 128:

  pu_rfft, pu_spectrum_normalize, the fused pu_harmonic_search (no sums written; it synchronises
  the stream once, which its time includes) and the whole periodicity_search (host work included).

One process; every stage is warmed up, then timed with HIP events (the whole search with the wall
clock around a synchronise); median with min - max.  What is timed is checked: the spectrum of row 0
against numpy's float64 rfft of the same float32 samples within the FFT's stated bound, the
normalised noise spectrum's mean near 1, and the search's best candidate at the injected pulse
train's frequency.

Yardsticks: (a) each kernel's compulsory HBM bytes over bench.py's HBM_PEAK_GBS; (b) torch.fft.rfft
of the same device tensor ("unavailable" if the installed torch cannot run it); (c)
folding.frequency_search of the same row over a 4096-trial grid, the per-trial route the FFT replaces.

    python scripts/spectrum_bench.py [--rounds 15] [--rows 1 256] [--out DIR]

Prints one JSON line; with --out also writes spectrum_bench.json there.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "radio-pulsar-utils_amd"))

N, TSAMP, NHARM, BLOCK, F0 = 2 ** 20, 64e-6, 16, 128, 7.3
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from pulsarutils import _hip, folding
    from pulsarutils import periodicity as pe
    t = _hip.require_gpu()
    lib = _hip.lib()
    dev = torch.device("cuda", 0)
    nfft, nb, nlev = N, N // 2, pe._nlev(NHARM)
    tobs = nfft * TSAMP
    thr = np.array([pe.power_threshold(pe.logp_from_sigma(6.0), 1 << lv) for lv in range(nlev)], np.float32)
    kmin, kmax = pe.bin_ranges(None, None, nfft, TSAMP, nlev, nb)
    result = {"shape_per_row": N, "dtype": "float32", "tsamp": TSAMP, "nharm": NHARM, "block": BLOCK,
              "hbm_peak_GBs": HBM_PEAK_GBS, "rows": {}}
    for rows in args.rows:
        x = torch.randn((rows, N), dtype=t.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        pulse = ((torch.arange(N, device=dev, dtype=t.float64) * (TSAMP * F0)) % 1.0 < 0.05).to(t.float32)
        x[0] += 0.3 * pulse
        mean = x.to(t.float64).sum(dim=1) / N
        spec = torch.empty((rows, nb + 1), dtype=t.complex64, device=dev)
        norm = torch.empty((rows, nb), dtype=t.float32, device=dev)
        ws, wp, wsb = pe._aligned(lib.pu_rfft_workspace_bytes(rows, nfft), dev)
        hws, hwp, hwsb = pe._aligned(lib.pu_harmonic_search_workspace_bytes(rows, nb, nlev), dev)
        cap = 1 << 16
        cbuf = torch.empty(cap * _hip.SPEC_CAND_DTYPE.itemsize, dtype=t.uint8, device=dev)
        count = ctypes.c_int64(0)
        st = _hip.stream_ptr()

        def fft():
            _hip.check(lib.pu_rfft(_hip.ptr(x), _hip.PU_F32, rows, N, N, _hip.ptr(mean), nfft, _hip.ptr(spec), nb + 1, wp,
                                   wsb, st), "pu_rfft")

        def normalize():
            _hip.check(lib.pu_spectrum_normalize(_hip.ptr(spec), rows, nb, nb + 1, BLOCK, _hip.ptr(norm), nb, st),
                       "pu_spectrum_normalize")

        def search():
            _hip.check(lib.pu_harmonic_search(_hip.ptr(norm), rows, nb, nb, nlev, None, 0, 0,
                                              thr.ctypes.data_as(ctypes.c_void_p), kmin.ctypes.data_as(ctypes.c_void_p),
                                              kmax.ctypes.data_as(ctypes.c_void_p), _hip.ptr(cbuf), cap,
                                              ctypes.byref(count), hwp, hwsb, st), "pu_harmonic_search")

        table = [None]

        def whole():
            table[0] = pe.periodicity_search(x, TSAMP, nharm=NHARM, sigma=6.0, block=BLOCK)

        stages = {"pu_rfft": fft, "pu_spectrum_normalize": normalize, "pu_harmonic_search_fused": search}
        rec = {}
        for name, fn in stages.items():  # in pipeline order: each leaves the next one's input
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            rec[name] = stats([timed(fn) for _ in range(args.rounds)])
        for _ in range(args.warmup):
            whole()
        rec["periodicity_search"] = stats([wall(whole) for _ in range(max(3, args.rounds // 3))])
        # ---- what was timed is right
        ref = np.fft.rfft(((x[0].cpu().numpy().astype(np.float64)) - float(mean[0])).astype(np.float32).astype(np.float64))
        got = spec[0].cpu().numpy().astype(np.complex128)
        ratio = float(np.linalg.norm(got - ref) / (math.log2(nfft) * 2.0 ** -24 * np.linalg.norm(ref)))
        assert ratio <= 8.0, ratio
        nmean = float(norm[rows - 1, 1:].mean())
        assert 0.9 < nmean < 1.1, nmean
        tab = table[0]
        assert len(tab) > 0 and tab["row"][0] == 0 and abs(tab["freq"][0] - F0) <= 1.0 / tobs, (tab["freq"][:3], tab["row"][:3])
        rec["checks"] = {"fft_error_over_log2n_eps": round(ratio, 3), "normalised_noise_mean": round(nmean, 4),
                         "best_freq_hz": float(tab["freq"][0]), "best_nharm": int(tab["nharm"][0]),
                         "best_logp": float(tab["logp"][0]), "candidates_raw": int(count.value),
                         "candidates_sifted": len(tab)}
        # ---- (a) compulsory HBM bytes
        two_pass = lib.pu_rfft_workspace_bytes(2, nfft) > lib.pu_rfft_workspace_bytes(1, nfft)
        hbm = {"pu_rfft": rows * (N * 4 + (nb + 1) * 8 + (2 * nb * 8 if two_pass else 0)),
               "pu_spectrum_normalize": rows * (nb * 8 + nb * 4),
               "pu_harmonic_search_fused": rows * nb * 4}
        rec["hbm"] = {k: {"bytes": v, "GBs": round(v / rec[k]["ms_median"] / 1e6, 1),
                          "frac_of_peak": round(v / rec[k]["ms_median"] / 1e6 / HBM_PEAK_GBS, 4)} for k, v in hbm.items()}
        # ---- (b) the vendor FFT on the same tensor
        try:
            def vendor():
                return torch.fft.rfft(x, n=nfft, dim=1)
            for _ in range(args.warmup):
                vendor()
            torch.cuda.synchronize()
            v = stats([timed(vendor) for _ in range(args.rounds)])
            verr = float(np.linalg.norm(vendor()[0].cpu().numpy().astype(np.complex128)
                                        - np.fft.rfft(x[0].cpu().numpy().astype(np.float64)))
                         / (math.log2(nfft) * 2.0 ** -24 * np.linalg.norm(ref)))
            rec["torch_fft_rfft"] = dict(v, pu_rfft_over_torch=round(rec["pu_rfft"]["ms_median"] / v["ms_median"], 3),
                                         error_over_log2n_eps=round(verr, 3))
        except Exception as e:  # noqa: BLE001 - any failure of the vendor route is "unavailable"
            rec["torch_fft_rfft"] = "unavailable (%s: %s)" % (type(e).__name__, str(e)[:120])
        # ---- (c) epoch folding of the same row over its documented 4096-trial grid
        if rows == 1:
            freqs = folding.frequency_grid(5.0, 5.0 + 4095 / (8 * tobs), tobs)[:4096]

            def epoch():
                folding.frequency_search(x[0], TSAMP, freqs=freqs, nbin=32)
            epoch()
            ef = stats([wall(epoch) for _ in range(5)])
            blind = int(math.ceil((500.0 - 0.1) * 8 * tobs))
            rec["frequency_search_4096_trials"] = dict(
                ef, us_per_trial=round(ef["ms_median"] * 1e3 / 4096, 3), blind_trials_0p1_to_500hz=blind,
                blind_ms_extrapolated=round(ef["ms_median"] * blind / 4096, 1),
                over_periodicity_search=round(ef["ms_median"] * blind / 4096 / rec["periodicity_search"]["ms_median"], 1))
        result["rows"][str(rows)] = rec
        del x, spec, norm, ws, hws, cbuf
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "spectrum_bench.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
