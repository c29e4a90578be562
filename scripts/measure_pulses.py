"""find_pulses at C2, piece by piece (HIP events, warm runs; profiles/pulses/README.md): the
search, the exact series of the selected trials, pu_series_events, the host clustering and the
whole call.  Run from the repository root.  `search-only` times plan.search alone; with
PULSARUTILS_HIP_LIB pointing at another build of the library it times that build's search."""
import json, statistics, sys, time
sys.path[:0] = ["radio-pulsar-utils_amd", "."]
import numpy as np
import torch
from pulsarutils import _hip, configs, dedispersion as dd, pulses, synth

cfg = configs.CONFIGS["C2"]
torch.cuda.set_device(0)
x = synth.pulsar_filterbank_device(cfg)
dms = dd.dedispersion_plan(cfg.nchan, cfg.dmmin, cfg.dmmax, cfg.start_freq, cfg.bandwidth, cfg.tsamp)
band = dict(start_freq=cfg.start_freq, bandwidth=cfg.bandwidth, sample_time=cfg.tsamp)
THR = 6.0


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        out = fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, statistics.median(ms), min(ms), max(ms)


outs, plan = dd.search_device(x, dms, cfg.nchan, **band)
ws = torch.empty(max(plan.workspace_bytes, 16), dtype=torch.uint8, device=x.device)
_, s_med, s_min, s_max = timed(lambda: plan.search(x, out=outs, workspace=ws), reps=10, warm=3)
res = {"lib": _hip._LIB_PATH, "ntrials": int(dms.size), "search_ms": [s_med, s_min, s_max]}
if len(sys.argv) > 1 and sys.argv[1] == "search-only":
    print(json.dumps(res))
    sys.exit(0)

snr = outs[2].cpu().numpy()
sel = np.flatnonzero(snr > THR * (1 - 1e-4)).astype(np.int32)
res["selected"] = int(sel.size)
res["snr_max"] = float(snr.max())
per = max(1, (1 << 30) // (24 * plan.nsamples))
res["batch_trials"] = per


def pieces():
    t_series = t_events = 0.0
    parts = []
    for b0 in range(0, sel.size, per):
        part = sel[b0:b0 + per]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        series = plan.exact_series(x, part)
        e[1].record()
        parts.append(_hip.series_events(series, THR, index=part))
        e[2].record()
        e[2].synchronize()
        t_series += e[0].elapsed_time(e[1])
        t_events += e[1].elapsed_time(e[2])
    return np.concatenate(parts), t_series, t_events


pieces()
runs = [pieces() for _ in range(3)]
events = runs[0][0]
res["events"] = int(events.size)
res["exact_series_ms"] = statistics.median(r[1] for r in runs)
res["series_events_ms"] = statistics.median(r[2] for r in runs)
cl = []
for _ in range(5):
    t0 = time.perf_counter()
    labels, reps = pulses.cluster_events(events)
    cl.append((time.perf_counter() - t0) * 1e3)
res["cluster_ms"] = statistics.median(cl)
res["pulses"] = int(reps.size)
tab, f_med, f_min, f_max = timed(lambda: pulses.find_pulses(x, dms, cfg.nchan, threshold=THR, plan=plan, **band),
                                 reps=3, warm=1)
res["find_pulses_total_ms"] = [f_med, f_min, f_max]
res["top"] = [{c: (np.asarray(tab[c])[i].item()) for c in tab.colnames} for i in range(min(3, len(tab)))]
print(json.dumps(res))
