"""Cost of pu_quantize_pack_transpose (the requantise + transpose + pack of cleanup_data)
against the torch composition a user would otherwise write, on one GPU at the C4 cleaning
shape: a 1024 x 2^18 float64 plane to 8-bit and to 2-bit SIGPROC rows.

    (x * scale[:, None] + offset[:, None]).round().clamp(0, top).to(torch.uint8).T.contiguous()

followed, for packed output, by the shift-and-or of the channel groups.  HIP events, warm,
the variants interleaved over ROUNDS rounds in one process; prints one JSON line with the
median and the minimum of each and the kernel's read rate (input bytes / time), and checks
once that both give the same bytes.

    python scripts/quantize_cost.py [nchans] [log2 nsamps] [rounds]
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "radio-pulsar-utils_amd"), REPO]
import torch  # noqa: E402
from pulsarutils import sigproc  # noqa: E402

nchans = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
nsamps = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 18)
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(7)
# a renormalised plane ((x - mu) / mu of ~10 % noise) and cleanup_data's kind of levels
x = torch.randn((nchans, nsamps), dtype=torch.float64, device=dev, generator=gen) * 0.1
sig = 0.05 + 0.1 * torch.rand(nchans, dtype=torch.float64, device=dev, generator=gen)


def levels(nbits):
    mean, sigma = {8: (96.0, 16.0), 2: (1.5, 1.0)}[nbits]
    return sigma / sig, torch.full((nchans,), mean, dtype=torch.float64, device=dev)


def torch_composition(nbits, scale, offset):
    top = (1 << nbits) - 1
    q = (x * scale[:, None] + offset[:, None]).round().clamp(0, top).to(torch.uint8).T.contiguous()
    if nbits == 8:
        return q
    per = 8 // nbits
    g = q.view(nsamps, nchans // per, per)
    out = g[:, :, 0].clone()
    for j in range(1, per):
        out |= g[:, :, j] << (j * nbits)
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


res = {"what": "requantise + transpose (+ pack) of a float64 plane, one GPU, HIP events, warm",
       "nchans": nchans, "nsamps": nsamps, "rounds": rounds, "input_bytes": x.numel() * 8}
for nbits in (8, 2):
    scale, offset = levels(nbits)
    variants = {"kernel": lambda: sigproc.quantize_pack_device(x, nbits, scale, offset),
                "torch": lambda: torch_composition(nbits, scale, offset)}
    same = torch.equal(variants["kernel"](), variants["torch"]())
    for fn in variants.values():  # warm
        for _ in range(3):
            timed(fn)
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    r = {"same_bytes": same}
    for k, v in ms.items():
        r[f"{k}_ms_median"] = round(statistics.median(v), 4)
        r[f"{k}_ms_min"] = round(min(v), 4)
    r["kernel_read_TBps"] = round(x.numel() * 8 / statistics.median(ms["kernel"]) / 1e9, 3)
    r["torch_over_kernel"] = round(statistics.median(ms["torch"]) / statistics.median(ms["kernel"]), 2)
    res[f"nbits{nbits}"] = r
print(json.dumps(res))
