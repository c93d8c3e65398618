"""GPU lab: the three fused optimizer steps over a full-fine-tune sized bucket (SD1.5 UNet: 859.5 M fp32 parameters, 3x3 conv weights
channels_last as HostBucket stores them; shapes from tests/golden/sd15_struct.json).

AdamW (csrc/optim.hip, the yardstick), Lion and Adafactor (csrc/optim_factored.hip) are timed in the same process on the same box with
hip events over ITERS steps each, every step on the other of two buffer sets (each set is tens of times the 256 MB of last-level cache, so
no step finds its operands cached).  Byte model per element: AdamW 32 B (p, m, v read + written, g read + cleared), Lion 24 B, Adafactor
28 B (pass 1 reads g, p; pass 2 reads g; pass 3 reads g, p, writes p, g) plus the factor state.  Adafactor's per-pass split comes from
the profiler's kernel table when it is available.

    python tools/bench_optim.py [--iters 10] [--out profiles/bench_optim.json]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hcp_diffusion_amd import kernels as K  # noqa: E402


def layout(shapes):
    """[(name, offset, shape, strides)] with 4-element segment padding, 3x3 weights channels_last."""
    rows, n = [], 0
    for name, shape in shapes.items():
        shape = tuple(shape)
        if len(shape) == 4 and shape[2:] == (3, 3):
            o, i = shape[0], shape[1]
            stride = (9 * i, 1, 3 * i, i)
        else:
            stride = tuple(math.prod(shape[k + 1:]) for k in range(len(shape)))
        rows.append((name, n, shape, stride))
        n += (math.prod(shape) + 3) // 4 * 4
    return rows, n


def timed(fn, iters):
    fn(0); fn(1)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i & 1)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "sd15_struct.json")))["shapes"]
    rows, n = layout(shapes)
    sets = []
    for _ in range(2):
        p = torch.randn(n, device=dev) * 0.05
        sets.append(dict(p=p, g=torch.empty(n, device=dev), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev),
                         table=K.AdafactorTable(rows, dev), step=torch.zeros(1, dtype=torch.int32, device=dev)))
    lr = torch.full((1,), 1e-6, dtype=torch.float32, device=dev)
    ss = torch.ones(1, dtype=torch.float32, device=dev)
    src = torch.randn(n, device=dev) * 1e-3

    def refill():
        for s in sets:
            s["g"].copy_(src)

    def adamw(k):
        s = sets[k]
        K.adamw_clip_fused(s["p"], s["g"], s["m"], s["v"], lr, s["step"], weight_decay=1e-3, sumsq_t=ss, max_norm=1.0)

    def lion(k):
        s = sets[k]
        K.lion_clip_fused(s["p"], s["g"], s["m"], lr, s["step"], weight_decay=1e-2, sumsq_t=ss, max_norm=1.0)

    def adafactor(k):
        s = sets[k]
        K.adafactor_step(s["p"], s["g"], s["table"], lr, s["step"], relative_step=False, weight_decay=1e-3, sumsq_t=ss, max_norm=1.0)

    res = {"n_params": n, "tensors": len(rows), "items": sets[0]["table"].items, "iters": args.iters}
    for name, fn, bytes_per in (("adamw", adamw, 32), ("lion", lion, 24), ("adafactor", adafactor, 28)):
        refill()                                              # (the steps clear g: zeros afterwards, same traffic)
        ms = timed(fn, args.iters)
        res[name] = {"ms": round(ms, 4), "GBps_model": round(bytes_per * n / ms / 1e6, 1)}
        print(f"{name}: {ms:.3f} ms  ({bytes_per} B/element -> {bytes_per * n / ms / 1e6:.0f} GB/s)", flush=True)
    res["lion_over_adamw"] = round(res["lion"]["ms"] / res["adamw"]["ms"], 4)
    res["adafactor_over_adamw"] = round(res["adafactor"]["ms"] / res["adamw"]["ms"], 4)
    try:                                                      # per-kernel split of the Adafactor step
        from torch.profiler import ProfilerActivity, profile
        refill()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for i in range(4):
                adafactor(i & 1)
            torch.cuda.synchronize()
        split = {}
        for e in prof.key_averages():
            if "af_" in e.key:
                split[e.key[:80]] = round(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)) / 4 / 1e3, 4)
        res["adafactor_split_ms"] = split
        for k_, v in split.items():
            print(f"  {k_}: {v} ms / step")
    except Exception as e:  # noqa: BLE001 - the split is a record, not a result
        res["adafactor_split_ms"] = f"profiler unavailable: {e}"
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
