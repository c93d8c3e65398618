"""GPU lab: the DreamArtist step (NativeTrainer(cfg_scale='3.0')) on the headline LoRA configuration at B = 4 — a UNet batch of 8 —
against the plain step at B = 8, which is the same UNet work, and the CFG loss kernel (csrc/pointwise.hip cfg_mse_kernel) on its own.

Both trainers live in one process on one box (SD1.5 architecture, random init, rank-8 LoRA on attention + feed-forward, captured steps,
as bench.py builds its headline leg) and are timed ALTERNATELY, ROUNDS times STEPS steps each, with a host clock around work that ends in
a device synchronise; the spread of the plain step's rounds is the yardstick for the difference.  What the CFG step adds: one copy of the
noisy latents and timesteps, and a loss kernel over twice the elements.

Byte model of the kernel, per target element: pred2 read twice over (8 B), target read (4 B), grad2 written twice over (8 B) = 20 B; the
mask adds 4 B (C channels) or 4 / C B (one channel).  At the step's shape (B 4, 4 x 64 x 64: 1.3 MB) every operand sits in cache and the
time is that of two launches; the same kernel is therefore also timed at a shape past the 256 MB last-level cache, on alternating
buffer sets, where the byte model says something.

    python tools/bench_dreamartist.py [--steps 20] [--rounds 5] [--out profiles/bench_dreamartist.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hcp_diffusion_amd import kernels as K  # noqa: E402
from hcp_diffusion_amd.trainer import NativeTrainer  # noqa: E402
from hcp_diffusion_amd.unet import NativeUNet2DConditionModel  # noqa: E402

LORA_PATTERNS = [r"re:.*\.attn.?$", r"re:.*\.ff$"]      # cfgs/train/examples/lora_conventional.yaml:10-12


def build(dev, **kw):
    torch.manual_seed(114514)
    with torch.device("meta"):
        unet = NativeUNet2DConditionModel()
    unet = unet.to_empty(device=dev)
    with torch.no_grad():
        for name, p in unet.named_parameters():
            if p.dim() > 1:
                p.normal_(0, p[0].numel() ** -0.5)
            elif "norm" in name and name.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    tr = NativeTrainer(unet, [dict(layers=LORA_PATTERNS, rank=8, lr=1e-4)], lr=1e-4, weight_decay=1e-3, scale_lr_factor=4, use_graph=True, **kw)
    with torch.no_grad():
        for blk in tr.bucket.blocks:
            blk.layer.W_up.normal_(0, 0.02)
    tr.bucket.pack()
    return tr


def kernel_time(B, C, H, W, iters, dev, sets=2):
    """ms per call (device events) of K.cfg_mse_masked_mean with the gradient, alternating `sets` buffer sets."""
    bufs = [(torch.randn(2 * B, C, H, W, device=dev), torch.randn(B, C, H, W, device=dev)) for _ in range(sets)]
    t = torch.randint(0, 1000, (B,), device=dev)
    part = torch.empty(K.CFG_MSE_PARTIALS, device=dev)

    def call(k):
        p, y = bufs[k % sets]
        K.cfg_mse_masked_mean(p, y, t, (1.0, 3.0, "cos"), partials=part)
    call(0); call(1)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        call(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dreamartist.py needs an MI355X (the product path has no CPU fallback)"
    dev = torch.device("cuda:0")
    legs = {"plain_b8": (build(dev), 8, 8), "cfg_b4": (build(dev, cfg_scale="3.0"), 4, 8)}
    data = {}
    torch.manual_seed(1)
    for name, (tr, B, rows) in legs.items():
        data[name] = (torch.randn(B, 4, 64, 64, device=dev), torch.randn(rows, 77, 768, device=dev).to(torch.bfloat16))
        for _ in range(args.warmup):
            tr.train_one_step(*data[name])
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    losses = {}
    for _ in range(args.rounds):                              # alternate the two legs: whatever else the host does hits both
        for name, (tr, _, _) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = tr.train_one_step(*data[name])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            losses[name] = float(loss.item())
    res = {"steps": args.steps, "rounds": args.rounds, "unet_batch": 8}
    for name, ts in times.items():
        res[name] = {"ms_per_step_rounds": [round(v, 3) for v in ts], "ms_per_step_median": round(statistics.median(ts), 3),
                     "spread_ms": round(max(ts) - min(ts), 3), "last_loss": losses[name]}
        print(f"{name}: median {statistics.median(ts):.3f} ms/step, rounds {[round(v, 3) for v in ts]}", flush=True)
    diff = res["cfg_b4"]["ms_per_step_median"] - res["plain_b8"]["ms_per_step_median"]
    res["cfg_minus_plain_ms"] = round(diff, 3)
    res["within_plain_spread"] = bool(diff <= res["plain_b8"]["spread_ms"])
    for tag, shape, iters in (("kernel_step_shape", (4, 4, 64, 64), 2000), ("kernel_hbm_shape", (64, 4, 512, 512), 20)):
        ms = kernel_time(*shape, iters, dev)
        n = shape[0] * shape[1] * shape[2] * shape[3]
        res[tag] = {"B_C_H_W": list(shape), "ms": round(ms, 5), "model_bytes": 20 * n, "GBps_model": round(20 * n / ms / 1e6, 1)}
        print(f"{tag} {shape}: {ms * 1e3:.2f} us, 20 B/element -> {20 * n / ms / 1e6:.0f} GB/s", flush=True)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
