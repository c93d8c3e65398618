"""GPU lab: per-step wall time of the sampling loops around the native SD1.5 UNet (B = 4, 64 x 64 latents, guided, 20 steps).

One process, ROUNDS alternating rounds, a host clock around work that ends in a device synchronisation:
  (a) NativeDDIMSampler.sample — the eager loop with host-side timestep / cat / coefficients per step;
  (b) NativeEulerSampler.sample, eager — one fused kernel + one advance launch between UNet calls, no host arithmetic;
  (c) NativeEulerSampler.sample(use_graph=True) — one captured graph {UNet forward, step, advance} replayed per step;
  (d) 20 replays of a graph that holds the UNet forward alone — the floor of (c).
Aim 1: (c) below (a).  Aim 2: (c) - (d) within the run-to-run spread of (d).
The step kernel alone is timed with device events; at 65 536 floats it is launch latency, not bandwidth — no roofline fraction is claimed.

    python tools/bench_sampler.py [--steps 20] [--rounds 5] [--out profiles/bench_sampler.json]
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
from hcp_diffusion_amd.sampler import NativeDDIMSampler, NativeEulerSampler  # noqa: E402
from hcp_diffusion_amd.unet import NativeUNet2DConditionModel  # noqa: E402


def build_unet(dev):
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
    return unet.eval()


def unet_only_graph(unet, lat, ehs):
    """A graph of the guided UNet forward alone on static inputs: what a step costs when nothing surrounds the UNet."""
    xin = torch.cat([lat, lat])
    t = torch.full((xin.shape[0],), 500, dtype=torch.long, device=lat.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        unet(xin, t, ehs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            unet(xin, t, ehs)
    torch.cuda.current_stream().wait_stream(side)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sampler.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sampler.py needs an MI355X (the product path has no CPU fallback)"
    dev, B, n = torch.device("cuda:0"), a.batch, a.steps
    unet = build_unet(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(B, 4, 64, 64, device=dev, generator=g)
    cond, unc = (torch.randn(B, 77, 768, device=dev, generator=g) for _ in range(2))
    ddim, euler = NativeDDIMSampler(), NativeEulerSampler(seed=0)
    kw = dict(guidance_scale=7.5, num_inference_steps=n)
    ug = unet_only_graph(unet, lat, torch.cat([unc, cond]))

    def unet_only():
        for _ in range(n):
            ug.replay()
    legs = {"a_ddim_eager": lambda: ddim.sample(unet, lat, cond, unc, **kw),
            "b_euler_eager": lambda: euler.sample(unet, lat, cond, unc, **kw),
            "c_euler_graph": lambda: euler.sample(unet, lat, cond, unc, use_graph=True, **kw),
            "d_unet_graph_only": unet_only}
    for fn in legs.values():                               # warm-up (lazy packing, the capture of (c))
        fn()
    torch.cuda.synchronize()
    assert euler.captures == 1, "leg (c) did not capture"
    same = torch.equal(legs["b_euler_eager"](), legs["c_euler_graph"]())
    times = {k: [] for k in legs}
    for _ in range(a.rounds):                              # alternate the legs: whatever else the host does hits all of them
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / n * 1e3)
    res = {"what": f"per-step wall time, SD1.5 UNet, B={B}, 64x64 latents, guided, {n} steps, {a.rounds} alternating rounds, one process",
           "graph_equals_eager_bits": same, "captures": euler.captures}
    for name, ts in times.items():
        res[name] = {"ms_per_step_rounds": [round(v, 3) for v in ts], "ms_per_step_median": round(statistics.median(ts), 3),
                     "spread_ms": round(max(ts) - min(ts), 3)}
        print(f"{name}: median {statistics.median(ts):.3f} ms/step, rounds {[round(v, 3) for v in ts]}", flush=True)
    med = {k: res[k]["ms_per_step_median"] for k in legs}
    res["c_minus_d_ms"] = round(med["c_euler_graph"] - med["d_unet_graph_only"], 3)
    res["aim_c_below_a"] = "met" if med["c_euler_graph"] < med["a_ddim_eager"] else "MISSED"
    res["aim_c_minus_d_within_spread_of_d"] = "met" if res["c_minus_d_ms"] <= res["d_unet_graph_only"]["spread_ms"] else "MISSED"

    # the step kernel alone (device events over back-to-back launches): launch latency at this size, not bandwidth
    tab, st = euler.table(n).to(dev), K.sampler_state(0, dev)
    x, eps2, mi = lat.clone(), torch.randn(2 * B, 4, 64, 64, device=dev, generator=g), torch.empty(2 * B, 4, 64, 64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        K.euler_step(x, eps2, tab, st, 7.5, out=x, model_in_next=mi)
    torch.cuda.synchronize()
    iters = 200
    e0.record()
    for _ in range(iters):
        K.euler_step(x, eps2, tab, st, 7.5, out=x, model_in_next=mi)
    e1.record()
    torch.cuda.synchronize()
    res["step_kernel_alone_us"] = round(e0.elapsed_time(e1) / iters * 1e3, 2)
    res["step_kernel_note"] = "65 536 floats: launch latency bound; time only, no bandwidth or roofline figure"
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
