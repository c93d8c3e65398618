"""GPU lab: what pyramid noise costs the captured step.  The headline LoRA configuration at B = 4 (SD1.5 architecture, random init,
rank-8 LoRA on attention + feed-forward, captured steps, as bench.py builds its headline leg) once with the plain step and once with
NativeTrainer(noise_cfg={'type': 'pyramid'}), both in one process on one box and timed ALTERNATELY, ROUNDS times STEPS steps each, with
a host clock around work that ends in a device synchronise; the spread of the plain step's rounds is the yardstick for the difference.

What the pyramid step adds: one randn for all level fields, the accumulate launch and the finish launch in place of add_noise (counted
below by running one eager make_noise of each trainer with its entry points wrapped), and, outside the graph, one 132-byte host-to-device
copy of the level table per step.

For comparison the same noise is also made the way a torch implementation makes it — per level one CPU randn, its copy to the device, one
F.interpolate, one multiply, one add; then std, a division and the add_noise formula — next to the native make_noise in eager mode.

    python tools/bench_noise.py [--steps 20] [--rounds 5] [--out profiles/bench_noise.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dreamartist import build  # noqa: E402
from hcp_diffusion_amd import kernels as K  # noqa: E402
from hcp_diffusion_amd.scheduler import pyramid_level_dims  # noqa: E402

PYRAMID = dict(type="pyramid", level=10, discount=0.9, step_size=2.0, resize_mode="bilinear")


def count_launches(tr, lat):
    """Device launches of one eager make_noise: calls of the torch generators and of the library's entry points it goes through."""
    names = [(torch, "randn"), (torch, "randn_like"), (torch, "randint"), (K, "add_noise"), (K, "pyramid_noise_accum"), (K, "pyramid_noise_finish")]
    n = [0]
    real = {}
    for mod, name in names:
        real[(mod, name)] = getattr(mod, name)
        setattr(mod, name, (lambda f: lambda *a, **k: (n.__setitem__(0, n[0] + 1), f(*a, **k))[1])(real[(mod, name)]))
    try:
        state = (random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state())
        tr.make_noise(lat)
        random.setstate(state[0]); torch.set_rng_state(state[1]); torch.cuda.set_rng_state(state[2])
    finally:
        for (mod, name), f in real.items():
            setattr(mod, name, f)
    return n[0]


def torch_style_noise(lat, acp, cfg):
    """The arithmetic of pyramid noise as plain torch calls: every level drawn on the CPU, resized, scaled and added by a launch each."""
    noise = torch.randn_like(lat)
    t = torch.randint(0, 1000, (lat.shape[0],), device=lat.device).long()
    b, c, h, w = noise.shape
    for i, (hn, wn) in enumerate(pyramid_level_dims(h, w, cfg["level"], cfg["step_size"]), start=1):
        noise += F.interpolate(torch.randn(b, c, hn, wn).to(noise), (h, w), None, cfg["resize_mode"]) * cfg["discount"] ** i
    normed = noise / noise.std()
    a = acp[t].view(-1, 1, 1, 1)
    return a ** 0.5 * lat + (1 - a) ** 0.5 * normed, noise, t


def eager_time(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_noise.py needs an MI355X (the product path has no CPU fallback)"
    dev = torch.device("cuda:0")
    B = 4
    legs = {"plain": build(dev), "pyramid": build(dev, noise_cfg=PYRAMID)}
    torch.manual_seed(1)
    random.seed(1)
    lat, ehs = torch.randn(B, 4, 64, 64, device=dev), torch.randn(B, 77, 768, device=dev).to(torch.bfloat16)
    launches = {name: count_launches(tr, lat) for name, tr in legs.items()}
    for tr in legs.values():
        for _ in range(args.warmup):
            tr.train_one_step(lat, ehs)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    losses, levels = {}, set()
    fill = legs["pyramid"]._pyramid.fill                  # (host side: which level counts the timed steps drew)
    legs["pyramid"]._pyramid.fill = lambda *a: (lambda dims: (levels.add(len(dims)), dims)[1])(fill(*a))
    for _ in range(args.rounds):                              # alternate the two legs: whatever else the host does hits both
        for name, tr in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = tr.train_one_step(lat, ehs)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            losses[name] = float(loss.item())
    res = {"steps": args.steps, "rounds": args.rounds, "batch": B, "launches_per_make_noise": launches,
           "launches_added_per_step": launches["pyramid"] - launches["plain"], "level_counts_seen": sorted(levels)}
    for name, ts in times.items():
        res[name] = {"ms_per_step_rounds": [round(v, 3) for v in ts], "ms_per_step_median": round(statistics.median(ts), 3),
                     "spread_ms": round(max(ts) - min(ts), 3), "last_loss": losses[name]}
        print(f"{name}: median {statistics.median(ts):.3f} ms/step, rounds {[round(v, 3) for v in ts]}", flush=True)
    diff = res["pyramid"]["ms_per_step_median"] - res["plain"]["ms_per_step_median"]
    res["pyramid_minus_plain_ms"] = round(diff, 3)
    res["within_plain_spread"] = bool(diff <= res["plain"]["spread_ms"])
    tr = legs["pyramid"]
    res["eager_make_noise_ms"] = {"native_pyramid": round(eager_time(lambda: tr.make_noise(lat), 200), 4),
                                  "torch_style_pyramid": round(eager_time(lambda: torch_style_noise(lat, tr.acp, PYRAMID), 200), 4),
                                  "native_plain": round(eager_time(lambda: legs["plain"].make_noise(lat), 200), 4)}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
