"""GPU lab: what LoRA dropout costs the step, through torch's op and through the native kernel (csrc/dropout.hip).

The headline LoRA configuration at B = 4 (SD1.5 architecture, random init, rank-8 LoRA on attention + feed-forward, as bench.py builds
its headline leg) three times in one process on one box: (a) dropout 0, (b) dropout 0.1 through torch's dropout, (c) dropout 0.1 through
`NativeTrainer(native_dropout=seed)`.  Timed ALTERNATELY, ROUNDS times STEPS steps each, with a host clock around work that ends in a
device synchronise; (a) and (b) are the yardsticks, measured on the code path the parent commit has.  Aim 1: (c) - (a) < (b) - (a).

The same three under the loop of `bench.py --seam --seam-graph` (module call, MSE, backward, clip_grad_norm_, FusedAdamW, loss.item();
`unet.enable_hip_graph()`): with torch dropout the module is not capturable and runs eagerly.  Aim 2: with native dropout it replays.

The kernel alone against torch `dropout` + `ops.add` at the step's largest and smallest dropped shapes (recorded from one eager forward
of the model), with its achieved bytes/s against the 4 B/element model (read y, write out; 6 with the residual) and, as the yardstick
for memory-bound, hcp_add_bf16 and a device copy at the same shapes.

    python tools/bench_dropout.py [--steps 20] [--rounds 5] [--out profiles/bench_dropout.json]
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
from hcp_diffusion_amd import ops  # noqa: E402
from hcp_diffusion_amd.trainer import NativeTrainer  # noqa: E402
from hcp_diffusion_amd.unet import NativeUNet2DConditionModel  # noqa: E402

LORA_PATTERNS = [r"re:.*\.attn.?$", r"re:.*\.ff$"]      # cfgs/train/examples/lora_conventional.yaml:10-12
LEGS = {"a_dropout0": dict(dropout=0.0), "b_torch_dropout": dict(dropout=0.1), "c_native_dropout": dict(dropout=0.1, native_dropout=0)}


def build(dev, dropout, use_graph, native_dropout=None):
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
    tr = NativeTrainer(unet, [dict(layers=LORA_PATTERNS, rank=8, lr=1e-4, dropout=dropout)], lr=1e-4, weight_decay=1e-3, scale_lr_factor=4,
                       use_graph=use_graph, native_dropout=native_dropout)
    with torch.no_grad():
        for blk in tr.bucket.blocks:
            blk.layer.W_up.normal_(0, 0.02)
    tr.bucket.pack()
    return tr


def seam_stepper(tr, lat, ehs):
    """One step of the reference trainer's loop around the native module (bench.py seam_loop), the module replaying its captured pair
    when it is capturable."""
    from hcp_diffusion_amd.optim import FusedAdamW
    from hcp_diffusion_amd.scheduler import NativeDDPMScheduler
    unet, B = tr.unet, lat.shape[0]
    sched = NativeDDPMScheduler()
    params = [p for blk in tr.bucket.blocks for p in (blk.layer.W_down, blk.layer.W_up)]
    opt = FusedAdamW([dict(params=params, lr=1e-4 * B)], weight_decay=1e-3)
    crit = torch.nn.MSELoss(reduction="none")
    unet.enable_hip_graph()
    replayed = [None]

    def step():
        noise = torch.randn_like(lat)
        t = torch.randint(0, 1000, (B,), device=lat.device).long()
        pred = unet(sched.add_noise(lat, noise, t), t, ehs).sample
        replayed[0] = type(pred.grad_fn).__name__ == "_GraphedFnBackward"
        loss = crit(pred.float(), noise.float()).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        opt.zero_grad(set_to_none=False)
        return loss.item()
    return step, replayed


def alternate(steppers, rounds, steps, warmup):
    for fn in steppers.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times, last = {n: [] for n in steppers}, {}
    for _ in range(rounds):                                # alternate the legs: whatever else the host does hits all of them
        for name, fn in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                v = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
            last[name] = float(v)
    out = {}
    for name, ts in times.items():
        out[name] = {"ms_per_step_rounds": [round(v, 3) for v in ts], "ms_per_step_median": round(statistics.median(ts), 3),
                     "spread_ms": round(max(ts) - min(ts), 3), "last_loss": last[name]}
        print(f"{name}: median {statistics.median(ts):.3f} ms/step, rounds {[round(v, 3) for v in ts]}", flush=True)
    a, b, c = (out[n]["ms_per_step_median"] for n in LEGS)
    out["b_minus_a_ms"], out["c_minus_a_ms"] = round(b - a, 3), round(c - a, 3)
    out["aim_c_cheaper_than_b"] = "met" if c - a < b - a else "MISSED"
    return out


def device_ms(fn, iters):
    fn(0); fn(1)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def dropped_shapes(tr, lat, ehs):
    """(shape, with residual) of every layer output one eager training forward of `tr` hands to the native dropout kernel."""
    seen, real = [], ops.dropout_residual

    def spy(y, residual, *a, **k):
        seen.append((tuple(y.shape), residual is not None))
        return real(y, residual, *a, **k)
    ops.dropout_residual = spy
    try:
        saved = tr._snapshot()
        tr.forward_backward(lat, ehs)
        tr._restore(saved)
        tr.bucket.grads.zero_()
    finally:
        ops.dropout_residual = real
    return seen


def kernel_alone(dev, shape, iters=200, sets=4):
    """One dropped layer output of `shape`: the native kernel (forward with and without residual, backward) against torch dropout (+ ops.add),
    alternating `sets` buffer sets and writing into preallocated outputs.  Yardsticks for what the memory system gives a pointwise
    kernel of the same traffic at the same shape: hcp_add_bf16 (read two, write one: the 6 B/element model) and a device copy (read one,
    write one: the 4 B model).  A dropout time at its yardstick's means the Philox work hides under the traffic (memory-bound); a
    longer one is the integer VALU work showing."""
    n = 1
    for s in shape:
        n *= s
    ys = [torch.randn(shape, device=dev).to(torch.bfloat16) for _ in range(sets)]
    rs = [torch.randn(shape, device=dev).to(torch.bfloat16) for _ in range(sets)]
    outs = [torch.empty_like(ys[0]) for _ in range(sets)]
    st = K.dropout_state(0, dev)
    nat_res = device_ms(lambda i: K.dropout_residual_fwd(ys[i % sets], rs[i % sets], st, 3, 0, 0.1, out=outs[i % sets]), iters)
    nat = device_ms(lambda i: K.dropout_residual_fwd(ys[i % sets], None, st, 3, 0, 0.1, out=outs[i % sets]), iters)
    bwd = device_ms(lambda i: K.dropout_bwd(ys[i % sets], st, 3, 0, 0.1, out=outs[i % sets]), iters)
    add = device_ms(lambda i: K.add(ys[i % sets], rs[i % sets]), iters)
    cpy = device_ms(lambda i: outs[i % sets].copy_(ys[i % sets]), iters)
    tor_res = device_ms(lambda i: ops.add(torch.nn.functional.dropout(ys[i % sets], 0.1, True), rs[i % sets]), iters)
    tor = device_ms(lambda i: torch.nn.functional.dropout(ys[i % sets], 0.1, True), iters)
    gbs = lambda bytes_per, ms: round(n * bytes_per / (ms * 1e-3) / 1e9, 1)
    us = lambda ms: round(ms * 1e3, 2)
    return {"shape": list(shape), "elements": n, "buffer_set_MB": round(sets * 3 * n * 2 / 1e6, 1),
            "native_fwd_residual_us": us(nat_res), "native_fwd_us": us(nat), "native_bwd_us": us(bwd),
            "yardstick_add_bf16_us": us(add), "yardstick_copy_us": us(cpy),
            "torch_dropout_plus_add_us": us(tor_res), "torch_dropout_us": us(tor),
            "native_fwd_residual_GBps_of_6B_model": gbs(6, nat_res), "native_fwd_GBps_of_4B_model": gbs(4, nat),
            "native_bwd_GBps_of_4B_model": gbs(4, bwd), "add_bf16_GBps_of_6B_model": gbs(6, add), "copy_GBps_of_4B_model": gbs(4, cpy),
            "native_fwd_residual_over_add": round(nat_res / add, 3), "native_fwd_over_copy": round(nat / cpy, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dropout.py needs an MI355X (the product path has no CPU fallback)"
    dev = torch.device("cuda:0")
    B = 4
    torch.manual_seed(1)
    lat, ehs = torch.randn(B, 4, 64, 64, device=dev), torch.randn(B, 77, 768, device=dev).to(torch.bfloat16)
    res = {"steps": args.steps, "rounds": args.rounds, "batch": B}
    # 1. NativeTrainer, captured steps
    legs = {name: build(dev, use_graph=True, **kw) for name, kw in LEGS.items()}
    res["native_trainer_captured"] = alternate({n: (lambda tr=tr: tr.train_one_step(lat, ehs)) for n, tr in legs.items()},
                                               args.rounds, args.steps, args.warmup)
    res["dropped_layers"] = len(legs["c_native_dropout"].unet._hcp_dropout.blocks)
    del legs
    torch.cuda.empty_cache()
    # 2. the reference trainer's loop around the module with enable_hip_graph()
    legs = {name: build(dev, use_graph=False, **kw) for name, kw in LEGS.items()}
    shapes = dropped_shapes(legs["c_native_dropout"], lat, ehs)         # what the step really drops: taken from the model, not assumed
    seams = {n: seam_stepper(tr, lat, ehs) for n, tr in legs.items()}
    res["seam_graph_loop"] = alternate({n: s[0] for n, s in seams.items()}, args.rounds, args.steps, args.warmup)
    res["seam_graph_loop"]["replayed"] = {n: bool(s[1][0]) for n, s in seams.items()}
    res["seam_graph_loop"]["aim_native_dropout_replays"] = "met" if seams["c_native_dropout"][1][0] else "MISSED"
    del legs, seams
    torch.cuda.empty_cache()
    # 3. the kernel alone at the step's largest and smallest dropped outputs, and the traffic the step's dropped outputs add up to
    numel = lambda sh: int(torch.Size(sh).numel())
    elems = sum(numel(sh) for sh, _ in shapes)
    with_res = sum(numel(sh) for sh, r in shapes if r)
    res["dropped_outputs"] = {"calls_per_forward": len(shapes), "elements_per_forward": elems, "elements_with_residual": with_res,
                              "distinct_shapes": sorted({sh for sh, _ in shapes}, key=numel),
                              # forward 4 B/element (6 with residual) + backward 4 B/element
                              "model_bytes_per_step": 4 * (elems - with_res) + 6 * with_res + 4 * elems}
    largest, smallest = max((sh for sh, _ in shapes), key=numel), min((sh for sh, _ in shapes), key=numel)
    res["kernel_alone"] = [kernel_alone(dev, largest), kernel_alone(dev, smallest)]
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
