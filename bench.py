"""bench.py — training images/sec, SD1.5 LoRA (rank 8) 512px bs=4/GPU, bf16, on N MI355X (BASELINE.json metric).

  python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]            (N=1)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path (reference train_ac.py:467-504) over one synthetic batch already resident in
HBM: make_noise -> native UNet forward -> masked MSE -> backward (dX everywhere, LoRA wgrads) -> [RCCL all-reduce of
the flat LoRA gradient bucket] -> global-norm clip + AdamW -> re-pack LoRA operands.  Random-init weights of the
SD1.5 architecture, synthetic latents [4,4,64,64] and text states [4,77,768] (no datasets/checkpoints offline).
Gradient checkpointing is OFF (288 GB HBM holds the activations; the reference default ON is a memory workaround).
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line.  --full adds everything else: the box identity and
fp32-atomics self-check before the run, and after it the roofline kernels, the secondary legs (grad-ckpt on, frozen text
encoder in the step, the reference-style eager loop) and the `cpu_baseline` leg (N=1 only), which times the oracle —
checker code, never the product.  --dump-outputs DIR writes what the last timed step left its caller (dump_outputs).
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_IMAGE_LORA_NOCKPT = 1.61e12      # BASELINE.md §2 (fwd 803.3 G + dX backward 803.3 G + LoRA side paths)
FLOP_PER_IMAGE_SDXL_LORA_NOCKPT = 13.5e12 # SDXL fwd ~6.76 TFLOP/img @1024px, x2 (fwd + dX backward)
FLOP_PER_IMAGE_FULLFT_NOCKPT = 2.41e12    # full fine-tune, ckpt off (fwd + dX + dW)
FLOP_PER_IMAGE_CNET_NOCKPT = 2.18e12      # SURVEY §8d without recompute: base fwd 803 + branch fwd 285 + branch bwd 2x285 + decoder dX ~518
MFMA_BF16_PEAK = 2.5e15                   # MI355X_MICROARCH.md: dense bf16 MFMA
LORA_PATTERNS = [r"re:.*\.attn.?$", r"re:.*\.ff$"]      # cfgs/train/examples/lora_conventional.yaml:10-12
DUMP_BUDGET_ELEMS = 16 * 2 ** 20 - 1024   # --dump-outputs: at most 64 MB of float32 in all


def dump_outputs(path, loss, tr, moments=True):
    """--dump-outputs: what the last timed step handed its caller, as DIR/<name>.npy (float32): `loss`, and per trained flat bucket
    of the trainer (`lora_unet`, `host<i>` = full fine-tune / plugin buckets, `lora_te`) the updated fp32 parameters `<bucket>_params`
    and — moments=True, NativeTrainer's own optimizer — the AdamW first moment `<bucket>_exp_avg` the step wrote: the fused
    optimizer kernel clears the gradients, the moment carries them.  An array longer than its share of the 64 MB budget is
    written as the same fixed, seeded sample of its elements (sorted indices, seed 0) on every run."""
    import numpy as np
    states = ([("lora_unet", tr._lora_state)] if tr._lora_state is not None else []) + \
             [(f"host{i}", st) for i, st in enumerate(tr.host_buckets)] + \
             ([("lora_te", tr._te_state)] if tr._te_state is not None else [])
    arrays = [(f"{name}_params", st.bucket.params) for name, st in states]
    if moments:
        arrays += [(f"{name}_exp_avg", st.exp_avg) for name, st in states]
    cap = (DUMP_BUDGET_ELEMS - 1) // max(1, len(arrays))
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "loss.npy"), np.asarray([float(loss)], dtype=np.float32))
    for name, t in arrays:
        t = t.detach().reshape(-1)
        if t.numel() > cap:
            idx = torch.randint(0, t.numel(), (cap,), generator=torch.Generator().manual_seed(0)).sort().values
            t = t[idx.to(t.device)]
        np.save(os.path.join(path, f"{name}.npy"), t.float().cpu().numpy())


def _wrap_lora_for_baseline(m, rank):
    """LoRA on the oracle UNet: the REFERENCE's own LoraLayer / LoraPatchContainer (executed from /root/reference through
    oracle/ref_shims.py) where that tree exists (the build container), else the pinned restatement oracle/lora_ref.py."""
    from oracle.ref_shims import reference_available
    if reference_available():
        import re
        from oracle.ref_shims import load_reference_lora
        layers, _ = load_reference_lora()
        named = dict(m.named_modules())
        params = []
        for pat in LORA_PATTERNS:
            rx = re.compile(pat[3:])
            for name in [n for n in named if rx.match(n)]:
                parent_name, _, host_name = name.rpartition(".")
                made = layers.LoraLayer.wrap_model(0, named[name], parent_block=named[parent_name], host_name=host_name, rank=rank, dropout=0.0)
                for blk in made.values():
                    blk.requires_grad_(True)
                    params += list(blk.parameters())
        return params, "the reference's own LoraPatchContainer (hcpdiff/models/lora_base_patch.py via oracle/ref_shims.py)"
    from oracle.lora_ref import wrap_lora
    wr = wrap_lora(m, LORA_PATTERNS, rank=rank)
    return [p for w in wr.values() for p in w.lora_block_0.parameters()], "merged-weight LoRA restatement (oracle/lora_ref.py)"


def cpu_baseline(batch=4, steps=3, grad_ckpt=True, budget_s=240.0):
    """The reference-equivalent CPU path: oracle UNet (fp32 PyTorch restatement of diffusers) + merged-weight
    LoRA as the reference computes it + MSE + clip_grad_norm_ + torch AdamW, batch 4, gradient checkpointing as
    train_base.yaml:69 (per ResnetBlock2D / Transformer2DModel, non-reentrant: train_ac.py:44-47), on the host cores:
    one warm-up step at batch 1, then up to `steps` timed steps (fewer if the time budget runs out)."""
    import torch.nn.functional as F
    from torch.utils.checkpoint import checkpoint
    from oracle.unet_sd15 import OracleUNet2DConditionModel, ResnetBlock2D, Transformer2DModel, add_noise, ddpm_alphas_cumprod
    torch.manual_seed(0)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = max(1, min(cores, int(os.environ.get("OMP_NUM_THREADS") or cores), 64))   # OMP_NUM_THREADS caps it: a CPU quota can be smaller than the affinity mask
    torch.set_num_threads(cores)
    m = OracleUNet2DConditionModel()
    m.requires_grad_(False)
    params, lora_kind = _wrap_lora_for_baseline(m, 8)
    if grad_ckpt:
        for mod in m.modules():
            if isinstance(mod, (ResnetBlock2D, Transformer2DModel)):
                mod.forward = (lambda f: (lambda *a: checkpoint(f, *a, use_reentrant=False)))(mod.forward)
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-3)
    acp = ddpm_alphas_cumprod()

    def step(B):
        x0 = torch.randn(B, 4, 64, 64); ehs = torch.randn(B, 77, 768)
        noise = torch.randn_like(x0); t = torch.randint(0, 1000, (B,))
        xt = add_noise(x0, noise, t, acp).requires_grad_(grad_ckpt)   # non-reentrant checkpoints need a graph-connected input
        pred = m(xt, t, ehs).sample
        F.mse_loss(pred, noise).backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step(); opt.zero_grad(set_to_none=True)
    step(1)                                        # warm-up (thread pool, allocator)
    t0, done = time.time(), 0
    while done < steps and (done == 0 or (time.time() - t0) * (done + 1) / done < budget_s):
        step(batch); done += 1
    dt = (time.time() - t0) / done
    return {"value": round(batch / dt, 4), "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{done} LoRA(r=8) training steps at batch {batch} after 1 warm-up step, 512px latents, fp32 oracle UNet + {lora_kind}, "
                      f"gradient checkpointing {'on' if grad_ckpt else 'off'}, torch {torch.__version__} CPU kernels ({dt:.1f} s/step)"}


def _pmc_record(kernel_key):
    """HBM bytes per launch of the roofline kernel from the committed PMC passes (profiles/pmc_roofline.json, written by
    tools/pmc_roofline.py from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs; rocprofv3 cannot nest inside this process)."""
    path = os.path.join(ROOT, "profiles", "pmc_roofline.json")
    if not os.path.exists(path):
        return None
    try:
        rec = json.load(open(path)).get(kernel_key)
    except (OSError, ValueError):
        return None
    return rec


def _time_rotating(calls, rounds=3):
    """Average seconds per call of `calls` (one closure per DISTINCT operand set, together larger than the 256 MB Infinity Cache)
    launched round-robin on torch's current stream between two HIP events: every launch reads its operands from HBM / a cold L2,
    as inside the training step — the same command under `rocprofv3 --kernel-trace` gives the per-launch durations committed in
    profiles/ (a loop over ONE 10 MB operand set read 8 % faster than the trace)."""
    for c in calls:
        c()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        for c in calls:
            c()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / (rounds * len(calls))


def dominant_kernel_roofline(dev):
    """The dominant kernel of the step is the implicit-GEMM 3x3 convolution (41% of the FLOPs); its most frequent
    instance is C320->320 at 64x64, batch 4.  Timed with HIP events on the stream it is launched on, over 24 rotating operand
    sets (24 x 12.3 MB of inputs = 296 MB; the output block is the allocator's)."""
    from hcp_diffusion_amd import kernels as K
    B, H, C = 4, 64, 320
    sets = [(torch.randn(B, H, H, C, device=dev).to(torch.bfloat16), (torch.randn(C, 3, 3, C, device=dev) * 0.02).to(torch.bfloat16)) for _ in range(24)]
    dt = _time_rotating([(lambda x=x, w=w: K.conv3x3(x, w, C)) for x, w in sets], rounds=2)
    flops = 2.0 * B * H * H * C * 9 * C
    ach = flops / dt / 1e12
    out = {"bound": "mfma", "kernel": "implicit-GEMM conv3x3 C320->320 @64x64, B=4 (gemm_pp_kernel<128,160,MODE 1, ring 4>)", "achieved": round(ach, 1),
           "peak": MFMA_BF16_PEAK / 1e12, "unit": "TFLOP/s", "frac": round(ach * 1e12 / MFMA_BF16_PEAK, 4),
           "algorithmic_bytes": 22.8e6, "avg_launch_us": round(dt * 1e6, 1), "timing": "HIP events, 24 rotating operand sets (296 MB of inputs), 48 launches",
           "traffic": None}
    rec = _pmc_record("conv3x3_c320_64x64_b4")
    if rec:                                        # FETCH_SIZE x 2 (gfx950 wide-read correction) + WRITE_SIZE, bytes per launch
        out["traffic"] = rec["hbm_bytes_per_launch"]
        out["traffic_source"] = f"profiles/pmc_roofline.json ({rec.get('source', '?')}, kernel sources at git {rec.get('git', '?')})"
        if rec.get("avg_launch_us_in_step") is not None:
            out["avg_launch_us_in_step"] = rec["avg_launch_us_in_step"]       # the same kernel template cut out of the captured step's trace
        if rec.get("us_rocprof_trace") is not None:                           # rocprofv3 --kernel-trace reads this kernel 7-10 % longer than events do
            out["avg_launch_us_rocprof_trace"] = rec["us_rocprof_trace"]      # (same box: 36.3 us with events, 39.9 us median under the tracer)
    return out


def family_roofline(batch):
    """`roofline_family` (VERDICT r5 next #4d): the algorithmic FLOPs of the two MFMA families of the SD1.5 LoRA step divided by the
    time their kernels take inside the captured step, from the committed rocprofv3 step summary (profiles/pmc_roofline.json "families",
    written by tools/pmc_roofline.py) — the `roofline` object above is the BEST kernel of the GEMM family, this is the family.
    FLOPs per image: UNet forward 803.3 G of which the attention cores 122.5 G; backward = the input-gradient
    pass (x 1 for GEMMs / convs, x 2.5 for the attention cores)."""
    rec = _pmc_record("families")
    if not rec or not rec.get("gemm_ms") or not rec.get("attention_ms"):
        return None
    gemm_flops = (803.3e9 - 122.5e9) * 2 * batch
    attn_flops = 122.5e9 * 3.5 * batch
    out = {"bound": "mfma", "peak": MFMA_BF16_PEAK / 1e12, "unit": "TFLOP/s", "batch": batch,
           "source": f"{rec.get('source')} (kernel sources at git {rec.get('git', '?')}); {rec.get('dispatches_per_step')} dispatches, "
                     f"{rec.get('kernel_ms_per_step')} ms of kernel time per step under the profiler"}
    for name, fl, ms, n in (("gemm_and_conv", gemm_flops, rec["gemm_ms"] + rec.get("splitk_reduce_ms", 0.0), rec.get("gemm_launches")),
                            ("attention", attn_flops, rec["attention_ms"], rec.get("attention_launches"))):
        ach = fl / (ms * 1e-3) / 1e12
        out[name] = {"flops_per_step": fl, "ms_per_step": round(ms, 3), "launches_per_step": n, "achieved": round(ach, 1),
                     "frac": round(ach * 1e12 / MFMA_BF16_PEAK, 4)}
    return out


def attention_roofline(dev):
    """Secondary roofline line, the north-star's named kernel: self-attention forward at the 64x64 level (B4 H8 N4096 d40)."""
    from hcp_diffusion_amd import kernels as K
    B, H, N, D = 4, 8, 4096, 40
    sets = []
    for _ in range(16):                            # 16 x (q, k, v, o) = 336 MB
        q, k, v = [torch.randn(B, N, H * D, device=dev).to(torch.bfloat16) for _ in range(3)]
        q = (q.float() * (D ** -0.5 * 1.4426950408889634)).to(torch.bfloat16)  # the form the UNet's attention modules call the kernel in:
        sets.append((q, k, v))                                                  # q * d^-0.5 * log2(e) out of the q|k|v projection group
    dt = _time_rotating([(lambda q=q, k=k, v=v: K.attention_fwd(q, k, v, H, q_prescaled=True)) for q, k, v in sets], rounds=2)
    flops = 4.0 * B * H * N * N * D
    out = {"kernel": "attn2_fwd_kernel<40,2,8 waves, pre-scaled Q, row-sum lazy rescale> B4 H8 N4096 d40", "achieved": round(flops / dt / 1e12, 1), "unit": "TFLOP/s",
           "frac": round(flops / dt / MFMA_BF16_PEAK, 4), "avg_launch_us": round(dt * 1e6, 1), "timing": "HIP events, 16 rotating operand sets, 32 launches"}
    rec = _pmc_record("attn_fwd_b4_h8_n4096_d40")
    if rec:
        out["mfma_busy"] = rec.get("mfma_busy"); out["traffic"] = rec.get("hbm_bytes_per_launch")
        out["traffic_source"] = f"profiles/pmc_roofline.json ({rec.get('source', '?')})"
        if rec.get("avg_launch_us_in_step") is not None:
            out["avg_launch_us_in_step"] = rec["avg_launch_us_in_step"]
    # the backward of the same problem (two launches: dQ, which also produces delta, then dK/dV), 2.5x the forward's FLOPs
    outs = [K.attention_fwd(q, k, v, H, q_prescaled=True) for q, k, v in sets]
    dos = [torch.randn(B, N, H * D, device=dev).to(torch.bfloat16) for _ in range(4)]
    db = _time_rotating([(lambda i=i: K.attention_bwd(*sets[i], outs[i][0], dos[i % 4], outs[i][1], H, q_prescaled=True)) for i in range(len(sets))], rounds=2)
    bwd = {"kernels": "attn2_bwd_dq_kernel<40,2> + attn2_bwd_dkv_kernel<40,2>", "avg_us_both_launches": round(db * 1e6, 1),
           "achieved": round(2.5 * flops / db / 1e12, 1), "frac": round(2.5 * flops / db / MFMA_BF16_PEAK, 4)}
    for key, name in (("attn_dq_b4_h8_n4096_d40", "dq"), ("attn_dkv_b4_h8_n4096_d40", "dkv")):
        r2 = _pmc_record(key)
        if r2:
            bwd[name] = {"mfma_busy": r2.get("mfma_busy"), "us_rocprof_trace": r2.get("us_rocprof_trace"), "avg_launch_us_in_step": r2.get("avg_launch_us_in_step")}
    out["backward"] = bwd
    return out


def main(emu=False):
    """emu=True is passed only by tests/emu/bench_emu.py, which has pointed hcp_diffusion_amd.kernels at the CPU interpreter build first: the
    same launcher, rank plumbing, trainer and JSON line with gloo and a two-level miniature UNet, so that the first multi-rank run of
    this file is not the one on the driver's 8-GPU node.  Timings of such a run mean nothing and the line says so."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", choices=["sd15", "sdxl", "dreambooth", "controlnet", "sd15te"], default="sd15",
                    help="sd15 = the headline metric (BASELINE.json configs[1]); sdxl = configs[3] (SDXL LoRA r16 1024px bs2); "
                         "dreambooth = configs[2] (SD1.5 full fine-tune, all 859.5 M parameters, bs2); controlnet = configs[4] (frozen SD1.5 + "
                         "trainable ControlNet branch, bs4); sd15te = the reference's default LoRA example, lora_unet r8 + "
                         "lora_text_encoder r4 with the prompt encoded inside the step (lora_conventional.yaml) — secondary lines")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--rank-lora", type=int, default=None)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true", help="also the box identity + atomics self-check, the roofline kernels, the secondary legs "
                    "and the CPU baseline (a plain run times the headline steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the loss and trained buckets of the last timed step as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-ckpt-line", action="store_true", help="with --full: skip the secondary grad-ckpt-on measurement (profiling runs)")
    ap.add_argument("--overlap", action="store_true", help="LoRA wgrad kernels on a side stream (measured slower)")
    ap.add_argument("--no-grouped-wgrad", action="store_true", help="one wgrad launch per layer instead of one grouped launch")
    ap.add_argument("--residual-stream", choices=["auto", "on", "off"], default="auto",
                    help="(hi | lo) residual stream of the transformer blocks (unet.set_residual_stream): auto = stacks of >= 2 blocks (SDXL)")
    ap.add_argument("--geglu-epilogue", action="store_true", help="opt-in: GEGLU product in the FF projection's epilogue (unet.set_geglu_epilogue; measured slower)")
    ap.add_argument("--grad-ckpt", action="store_true", help="enable_gradient_checkpointing() as the reference defaults to "
                    "(train_base.yaml:69): +1 forward per step; a secondary line, the headline runs without (288 GB HBM)")
    ap.add_argument("--seam", action="store_true", help="secondary line: time the step the way the REFERENCE's Trainer drives the native "
                    "modules (train_ac.py:467-504 restated: eager module calls, torch autograd, clip_grad_norm_, optimizer.step(), "
                    "zero_grad, loss.item() every step) instead of NativeTrainer's captured step; sd15 workload, 1 GPU")
    ap.add_argument("--seam-optimizer", choices=["fused", "torch"], default="fused")
    ap.add_argument("--seam-graph", action="store_true", help="with --seam: unet.enable_hip_graph() — the module replays captured forward / "
                    "backward hipGraphs under the same eager trainer loop")
    ap.add_argument("--comm", choices=["torch", "abi"], default=os.environ.get("HCP_COMM", "torch"),
                    help="gradient exchange: torch.distributed (backend nccl = RCCL) or RCCL through the C ABI (hcp_allreduce_flat / "
                         "hcp_reduce_scatter_flat / hcp_allgather_flat, csrc/comm.hip)")
    ap.add_argument("--exchange", choices=["plain", "overlap", "overlap-bf16"], default="plain",
                    help="sharded host buckets (dreambooth / controlnet, N > 1): 'overlap' = chunks reduce-scattered from backward on a side "
                         "stream; 'overlap-bf16' = also bf16 gradients and parameters on the wire (DDP bf16_compress_hook numerics)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher — one process per GPU, as the reference's
        # `accelerate launch -m hcpdiff.train_ac` does (README.md:85-92, train_ac.py:117-128)
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(sys.argv[0])] + sys.argv[1:]
        os.execv(sys.executable, cmd)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)")
    if emu:                                        # tests/emu/bench_emu.py (the launcher / rank plumbing on the CPU interpreter): see main()'s docstring
        dev = torch.device("cpu")
        args.no_graph, args.no_cpu_baseline, args.no_ckpt_line = True, True, True
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            torch.distributed.init_process_group("gloo")
    else:
        assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (the product path has no CPU fallback)"
        assert torch.cuda.device_count() >= (args.gpus if world > 1 else 1), \
            f"--gpus {args.gpus} but only {torch.cuda.device_count()} visible"
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            torch.distributed.init_process_group("nccl", device_id=dev)       # nccl == RCCL on ROCm
    if world > 1:
        assert torch.distributed.get_world_size() == args.gpus

    if not emu and args.full:
        # which box is this, and do its fp32 atomic adds add?  (one box of round 5 gave wrong sums in every atomics-based
        # kernel for the length of a process; a run on such a box stops here, with the box's identity in the log)
        from hcp_diffusion_amd import kernels as _K
        if rank == 0:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            try:
                from box_info import box_info
                print(f"[bench] box: {json.dumps(box_info(local_rank))}", file=sys.stderr, flush=True)
            except Exception as e:  # noqa: BLE001 - identification only
                print(f"[bench] box identification failed: {e}", file=sys.stderr, flush=True)
        _K.atomics_selfcheck(dev)
    from hcp_diffusion_amd.comm import make_comm
    from hcp_diffusion_amd.trainer import NativeTrainer
    from hcp_diffusion_amd.unet import SDXL_CONFIG, NativeUNet2DConditionModel
    comm = make_comm(dev, kind=args.comm) if world > 1 else None

    sdxl = args.workload == "sdxl"
    fullft = args.workload == "dreambooth"
    cnet = args.workload == "controlnet"
    te = args.workload == "sd15te"
    args.batch = args.batch or (2 if (sdxl or fullft) else 4)
    args.rank_lora = args.rank_lora or (16 if sdxl else 8)
    torch.manual_seed(114514)                      # same weights on every rank (train_base.yaml:5)
    lat_hw, ctx_dim = (128 if sdxl else 64), (2048 if sdxl else 768)
    if emu:                                        # two-level miniature with the SD1.5 block types (head dims 40 / 80), 8x8 latents
        lat_hw, ctx_dim = 8, 32
        cfg = dict(block_out_channels=(40, 80), layers_per_block=1, num_attention_heads=1, cross_attention_dim=32, norm_num_groups=8,
                   down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
        unet = NativeUNet2DConditionModel(**cfg)
    else:
        with torch.device("meta"):
            unet = NativeUNet2DConditionModel(**SDXL_CONFIG) if sdxl else NativeUNet2DConditionModel()
        unet = unet.to_empty(device=dev)
    with torch.no_grad():                          # random-init weights of the SD1.5 architecture, generated on the GPU
        for name, p in unet.named_parameters():
            if p.dim() > 1:
                p.normal_(0, p[0].numel() ** -0.5)
            elif "norm" in name and name.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    if args.grad_ckpt:
        unet.enable_gradient_checkpointing()
    if args.residual_stream != "auto":
        unet.set_residual_stream(args.residual_stream == "on")
    if args.geglu_epilogue:
        unet.set_geglu_epilogue(True)
    plugin_input = None
    frozen_te_leg = False
    xkw = dict(overlap_exchange=args.exchange != "plain", **(dict(grad_wire="bf16", param_wire="bf16") if args.exchange == "overlap-bf16" else {}))
    if os.environ.get("HCP_BENCH_FORCE_SHARD") == "1" and world == 1:      # lab: the sharded machinery's own cost (casts, chunked launches,
        xkw["shard_optimizer"] = "force"                                   # side-stream branch) on one GPU, collectives = copies
    if cnet:                                       # cfgs/plugins/plugin_controlnet.yaml: frozen host + trainable branch, lr 1e-4
        from hcp_diffusion_amd.controlnet import make_controlnet
        plug = make_controlnet(unet)
        with torch.no_grad():                      # zero convs leave a freshly built branch without gradient flow upstream:
            for m in list(plug.controlnet_down_blocks) + [plug.controlnet_mid_block, plug.cond_head[-1]]:
                m.weight.normal_(0, 0.02)          # time the steady state ("after some training") instead
        tr = NativeTrainer(unet, None, lr=1e-4, weight_decay=1e-3, scale_lr_factor=args.batch * world, use_graph=not args.no_graph,
                           plugins=[(plug, 1e-4)], comm=comm, **xkw)
        torch.manual_seed(114514 + rank)
        plugin_input = dict(cond=torch.rand(args.batch, 3, 512, 512, device=dev))
    elif fullft:                                   # cfgs/train/examples/DreamBooth.yaml:6-10: unet: [{lr: 1e-6, layers: ['']}]
        tr = NativeTrainer(unet, None, lr=1e-6, weight_decay=1e-3, scale_lr_factor=args.batch * world, use_graph=not args.no_graph,
                           train_cfg=[dict(layers=[""], lr=1e-6)], comm=comm, **xkw)
        torch.manual_seed(114514 + rank)
    else:
        text_encoder = None
        frozen_te_leg = (args.full and args.workload == "sd15" and world == 1 and not emu and not args.no_ckpt_line and not args.no_graph and not args.seam)

        def build_clip():                          # CLIP-L text encoder (cfgs/te_struct.txt), random init
            from hcp_diffusion_amd.text_encoder import NativeCLIPTextModel
            with torch.device("meta"):
                enc = NativeCLIPTextModel()
            enc = enc.to_empty(device=dev)
            with torch.no_grad():
                for name, p in enc.named_parameters():
                    if "embedding" in name:
                        p.normal_(0, 0.02)
                    elif p.dim() > 1:
                        p.normal_(0, p[0].numel() ** -0.5)
                    elif "norm" in name and name.endswith("weight"):
                        p.fill_(1.0)
                    else:
                        p.zero_()
            return enc
        if te:                                     # sd15te: + lora_text_encoder rank 4 lr 1e-5 (the frozen-TE secondary leg of the headline
            text_encoder = build_clip()            # builds its encoder AFTER the headline loop: the timed process is the one of rounds 1-4)
        tr = NativeTrainer(unet, [dict(layers=LORA_PATTERNS, rank=args.rank_lora, lr=1e-4)], lr=1e-4, weight_decay=1e-3,
                           scale_lr_factor=args.batch * world, use_graph=not args.no_graph, overlap_wgrad=args.overlap,
                           grouped_wgrad=not args.no_grouped_wgrad, text_encoder=text_encoder,
                           lora_te_cfg=[dict(layers=[r"re:.*self_attn$", r"re:.*mlp$"], rank=4, lr=1e-5)] if te else None, comm=comm)
        torch.manual_seed(114514 + rank)           # set_seed(seed + local_rank), train_ac.py:128
        buckets = [tr.bucket] + ([tr.te_bucket] if te else [])
        with torch.no_grad():                      # non-zero W_up so every LoRA path carries signal
            for bk in buckets:
                for blk in bk.blocks:
                    blk.layer.W_up.normal_(0, 0.02)
        for bk in buckets:
            if world > 1:                          # identical LoRA init on every rank (DDP broadcasts rank 0's)
                torch.distributed.broadcast(bk.params, 0)
            bk.pack()
    B = args.batch
    added = None
    if sdxl:                                       # [2,4,128,128], ctx [2,77,2048], pooled [2,1280], crop_info [2,6]
        latents = torch.randn(B, 4, lat_hw, lat_hw, device=dev)
        ehs = torch.randn(B, 77, ctx_dim, device=dev).to(torch.bfloat16)
        added = dict(text_embeds=torch.randn(B, 1280, device=dev),
                     time_ids=torch.tensor([[1024.0, 1024.0, 0.0, 0.0, 1024.0, 1024.0]] * B, device=dev))
    else:
        latents = torch.randn(B, 4, lat_hw, lat_hw, device=dev)
        ehs = torch.randn(B, 77, ctx_dim, device=dev).to(torch.bfloat16)

    prompt_ids = None
    if te:                                         # random token ids in [0, 49407], BOS / EOS at the ends; no precomputed states
        prompt_ids = torch.randint(0, 49406, (B, 77), device=dev)
        prompt_ids[:, 0] = 49406; prompt_ids[:, -1] = 49407
        ehs = None

    def sync():
        if world > 1:
            torch.distributed.barrier()
        if not emu:
            torch.cuda.synchronize()

    def seam_loop(graph, steps, warmup):
        """What the reference's Trainer does with the native modules behind its seams (tests/test_reference_trainer.py runs its
        real code on the CPU interpreter; /root/reference does not exist on the GPU box, so the loop is restated here):
        TEUnetWrapper-style module call, MSE(reduction none).mean(), loss.backward(), accelerator.clip_grad_norm_,
        optimizer.step(), zero_grad(set_to_none=False), loss.item().  graph: unet.enable_hip_graph().  -> (seconds, last loss)"""
        from hcp_diffusion_amd.optim import FusedAdamW
        from hcp_diffusion_amd.scheduler import NativeDDPMScheduler
        sched = NativeDDPMScheduler()
        if fullft:                                 # DreamBooth.yaml:6-10: every UNet parameter (the flat HostBucket NativeTrainer built is reused by the module graph)
            params = [p for p in unet.parameters() if p.requires_grad]
        else:
            params = [p for blk in tr.bucket.blocks for p in (blk.layer.W_down, blk.layer.W_up)]
        opt = (FusedAdamW if args.seam_optimizer == "fused" else torch.optim.AdamW)([dict(params=params, lr=(1e-6 if fullft else 1e-4) * B)], weight_decay=1e-3)
        crit = torch.nn.MSELoss(reduction="none")
        if graph:
            unet.enable_hip_graph()
        def seam_step():
            noise = torch.randn_like(latents)
            t = torch.randint(0, 1000, (B,), device=dev).long()
            pred = unet(sched.add_noise(latents, noise, t), t, ehs).sample
            loss = crit(pred.float(), noise.float()).mean()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)              # accelerator.clip_grad_norm_(TE_unet.trainable_parameters(), ...), train_ac.py:485-490
            opt.step()
            opt.zero_grad(set_to_none=False)
            return loss.item()
        for _ in range(warmup):
            seam_step()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            lv = seam_step()
        sync()
        return time.perf_counter() - t0, lv

    if args.seam:
        assert args.workload in ("sd15", "dreambooth") and world == 1
        dt, lv = seam_loop(args.seam_graph, args.steps, args.warmup)
        if not math.isfinite(lv):
            raise RuntimeError(f"bench.py --seam: the training loss after the timed loop is not finite ({lv}): the measurement is void")
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, lv, tr, moments=False)      # (the eager loop's optimizer keeps its own moments)
        print(json.dumps({"metric": ("training images/sec, SD1.5 full fine-tune (DreamBooth) 512px bs=%d" % B if fullft else "training images/sec, SD1.5 LoRA 512px bs=4") +
                                    ", native modules driven the reference trainer's way (eager seam)",
                          "value": round(B * args.steps / dt, 2), "unit": "images/sec", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(dt / args.steps * 1e3, 3), "optimizer": args.seam_optimizer, "unet_hip_graph": bool(args.seam_graph),
                          "final_loss": round(lv, 5),
                          "config": {"workload": ("SD1.5 UNet full fine-tune bf16 bs=%d" % B if fullft else "SD1.5 UNet LoRA rank=%d bf16 bs=%d" % (args.rank_lora, B)) +
                                     ", eager loop, clip_grad_norm_ + %s AdamW + loss.item() per step" % args.seam_optimizer}}), flush=True)
        return
    for _ in range(args.warmup):
        tr.train_one_step(latents, ehs, None, added, plugin_input, prompt_ids)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.train_one_step(latents, ehs, None, added, plugin_input, prompt_ids)
    sync()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], device=dev)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = tmax.item()
    loss_v = float(loss.item())
    # (round 5: NaN losses in some graph-replay runs went unnoticed for three rounds because nobody read `final_loss` — LAB_NOTEBOOK.
    #  The line now says so itself: `loss_finite`, and `invalid` when it is not — such a run's timing is void, the exp2-overflow
    #  fallback of the attention forward alone makes its steps slower)
    loss_ok = math.isfinite(loss_v)
    if not loss_ok:
        print(f"bench.py: the training loss after the timed loop is not finite ({loss_v}): the measurement is void", file=sys.stderr, flush=True)
    if rank == 0 and args.dump_outputs:            # before any --full leg trains further
        dump_outputs(args.dump_outputs, loss_v, tr)
    if rank == 0:
        ips = world * B * args.steps / dt
        out = {
            "metric": ("training images/sec (whole node), SDXL LoRA 1024px bs=%d/GPU" % B) if sdxl else
                      ("training images/sec (whole node), SD1.5 full fine-tune (DreamBooth) 512px bs=%d/GPU" % B) if fullft else
                      ("training images/sec (whole node), SD1.5 + ControlNet branch training 512px bs=%d/GPU" % B) if cnet else
                      ("training images/sec (whole node), SD1.5 LoRA on UNet + text encoder 512px bs=%d/GPU" % B) if te else
                      "training images/sec (whole node), SD1.5 LoRA 512px bs=4/GPU", "value": round(ips, 2) if loss_ok else None, "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": ("SDXL-base UNet LoRA rank=%d bf16, bs=%d/GPU, 1024x1024 (128x128 latents), 77x2048 context + text_time "
                                    "cond, random-init weights, cached latents, grad-ckpt off" % (args.rank_lora, B) if sdxl else
                                    "SD1.5 UNet full fine-tune (all 859.5 M params, fp32 masters + AdamW), bf16 compute, bs=%d/GPU, "
                                    "512x512, 77-token context, random-init weights, cached latents, grad-ckpt off" % B if fullft else
                                    "frozen SD1.5 UNet + trainable ControlNet branch (361 M params, fp32 masters + AdamW), bf16 compute, "
                                    "bs=%d/GPU, 512x512 + control image [B,3,512,512], random-init weights, grad-ckpt off" % B if cnet else
                                    "SD1.5 UNet LoRA rank=%d + CLIP-L text-encoder LoRA rank=4 (prompt encoded inside the step, gradient through "
                                    "the cross-attention K/V projections), bf16, bs=%d/GPU, 512x512, random-init weights, cached latents, "
                                    "grad-ckpt off" % (args.rank_lora, B) if te else
                                    "SD1.5 UNet LoRA rank=%d bf16, bs=%d/GPU, 512x512 (64x64 latents), 77-token context, "
                                    "random-init weights, cached latents, grad-ckpt off" % (args.rank_lora, B)),
                       "global_batch": B * world, "parallelism": f"dp{world}", "rccl_ranks": world, **({"exchange": args.exchange} if (fullft or cnet) else {}),
                       "comm": ("RCCL via " + ("C ABI (hcp_allreduce_flat)" if args.comm == "abi" else "torch.distributed")) if world > 1 else "none",
                       "hip_graph": not args.no_graph,
                       "gradient_checkpointing": bool(args.grad_ckpt)},
            "final_loss": round(loss_v, 5) if loss_ok else None, "loss_finite": loss_ok, **({} if loss_ok else {"invalid": "non-finite training loss"}),
            "step_mfma_frac": round(ips / world * (FLOP_PER_IMAGE_SDXL_LORA_NOCKPT if sdxl else FLOP_PER_IMAGE_FULLFT_NOCKPT if fullft
                                                   else FLOP_PER_IMAGE_CNET_NOCKPT if cnet
                                                   else FLOP_PER_IMAGE_LORA_NOCKPT) / MFMA_BF16_PEAK, 4),
        }
        if args.full and not emu:
            # the two roofline kernels are timed HERE, straight after the headline loop: after the grad-ckpt leg below (graphs re-captured,
            # pools released) the caching allocator answers the per-call output allocations with fresh hipMallocs and the 37 us convolution
            # reads 48-60 us (measured, same box, same binary)
            roof, roof_attn = dominant_kernel_roofline(dev), attention_roofline(dev)
        if args.full and world == 1 and args.workload == "sd15" and not args.grad_ckpt and not args.no_graph and not args.no_ckpt_line:
            # the reference's default (train_base.yaml:69 gradient_checkpointing: True) timed beside the headline: same
            # trainer, every ResnetBlock2D / Transformer2DModel segment recomputed in backward, graphs re-captured
            unet.enable_gradient_checkpointing()
            tr._graph_cache.clear()
            k2 = max(5, min(args.steps, 20))
            for _ in range(3):
                tr.train_one_step(latents, ehs, None, added, plugin_input, prompt_ids)
            sync()
            t1 = time.perf_counter()
            for _ in range(k2):
                tr.train_one_step(latents, ehs, None, added, plugin_input, prompt_ids)
            sync()
            d2 = time.perf_counter() - t1
            out["grad_ckpt_on"] = {"value": round(B * k2 / d2, 2), "unit": "images/sec", "ms_per_step": round(d2 / k2 * 1e3, 3),
                                   "steps": k2, "note": "same workload with enable_gradient_checkpointing() (+1 forward per step)"}
            unet.disable_gradient_checkpointing()
            tr._graph_cache.clear()
        if world == 1 and args.workload == "sd15" and frozen_te_leg and not args.grad_ckpt:
            tr.text_encoder = build_clip().requires_grad_(False).eval()       # frozen: no TE LoRA, NativeTrainer only calls it under no_grad
            # What TEUnetWrapper.forward does EVERY step (models/wrapper.py:14-30): the FROZEN text encoder runs inside the step on the
            # batch's prompt ids; the headline feeds pre-computed states (north_star scopes the path to the UNet + LoRA).  Same trainer,
            # same LoRA, no TE LoRA: the batch carries prompt_ids instead of encoder_hidden_states (its own captured graph).
            try:                                   # (secondary legs never take the headline line down with them)
                pid = torch.randint(0, 49406, (B, 77), device=dev); pid[:, 0] = 49406; pid[:, -1] = 49407
                k3 = max(5, min(args.steps, 20))
                for _ in range(3):
                    tr.train_one_step(latents, None, None, added, plugin_input, pid)
                sync()
                t1 = time.perf_counter()
                for _ in range(k3):
                    tr.train_one_step(latents, None, None, added, plugin_input, pid)
                sync()
                d3 = time.perf_counter() - t1
                out["frozen_te_in_step"] = {"value": round(B * k3 / d3, 2), "unit": "images/sec", "ms_per_step": round(d3 / k3 * 1e3, 3), "steps": k3,
                                            "note": "same step with the frozen native CLIP-L encoding prompt_ids [B,77] inside the captured step "
                                                    "(TEUnetWrapper.forward, models/wrapper.py:20), no text-encoder LoRA"}
            except Exception as e:                 # noqa: BLE001
                out["frozen_te_in_step"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            # ... and what a reference user gets who keeps the reference's OWN trainer loop over the native modules (INTEGRATION.md
            # "Keeping the reference's loop"): eager trainer, unet.enable_hip_graph() as the mi355x overlay sets it.  LAST: it switches the module to graph replay.
            try:
                k4 = max(5, min(args.steps, 20))
                d4, lv4 = seam_loop(True, k4, 5)
                if not math.isfinite(lv4):
                    raise RuntimeError("non-finite loss")
                out["seam_graph"] = {"value": round(B * k4 / d4, 2), "unit": "images/sec", "ms_per_step": round(d4 / k4 * 1e3, 3), "steps": k4,
                                     "note": "the reference Trainer's loop restated (train_ac.py:467-504: eager module call, clip_grad_norm_, fused "
                                             "AdamW, zero_grad, loss.item() every step) over the native modules with unet.enable_hip_graph()"}
            except Exception as e:                 # noqa: BLE001
                out["seam_graph"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        if emu:
            out["data"] = "synthetic (HCP_BENCH_BACKEND=emu: launcher / rank plumbing check on the CPU interpreter, timings meaningless)"
            out["config"]["comm"] = "gloo via torch.distributed" if world > 1 else "none"
            print(json.dumps(out), flush=True)
            if world > 1:
                torch.distributed.barrier()
                torch.distributed.destroy_process_group()
            return
        if args.full:
            out["roofline"] = roof
            out["roofline_attention"] = roof_attn
            if args.workload == "sd15" and B == 4:
                fam = family_roofline(B)
                if fam:
                    out["roofline_family"] = fam
            if world == 1 and not args.no_cpu_baseline and args.workload == "sd15":
                out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if not loss_ok:                                # a void measurement must not read as a result: value is null, exit code 3
        raise SystemExit(3)


if __name__ == "__main__":
    main()
