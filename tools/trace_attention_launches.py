"""GPU-only: record every attention launch (kernels.LAUNCHES, kinds attn_fwd / attn_bwd) of one eager training step of each benchmark
workload — plus, since those workloads take ready-made text states, one forward + backward of each native CLIP text encoder (causal,
12 x 64 and 20 x 64 heads at 77 tokens, at the workload's batch) and one SD1.5 and one SDXL step with an attn_mask (the masked kernels
at their real shape) — and write the distinct launch descriptors, with who issues them and how often, as sorted JSON.

  python tools/trace_attention_launches.py [out.json]          (default: tests/golden/attention_launches.json)

tests/test_attention_launches.py checks every descriptor at its real shape against float64 and that a fresh trace equals this fixture."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hcp_diffusion_amd import kernels as K  # noqa: E402
from workloads import BATCH, setup  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "attention_launches.json")
KINDS = ("attn_fwd", "attn_bwd")
WORKLOADS = ("sd15", "dreambooth", "controlnet", "sdxl")
EXTRA = ("clip_l", "clip_bigg", "sd15_masked", "sdxl_masked")
TE_LORA = [r"re:.*self_attn$", r"re:.*mlp$"]
CLIP_BIGG = dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                 max_position_embeddings=77)


def _recorded(fn):
    K.LAUNCHES = []
    try:
        fn()
        torch.cuda.synchronize()
        launches = K.LAUNCHES
    finally:
        K.LAUNCHES = None
    counts = {}
    for d in launches:
        if d["kind"] not in KINDS:
            continue
        key = json.dumps(d, sort_keys=True)
        counts[key] = counts.get(key, 0) + 1
    return counts


def _attn_mask(B, dev):
    """[B, 77], 1 = attend: a different prompt length per batch row, token 0 always visible."""
    m = torch.zeros(B, 77, device=dev)
    for b in range(B):
        m[b, :77 - 9 * b - 5] = 1
    return m


def trace_workload(name, dev="cuda:0"):
    """{descriptor json: count} of one eager step (after a warm-up step that does the lazy packing; never a graph replay)."""
    dev = torch.device(dev)
    if name in ("clip_l", "clip_bigg"):
        from hcp_diffusion_amd.lora import make_lora
        from hcp_diffusion_amd.text_encoder import CLIP_L_CONFIG, NativeCLIPTextModel
        B = BATCH["sd15"] if name == "clip_l" else BATCH["sdxl"]
        with torch.device("meta"):
            te = NativeCLIPTextModel(**(CLIP_L_CONFIG if name == "clip_l" else CLIP_BIGG))
        te = te.to_empty(device=dev)
        with torch.no_grad():
            for n, p in te.named_parameters():
                p.normal_(0, 0.02) if p.dim() > 1 else p.fill_(1.0 if n.endswith("weight") else 0.0)
        te.requires_grad_(False)
        _, group, bucket = make_lora(te, [dict(layers=TE_LORA, rank=4)])
        with torch.no_grad():
            for blk in bucket.blocks:
                blk.layer.W_up.normal_(0, 0.02)
        bucket.pack()
        ids = torch.randint(0, 49408, (B, 77), device=dev)

        def step():
            te(ids).float().square().mean().backward()
        step()
        counts = _recorded(step)
        del te, group, bucket
    else:
        masked = name.endswith("_masked")
        w = name.split("_")[0]
        tr, lat, ehs, kw = setup(w, BATCH[w], dev)
        if masked:
            kw["attn_mask"] = _attn_mask(BATCH[w], dev)
        tr.train_one_step(lat, ehs, **kw)
        counts = _recorded(lambda: tr.train_one_step(lat, ehs, **kw))
        del tr
    torch.cuda.empty_cache()
    return counts


def trace_all(names=WORKLOADS + EXTRA):
    merged = {}
    for w in names:
        for key, n in trace_workload(w).items():
            merged.setdefault(key, {})[w] = n
    out = []
    for key in sorted(merged):
        out.append(dict(desc=json.loads(key), count=dict(sorted(merged[key].items()))))
    return out


def dumps(entries):
    """deterministic text: one descriptor per line."""
    lines = [json.dumps(e, sort_keys=True, separators=(",", ":")) for e in entries]
    return "[\n" + ",\n".join(lines) + "\n]\n"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    entries = trace_all()
    with open(path, "w") as f:
        f.write(dumps(entries))
    print(f"{len(entries)} distinct launch descriptors -> {path}")


if __name__ == "__main__":
    main()
