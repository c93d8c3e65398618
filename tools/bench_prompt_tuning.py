"""ms/step of the headline SD1.5 configuration (UNet LoRA rank 8, bs 4, 512px, captured step) plus prompt tuning: a frozen CLIP-L text
encoder encodes the prompt inside the step and one trained 4-vector word sits in every prompt (lora_anime_character.yaml's subject
token without the encoder LoRA).  Prints one JSON line.

    python tools/bench_prompt_tuning.py --steps 20 --warmup 3
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LORA_PATTERNS = [r"re:.*\.attn.?$", r"re:.*\.ff$"]


def _init_(mod):
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if "embedding" in name:
                p.normal_(0, 0.02)
            elif p.dim() > 1:
                p.normal_(0, p[0].numel() ** -0.5)
            elif "norm" in name and name.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    return mod


class _Tokenizer:                                   # add_tokens / __call__ / model_max_length: what EmbeddingPTHook.hook uses
    model_max_length = 77

    def __init__(self):
        self.added = {}

    def add_tokens(self, words):
        for w in words:
            self.added.setdefault(w, 49408 + len(self.added))

    def __call__(self, text):
        return argparse.Namespace(input_ids=[49406] + [self.added[w] for w in text.split()] + [49407])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()
    from hcp_diffusion_amd.prompt_tuning import EmbeddingPTHook
    from hcp_diffusion_amd.text_encoder import NativeCLIPTextModel
    from hcp_diffusion_amd.trainer import NativeTrainer
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    dev = torch.device("cuda:0")
    torch.manual_seed(114514)
    with torch.device("meta"):
        unet, te = NativeUNet2DConditionModel(), NativeCLIPTextModel()
    unet, te = _init_(unet.to_empty(device=dev)), _init_(te.to_empty(device=dev))
    word = torch.nn.Parameter(torch.randn(4, 768, device=dev) * 0.02, requires_grad=False)
    tk = _Tokenizer()
    EmbeddingPTHook.hook({"sks": word}, tk, te, N_repeats=1)
    B = args.batch
    tr = NativeTrainer(unet, [dict(layers=LORA_PATTERNS, rank=8, lr=1e-4)], lr=1e-4, weight_decay=1e-3, scale_lr_factor=B, use_graph=True,
                       text_encoder=te, pt_cfg=[dict(name="sks", lr=3e-3)], pt_words={"sks": word})
    with torch.no_grad():
        for blk in tr.bucket.blocks:
            blk.layer.W_up.normal_(0, 0.02)
    tr.bucket.pack()
    latents = torch.randn(B, 4, 64, 64, device=dev)
    ids = torch.randint(0, 49406, (B, 77), device=dev)
    ids[:, 0] = 49406; ids[:, 30:] = 49407
    ids[:, 3] = tk.added["sks"]
    for _ in range(args.warmup):
        tr.train_one_step(latents, prompt_ids=ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.train_one_step(latents, prompt_ids=ids)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lv = float(loss.item())
    print(json.dumps({"metric": "ms/step, SD1.5 LoRA 512px bs=%d + one trained 4-vector word, prompt encoded in the captured step" % B,
                      "value": round(dt / args.steps * 1e3, 3), "unit": "ms/step", "steps": args.steps, "warmup": args.warmup,
                      "loss_finite": math.isfinite(lv), "word_grad_reaches": bool(word.detach().abs().sum().item() > 0),
                      "config": {"unet_lora_rank": 8, "text_encoder": "CLIP-L frozen, random init", "word_vectors": 4, "batch": B}}), flush=True)


if __name__ == "__main__":
    main()
