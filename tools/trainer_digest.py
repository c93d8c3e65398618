"""Bit-level fingerprint of NativeTrainer on the CPU interpreter build: a few steps of the micro model per configuration, then a
SHA-256 over the bytes of the loss, every bucket's parameters and every optimizer-state tensor.  Two checkouts whose digests agree
computed the same training, bit for bit — the evidence a refactor of the trainer rests on (profiles/trainer_digest.json).

    python tools/trainer_digest.py                         # {configuration: digest} as JSON on stdout
    python tools/trainer_digest.py --record branch --json profiles/trainer_digest.json --commit $(git rev-parse HEAD)

Only API that every version of the trainer has: the constructor, train_data_list, _states(), st.bucket.params, st.tensors()."""
import argparse
import hashlib
import json
import pathlib
import random
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from conftest import emu_cdll                                                    # noqa: E402
from hcp_diffusion_amd import kernels as K                                       # noqa: E402
from hcp_diffusion_amd.trainer import NativeTrainer                              # noqa: E402

ATTN, FF, TE = [r"re:.*\.attn.?$"], [r"re:.*\.ff$"], [r"re:.*self_attn$", r"re:.*mlp$"]
TCFG = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=77)


def _unet(**cfg):
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, seeded_init_
    cfg = dict(MICRO_CONFIG, **cfg)
    nat = NativeUNet2DConditionModel(**cfg)
    nat.load_state_dict(seeded_init_(OracleUNet2DConditionModel(**cfg), 1).state_dict())
    return nat


def _batch(seed, B=1, **extra):
    g = torch.Generator().manual_seed(seed)
    return dict(latents=torch.randn(B, 4, 8, 8, generator=g), encoder_hidden_states=torch.randn(B, 24, 32, generator=g), **extra)


def _lora(**kw):
    return lambda: (NativeTrainer(_unet(), [dict(layers=ATTN, rank=4, lr=1e-2), dict(layers=FF, rank=4, lr=1e-4)], lr=1e-3, **kw), None)


def _host_lora(optimizer):
    return lambda: (NativeTrainer(_unet(), [dict(layers=ATTN, rank=4)], lr=1e-3, optimizer=optimizer,
                                  train_cfg=[dict(layers=["conv_in", "conv_out"], lr=1e-3)]), None)


def _sharded():
    return NativeTrainer(_unet(), None, lr=1e-3, train_cfg=[dict(layers=[""])], shard_optimizer="force", overlap_exchange=True,
                         grad_wire="bf16", param_wire="bf16"), None


def _text():
    from hcp_diffusion_amd.prompt_tuning import EmbeddingPTHook
    from hcp_diffusion_amd.text_encoder import NativeCLIPTextModel
    from oracle.clip_ref import OracleCLIPTextModel
    from oracle.unet_sd15 import seeded_init_
    from pt_ref import StubTokenizer
    nt = NativeCLIPTextModel(**TCFG)
    nt.load_state_dict(seeded_init_(OracleCLIPTextModel(**TCFG), 2).state_dict())
    tk = StubTokenizer(100)
    words = {"sks": torch.nn.Parameter(torch.randn(4, 64, generator=torch.Generator().manual_seed(7)) * 0.3, requires_grad=False)}
    EmbeddingPTHook.hook(words, tk, nt, N_repeats=1)
    tr = NativeTrainer(_unet(cross_attention_dim=64), [dict(layers=ATTN + FF, rank=4)], lr=1e-3, text_encoder=nt,
                       lora_te_cfg=[dict(layers=TE, rank=4, lr=1e-4)], pt_cfg=[dict(name="sks", lr=3e-3)], pt_words=words,
                       cfg_scale="1.0-3.0:cos")

    def data(step):                                          # B = 2 latents, 2B prompts (negatives first), the word in every prompt
        g = torch.Generator().manual_seed(40 + step)
        ids = torch.randint(0, 98, (4, 77), generator=g)
        ids[:, 0], ids[:, 40:], ids[:, 3] = 98, 99, tk.added["sks"]
        return [dict(latents=torch.randn(2, 4, 8, 8, generator=g), prompt_ids=ids)]
    return tr, data


CONFIGS = {
    "a_lora_two_lrs_ema": _lora(ema=dict(decay_max=0.99)),
    "b_fullft_sharded_overlap_bf16_wires": _sharded,
    "c_lion": _host_lora({"type": "lion", "betas": (0.9, 0.99)}),
    "d_adafactor": _host_lora({"type": "adafactor", "lr": None, "relative_step": False}),
    "d_adafactor_beta1": _host_lora({"type": "adafactor", "lr": None, "relative_step": False, "beta1": 0.9}),
    "e_text_encoder_lora_words_cfg_scale": _text,
    "f_pyramid_zero_terminal": _lora(noise_cfg=dict(type="pyramid", level=4, discount=0.8, zero_terminal=True)),
    "g_sample_min_snr_accum2_two_datasets": _lora(loss_type="sample", loss_cfg=dict(type="min_snr", gamma=5.0), gradient_accumulation_steps=2),
}


def digest(name):
    torch.manual_seed(0)
    tr, data = CONFIGS[name]()
    g = torch.Generator().manual_seed(5)
    for bk in (tr.bucket, tr.te_bucket):                     # (a LoRA starts with W_up = 0: nothing would reach W_down)
        if bk is not None:
            with torch.no_grad():
                for blk in bk.blocks:
                    blk.layer.W_up.copy_(torch.randn(blk.layer.W_up.shape, generator=g) * 0.05)
            bk.pack()
    torch.manual_seed(123)
    random.seed(123)
    h = hashlib.sha256()
    for step in range(3 if tr.accum == 1 else 2 * tr.accum):
        batches = data(step) if data else [_batch(10 + step, B=2), _batch(20 + step, loss_weight=0.5)] if tr.accum > 1 else [_batch(10 + step, B=2)]
        h.update(tr.train_data_list(batches).detach().cpu().numpy().tobytes())
    for st in tr._states():
        for t in [st.bucket.params] + list(st.tensors()):
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--only", nargs="*", default=list(CONFIGS))
    ap.add_argument("--record", help="store the digests under this key of --json")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "trainer_digest.json"))
    ap.add_argument("--commit", help="with --record: the commit the digests were taken on")
    args = ap.parse_args()
    K._set_backend_for_tests(emu_cdll())
    out = {name: digest(name) for name in args.only}
    print(json.dumps(out, indent=1))
    if args.record:
        path = pathlib.Path(args.json)
        doc = json.loads(path.read_text()) if path.exists() else {}
        doc[args.record] = dict(out, **({"commit": args.commit} if args.commit else {}))
        path.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
