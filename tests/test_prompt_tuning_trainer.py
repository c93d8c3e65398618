"""NativeTrainer with trained custom words (tokenizer_pt.train): textual inversion against an fp32 oracle loop (oracle UNet + CLIP, the
restated EmbeddingPTHook, torch AdamW with weight_decay 5e-4), clip membership next to UNet / text-encoder LoRA (train_ac.py:483-500),
graph against eager, two gloo ranks against one process, and the word files against the reference's load_emb / save_emb."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from hcp_diffusion_amd import kernels as K
from hcp_diffusion_amd.prompt_tuning import EmbeddingPTHook
from hcp_diffusion_amd.text_encoder import NativeCLIPTextModel
from pt_ref import RefEmbeddingPTHook, StubTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TCFG = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=77)
UNET_LORA = [r"re:.*\.attn.?$", r"re:.*\.ff$"]
TE_LORA = [r"re:.*self_attn$", r"re:.*mlp$"]


def _models(dev):
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    from oracle.clip_ref import OracleCLIPTextModel
    from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, seeded_init_
    ucfg = dict(MICRO_CONFIG, cross_attention_dim=64)
    ou = seeded_init_(OracleUNet2DConditionModel(**ucfg), 1); ot = seeded_init_(OracleCLIPTextModel(**TCFG), 2)
    nu = NativeUNet2DConditionModel(**ucfg); nu.load_state_dict(ou.state_dict()); nu.to(dev)
    nt = NativeCLIPTextModel(**TCFG); nt.load_state_dict(ot.state_dict()); nt.to(dev)
    ou.requires_grad_(False); ot.requires_grad_(False)
    return ou, ot, nu, nt


def _word(n=4, seed=7):
    return torch.randn(n, 64, generator=torch.Generator().manual_seed(seed)) * 0.3


def _hook_native(nt, vec, dev, name="sks"):
    tk = StubTokenizer(100)
    words = {name: torch.nn.Parameter(vec.clone().to(dev), requires_grad=False)}
    EmbeddingPTHook.hook(words, tk, nt, N_repeats=1)
    return words, tk.added[name]


def _batch(tid, B=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 98, (B, 77), generator=g); ids[:, 0] = 98; ids[:, 40:] = 99
    for b in range(B):
        ids[b, 2 + 3 * b] = tid
    return (ids, torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 4, 8, 8, generator=g), torch.tensor([100, 800][:B] + [500] * (B - 2)))


def test_textual_inversion_steps_vs_oracle_adamw(backend):
    """tokenizer_pt.train alone (TextualInversion.yaml): frozen UNet and encoder, one 4-vector word.  Per step: the word's gradient vs
    autograd through the oracle pair + restated hook, then the native AdamW (weight_decay 5e-4, no clip even with a tiny max_grad_norm)
    vs torch AdamW fed the same gradient."""
    from hcp_diffusion_amd.trainer import NativeTrainer
    from oracle.unet_sd15 import add_noise, ddpm_alphas_cumprod
    dev = backend.device
    ou, ot, nu, nt = _models(dev)
    vec = _word()
    words, tid = _hook_native(nt, vec, dev)
    po = torch.nn.Parameter(vec.clone())
    RefEmbeddingPTHook(ot.text_model.embeddings.token_embedding, N_word=75, N_repeats=1).add_emb(po, tid)
    tr = NativeTrainer(nu, None, lr=1e-3, text_encoder=nt, pt_cfg=[dict(name="sks", lr=3e-3)], pt_words=words, max_grad_norm=1e-4)
    assert tr.pt_words["sks"] is words["sks"] and words["sks"].requires_grad
    opt = torch.optim.AdamW([po], lr=3e-3, weight_decay=5e-4)
    acp = ddpm_alphas_cumprod()
    for step in range(3):
        ids, x0, noise, t = _batch(tid, seed=10 + step)
        po.grad = None
        lo = F.mse_loss(ou(add_noise(x0, noise, t, acp), t, ot.encode(ids)).sample, noise)
        lo.backward()
        tr.make_noise = lambda lat: (K.add_noise(lat, noise.to(dev), t.to(dev), tr.acp), noise.to(dev), t.to(dev))
        ln = tr.forward_backward(x0.to(dev), None, prompt_ids=backend.to(ids))
        assert abs(lo.item() - ln.item()) / lo.item() < 2e-2
        gn = tr.pt_bucket.grads.clone().cpu()
        assert po.grad.norm() > 0 and F.cosine_similarity(po.grad.flatten(), gn, dim=0).item() > 0.99
        assert (gn.norm() / po.grad.norm()).item() == pytest.approx(1.0, abs=5e-2)
        po.grad = gn.view_as(po).clone()
        opt.step()
        tr.all_reduce(); tr.optimizer_step()
        pn = words["sks"].detach().cpu()
        assert ((pn - po.detach()).abs().max() / po.detach().abs().max()).item() < 1e-5, step
        assert tr.pt_bucket.grads.abs().max().item() == 0              # the fused step leaves the gradients zeroed


def test_lora_plus_word_clip_membership(backend):
    """lora_anime_character.yaml: UNet LoRA + text-encoder LoRA + a trained word.  The encoder trains, so the word is inside the global
    clip (TE_unet.trainable_parameters() holds emb_train) and then stepped by its own AdamW (weight_decay 5e-4)."""
    from hcp_diffusion_amd.trainer import NativeTrainer
    dev = backend.device
    _, _, nu, nt = _models(dev)
    words, tid = _hook_native(nt, _word(), dev)
    tr = NativeTrainer(nu, [dict(layers=UNET_LORA, rank=4)], lr=1e-3, text_encoder=nt, lora_te_cfg=[dict(layers=TE_LORA, rank=4, lr=1e-4)],
                       pt_cfg=[dict(name="sks", lr=3e-3)], pt_words=words, max_grad_norm=1e-3)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for bk in (tr.bucket, tr.te_bucket):
            for blk in bk.blocks:
                blk.layer.W_up.copy_(torch.randn(blk.layer.W_up.shape, generator=g) * 0.05)
            bk.pack()
    ids, x0, noise, t = _batch(tid)
    tr.make_noise = lambda lat: (K.add_noise(lat, noise.to(dev), t.to(dev), tr.acp), noise.to(dev), t.to(dev))
    tr.forward_backward(x0.to(dev), None, prompt_ids=backend.to(ids))
    bks = [tr.bucket, tr.te_bucket, tr.pt_bucket]
    grads = [b.grads.clone().cpu() for b in bks]
    params = [torch.nn.Parameter(b.params.clone().cpu()) for b in bks]
    assert all(gr.norm() > 0 for gr in grads)
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    torch.nn.utils.clip_grad_norm_(params, 1e-3)                       # one clip over all three
    opt = torch.optim.AdamW([dict(params=[params[0]], lr=1e-3), dict(params=[params[1]], lr=1e-4)], weight_decay=1e-3)
    opt_pt = torch.optim.AdamW([params[2]], lr=3e-3, weight_decay=5e-4)
    opt.step(); opt_pt.step()
    tr.all_reduce(); tr.optimizer_step()
    for p, b in zip(params, bks):
        got = b.params.cpu()
        assert ((got - p.detach()).abs().max() / p.detach().abs().max()).item() < 1e-5


@pytest.mark.gpu
def test_textual_inversion_graph_equals_eager_bitwise():
    """The whole step captured (the prompt-tuning kernels, the word's AdamW) against eager: the same word after 4 steps, bit for bit."""
    from hcp_diffusion_amd.trainer import NativeTrainer
    res = []
    for use_graph in (False, True):
        _, _, nu, nt = _models("cuda")
        words, tid = _hook_native(nt, _word(), "cuda")
        tr = NativeTrainer(nu, None, lr=1e-3, text_encoder=nt, pt_cfg=[dict(name="sks", lr=3e-3)], pt_words=words, use_graph=use_graph)
        _, _, noise, t = _batch(tid)
        noise, t = noise.cuda(), t.cuda()
        tr.make_noise = lambda lat: (K.add_noise(lat, noise, t, tr.acp), noise, t)
        for step in range(4):
            ids, x0, _, _ = _batch(tid, seed=20 + step)
            tr.train_one_step(x0.cuda(), prompt_ids=ids.cuda())
        torch.cuda.synchronize()
        res.append(words["sks"].detach().clone())
    assert not torch.equal(res[0], _word().cuda())
    assert torch.equal(res[0], res[1])


def _dist_trainer():
    from hcp_diffusion_amd.trainer import NativeTrainer
    _, _, nu, nt = _models("cpu")
    words, tid = _hook_native(nt, _word(), "cpu")
    return NativeTrainer(nu, None, lr=1e-3, text_encoder=nt, pt_cfg=[dict(name="sks", lr=1e-2)], pt_words=words), words, tid


def _dist_worker(rank, world, port, out):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from conftest import emu_cdll
    K._set_backend_for_tests(emu_cdll())
    tr, words, tid = _dist_trainer()
    assert tr.world == world
    ids, x0, noise, t = _batch(tid)
    sl = slice(rank, rank + 1)
    tr.make_noise = lambda lat: (K.add_noise(lat, noise[sl], t[sl], tr.acp), noise[sl], t[sl])
    tr.forward_backward(x0[sl].contiguous(), None, prompt_ids=ids[sl].contiguous())
    tr.all_reduce()
    g = tr.pt_bucket.grads.clone() / world
    tr.optimizer_step()
    torch.save({"grads": g, "params": words["sks"].detach().clone()}, os.path.join(out, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
def test_two_rank_gloo_matches_single_process(tmp_path):
    port = 29500 + os.getpid() % 2000 + 29
    mp.spawn(_dist_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["grads"], r1["grads"])
    from conftest import emu_cdll
    K._set_backend_for_tests(emu_cdll())
    try:
        tr, words, tid = _dist_trainer()
        ids, x0, noise, t = _batch(tid)
        tr.make_noise = lambda lat: (K.add_noise(lat, noise, t, tr.acp), noise, t)
        tr.forward_backward(x0, None, prompt_ids=ids)
        g = tr.pt_bucket.grads.clone()
        tr.optimizer_step()
        assert F.cosine_similarity(g, r0["grads"], dim=0).item() > 0.9999
        assert ((g - r0["grads"]).norm() / g.norm()).item() < 1e-2
        assert (words["sks"].detach() - r0["params"]).abs().max().item() < 2.5e-2
    finally:
        K._set_backend_for_tests(None)


def test_word_files_round_trip(backend, tmp_path):
    """save_model writes {word}-{step}.pt in the reference layout, the text encoder's file leaves emb_ex. out; load_emb reads both
    layouts.  Where the reference tree exists its own load_emb / save_emb are the other side."""
    from hcp_diffusion_amd.ckpt import CkptManagerNative, load_emb, save_emb
    from hcp_diffusion_amd.trainer import NativeTrainer
    dev = backend.device
    _, _, nu, nt = _models(dev)
    words, tid = _hook_native(nt, _word(), dev)
    tr = NativeTrainer(nu, [dict(layers=UNET_LORA, rank=4)], lr=1e-3, text_encoder=nt, lora_te_cfg=[dict(layers=TE_LORA, rank=4)],
                       pt_cfg=[dict(name="sks", lr=3e-3)], pt_words=words)
    mgr = CkptManagerNative(fmt="ckpt"); mgr.set_save_dir(str(tmp_path))
    paths = tr.save_model(mgr, 5)
    f = tmp_path / "sks-5.pt"
    assert str(f) in paths
    st = torch.load(f)
    assert set(st) == {"string_to_param", "name"} and st["name"] == "sks-5"
    assert torch.equal(st["string_to_param"]["*"], words["sks"].detach().cpu())
    assert st["string_to_param"]["*"].untyped_storage().nbytes() == 4 * 64 * 4          # the vectors, not the whole bucket
    te = torch.load(tmp_path / "text_encoder-5.ckpt")
    assert not any("emb_ex." in k for sec in te.values() for k in _keys(sec))
    assert torch.equal(load_emb(str(f)), words["sks"].detach().cpu())
    torch.save({"emb_params": torch.ones(2, 64), "name": "old"}, tmp_path / "old.pt")
    assert torch.equal(load_emb(str(tmp_path / "old.pt")), torch.ones(2, 64))
    if os.path.isdir("/root/reference/hcpdiff"):
        from test_prompt_tuning import _load_reference_pt_hook
        _, nu_ref = _load_reference_pt_hook()
        assert torch.equal(nu_ref.load_emb(str(f)), words["sks"].detach().cpu())
        nu_ref.save_emb(str(tmp_path / "theirs.pt"), torch.full((3, 64), 2.0))
        assert torch.equal(load_emb(str(tmp_path / "theirs.pt")), torch.full((3, 64), 2.0))
        save_emb(str(tmp_path / "ours.pt"), torch.full((1, 64), 3.0))
        assert torch.equal(nu_ref.load_emb(str(tmp_path / "ours.pt")), torch.full((1, 64), 3.0))


def _keys(sec):
    if isinstance(sec, dict):
        for k, v in sec.items():
            if isinstance(v, dict):
                yield from (f"{k}.{x}" for x in _keys(v))
            else:
                yield k
