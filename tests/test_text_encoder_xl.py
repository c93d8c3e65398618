"""SDXL text path: exact GELU, the pooled projection kernels, NativeCLIPTextModel with hidden_act / projection_dim, the composed
clip_B + clip_bigG pair, the gradient into the UNet's text_embeds, the trainer step and the checkpoint names.  The torch restatement
(tests/clip_xl_ref.py) is pinned against the installed transformers first; everything native is compared with it."""
import os

import pytest
import torch
import torch.nn.functional as F

from clip_xl_ref import RefCLIPTextModelXL, RefSDXLTextEncoder, pool_ref
from hcp_diffusion_amd import kernels as K
from hcp_diffusion_amd.lora import make_lora
from hcp_diffusion_amd.text_encoder import NativeCLIPTextModel, NativeSDXLTextEncoder
from oracle.lora_ref import wrap_lora
from oracle.unet_sd15 import seeded_init_

TE_LORA = [r"re:.*self_attn$", r"re:.*mlp$"]                  # cfgs/train/examples/lora_sdxl.yaml: both encoders
UNET_LORA = [r"re:.*\.attn.?$", r"re:.*\.ff$"]
TINY_XL = dict(vocab_size=100, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, max_position_embeddings=77)
XL = dict(hidden_act="gelu", projection_dim=96)
HAVE_REFERENCE = os.path.isdir("/root/reference/hcpdiff")


def _ids(B, L=77, seed=1, eos=(40, 30, 76, 1, 55, 12)):
    """BOS 98, words, EOS 99 from a per-row position on (CLIP pads with EOS: the FIRST maximum is the EOS token)."""
    ids = torch.randint(1, 98, (B, L), generator=torch.Generator().manual_seed(seed))
    ids[:, 0] = 98
    for m in range(B):
        ids[m, eos[m % len(eos)]:] = 99
    return ids


def test_helper_matches_installed_transformers_with_projection():
    """hidden_act = gelu, EOS pooling and text_projection of the restatement vs transformers' CLIPTextModelWithProjection on the same
    weights, fp32 on the CPU: hidden_states[-2] (SDXL's clip_skip = 1 states) and text_embeds."""
    tr = pytest.importorskip("transformers")
    cfg = tr.CLIPTextConfig(**TINY_XL, hidden_act="gelu", projection_dim=96, bos_token_id=0, eos_token_id=2, pad_token_id=1)
    theirs = tr.CLIPTextModelWithProjection(cfg).eval()
    ours = seeded_init_(RefCLIPTextModelXL(**TINY_XL, **XL), 5)
    want = list(theirs.state_dict())
    prefixed = any(k.startswith("text_model.") for k in want)
    sd = {(k if prefixed or not k.startswith("text_model.") else k[len("text_model."):]): v for k, v in ours.state_dict().items()}
    missing, unexpected = theirs.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing)
    ids = _ids(3)
    ids[1, 10] = 99                                           # the maximum id twice (and the EOS padding): the first wins
    with torch.no_grad():
        out = theirs(input_ids=ids, output_hidden_states=True)
        states, pooled = ours.encode_xl(ids, clip_skip=1, final_norm=False)
    assert torch.allclose(out.hidden_states[-2], states, rtol=1e-4, atol=1e-5)
    assert torch.allclose(out.text_embeds, pooled, rtol=1e-4, atol=1e-5)
    quick = seeded_init_(RefCLIPTextModelXL(**TINY_XL, projection_dim=96), 5)
    with torch.no_grad():
        assert not torch.allclose(quick.encode_xl(ids)[1], pooled, atol=1e-3)          # (hidden_act is not ignored)


@pytest.mark.parametrize("n", [8 * 1001, 8 * 1001 + 3])
def test_gelu_fwd_bwd_against_float64(backend, n):
    """hcp_gelu element by element (16-byte body, scalar tail of 3): inputs across +-8 with 0 and the far-negative tail where Phi
    underflows.  Bound of test_gelu_and_silu_elementwise_against_float64 (the GEGLU form of the same device helper): one bf16 rounding
    of the result, 2^-8 relative, + 1e-6 absolute for the approximation."""
    x = torch.linspace(-8.0, 8.0, n - 8)
    x = torch.cat([x, torch.tensor([0.0, -0.0, -8.0, -7.5, -6.0, 8.0, 1e-3, -1e-3])]).bfloat16()[:n].contiguous()
    assert x.numel() == n
    xd = x.double()
    cdf = 0.5 * (1 + torch.erf(xd / 2 ** 0.5)); pdf = torch.exp(-0.5 * xd * xd) / (2 * torch.pi) ** 0.5
    tol = lambda ref: ref.abs() * 2.0 ** -8 + 1e-6
    y = K.gelu(backend.to(x)).float().cpu().double()
    ref = xd * cdf
    assert ((y - ref).abs() <= tol(ref)).all(), ((y - ref).abs() - tol(ref)).max()
    dy = (torch.arange(n) % 5 - 2).bfloat16().contiguous()                         # -2 .. 2: exact in bf16
    dx = K.gelu(backend.to(x), backend.to(dy)).float().cpu().double()
    refg = dy.double() * (cdf + xd * pdf)
    assert ((dx - refg).abs() <= tol(refg)).all(), ((dx - refg).abs() - tol(refg)).max()
    from hcp_diffusion_amd import ops
    xa = backend.to(x).requires_grad_()
    ops.gelu(xa).backward(backend.to(dy))
    assert torch.equal(xa.grad.float().cpu().double(), dx)


def _pool_case(backend, C, P, B, r, L=77):
    g = torch.Generator().manual_seed(C + r)
    M = B * r
    x = torch.randn(M, L, C, generator=g).bfloat16()
    ids = torch.randint(0, 50, (M, L), generator=g)
    eos = [1, 40, 76, 40, 5, 76][:M] if M > 2 else [76, 1]
    for m, p in enumerate(eos):
        ids[m, p] = 99
    ids[1, 60] = 99                                            # row 1: the maximum id twice, the first (40 / 1) must win
    gam = 1 + 0.1 * torch.randn(C, generator=g); bet = 0.1 * torch.randn(C, generator=g)
    w = torch.randn(P, C, generator=g) * C ** -0.5
    d = torch.randn(B, P, generator=g)
    order = C ** 0.5 * 2.0 ** -24                               # another order of an fp32 sum of C terms (random-walk model of its roundings)
    for wt in (w.bfloat16(), w):                                # packed bf16 (the model's frozen copy) and fp32
        ref = {}
        for dt in (torch.float64, torch.float32):
            xx = x.to(dt).requires_grad_()
            y = pool_ref(xx, ids, gam, bet, wt, r, dt)
            (y * d.to(dt)).sum().backward()
            ref[dt] = (y.detach().double(), (xx.grad.bfloat16() if dt == torch.float32 else xx.grad).double())
        y64, g64 = ref[torch.float64]
        e32_f = ((ref[torch.float32][0] - y64).abs().max() / y64.abs().max()).item()
        e32_b = ((ref[torch.float32][1] - g64).abs().max() / g64.abs().max()).item()
        pooled, pos, stats = K.clip_pool_fwd(backend.to(x), backend.to(ids), backend.to(gam), backend.to(bet), backend.to(wt), r)
        assert pos.cpu().tolist() == eos and pooled.dtype == torch.float32 and tuple(pooled.shape) == (B, P)
        ef = ((pooled.cpu().double() - y64).abs().max() / y64.abs().max()).item()
        dx = K.clip_pool_bwd(backend.to(x), pos, stats, backend.to(gam), backend.to(wt), backend.to(d), r)
        dxc = dx.float().cpu().double()
        eb = ((dxc - g64).abs().max() / g64.abs().max()).item()
        print(f"clip_pool C={C} P={P} r={r} w={wt.dtype}: fwd {ef:.3g} (fp32 torch {e32_f:.3g})  bwd {eb:.3g} (fp32 torch, bf16 out {e32_b:.3g})")
        off = torch.ones(M, L, dtype=torch.bool); off[torch.arange(M), torch.tensor(eos)] = False
        assert (dxc[off] == 0).all() and (dxc[~off] != 0).any(-1).all()
        assert ef <= 4 * e32_f + order and eb <= 4 * e32_b + order


@pytest.mark.parametrize("r", [1, 2])
def test_clip_pool_fwd_bwd_against_float64(backend, r):
    """hcp_clip_pool_fwd / _bwd at C = 128, P = 96, L = 77, B = 3: EOS at 1, 40 and 76, one row with the maximum id twice, and (r = 2) a
    prompt whose two chunks end at different positions; positions exact, dx exactly zero off the EOS tokens.
    Tolerance: max |err| / max |ref| against float64 on the same bf16 inputs; a float32 torch evaluation measures 1.0e-7 (r = 1) / 2.8e-7
    (r = 2) forward and, rounded to the kernel's bf16 output, 1.9e-3 / 2.2e-3 backward (2.2e-7 / 2.2e-3 at C = P = 1280).  Gate: 4 x that
    (recomputed in the test) + sqrt(C) 2^-24 for the different summation order.  Native measures 0.8e-7 .. 3e-7 and 2e-3."""
    _pool_case(backend, 128, 96, 3, r)


@pytest.mark.gpu
def test_clip_pool_at_bigg_width():
    """The real width, C = P = 1280, B = 2 (more than one 512-column pass per wave, 80 column slices): same gate."""
    from conftest import Backend, gpu_box_check
    gpu_box_check()
    K._set_backend_for_tests(None)
    _pool_case(Backend("gpu"), 1280, 1280, 2, 1)


def _te_pair(dev, seed=5, cfg=TINY_XL, xl=XL, **kw):
    ref = seeded_init_(RefCLIPTextModelXL(**cfg, **xl), seed)
    nat = NativeCLIPTextModel(**cfg, **xl, **kw)
    nat.load_state_dict(ref.state_dict())
    ref.requires_grad_(False); nat.requires_grad_(False)
    return ref, nat.to(dev)


def _sync_lora(wr, group, gen, scale=0.05):
    with torch.no_grad():
        for path, w in wr.items():
            blk = group.plugin_dict[path]
            w.lora_block_0.layer.W_up.copy_(torch.randn(w.lora_block_0.layer.W_up.shape, generator=gen) * scale)
            blk.layer.W_down.copy_(w.lora_block_0.layer.W_down); blk.layer.W_up.copy_(w.lora_block_0.layer.W_up)


def _flat_grads(wr, group, paths=None):
    paths = list(wr) if paths is None else paths
    grad = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)          # (a layer past clip_skip without a pooled head: unused)
    go = torch.cat([grad(p).flatten() for k in paths for p in (wr[k].lora_block_0.layer.W_down, wr[k].lora_block_0.layer.W_up)])
    gn = torch.cat([grad(p).flatten().float().cpu() for k in paths for p in (group.plugin_dict[k].layer.W_down, group.plugin_dict[k].layer.W_up)])
    return go, gn


@pytest.mark.parametrize("n_repeats,with_mask", [(1, False), (1, True), (2, False), (2, True)])
def test_tiny_xl_encoder_forward_vs_helper(backend, n_repeats, with_mask):
    """hidden_act = gelu, projection_dim = 96, clip_skip = 1, clip_final_norm = False: states and pooled vs the restatement (the gate of
    test_tiny_text_encoder_forward_vs_oracle); without projection_dim the answer keeps today's form."""
    ref, nat = _te_pair(backend.device, clip_skip=1, clip_final_norm=False, N_repeats=n_repeats)
    ids = _ids(2 * n_repeats).reshape(2, -1)
    mask = None
    if with_mask:
        mask = torch.ones(2, 77 * n_repeats); mask[0, 60:77] = 0
    with torch.no_grad():
        rs, rp = ref.encode_xl(ids, clip_skip=1, final_norm=False, attention_mask=mask, n_repeats=n_repeats)
        ns, np_ = nat(backend.to(ids), attention_mask=backend.to(mask) if with_mask else None, output_hidden_states=True)
    assert ns.shape == rs.shape == (2, 75 * n_repeats + 2, 128) and np_.shape == rp.shape == (2, 96) and np_.dtype == torch.float32
    assert ((ns.float().cpu() - rs).norm() / rs.norm()).item() < 2e-2
    assert ((np_.cpu() - rp).norm() / rp.norm()).item() < 2e-2
    plain = NativeCLIPTextModel(**TINY_XL, hidden_act="gelu").to(backend.device)
    assert "text_projection.weight" not in plain.state_dict() and plain.config["projection_dim"] is None
    with torch.no_grad():
        assert torch.is_tensor(plain(backend.to(ids[:, :77].contiguous())))


@pytest.mark.parametrize("n_repeats,with_mask,final_norm", [(1, False, True), (2, True, False)])
def test_tiny_xl_encoder_lora_gradients_vs_helper(backend, n_repeats, with_mask, final_norm):
    """Rank-4 LoRA on self_attn + mlp, a loss on BOTH outputs, clip_skip = 1: the last layer's blocks get their gradient through the
    pooled path alone — non-zero and matching; all blocks: the gates of test_tiny_text_encoder_lora_gradients_vs_oracle.  Second case:
    two chunks per prompt with different EOS positions (the pooled mean's 1 / r and per-chunk tokens in the backward), an attention
    mask and clip_final_norm = False.  A trainable final_layer_norm / text_projection is refused."""
    r = n_repeats
    ref, nat = _te_pair(backend.device, clip_skip=1, clip_final_norm=final_norm, N_repeats=r)
    wr = wrap_lora(ref, TE_LORA, rank=4)
    _, group, bucket = make_lora(nat, [dict(layers=TE_LORA, rank=4)])
    assert sorted(k for k in ref.state_dict() if "lora" in k) == sorted(k for k in nat.state_dict() if "lora" in k)
    gen = torch.Generator().manual_seed(9)
    _sync_lora(wr, group, gen)
    bucket.pack()
    ids = _ids(2 * r, seed=4).reshape(2, -1)
    mask = None
    if with_mask:
        mask = torch.ones(2, 77 * r); mask[0, 60:77] = 0
    ts, tp = torch.randn(2, 75 * r + 2, 128, generator=gen), torch.randn(2, 96, generator=gen)
    rs, rp = ref.encode_xl(ids, clip_skip=1, final_norm=final_norm, attention_mask=mask, n_repeats=r)
    lo = F.mse_loss(rs, ts) + F.mse_loss(rp, tp)
    lo.backward()
    ns, np_ = nat(backend.to(ids), attention_mask=backend.to(mask) if with_mask else None)
    ln = F.mse_loss(ns.float(), backend.to(ts)) + F.mse_loss(np_, backend.to(tp))
    ln.backward()
    assert abs(lo.item() - ln.item()) / lo.item() < 2e-2
    go, gn = _flat_grads(wr, group)
    assert F.cosine_similarity(go, gn, dim=0).item() > 0.995
    assert (gn.norm() / go.norm()).item() == pytest.approx(1.0, abs=3e-2)
    last = [k for k in wr if ".layers.2." in k]
    assert len(last) == 6
    go, gn = _flat_grads(wr, group, last)
    assert go.norm().item() > 0 and gn.norm().item() > 0
    assert F.cosine_similarity(go, gn, dim=0).item() > 0.995
    assert (gn.norm() / go.norm()).item() == pytest.approx(1.0, abs=3e-2)
    nat.text_projection.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        nat(backend.to(ids))


CFG_B = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=77)
CFG_G = dict(vocab_size=100, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77)
XL_G = dict(hidden_act="gelu", projection_dim=64)               # = the tiny SDXL UNet's pooled width (256 - 6 x 32)


def _pairs(dev, **sel):
    rb, nb = _te_pair(dev, 2, CFG_B, {}, **sel)
    rg, ng = _te_pair(dev, 3, CFG_G, XL_G, **sel)
    rsel = dict(clip_skip=sel.get("clip_skip", 0), final_norm=sel.get("clip_final_norm", True), n_repeats=sel.get("N_repeats", 1))
    return RefSDXLTextEncoder(rb, rg, **rsel), NativeSDXLTextEncoder(nb, ng)


def _pair_ids(B=2):
    return torch.cat([_ids(B, seed=7), _ids(B, seed=8, eos=(20, 66))], -1)


def test_composed_pair_outputs(backend):
    """[B, 2 x 77] ids, different per half -> states [B, 77, 64 + 128] = (clip_B | clip_bigG) on channels, pooled = [None, bigG's]."""
    ref, nat = _pairs(backend.device, clip_skip=1)
    ids = _pair_ids()
    assert not torch.equal(ids[:, :77], ids[:, 77:])
    with torch.no_grad():
        rs, rp = ref(ids)
        ns, np_ = nat(backend.to(ids), output_hidden_states=True)
        only_b = nat.clip_B(backend.to(ids[:, :77].contiguous()))
    assert tuple(ns.shape) == (2, 77, 192) and torch.equal(ns[..., :64], only_b)
    assert ((ns.float().cpu() - rs).norm() / rs.norm()).item() < 2e-2
    assert isinstance(np_, list) and len(np_) == 2 and np_[0] is None and rp[0] is None
    assert ((np_[1].cpu() - rp[1]).norm() / rp[1].norm()).item() < 2e-2
    emb = nat.get_input_embeddings()
    assert emb[0] is nat.clip_B.text_model.embeddings.token_embedding and emb[1] is nat.clip_bigG.text_model.embeddings.token_embedding
    assert nat.device == ns.device and nat.dtype == torch.float32
    with pytest.raises(ValueError):
        nat(backend.to(ids[:, :153]))


def _sdxl_unets(dev):
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    from oracle.unet_sd15 import OracleUNet2DConditionModel
    from test_model import TINY_SDXL_CONFIG
    ucfg = dict(TINY_SDXL_CONFIG, cross_attention_dim=192)
    ou = seeded_init_(OracleUNet2DConditionModel(**ucfg), 1)
    nu = NativeUNet2DConditionModel(**ucfg); nu.load_state_dict(ou.state_dict()); nu.to(dev)
    ou.requires_grad_(False)
    return ou, nu


CROP = torch.tensor([[64.0, 64.0, 0.0, 0.0, 64.0, 64.0]] * 2)


def test_text_embeds_gradient_through_the_unet(backend):
    """A text_embeds that requires grad receives one through add_embedding (the pooled vector's way into the UNet)."""
    ou, nu = _sdxl_unets(backend.device)
    nu.requires_grad_(False)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 8, 8, generator=g); t = torch.tensor([5, 500]); ehs = torch.randn(2, 77, 192, generator=g)
    te_o = torch.randn(2, 64, generator=g).requires_grad_(); te_n = backend.to(te_o.detach().clone()).requires_grad_()
    ou(x, t, ehs, added_cond_kwargs=dict(text_embeds=te_o, time_ids=CROP)).sample.square().mean().backward()
    to = backend.to
    nu(to(x), to(t), to(ehs.bfloat16()), added_cond_kwargs=dict(text_embeds=te_n, time_ids=to(CROP))).sample.float().square().mean().backward()
    assert te_n.grad is not None and te_o.grad.norm().item() > 0
    assert F.cosine_similarity(te_o.grad.flatten(), te_n.grad.flatten().float().cpu(), dim=0).item() > 0.99
    assert (te_n.grad.norm().item() / te_o.grad.norm().item()) == pytest.approx(1.0, abs=5e-2)


def _trainer(dev, use_graph=False):
    from hcp_diffusion_amd.trainer import NativeTrainer
    ou, nu = _sdxl_unets(dev)
    ref, nat = _pairs(dev, clip_skip=1)
    tr = NativeTrainer(nu, [dict(layers=UNET_LORA, rank=4)], lr=1e-3, text_encoder=nat, lora_te_cfg=[dict(layers=TE_LORA, rank=4)], use_graph=use_graph)
    return ou, ref, tr


def test_pair_plus_sdxl_unet_lora_step_vs_helper(backend):
    """lora_sdxl.yaml's step: prompt_ids [B, 2 x 77] encoded inside the step, text_embeds = pooled[-1] with the batch's time_ids; loss, the
    UNet's and BOTH encoders' LoRA gradients vs the torch restatement (gates of test_unet_plus_text_encoder_lora_step_vs_oracle)."""
    from oracle.unet_sd15 import add_noise, ddpm_alphas_cumprod
    dev = backend.device
    ou, ref, tr = _trainer(dev)
    wu, wt = wrap_lora(ou, UNET_LORA, rank=4), wrap_lora(ref, TE_LORA, rank=4)
    assert any(k.startswith("clip_B.") for k in wt) and any(k.startswith("clip_bigG.") for k in wt)
    assert sorted(wt) == sorted(tr.lora_te_group.plugin_dict)
    gen = torch.Generator().manual_seed(3)
    _sync_lora(wu, tr.lora_group, gen); _sync_lora(wt, tr.lora_te_group, gen)
    tr.bucket.pack(); tr.te_bucket.pack()
    x0 = torch.randn(2, 4, 8, 8, generator=gen); noise = torch.randn(2, 4, 8, 8, generator=gen)
    t = torch.tensor([100, 800]); ids = _pair_ids()
    states, pooled = ref(ids)
    pred = ou(add_noise(x0, noise, t, ddpm_alphas_cumprod()), t, states, added_cond_kwargs=dict(text_embeds=pooled[-1], time_ids=CROP)).sample
    lo = F.mse_loss(pred, noise)
    lo.backward()
    tr.make_noise = lambda lat: (K.add_noise(lat, noise.to(dev), t.to(dev), tr.acp), noise.to(dev), t.to(dev))
    ln = tr.forward_backward(x0.to(dev), None, prompt_ids=ids.to(dev), added_cond_kwargs=dict(time_ids=CROP.to(dev)))
    assert abs(lo.item() - ln.item()) / lo.item() < 2e-2
    gu_o, gu_n = _flat_grads(wu, tr.lora_group)
    assert F.cosine_similarity(gu_o, gu_n, dim=0).item() > 0.995
    for name in ("clip_B.", "clip_bigG."):
        go, gn = _flat_grads(wt, tr.lora_te_group, [k for k in wt if k.startswith(name)])
        assert go.norm().item() > 0 and F.cosine_similarity(go, gn, dim=0).item() > 0.99, name
        assert (gn.norm() / go.norm()).item() == pytest.approx(1.0, abs=5e-2), name
    last = [k for k in wt if k.startswith("clip_bigG.") and ".layers.1." in k]          # reached through text_embeds only (clip_skip = 1)
    go, gn = _flat_grads(wt, tr.lora_te_group, last)
    assert go.norm().item() > 0 and gn.norm().item() > 0 and F.cosine_similarity(go, gn, dim=0).item() > 0.99
    with pytest.raises(ValueError):
        tr.forward_backward(x0.to(dev), None, prompt_ids=ids.to(dev))                # an SDXL pair without the batch's time_ids


@pytest.mark.gpu
def test_pair_trainer_graph_equals_eager():
    """The same steps through NativeTrainer with the whole step captured and eager: equal losses and equal updated factors, to the gates
    of the existing graph-vs-eager tests (tests/test_trainer.py) — the loss and the bias / norm-affine gradients are fp32 atomic sums, so
    two runs agree to rounding, not bit for bit: 1e-5 relative per step (test_graph_two_datasets_equal_eager) on the losses, 1e-4 of the
    largest factor after a trajectory of steps at lr 1e-3 (test_graph_cache_per_latent_shape) on both buckets."""
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)                                   # make_lora draws W_down from the global generator
        _, _, tr = _trainer("cuda", use_graph)
        gen = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for b in (tr.bucket, tr.te_bucket):
                for blk in b.blocks:
                    blk.layer.W_up.copy_(torch.randn(blk.layer.W_up.shape, generator=gen) * 0.05)
        tr.bucket.pack(); tr.te_bucket.pack()
        noise = torch.randn(2, 4, 8, 8, generator=gen).cuda(); t = torch.tensor([100, 800]).cuda()
        tr.make_noise = lambda lat: (K.add_noise(lat, noise, t, tr.acp), noise, t)
        losses = []
        for step in range(3):
            x0 = torch.randn(2, 4, 8, 8, generator=gen).cuda()
            ids = torch.cat([_ids(2, seed=20 + step), _ids(2, seed=40 + step, eos=(20, 66))], -1).cuda()
            losses.append(tr.train_one_step(x0, prompt_ids=ids, added_cond_kwargs=dict(time_ids=CROP.cuda())).clone())
        torch.cuda.synchronize()
        res.append((torch.stack(losses).cpu(), tr.bucket.params.detach().cpu().clone(), tr.te_bucket.params.detach().cpu().clone()))
    assert torch.isfinite(res[0][0]).all() and not torch.equal(res[0][2], torch.zeros_like(res[0][2]))
    (le, pe, te), (lg, pg, tg) = res
    figs = [((le - lg).abs() / le.abs()).max().item(), ((pe - pg).abs().max() / pe.abs().max()).item(), ((te - tg).abs().max() / te.abs().max()).item()]
    print(f"graph vs eager: loss {figs[0]:.3g} unet factors {figs[1]:.3g} text-encoder factors {figs[2]:.3g}")
    assert figs[0] < 1e-5 and figs[1] < 1e-4 and figs[2] < 1e-4


@pytest.mark.gpu
def test_bigg_width_forward_and_lora_grads_vs_helper():
    """bigG's width at reduced depth (1280, 20 heads x 64, MLP 5120, projection 1280, 4 layers, B = 2, seeded weights, clip_skip = 1): states,
    pooled and rank-4 LoRA gradients vs the fp32 restatement computed on the CPU.
    Gate: the restatement under torch.autocast("cpu", bfloat16) against itself in fp32 — same weights, the SAME LoRA factors (the global
    generator that wrap_lora draws W_down from is seeded as here), ids and loss — measures relative L2 7.33e-3 on the states, 8.21e-3 on
    pooled, and on the flat LoRA gradient (float64 arithmetic: a float32 cosine is noise at this level) 1 - cosine = 5.81e-5, norm ratio
    1.00067, relative L2 1.081e-2: the reference mode's own error.
    Native must stay within 1.5 x each; the norm ratio may leave 1 by no more than the gradient's relative L2 bound (| |a| - |b| | <=
    |a - b|).  Measured on the MI355X: 7.5e-3, 8.2e-3, 1 - cosine 4.7e-5, relative L2 9.7e-3, ratio 1.0006."""
    REF = dict(states=7.33e-3, pooled=8.21e-3, grad_cos=5.81e-5, grad_l2=1.081e-2)
    cfg = dict(vocab_size=1000, hidden_size=1280, intermediate_size=5120, num_hidden_layers=4, num_attention_heads=20, max_position_embeddings=77)
    ref, nat = _te_pair("cuda", 4, cfg, dict(hidden_act="gelu", projection_dim=1280), clip_skip=1)
    torch.manual_seed(0)                                       # wrap_lora draws W_down from the global generator
    wr = wrap_lora(ref, TE_LORA, rank=4)
    _, group, bucket = make_lora(nat, [dict(layers=TE_LORA, rank=4)])
    gen = torch.Generator().manual_seed(6)
    _sync_lora(wr, group, gen, 0.02)
    bucket.pack()
    ids = torch.randint(0, 998, (2, 77), generator=gen); ids[:, 0] = 998; ids[0, 30:] = 999; ids[1, 50:] = 999
    ts, tp = torch.randn(2, 77, 1280, generator=gen), torch.randn(2, 1280, generator=gen)
    rs, rp = ref.encode_xl(ids, clip_skip=1)
    (F.mse_loss(rs, ts) + F.mse_loss(rp, tp)).backward()
    ns, np_ = nat(ids.cuda())
    (F.mse_loss(ns.float(), ts.cuda()) + F.mse_loss(np_, tp.cuda())).backward()
    es = ((ns.float().cpu() - rs.detach()).norm() / rs.norm()).item()
    ep = ((np_.detach().cpu() - rp.detach()).norm() / rp.norm()).item()
    go, gn = (g.double() for g in _flat_grads(wr, group))
    eg = 1.0 - (go @ gn / (go.norm() * gn.norm())).item()
    el = ((gn - go).norm() / go.norm()).item()
    ratio = (gn.norm() / go.norm()).item()
    print(f"bigG width: states {es:.3g} pooled {ep:.3g} 1-cos(grad) {eg:.3g} rel L2(grad) {el:.3g} norm ratio {ratio:.5f}")
    assert es <= 1.5 * REF["states"] and ep <= 1.5 * REF["pooled"]
    assert eg <= 1.5 * REF["grad_cos"] and el <= 1.5 * REF["grad_l2"] and abs(ratio - 1.0) <= 1.5 * REF["grad_l2"]


def test_name_contract_with_transformers_and_webui(backend):
    """state_dict keys of the native pair == transformers' CLIPTextModel / CLIPTextModelWithProjection under clip_B. / clip_bigG.
    (position_ids buffers aside); lora_convert maps a clip_bigG ... mlp.fc2 block to lora_te2_... and back."""
    tr = pytest.importorskip("transformers")
    from hcp_diffusion_amd import lora_convert
    cb = tr.CLIPTextModel(tr.CLIPTextConfig(**CFG_B, hidden_act="quick_gelu"))
    cg = tr.CLIPTextModelWithProjection(tr.CLIPTextConfig(**CFG_G, **XL_G))

    def keys(m):       # transformers 5 holds CLIPTextModel's transformer flat and writes / reads checkpoints with the text_model. prefix
        ks = [k for k in m.state_dict() if "position_ids" not in k]
        flat = not any(k.startswith("text_model.") for k in ks)
        return {k if (k.startswith("text_projection.") or not flat) else f"text_model.{k}": tuple(v.shape) for k, v in m.state_dict().items() if k in ks}
    want = {f"clip_B.{k}" for k in keys(cb)} | {f"clip_bigG.{k}" for k in keys(cg)}
    _, nat = _pairs(backend.device)
    assert set(nat.state_dict()) == want
    assert {k: tuple(v.shape) for k, v in nat.clip_bigG.state_dict().items()} == keys(cg)
    host = "clip_bigG.text_model.encoder.layers.1.mlp.fc2"
    sd_te = {f"{host}.___.layer.W_down": torch.randn(4, 256), f"{host}.___.layer.W_up": torch.randn(128, 4), f"{host}.___.alpha": torch.tensor(4.0)}
    web = lora_convert.to_webui({}, sd_te, sdxl=True)
    assert "lora_te2_text_model_encoder_layers_1_mlp_fc2.lora_down.weight" in web and not any(k.startswith("lora_te1_") for k in web)
    back = lora_convert.from_webui(web, sdxl=True)[0]["lora"]                # ({'lora': text-encoder part}, {'lora': UNet part})
    assert set(back) == set(sd_te) and all(torch.equal(back[k].float(), sd_te[k]) for k in sd_te)


def test_pair_lora_checkpoint_round_trip(backend, tmp_path):
    """save_model writes both encoders' blocks to the text_encoder file under clip_B. / clip_bigG. names; a fresh pair loads them by name
    and answers bit-identically."""
    from hcp_diffusion_amd.ckpt import CkptManagerNative, NativeModelLoader
    _, _, tr = _trainer(backend.device)
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for blk in tr.te_bucket.blocks:
            blk.layer.W_up.copy_(torch.randn(blk.layer.W_up.shape, generator=gen) * 0.05)
    tr.te_bucket.pack()
    mgr = CkptManagerNative()
    mgr.set_save_dir(str(tmp_path))
    paths = tr.save_model(mgr, step=3)
    assert [os.path.basename(p) for p in paths] == ["unet-3.safetensors", "text_encoder-3.safetensors"]
    sd = mgr.load_ckpt(paths[1])["lora"]
    assert len(sd) == 2 * 2 * 6 * 3                             # 2 encoders x 2 layers x (q, k, v, out, fc1, fc2) x (W_down, W_up, alpha)
    assert "clip_B.text_model.encoder.layers.0.self_attn.q_proj.___.layer.W_down" in sd
    assert "clip_bigG.text_model.encoder.layers.1.mlp.fc2.___.layer.W_up" in sd
    _, fresh = _pairs(backend.device, clip_skip=1)
    NativeModelLoader(fresh).load_lora([dict(path=paths[1], alpha=1.0)])
    ids = backend.to(_pair_ids())
    with torch.no_grad():
        s0, p0 = tr.text_encoder(ids)
        s1, p1 = fresh(ids)
    assert torch.equal(s0, s1) and torch.equal(p0[1], p1[1])


@pytest.mark.skipif(not HAVE_REFERENCE, reason="reference tree only exists in the build container")
def test_pair_matches_the_reference_compose_text_encoder(backend):
    """The reference's OWN ComposeTextEncoder with a TEEXHook on each encoder (compose_textencoder.py:75-91, textencoder_ex.py:61-81),
    run over the restatement exposed with transformers' output fields, returns the tuple NativeSDXLTextEncoder returns."""
    import importlib.util
    pytest.importorskip("einops")
    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
        return mod
    teex = load("_hcp_ref_teex_xl", "/root/reference/hcpdiff/models/textencoder_ex.py")
    comp = load("_hcp_ref_compose_xl", "/root/reference/hcpdiff/models/compose/compose_textencoder.py")
    ref, nat = _pairs(backend.device, clip_skip=1)

    class _Out(dict):
        pooler_output = None

    class HFLike(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m, self.text_model, self.config = m, m.text_model, {}

        def forward(self, input_ids, attention_mask=None, position_ids=None, **kw):
            hs = self.m.hidden_states(input_ids, position_ids, attention_mask)
            out = _Out(hidden_states=hs, last_hidden_state=self.text_model.final_layer_norm(hs[-1]))
            if hasattr(self.m, "text_projection"):                                   # CLIPTextModelWithProjection: pooler_output = text_embeds
                out.pooler_output = self.m.text_projection(out["last_hidden_state"][torch.arange(len(input_ids)), input_ids.argmax(-1)])
            return out

    hosts = [("clip_B", HFLike(ref.clip_B).eval()), ("clip_bigG", HFLike(ref.clip_bigG).eval())]
    for _, h in hosts:
        teex.TEEXHook(h, tokenizer=None, N_repeats=1, clip_skip=1, device="cpu")
    theirs = comp.ComposeTextEncoder(hosts)
    ids = _pair_ids()
    with torch.no_grad():
        ts, tp = theirs(ids, output_hidden_states=True)
        ns, np_ = nat(backend.to(ids), output_hidden_states=True)
    assert tp[0] is None and np_[0] is None and len(tp) == len(np_) == 2
    assert ts.shape == ns.shape and ((ns.float().cpu() - ts).norm() / ts.norm()).item() < 2e-2
    assert ((np_[1].cpu() - tp[1]).norm() / tp[1].norm()).item() < 2e-2
