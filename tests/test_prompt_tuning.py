"""Prompt tuning (tokenizer_pt: textual inversion, DreamArtist, the character-LoRA recipe's subject token) on the native CLIP encoder.

Kernels (csrc/embedding.hip) against the row layout of the reference's EmbeddingPTHook restated in tests/pt_ref.py: forward bit for bit,
backward against a float64 segmented sum.  Encoder: native states and custom-vector gradients against the oracle CLIP driven through the
restated hook, the reference's own class where its tree exists, and a committed fixture that class produced (tools/gen_pt_golden.py).
Trainer: textual inversion against an fp32 torch AdamW loop, clip membership with LoRA, graph against eager, data parallel, checkpoints."""
import importlib
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from hcp_diffusion_amd import kernels as K
from hcp_diffusion_amd.prompt_tuning import EmbeddingPTHook
from hcp_diffusion_amd.text_encoder import NativeCLIPTextModel
from oracle.clip_ref import CLIP_L_CONFIG, TINY_CLIP_CONFIG, OracleCLIPTextModel
from oracle.unet_sd15 import seeded_init_
from pt_ref import RefEmbeddingPTHook, StubTokenizer, backward_f64, expected_rows, forward_rows_f32

GOLD = os.path.join(os.path.dirname(__file__), "golden")
REF = "/root/reference/hcpdiff"
TE_LORA = [r"re:.*self_attn$", r"re:.*mlp$"]


def _tables(vocab, C, npos=77, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(vocab, C, generator=g), torch.randn(npos, C, generator=g) * 0.1


def _words(vocab, C, nvecs, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {vocab + i: torch.randn(n, C, generator=g) for i, n in enumerate(nvecs)}


def _cmap(vocab, emb):
    order = sorted(emb)
    cmap = torch.zeros(max(order) - vocab + 1, 2, dtype=torch.int32)
    off = 0
    for t in order:
        cmap[t - vocab] = torch.tensor([off, emb[t].shape[0]]); off += emb[t].shape[0]
    return torch.cat([emb[t] for t in order]).contiguous(), cmap, order


def _ids(B, R, W, vocab, placements, seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab - 2, (B, R * W), generator=g)
    for b, pos, tid in placements:
        ids[b, pos] = tid
    return ids


# (B, R, nvecs, placements (b, position, word index), with position_ids)
CASES = {
    "one_vec": (2, 1, [1], [(0, 3, 0), (1, 10, 0)], False),
    "four_vec_repeated_adjacent": (2, 1, [4, 2], [(0, 5, 0), (0, 6, 1), (0, 20, 0), (1, 1, 1), (1, 2, 0), (1, 0, 1)], False),
    "cut_at_boundary": (2, 1, [4], [(0, 74, 0), (1, 75, 0)], False),
    "repeats2": (3, 2, [4, 1], [(0, 70, 0), (0, 80, 1), (1, 150, 0), (2, 76, 1), (2, 77, 0)], False),
    "position_ids": (2, 2, [3], [(0, 7, 0), (1, 100, 0)], True),
}


def _case(name, vocab=100, C=64, n_word=75):
    B, R, nvecs, pl, with_pos = CASES[name]
    tok, pos = _tables(vocab, C)
    emb = _words(vocab, C, nvecs)
    ids = _ids(B, R, n_word + 2, vocab, [(b, p, vocab + w) for b, p, w in pl])
    pids = torch.randint(0, 77, (B * R, n_word + 2), generator=torch.Generator().manual_seed(4)) if with_pos else None
    return tok, pos, emb, ids, pids, R, n_word


@pytest.mark.parametrize("name", list(CASES))
def test_embedding_pt_forward_bit_exact(backend, name):
    tok, pos, emb, ids, pids, R, n_word = _case(name)
    table, cmap, _ = _cmap(tok.shape[0], emb)
    out, src = K.embedding_pt_fwd(backend.to(tok), backend.to(ids), backend.to(pos), R, n_word, position_ids=backend.to(pids) if pids is not None else None,
                                  custom_table=backend.to(table), custom_map=backend.to(cmap))
    rows = expected_rows(ids, tok.shape[0], emb, R, n_word)
    ref = forward_rows_f32(rows, tok, pos, emb, pids).to(torch.bfloat16)
    assert out.shape == ref.shape == (ids.shape[0] * R, n_word + 2, tok.shape[1])
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))
    # the source map names a custom row exactly where the reference put a custom vector
    offs, o = {}, 0
    for t in sorted(emb):
        offs[t] = o; o += emb[t].shape[0]
    want = torch.tensor([[s[1] if s[0] == "t" else -1 - (offs[s[1]] + s[2]) for s in r] for r in rows], dtype=torch.int32)
    assert torch.equal(src.cpu(), want)


@pytest.mark.parametrize("name", ["four_vec_repeated_adjacent", "repeats2", "cut_at_boundary"])
def test_embedding_pt_backward_segmented_sum(backend, name):
    tok, pos, emb, ids, pids, R, n_word = _case(name)
    table, cmap, order = _cmap(tok.shape[0], emb)
    out, src = K.embedding_pt_fwd(backend.to(tok), backend.to(ids), backend.to(pos), R, n_word, custom_table=backend.to(table),
                                  custom_map=backend.to(cmap))
    dx = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16)
    g = K.embedding_pt_bwd(backend.to(dx), src, backend.to(torch.full(table.shape, float("nan"))))      # beta 0 never reads the buffer
    ref = backward_f64(expected_rows(ids, tok.shape[0], emb, R, n_word), dx, emb)
    ref = torch.cat([ref[t] for t in order])
    got = g.cpu().double()
    assert ((got - ref).norm() / ref.norm()).item() <= 1e-6
    if name == "cut_at_boundary":                               # vectors pushed past row 75 get no gradient
        assert ref[3].abs().sum() == 0 and got[3].abs().sum() == 0
    g2 = K.embedding_pt_bwd(backend.to(dx), src, backend.to(torch.zeros(table.shape)))
    assert torch.equal(g.cpu().view(torch.int32), g2.cpu().view(torch.int32))                        # bit-reproducible
    base = torch.randn(table.shape, generator=torch.Generator().manual_seed(8))
    g3 = K.embedding_pt_bwd(backend.to(dx), src, backend.to(base.clone()), accumulate=True)
    assert torch.equal(g3.cpu(), base + g.cpu())                                                      # beta = 1 adds


def test_embedding_pt_unregistered_ids_read_the_clipped_row(backend):
    """An id >= vocab without a word (or a map entry of width 0) and a negative id read the clipped token row, never out of bounds."""
    tok, pos = _tables(100, 64)
    emb = _words(100, 64, [2])
    table, cmap, _ = _cmap(100, emb)
    ids = _ids(1, 1, 77, 100, [(0, 4, 100), (0, 9, 5000), (0, 12, -3)])
    out, src = K.embedding_pt_fwd(backend.to(tok), backend.to(ids), backend.to(pos), 1, 75, custom_table=backend.to(table), custom_map=backend.to(cmap))
    s = src.cpu()[0]
    assert s[4] == -1 and s[5] == -2 and s[10] == 99 and s[13] == 0


def test_embedding_pt_rejects_bad_arguments():
    from hcp_diffusion_amd import _lib
    lib = _lib.load()
    N = None
    assert lib.hcp_embedding_pt_fwd_bf16(N, 1, 1, 77, 75, N, 100, N, N, 77, N, 0, N, 0, N, N, 64, N) < 0
    one = 16
    assert lib.hcp_embedding_pt_fwd_bf16(one, 1, 1, 70, 75, one, 100, one, N, 77, N, 0, N, 0, one, one, 64, N) < 0     # r*w < r*n_word + 1
    assert b"n_word" in lib.hcp_last_error()
    assert lib.hcp_embedding_pt_bwd_f32(N, N, 0, 64, N, 1, 0, N) < 0


# ---------------------------------------------------------------- encoder

def _te_pair(dev, n_repeats=1, seed=5):
    ora = seeded_init_(OracleCLIPTextModel(**TINY_CLIP_CONFIG), seed)
    nat = NativeCLIPTextModel(**TINY_CLIP_CONFIG, N_repeats=n_repeats)
    nat.load_state_dict(ora.state_dict())
    return ora, nat.to(dev)


def _hook_both(ora, nat, words, dev, n_repeats, trainable=True):
    """The restated reference hook on the oracle, the native twin on the native encoder, the same vectors (separate Parameters)."""
    tok_o, tok_n = StubTokenizer(100), StubTokenizer(100)
    po = {w: torch.nn.Parameter(v.clone(), requires_grad=trainable) for w, v in words.items()}
    pn = {w: torch.nn.Parameter(v.clone().to(dev), requires_grad=trainable) for w, v in words.items()}
    tok_o.add_tokens(list(po)); tok_n.add_tokens(list(pn))
    ho = RefEmbeddingPTHook(ora.text_model.embeddings.token_embedding, N_word=75, N_repeats=n_repeats)
    for w in po:
        ho.add_emb(po[w], tok_o.added[w])
    hn = EmbeddingPTHook.hook(pn, tok_n, nat, N_repeats=n_repeats)
    return po, pn, ho, hn, tok_n


@pytest.mark.parametrize("n_repeats", [1, 2])
def test_tiny_encoder_with_custom_words_vs_oracle(backend, n_repeats):
    dev = backend.device
    ora, nat = _te_pair(dev, n_repeats)
    ora.requires_grad_(False); nat.requires_grad_(False)
    g = torch.Generator().manual_seed(11)
    words = {"pt-a": torch.randn(4, 128, generator=g) * 0.5, "pt-b": torch.randn(1, 128, generator=g) * 0.5}
    po, pn, ho, hn, tk = _hook_both(ora, nat, words, dev, n_repeats)
    ida, idb = tk.added["pt-a"], tk.added["pt-b"]
    ids = torch.randint(0, 98, (2, 77 * n_repeats), generator=g); ids[:, 0] = 98
    ids[0, 3] = ida; ids[0, 4] = idb; ids[1, 20] = ida; ids[1, 73] = ida
    target = torch.randn(2, 75 * n_repeats + 2, 128, generator=g)
    ref = ora.encode(ids, n_repeats=n_repeats)
    F.mse_loss(ref, target).backward()
    out = nat(backend.to(ids))
    assert out.shape == ref.shape
    assert ((out.float().cpu() - ref.detach()).norm() / ref.norm()).item() < 2e-2
    F.mse_loss(out.float(), backend.to(target)).backward()
    go = torch.cat([po[w].grad.flatten() for w in words]); gn = torch.cat([pn[w].grad.flatten().cpu() for w in words])
    assert go.norm() > 0 and F.cosine_similarity(go, gn, dim=0).item() > 0.995
    assert (gn.norm() / go.norm()).item() == pytest.approx(1.0, abs=3e-2)
    assert torch.equal(nat.get_input_embeddings().weight, nat.text_model.embeddings.token_embedding.weight)


def test_encoder_hook_changes_the_output_and_refuses_unknown_ids(backend):
    """Without a hook the custom words would be ignored (read out of the table); with it they are the words' vectors.  Ids beyond the
    vocabulary without a word are refused while they are on the host."""
    dev = backend.device
    ora, nat = _te_pair(dev)
    ora.requires_grad_(False); nat.requires_grad_(False)
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(0, 98, (1, 77), generator=g)
    with torch.no_grad():
        plain = nat(backend.to(ids)).float().cpu()
    _, pn, _, hn, tk = _hook_both(ora, nat, {"w": torch.randn(2, 128, generator=g)}, dev, 1, trainable=False)
    ids2 = ids.clone(); ids2[0, 5] = tk.added["w"]
    with torch.no_grad():
        hooked = nat(backend.to(ids2)).float().cpu()
        same = nat(backend.to(ids)).float().cpu()
    assert torch.equal(same, plain) and not torch.allclose(hooked, plain, atol=1e-2)
    if not backend.is_gpu:
        ids3 = ids.clone(); ids3[0, 7] = 150
        with pytest.raises(KeyError):
            nat(ids3)
    hn.remove()
    assert getattr(nat.text_model.embeddings.token_embedding, "emb_ex", None) is None


def _load_reference_pt_hook():
    """The reference's own EmbeddingPTHook, executed where it lies (oracle/ref_shims.py stubs the packages; loguru is stubbed here)."""
    from oracle.ref_shims import load_reference_lora
    load_reference_lora()
    if "loguru" not in sys.modules:
        lg = types.ModuleType("loguru")
        lg.logger = types.SimpleNamespace(info=lambda *a, **k: None)
        sys.modules["loguru"] = lg
    return importlib.import_module("hcpdiff.models.text_emb_ex").EmbeddingPTHook, importlib.import_module("hcpdiff.utils.net_utils")


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
def test_reference_hook_class_drives_native_and_oracle_alike():
    """The reference's own EmbeddingPTHook.hook(...) attached to NativeCLIPTextModel (read by the native path) and to the oracle CLIP
    (fires as torch hooks): same states."""
    RefHook, _ = _load_reference_pt_hook()
    ora, nat = _te_pair("cpu", 2)
    from conftest import emu_cdll
    K._set_backend_for_tests(emu_cdll())
    try:
        g = torch.Generator().manual_seed(13)
        words = {"pt-x": torch.randn(3, 128, generator=g), "pt-y": torch.randn(2, 128, generator=g)}
        to, tn = StubTokenizer(100), StubTokenizer(100)
        RefHook.hook({w: torch.nn.Parameter(v.clone()) for w, v in words.items()}, to, _HFish(ora), N_repeats=2)
        RefHook.hook({w: torch.nn.Parameter(v.clone()) for w, v in words.items()}, tn, nat, N_repeats=2)
        ids = torch.randint(0, 98, (2, 154), generator=g)
        ids[0, 10] = to.added["pt-x"]; ids[0, 11] = to.added["pt-y"]; ids[1, 76] = to.added["pt-x"]; ids[1, 120] = to.added["pt-y"]
        with torch.no_grad():
            ref = ora.encode(ids, n_repeats=2)
            out = nat(ids).float()
        assert ((out - ref).norm() / ref.norm()).item() < 2e-2
    finally:
        K._set_backend_for_tests(None)


class _HFish:
    """get_input_embeddings() of a transformers CLIPTextModel, for the oracle."""

    def __init__(self, m):
        self.m = m

    def get_input_embeddings(self):
        return self.m.text_model.embeddings.token_embedding


def test_encoder_matches_the_reference_hook_fixture(backend):
    """tests/golden/pt_reference.pt: states the reference's own EmbeddingPTHook produced on the oracle (tools/gen_pt_golden.py)."""
    gold = torch.load(os.path.join(GOLD, "pt_reference.pt"))
    nat = NativeCLIPTextModel(**gold["config"], N_repeats=gold["n_repeats"])
    nat.load_state_dict(gold["state"]); nat.to(backend.device)
    tk = StubTokenizer(gold["config"]["vocab_size"])
    words = {w: torch.nn.Parameter(v.to(backend.device)) for w, v in gold["words"].items()}
    EmbeddingPTHook.hook(words, tk, nat, N_repeats=gold["n_repeats"])
    with torch.no_grad():
        out = nat(backend.to(gold["ids"])).float().cpu()
    ref = gold["states"]
    assert ((out - ref).norm() / ref.norm()).item() < 2e-2
    emb_rows = gold["embeddings"]               # the hook's output before the encoder: bit for bit after bf16 rounding
    from hcp_diffusion_amd import ops
    e = nat.text_model.embeddings
    x = ops.embedding_pt(backend.to(gold["ids"]).contiguous(), e.token_embedding.weight.detach(), e.position_embedding.weight.detach(),
                         e.token_embedding.emb_ex)
    assert torch.equal(x.cpu().view(torch.int16), emb_rows.to(torch.bfloat16).view(torch.int16))


@pytest.mark.gpu
def test_clip_l_full_size_four_vector_word_vs_oracle():
    """Full CLIP-L (seeded), B = 4 prompts each holding a 4-vector word: states and the word's gradient vs the fp32 oracle."""
    ora = seeded_init_(OracleCLIPTextModel(**CLIP_L_CONFIG), 4)
    nat = NativeCLIPTextModel(**CLIP_L_CONFIG)
    nat.load_state_dict(ora.state_dict()); nat.to("cuda")
    ora.requires_grad_(False); nat.requires_grad_(False)
    gen = torch.Generator().manual_seed(21)
    v = torch.randn(4, 768, generator=gen) * 0.02
    po, pn = torch.nn.Parameter(v.clone()), torch.nn.Parameter(v.clone().cuda())
    ho = RefEmbeddingPTHook(ora.text_model.embeddings.token_embedding, N_word=75, N_repeats=1); ho.add_emb(po, 49408)
    tk = StubTokenizer(49408, bos=49406, eos=49407)
    EmbeddingPTHook.hook({"sks": pn}, tk, nat, N_repeats=1)
    ids = torch.randint(0, 49406, (4, 77), generator=gen); ids[:, 0] = 49406; ids[:, 30:] = 49407
    for b in range(4):
        ids[b, 2 + 5 * b] = 49408
    target = torch.randn(4, 77, 768, generator=gen)
    ref = ora.encode(ids)
    F.mse_loss(ref, target).backward()
    out = nat(ids.cuda())
    assert ((out.float().cpu() - ref.detach()).norm() / ref.norm()).item() < 2e-2
    F.mse_loss(out.float(), target.cuda()).backward()
    assert F.cosine_similarity(po.grad.flatten(), pn.grad.flatten().cpu(), dim=0).item() > 0.99
