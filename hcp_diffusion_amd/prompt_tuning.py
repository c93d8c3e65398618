"""Prompt tuning on the native CLIP text encoder: trainable custom words (textual inversion, DreamArtist, the character-LoRA recipe's
subject token — ``tokenizer_pt`` in the reference's configs).

The reference installs ``EmbeddingPTHook`` (hcpdiff/models/text_emb_ex.py:21-87) on ``text_encoder.get_input_embeddings()``: a plugin
named ``emb_ex`` whose ``emb`` dict maps every custom token id (appended to the tokenizer, so >= vocab) to its vectors [n_vec, C].
NativeCLIPTextModel never calls the ``token_embedding`` module — it reads the hook's ``emb`` / ``N_word`` / ``N_repeats`` instead and
runs csrc/embedding.hip (``ops.embedding_pt``).  Either hook class works: the reference's own, or ``EmbeddingPTHook`` below, a
restatement usable without ``hcpdiff`` (same name, attributes, ``hook`` / ``hook_from_dir`` class methods, submodule placement).

``PTBucket`` re-homes the trained words into one flat fp32 bucket for NativeTrainer (per-word lr segments, fused AdamW), and the
backward kernel adds their gradients straight into it.
"""
import os
import weakref

import torch
from torch import nn

from .patch_api import BasePluginBlock


class EmbeddingPTHook(BasePluginBlock):
    """Native twin of the reference's EmbeddingPTHook: a data holder.  It registers no torch hooks — the native encoder reads it."""

    def __init__(self, token_embedding: nn.Embedding, N_word=75, N_repeats=3):
        super().__init__("emb_ex")
        self.host = weakref.ref(token_embedding)
        setattr(token_embedding, "emb_ex", self)          # SinglePluginBlock.__init__ (plugin.py:112)
        self.N_word, self.N_repeats = N_word, N_repeats
        self.num_embeddings, self.embedding_dim = token_embedding.num_embeddings, token_embedding.embedding_dim
        self.emb = {}
        self.emb_train = nn.ParameterList()

    def add_emb(self, emb: nn.Parameter, token_id: int):
        self.emb[token_id] = emb

    def remove(self):
        host = self.host()
        if host is not None:
            delattr(host, self.name)

    @classmethod
    def hook(cls, ex_words_emb, tokenizer, text_encoder, log=False, **kwargs):
        """text_emb_ex.py:72-82: add the words to the tokenizer, attach the hook, register every word's vectors under its token id."""
        word_list = list(ex_words_emb.keys())
        tokenizer.add_tokens(word_list)
        token_ids = tokenizer(" ".join(word_list)).input_ids[1:-1]
        embedding_hook = cls(text_encoder.get_input_embeddings(), N_word=tokenizer.model_max_length - 2, **kwargs)
        for tid, word in zip(token_ids, word_list):
            embedding_hook.add_emb(ex_words_emb[word], tid)
            if log:
                print(f"hook: {word}, len: {ex_words_emb[word].shape[0]}, id: {tid}")
        return embedding_hook

    @classmethod
    def hook_from_dir(cls, emb_dir, tokenizer, text_encoder, log=True, device="cuda:0", **kwargs):
        from .ckpt import load_emb
        ex_words_emb = {file[:-3]: nn.Parameter(load_emb(os.path.join(emb_dir, file)).to(device), requires_grad=False)
                        for file in os.listdir(emb_dir) if file.endswith(".pt")}
        return cls.hook(ex_words_emb, tokenizer, text_encoder, log, **kwargs), ex_words_emb


def find_hook(text_encoder):
    """The ``emb_ex`` plugin on the encoder's token embedding (either class), or None."""
    emb = text_encoder.get_input_embeddings() if hasattr(text_encoder, "get_input_embeddings") else None
    return getattr(emb, "emb_ex", None) if emb is not None else None


class _Layout:
    """What the kernels read for one state of a hook: the words in table order, the dense id map, and the flat table when the words
    already lie back to back in one fp32 storage (a PTBucket's parameters: no copy per call)."""

    def __init__(self, items, vocab, device):
        self.items = items                                   # [(token id, parameter)] in table order
        self.params = [p for _, p in items]
        self.rows = [p.shape[0] for p in self.params]
        self.n_rows = sum(self.rows)
        cmap = torch.zeros((max((t for t, _ in items), default=vocab - 1) - vocab + 1, 2), dtype=torch.int32)
        off = 0
        for (t, p), n in zip(items, self.rows):
            cmap[t - vocab] = torch.tensor([off, n], dtype=torch.int32)
            off += n
        self.cmap = cmap.to(device)
        self.flat = None
        if self.params and all(p.dtype == torch.float32 and p.is_contiguous() for p in self.params):
            p0 = self.params[0]
            st, o = p0.untyped_storage().data_ptr(), p0.storage_offset()
            ok = True
            for p in self.params:
                if p.untyped_storage().data_ptr() != st or p.storage_offset() != o:
                    ok = False
                    break
                o += p.numel()
            if ok:
                C = p0.shape[1]
                self.flat = p0.detach().as_strided((self.n_rows, C), (C, 1), p0.storage_offset())

    def table(self):
        if not self.params:
            return None
        if self.flat is not None:
            return self.flat
        return torch.cat([p.detach().float().reshape(p.shape[0], -1) for p in self.params]).contiguous()


def layout(hook, device):
    """Cached _Layout of the hook's current words.  Table order: the order a PTBucket laid them out in (trained words first), else by
    token id.  Rebuilt when a word, a parameter or its storage changes (host work only, no device sync)."""
    order = getattr(hook, "_pt_order", None)
    tids = list(order) + sorted(t for t in hook.emb if t not in order) if order else sorted(hook.emb)
    items = [(t, hook.emb[t]) for t in tids]
    for t, p in items:
        if t < hook.num_embeddings:
            raise ValueError(f"prompt tuning: custom token id {t} lies inside the vocabulary ({hook.num_embeddings})")
        if p.dim() != 2 or p.shape[1] != hook.embedding_dim:
            raise ValueError(f"prompt tuning: word {t} has vectors of shape {tuple(p.shape)}, expected [n, {hook.embedding_dim}]")
        if p.device != torch.device(device):
            raise ValueError(f"prompt tuning: word {t} lives on {p.device}, the ids on {device}")
    key = (str(device), tuple((t, id(p), tuple(p.shape), p.data_ptr(), p.dtype) for t, p in items))
    hit = getattr(hook, "_pt_layout", None)
    if hit is None or hit[0] != key:
        hit = (key, _Layout(items, hook.num_embeddings, device))
        hook._pt_layout = hit
    return hit[1]


def check_ids(hook, ids):
    """Host-side refusal of custom ids without a registered word (the reference raises KeyError on them).  Only for ids already on
    the host — a device tensor would cost a sync; there the kernel reads the clipped table row (csrc/embedding.hip)."""
    if ids.is_cuda:
        return
    bad = sorted({int(t) for t in ids[ids >= hook.num_embeddings].unique().tolist()} - set(int(t) for t in hook.emb))
    if bad:
        raise KeyError(f"prompt tuning: token ids {bad[:8]} are beyond the vocabulary ({hook.num_embeddings}) and no word is registered for them")


class PTBucket:
    """The trained words of a hook in ONE flat fp32 bucket (NativeTrainer): each Parameter's storage is re-homed into ``params`` (the
    objects keep their identity — the hook's ``emb`` dict and the caller's word dict still hold them), ``grads`` is where the backward
    kernel adds their gradients (``hook._pt_sink``), and ``segments`` are the per-word (offset, numel, lr) of the optimizer."""

    def __init__(self, hook, words):
        """words: [(name, parameter, lr)] in cfg order; every parameter must be registered in hook.emb."""
        by_param = {id(p): t for t, p in hook.emb.items()}
        order, segs, off = [], [], 0
        for name, p, lr in words:
            if id(p) not in by_param:
                raise ValueError(f"prompt tuning: word {name!r} is not registered in the embedding hook")
            order.append(by_param[id(p)])
            segs.append((off, p.numel(), lr))
            off += p.numel()
        dev = words[0][1].device
        self.params = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(off, dtype=torch.float32, device=dev)
        self.segments, self.names = segs, [w[0] for w in words]
        self.words = [w[1] for w in words]
        with torch.no_grad():
            for (o, n, _), p in zip(segs, self.words):
                self.params[o:o + n].copy_(p.detach().reshape(-1))
                p.data = self.params[o:o + n].view(p.shape)
                p.requires_grad_(True)
                p.grad = self.grads[o:o + n].view(p.shape)
        self.hook = hook
        hook._pt_order = order
        hook._pt_sink = self.grads.view(-1, hook.embedding_dim)
        if hasattr(hook, "emb_train"):                        # train_ac.py:355: the trained words are submodules of the hook
            for p in self.words:
                if all(p is not q for q in hook.emb_train):
                    hook.emb_train.append(p)

    def refresh(self):                                        # (bucket protocol of NativeTrainer: the kernels read fp32 directly)
        pass

    def named_tensors(self):
        return list(zip(self.names, self.words))
