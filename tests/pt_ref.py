"""TEST ORACLE: restatement of the reference's EmbeddingPTHook (hcpdiff/models/text_emb_ex.py:21-69) in plain torch, for the oracle CLIP
text model (oracle/clip_ref.py calls ``token_embedding`` as a module, so the hook's forward pre-hook and forward hook fire there as they
do on transformers' CLIPTextModel).  Also: a float64 restatement of the forward row layout for the kernel tests, and a tokenizer stub
with the two methods EmbeddingPTHook.hook uses."""
import torch
from torch import nn


class RefEmbeddingPTHook(nn.Module):
    def __init__(self, token_embedding, N_word=75, N_repeats=3):
        super().__init__()
        self.name = "emb_ex"
        self._host = [token_embedding]
        setattr(token_embedding, "emb_ex", self)
        self.handle_pre = token_embedding.register_forward_pre_hook(self.pre_hook)
        self.handle = token_embedding.register_forward_hook(lambda host, fea_in, fea_out: self(fea_in, fea_out))
        self.N_word, self.N_repeats = N_word, N_repeats
        self.num_embeddings, self.embedding_dim = token_embedding.num_embeddings, token_embedding.embedding_dim
        self.emb = {}
        self.emb_train = nn.ParameterList()

    def add_emb(self, emb, token_id):
        self.emb[token_id] = emb

    def pre_hook(self, host, input_ids):
        x = input_ids[0]
        self.input_ids = x.reshape(x.shape[0] // self.N_repeats, -1)          # '(b r) w -> b (r w)'
        return self.input_ids.clip(0, self.num_embeddings - 1)

    def forward(self, fea_in, inputs_embeds):
        rep_idxs_B = self.input_ids >= self.num_embeddings
        BOS = inputs_embeds[0, 0, :].expand(self.N_repeats, 1, -1)
        EOS = inputs_embeds[0, -1, :].expand(self.N_repeats, 1, -1)
        out = []
        for item, rep_idxs, ids_raw in zip(inputs_embeds, rep_idxs_B, self.input_ids):
            item_new, last = [], 0
            for rep_idx in torch.where(rep_idxs)[0].tolist():
                item_new.append(item[last:rep_idx, :])
                item_new.append(self.emb[ids_raw[rep_idx].item()].to(dtype=item.dtype))
                last = rep_idx + 1
            item_new.append(item[last:, :])
            rep = torch.cat(item_new, dim=0)[1:self.N_word * self.N_repeats + 1, :]
            rep = rep.reshape(self.N_repeats, self.N_word, -1)
            out.append(torch.cat([BOS, rep, EOS], dim=1))
        return torch.cat(out, dim=0)

    def remove(self):
        self.handle_pre.remove(); self.handle.remove()
        delattr(self._host[0], self.name)


def expected_rows(ids, vocab, emb, n_repeats, n_word):
    """Per output row of the forward, its source: ('t', token row) or ('c', token id, vector index).  ids [B, r*w] int64."""
    B = ids.shape[0]
    bos, eos = ("t", int(ids[0, 0].clamp(0, vocab - 1))), ("t", int(ids[0, -1].clamp(0, vocab - 1)))
    rows = []
    for b in range(B):
        seq = []
        for t in ids[b].tolist():
            if t >= vocab:
                seq += [("c", t, k) for k in range(emb[t].shape[0])]
            else:
                seq.append(("t", min(max(t, 0), vocab - 1)))
        keep = seq[1:n_word * n_repeats + 1]
        for k in range(n_repeats):
            rows.append([bos] + keep[k * n_word:(k + 1) * n_word] + [eos])
    return rows


def forward_rows_f32(rows, tok, pos, emb, position_ids=None):
    """fp32 src + pos per row (what the kernel must round to bf16 bit for bit)."""
    out = []
    for i, r in enumerate(rows):
        o = []
        for j, s in enumerate(r):
            v = tok[s[1]] if s[0] == "t" else emb[s[1]][s[2]]
            p = int(position_ids[i, j]) if position_ids is not None else j
            o.append(v.float() + pos[p].float())
        out.append(torch.stack(o))
    return torch.stack(out)


def backward_f64(rows, dx, emb):
    """{token id: float64 [n_vec, C]} = segmented sum of dX over the rows each vector landed in."""
    g = {t: torch.zeros(e.shape, dtype=torch.float64) for t, e in emb.items()}
    d = dx.double()
    for i, r in enumerate(rows):
        for j, s in enumerate(r):
            if s[0] == "c":
                g[s[1]][s[2]] += d[i, j]
    return g


class StubTokenizer:
    """What EmbeddingPTHook.hook needs of a CLIPTokenizer: add_tokens, __call__(text).input_ids (BOS ... EOS), model_max_length."""

    def __init__(self, vocab, model_max_length=77, bos=None, eos=None):
        self.vocab, self.model_max_length = vocab, model_max_length
        self.bos, self.eos = (vocab - 2 if bos is None else bos), (vocab - 1 if eos is None else eos)
        self.added = {}

    def add_tokens(self, words):
        for w in words:
            if w not in self.added:
                self.added[w] = self.vocab + len(self.added)

    def __call__(self, text):
        class _Out:
            pass
        o = _Out()
        o.input_ids = [self.bos] + [self.added[w] for w in text.split()] + [self.eos]
        return o
