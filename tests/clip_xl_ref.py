"""TEST HELPER: plain-torch restatement of what SDXL's text path adds over CLIP-L — ``hidden_act`` ("gelu": exact erf GELU), the
pooled output of ``CLIPTextModelWithProjection`` (``text_projection(final_layer_norm(last)[eos])``, eos = first position of the
maximum id: transformers' rule for ``eos_token_id == 2``) and the composed pair (hcpdiff/models/compose/compose_textencoder.py:75-91
with a TEEXHook on each encoder, textencoder_ex.py:65-81).  Built on the CLIP-L oracle (oracle/clip_ref.py); pinned against the
installed transformers by tests/test_text_encoder_xl.py."""
import torch
import torch.nn.functional as F
from torch import nn

from oracle.clip_ref import CLIPMLP, OracleCLIPTextModel


class _GeluMLP(CLIPMLP):
    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class RefCLIPTextModelXL(OracleCLIPTextModel):
    """Parameter names of transformers' CLIPTextModel(WithProjection): ``text_model.*`` (+ ``text_projection.weight``)."""

    def __init__(self, hidden_act="quick_gelu", projection_dim=None, **cfg):
        super().__init__(**cfg)
        assert hidden_act in ("quick_gelu", "gelu")
        if hidden_act == "gelu":
            for layer in self.text_model.encoder.layers:
                layer.mlp.__class__ = _GeluMLP
        if projection_dim is not None:
            self.text_projection = nn.Linear(self.config["hidden_size"], projection_dim, bias=False)

    def encode_xl(self, input_ids, clip_skip=0, final_norm=True, attention_mask=None, n_repeats=1):
        """(states, pooled) as TEEXHook.forward_hook returns them: states = encode(...); pooled = the r chunks' text_embeds averaged
        (None without a projection)."""
        B, r = input_ids.shape[0], n_repeats
        ids = input_ids.reshape(B * r, -1)
        mask = attention_mask.reshape(B * r, -1) if attention_mask is not None else None
        hs = self.hidden_states(ids, None, mask)
        h = hs[-clip_skip - 1]
        h = self.text_model.final_layer_norm(h) if final_norm else h
        if r > 1:
            h = h.reshape(B, r, *h.shape[1:])
            h = torch.cat([h[:, 0, :1, :], h[:, :, 1:-1, :].flatten(1, 2), h[:, -1, -1:, :]], dim=1)
        pooled = None
        if hasattr(self, "text_projection"):
            last = self.text_model.final_layer_norm(hs[-1])
            eos = ids.argmax(-1)                                       # torch: the first of several maxima
            pooled = self.text_projection(last[torch.arange(B * r), eos]).reshape(B, r, -1).mean(1)
        return h, pooled


class RefSDXLTextEncoder(nn.Module):
    def __init__(self, clip_B, clip_bigG, **sel):
        super().__init__()
        self.clip_B, self.clip_bigG, self.sel = clip_B, clip_bigG, sel

    def forward(self, input_ids, attention_mask=None):
        a, b = input_ids.chunk(2, dim=-1)
        sa, pa = self.clip_B.encode_xl(a, attention_mask=attention_mask, **self.sel)
        sb, pb = self.clip_bigG.encode_xl(b, attention_mask=attention_mask, **self.sel)
        return torch.cat([sa, sb], -1), [pa, pb]


def pool_ref(x, ids, gamma, beta, w, r, dtype):
    """The pooling kernel's definition on the given inputs, evaluated in `dtype`: LayerNorm of the first-maximum token, projection,
    mean over the r chunks.  x [B*r, L, C]."""
    M, _, C = x.shape
    tok = x.to(dtype)[torch.arange(M), ids.argmax(-1)]
    y = F.layer_norm(tok, (C,), gamma.to(dtype), beta.to(dtype), 1e-5) @ w.to(dtype).T
    return y.reshape(M // r, r, -1).mean(1)
