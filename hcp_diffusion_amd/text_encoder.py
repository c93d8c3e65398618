"""Native CLIP text encoder — the host of the reference's text-encoder LoRA.

The reference's default LoRA example trains ``lora_text_encoder`` next to ``lora_unet``
(cfgs/train/examples/lora_conventional.yaml:14-19: rank-4 blocks on ``re:.*self_attn$`` and ``re:.*mlp$``), which makes the
whole ``TEUnetWrapper`` differentiable (hcpdiff/models/wrapper.py:14-30, train_ac.py:61,160-162): the prompt is encoded inside
the step, and the UNet's cross-attention K/V projections pass a gradient back into the encoder's LoRA factors.

Same module tree, parameter names and shapes as transformers' ``CLIPTextModel`` as dumped in the reference's cfgs/te_struct.txt
(``text_model.embeddings.token_embedding`` ... ``text_model.final_layer_norm``), so checkpoints load by name and the
``re:.*self_attn$`` / ``re:.*mlp$`` selectors wrap the same Linear leaves.  Every leaf is a ``HipLinear`` / ``HipLayerNorm``:
LoRA blocks are the UNet's own ``LoraHipLayer`` (one flat bucket, grouped weight-gradient launch, fused clip + AdamW).
Kernels: ``hcp_embedding_bf16`` (or, with a prompt-tuning ``emb_ex`` hook on ``token_embedding``,
``hcp_embedding_pt_fwd_bf16`` / ``_bwd_f32``: prompt_tuning.py), LayerNorm, fused-LoRA GEMM, flash attention with ``causal=1`` (12 x 64 heads, 77 tokens),
``hcp_quick_gelu``.  Output selection follows ``TEEXHook.forward_hook`` (textencoder_ex.py:62-79) for N_repeats = 1:
``final_layer_norm(hidden_states[-clip_skip-1])``; ``N_repeats`` > 1 (``tokenizer_repeats``) encodes [B, r x 77] ids as B r prompts and stitches
the chunks back with one BOS and one EOS, as the hook does.

SDXL: ``hidden_act="gelu"`` (``hcp_gelu``) and ``projection_dim`` (``text_projection.weight``; the pooled output
``text_projection(final_layer_norm(last)[eos])`` from ``hcp_clip_pool_fwd`` / ``_bwd``) make the same class bigG's
``CLIPTextModelWithProjection``; ``NativeSDXLTextEncoder`` composes ``clip_B`` and ``clip_bigG`` like the reference's ``ComposeTextEncoder``.
"""
import json
import os

import torch
from torch import nn

from . import kernels as K
from . import ops
from .dropout import NativeDropoutMixin
from .layers import HipLayerNorm, HipLinear

BF16 = torch.bfloat16
CLIP_L_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                     max_position_embeddings=77)


# what bigG (CLIPTextModelWithProjection, SDXL's text_encoder_2) adds over CLIP-L: the MLP activation and the pooled projection
_XL_DEFAULTS = dict(hidden_act="quick_gelu", projection_dim=None)
CONFIG_KEYS = tuple(CLIP_L_CONFIG) + tuple(_XL_DEFAULTS)


class _Config(dict):
    __getattr__ = dict.__getitem__          # transformers configs answer cfg.hidden_size as well as cfg['hidden_size']


def _call(m, x, residual=None):
    return m(x, residual=residual) if residual is not None else m(x)


class CLIPAttention(nn.Module):
    def __init__(self, c, heads):
        super().__init__()
        self.k_proj = HipLinear(c, c); self.v_proj = HipLinear(c, c); self.q_proj = HipLinear(c, c); self.out_proj = HipLinear(c, c)
        self.heads = heads

    def forward(self, x, residual, key_bias=None):
        q, k, v = self.q_proj(x), self.k_proj(x), self.v_proj(x)
        return _call(self.out_proj, ops.attention(q, k, v, self.heads, key_bias=key_bias, causal=True), residual)


_ACTS = {"quick_gelu": ops.quick_gelu, "gelu": ops.gelu}          # CLIP-L / clip_B: quick_gelu; bigG: exact erf GELU (config.json hidden_act)


class CLIPMLP(nn.Module):
    def __init__(self, c, inner, act="quick_gelu"):
        super().__init__()
        self.fc1 = HipLinear(c, inner); self.fc2 = HipLinear(inner, c)
        self.act = _ACTS[act]

    def forward(self, x, residual):
        return _call(self.fc2, self.act(self.fc1(x)), residual)


class CLIPEncoderLayer(nn.Module):
    def __init__(self, c, heads, inner, act="quick_gelu"):
        super().__init__()
        self.self_attn = CLIPAttention(c, heads)
        self.layer_norm1 = HipLayerNorm(c, eps=1e-5)
        self.mlp = CLIPMLP(c, inner, act)
        self.layer_norm2 = HipLayerNorm(c, eps=1e-5)

    def forward(self, x, key_bias=None):
        h, x = self.layer_norm1(x, fork=True)                 # fork: backward adds the residual-path gradient inside the LN kernel
        x = self.self_attn(h, x, key_bias)                    # residual add fused into the out_proj GEMM epilogue
        h, x = self.layer_norm2(x, fork=True)
        return self.mlp(h, x)


class _Embeddings(nn.Module):
    def __init__(self, vocab, c, npos):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, c)
        self.position_embedding = nn.Embedding(npos, c)


class _Encoder(nn.Module):
    def __init__(self, c, heads, inner, n, act="quick_gelu"):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(c, heads, inner, act) for _ in range(n)])


class _TextTransformer(nn.Module):
    def __init__(self, vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, max_position_embeddings,
                 hidden_act="quick_gelu"):
        super().__init__()
        self.embeddings = _Embeddings(vocab_size, hidden_size, max_position_embeddings)
        self.encoder = _Encoder(hidden_size, num_attention_heads, intermediate_size, num_hidden_layers, hidden_act)
        self.final_layer_norm = HipLayerNorm(hidden_size, eps=1e-5)


class NativeCLIPTextModel(NativeDropoutMixin, nn.Module):
    dropout_module_index = 1
    def __init__(self, clip_skip=0, clip_final_norm=True, N_repeats=1, **cfg):
        super().__init__()
        self.config = _Config({**CLIP_L_CONFIG, **_XL_DEFAULTS, **{k: v for k, v in cfg.items() if k in CONFIG_KEYS}})
        if self.config["hidden_act"] not in _ACTS:
            raise NotImplementedError(f"hcp_diffusion_amd: text-encoder hidden_act={self.config['hidden_act']!r} (quick_gelu or gelu)")
        if self.config["hidden_size"] // self.config["num_attention_heads"] not in (40, 64, 80, 160):
            raise NotImplementedError("hcp_diffusion_amd: text-encoder head width must be one of 40/64/80/160")
        self.text_model = _TextTransformer(**{k: v for k, v in self.config.items() if k != "projection_dim"})
        if self.config["projection_dim"] is not None:         # CLIPTextModelWithProjection: same names, plus text_projection.weight
            self.text_projection = nn.Linear(self.config["hidden_size"], self.config["projection_dim"], bias=False)
        self.clip_skip, self.clip_final_norm, self.N_repeats = clip_skip, clip_final_norm, N_repeats

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    @property
    def dtype(self):                                   # utils/pipe_hook.py:25-26 casts the prompt states to text_encoder.dtype
        return self.text_model.final_layer_norm.weight.dtype

    def get_input_embeddings(self):              # transformers' CLIPTextModel API: EmbeddingPTHook.hook attaches its plugin here
        return self.text_model.embeddings.token_embedding

    def enable_hip_graph(self, on=True):
        """As NativeUNet2DConditionModel.enable_hip_graph: under an ordinary eager trainer loop the encoder's forward and backward
        (text-encoder LoRA training, lora_conventional.yaml:14-19) replay captured hipGraphs, one pair per input signature."""
        self._hip_graph, self._hip_graphs = bool(on), {}
        self._hcp_capturable = None
        if getattr(self, "_hcp_dropout", None) is not None:
            self._hcp_dropout._key = None              # renumber the dropout layers at the next forward
        self.pack_projection()

    def forward(self, input_ids, position_ids=None, attention_mask=None, output_hidden_states=None):
        if (getattr(self, "_hip_graph", False) and torch.is_grad_enabled() and input_ids.is_cuda
                and not torch.cuda.is_current_stream_capturing()):
            from . import graphed
            # prompt tuning stays eager: the hook's word dict is Python state read at every call (words can be added or re-homed between
            # steps, like the per-step forward hooks capturable() refuses), and the custom vectors' gradient leaves through autograd or
            # the trainer's sink, not through the LoRA / host buckets the captured backward writes.  (NativeTrainer(use_graph=True)
            # captures the whole step, the prompt-tuning kernels included.)
            # With projection_dim the forward has two outputs (states, pooled) and stays eager as well: graphed.call replays one output
            # tensor and its gradient.  (NativeTrainer(use_graph=True) captures the whole step, both outputs included.)
            if (getattr(self.text_model.embeddings.token_embedding, "emb_ex", None) is None and self.config["projection_dim"] is None
                    and graphed.capturable_cached(self)[0]):
                ins = [input_ids, position_ids, attention_mask]
                key = tuple(None if t is None else (tuple(t.shape), t.dtype) for t in ins)
                x = graphed.call(self, ins, lambda i_, p_, m_: self._forward_impl(i_, p_, m_), self._hip_graphs, key)
                return (x, None) if output_hidden_states is not None else x
        return self._forward_impl(input_ids, position_ids, attention_mask, output_hidden_states)

    def _forward_impl(self, input_ids, position_ids=None, attention_mask=None, output_hidden_states=None):
        """int64 [B, L] token ids -> bf16 [B, L, C] conditioning states (TEEXHook's selection).  attention_mask [B, L] (1 = attend) is
        combined with the causal mask like transformers' CLIPTextTransformer does; token 0 must stay visible.
        Called the way the reference's wrapper calls its hooked text encoder — ``TE(ids, position_ids=..., attention_mask=...,
        output_hidden_states=True)[0]`` (models/wrapper.py:20,64) — it answers with the hook's tuple ``(states, pooled_output)``
        (pooled_output None: CLIP-L's pooled vector is not used by the SD1.x path)."""
        tm = self.text_model
        B, r = input_ids.shape[0], self.N_repeats
        ids_in = input_ids
        self._native_dropout_begin()                   # native LoRA dropout: this forward's count, before any layer runs
        if r > 1:                                                 # TEEXHook.forward_hook_input (textencoder_ex.py:57-59): 'b (r w) -> (b r) w'
            if input_ids.dim() != 2 or input_ids.shape[1] % r:
                raise ValueError(f"token ids [B, {r} x L] expected for N_repeats={r}, got {tuple(input_ids.shape)}")
            input_ids = input_ids.reshape(B * r, -1)
            attention_mask = attention_mask.reshape(B * r, -1) if attention_mask is not None else None
            position_ids = position_ids.reshape(B * r, -1) if position_ids is not None else None
        if input_ids.dim() != 2 or input_ids.shape[1] > self.config["max_position_embeddings"]:
            raise ValueError(f"expected token ids [B, L <= {self.config['max_position_embeddings']}], got {tuple(input_ids.shape)}")
        if attention_mask is not None and tuple(attention_mask.shape) != tuple(input_ids.shape):
            raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not match input_ids {tuple(input_ids.shape)}")
        emb = tm.embeddings
        if torch.is_grad_enabled() and (emb.token_embedding.weight.requires_grad or emb.position_embedding.weight.requires_grad):
            raise NotImplementedError("hcp_diffusion_amd: the token / position tables are frozen (prompt tuning trains custom words: prompt_tuning.py)")
        hook = getattr(emb.token_embedding, "emb_ex", None)
        if hook is None:
            x = K.embedding(emb.token_embedding.weight.detach(), input_ids.contiguous(), emb.position_embedding.weight.detach(), position_ids)
        else:                   # prompt tuning: EmbeddingPTHook's pre-hook regroups the ids to [B, r*w] (text_emb_ex.py:33-36)
            from .prompt_tuning import check_ids
            if hook.N_repeats != r or input_ids.shape[1] != hook.N_word + 2:
                raise ValueError(f"prompt tuning: the embedding hook expects N_repeats={hook.N_repeats} chunks of {hook.N_word + 2} ids, "
                                 f"the encoder has N_repeats={r} and {input_ids.shape[1]} ids per chunk")
            ids_b = ids_in.reshape(B, -1).contiguous()
            check_ids(hook, ids_b)
            x = ops.embedding_pt(ids_b, emb.token_embedding.weight.detach(), emb.position_embedding.weight.detach(), hook,
                                 position_ids.contiguous() if position_ids is not None else None)
        key_bias = None
        if attention_mask is not None:       # [B, L], 1 = attend (wrapper.py:20 passes the tokenizer's mask when encoder_attention_mask is on)
            key_bias = ((1.0 - attention_mask.to(torch.float32)) * -1.0e9).contiguous()       # additive on the keys, on top of the causal mask
        layers = tm.encoder.layers
        proj = self.config["projection_dim"] is not None
        if proj and torch.is_grad_enabled() and (self.text_projection.weight.requires_grad or tm.final_layer_norm.weight.requires_grad
                                                 or tm.final_layer_norm.bias.requires_grad):
            raise NotImplementedError("hcp_diffusion_amd: final_layer_norm and text_projection are frozen on the pooled-output path")
        n_states = len(layers) - self.clip_skip               # the states are hidden_states[-clip_skip-1] = the output of this many layers
        sel = x
        for i, layer in enumerate(layers[:len(layers) if proj else n_states]):        # the pooled output needs the last layer
            x = layer(x, key_bias)
            if i < n_states:
                sel = x
        if proj:      # text_embeds = text_projection(final_layer_norm(last)[eos]), mean over the r chunks (textencoder_ex.py:73-76)
            pooled, _ = ops.clip_pool(x, input_ids.contiguous(), tm.final_layer_norm, self._projection_weight(), r)
        x = tm.final_layer_norm(sel) if self.clip_final_norm else sel
        if r > 1:       # textencoder_ex.py:68-72: one BOS (first chunk), every chunk's inner tokens, one EOS (last chunk) -> [B, r*(L-2)+2, C]
            x = x.reshape(B, r, *x.shape[1:])
            x = torch.cat([x[:, 0, :1, :], x[:, :, 1:-1, :].flatten(1, 2), x[:, -1, -1:, :]], dim=1)
        if proj:
            return x, pooled
        return (x, None) if output_hidden_states is not None else x

    def pack_projection(self):
        """The bf16 copy of text_projection.weight the pooling kernel reads.  Made here — after load_state_dict, a device / dtype move
        (``_apply``) and enable_hip_graph() — so that a graph capture finds it ready."""
        if self.config["projection_dim"] is not None and not self.text_projection.weight.is_meta:
            w = self.text_projection.weight
            self._proj_bf16 = ((w._version, w.data_ptr(), w.device), w.detach().to(BF16).contiguous())

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.pack_projection()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.pack_projection()
        return out

    def _projection_weight(self):
        """The packed copy; re-made when the weight was written in place since.  Never cached from inside a capture: a tensor allocated
        there lives in the graph's pool and is filled only on replay, so that call converts in the graph instead and keeps nothing."""
        w = self.text_projection.weight
        key = (w._version, w.data_ptr(), w.device)
        hit = getattr(self, "_proj_bf16", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        if w.is_cuda and torch.cuda.is_current_stream_capturing():
            return w.detach().to(BF16).contiguous()
        self.pack_projection()
        return self._proj_bf16[1]

    @classmethod
    def from_pretrained(cls, path=None, subfolder="text_encoder", device="cuda", pretrained_model_name_or_path=None, hip_graph=False,
                        native_dropout=None, **kw):
        """A diffusers / transformers directory (config.json + model.safetensors) by parameter name (hip_graph: enable_hip_graph();
        native_dropout: <seed> = enable_native_dropout(seed))."""
        from safetensors.torch import load_file
        path = path if path is not None else pretrained_model_name_or_path
        root = os.path.join(path, subfolder) if subfolder and os.path.isdir(os.path.join(path, subfolder)) else path
        cfg = json.load(open(os.path.join(root, "config.json")))
        sd = load_file(os.path.join(root, "model.safetensors"))
        if "text_projection.weight" not in sd:            # a plain CLIPTextModel's config.json carries projection_dim too: no pooled head
            cfg = {k: v for k, v in cfg.items() if k != "projection_dim"}
        model = cls(**kw, **{k: cfg[k] for k in CONFIG_KEYS if k in cfg})
        own = model.state_dict()
        sd = {k: v for k, v in sd.items() if k in own}                   # position_ids buffer etc. are ignored
        missing = [k for k in own if k not in sd]
        if missing:
            raise ValueError(f"text-encoder checkpoint lacks {len(missing)} tensors, e.g. {missing[:3]}")
        model.load_state_dict(sd)
        model = model.to(device)
        if native_dropout is not None:
            model.enable_native_dropout(native_dropout)
        if hip_graph:
            model.enable_hip_graph()
        return model


class NativeSDXLTextEncoder(nn.Module):
    """SDXL's text path: the reference's ``ComposeTextEncoder([('clip_B', ...), ('clip_bigG', ...)])`` with a ``TEEXHook`` on each encoder
    (hcpdiff/models/compose/compose_textencoder.py:75-91), on two native encoders.  The children keep the reference's names, so the
    ``re:.*self_attn$`` / ``re:.*mlp$`` selectors of cfgs/train/examples/lora_sdxl.yaml, ``re:clip_bigG.*mlp$``, checkpoints
    (``clip_B.text_model...`` / ``clip_bigG.text_model...`` / ``clip_bigG.text_projection.weight``) and lora_convert's ``lora_te1_`` /
    ``lora_te2_`` keys line up.  ``forward`` answers with the hooked pair's tuple ``(states [B, L, C_B + C_bigG], [pooled_B, pooled_bigG])``
    — ``pooled_B`` is None (a plain CLIPTextModel host: no projection) — of which SDXLTEUnetWrapper (models/wrapper.py:57-74) feeds
    ``pooled[-1]`` to the UNet as ``text_embeds``."""

    def __init__(self, clip_B, clip_bigG):
        super().__init__()
        if clip_bigG.config["projection_dim"] is None:
            raise ValueError("NativeSDXLTextEncoder: clip_bigG must be built with projection_dim (CLIPTextModelWithProjection)")
        self.clip_B, self.clip_bigG = clip_B, clip_bigG
        self.model_names = ["clip_B", "clip_bigG"]

    @property
    def device(self):
        return self.clip_bigG.device

    @property
    def dtype(self):
        return self.clip_bigG.dtype

    def get_input_embeddings(self):
        return [getattr(self, name).get_input_embeddings() for name in self.model_names]

    def enable_native_dropout(self, seed=0):
        """Forwarded to the children, each with its own state tensor (seed + 1, seed + 2): they are top-level modules of their own."""
        for i, name in enumerate(self.model_names):
            getattr(self, name).enable_native_dropout(seed, module_index=1 + i)
        return self

    def disable_native_dropout(self):
        for name in self.model_names:
            getattr(self, name).disable_native_dropout()
        return self

    def enable_hip_graph(self, on=True):
        """Forwarded to the children: clip_B replays captured graphs; clip_bigG (two outputs) stays eager (NativeCLIPTextModel.forward)."""
        for name in self.model_names:
            getattr(self, name).enable_hip_graph(on)

    def forward(self, input_ids, attention_mask=None, position_ids=None, output_hidden_states=None):
        """int64 [B, 2 x L] ids (clip_B's tokens | clip_bigG's tokens; L = r x 77 with N_repeats = r) -> (bf16 [B, L', C_B + C_bigG], [None, fp32 [B, P]])."""
        if input_ids.shape[-1] % 2:
            raise ValueError(f"token ids [B, 2 x L] expected (one half per encoder), got {tuple(input_ids.shape)}")
        states, pooled = [], []
        for name, ids in zip(self.model_names, input_ids.chunk(2, dim=-1)):
            s, p = getattr(self, name)(ids.contiguous(), position_ids=position_ids, attention_mask=attention_mask, output_hidden_states=True)
            states.append(s); pooled.append(p)
        return ops.concat_channels(states[0].contiguous(), states[1].contiguous()), pooled

    @classmethod
    def from_pretrained(cls, path=None, device="cuda", pretrained_model_name_or_path=None, hip_graph=False, native_dropout=None, **kw):
        """A diffusers SDXL directory: ``text_encoder/`` -> clip_B, ``text_encoder_2/`` -> clip_bigG.  kw (clip_skip, clip_final_norm,
        N_repeats) goes to both encoders, as the reference hooks both with one setting."""
        path = path if path is not None else pretrained_model_name_or_path
        pair = cls(NativeCLIPTextModel.from_pretrained(path, subfolder="text_encoder", device=device, **kw),
                   NativeCLIPTextModel.from_pretrained(path, subfolder="text_encoder_2", device=device, **kw))
        if native_dropout is not None:
            pair.enable_native_dropout(native_dropout)
        if hip_graph:
            pair.enable_hip_graph()
        return pair
