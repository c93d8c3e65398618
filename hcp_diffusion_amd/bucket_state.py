"""What NativeTrainer keeps per flat bucket: the optimizer's state and fused step (`_OptState`), the `optimizer=` defaults, the chunk layout
of a sharded host bucket, the communicator of a graph warm-up.  The buckets (lora.LoraBucket, fullft.HostBucket, prompt_tuning.PTBucket)
share `params`, `grads`, ``named_tensors()`` -> [(name, parameter)] and ``refresh()`` (the bf16 operands <- the fp32 masters)."""
import math

import torch

from . import kernels as K
from .comm import NullComm


class _OptState:
    """Optimizer state of one flat bucket (AdamW, Lion or Adafactor: `opt`, the resolved `optimizer=` argument of NativeTrainer).

    segments: [(offset, numel, lr)] — one per cfg item whose parameters lie contiguously in the bucket (the reference builds one
    optimizer param group per ``lora_unet`` / ``lora_text_encoder`` item, each with its own lr: cfg_net_tools.py:108-123); each
    segment has its own device-resident lr and step counter, all segments share the bucket's squared-norm scalar.
    shard=True (full fine-tune / plugin buckets under data parallelism): this rank owns slice `rank` of every chunk of the bucket
    (`parts`: [(chunk id, lo, hi, own, offset into the rank-local state)]) — moments and the reduce-scattered gradient exist for those
    slices only (optimizer memory and HBM traffic / world).  grad_wire / param_wire 'bf16': the gradients leave, and the updated
    parameters return, as bf16 (half the bytes on xGMI; the fp32 masters of a slice then live on its owner only).
    weight_decay: this state's own (the prompt-tuning words), before the optimizer dict's, before default_wd (the trainer's); clipped:
    inside the global-norm clip (the words are when the text encoder trains too); ema: None, or the EMA copy of `params`."""

    def __init__(self, bucket, lr, device, segments=None, comm=None, shard=False, grad_wire="fp32", param_wire="fp32", opt=None,
                 betas=(0.9, 0.999), eps=1e-8, default_wd=1e-3, weight_decay=None, clipped=True):
        self.bucket = bucket
        self.opt = opt or {"type": "adamw"}              # the optimizer's own state follows its type (NativeTrainer `optimizer=`)
        self.betas, self.eps, self.clipped, self.ema = betas, eps, clipped, None
        self.weight_decay = weight_decay if weight_decay is not None else self.opt.get("weight_decay", default_wd)
        kind = self.opt["type"]
        n = bucket.params.numel()
        self.shard = bool(shard and comm is not None and (comm.world > 1 or shard == "force"))
        self.parts = []
        self.gwire = self.gshard_w = self.pwire = None
        if self.shard:
            assert not segments, "sharded bucket: one lr"
            off = 0
            for cid, lo, hi in getattr(bucket, "chunks", [(2, 0, n)]):
                assert (hi - lo) % comm.world == 0, "sharded bucket: every chunk padded to a multiple of world"
                own = (hi - lo) // comm.world
                self.parts.append((cid, lo, hi, own, off)); off += own
            self.own = off
            self.gshard = torch.zeros(self.own, dtype=torch.float32, device=device)
            self.gwire = torch.zeros(n, dtype=torch.bfloat16, device=device) if grad_wire == "bf16" else None
            self.gshard_w = torch.zeros(self.own, dtype=torch.bfloat16, device=device) if grad_wire == "bf16" else None
            self.pwire = torch.zeros(n, dtype=torch.bfloat16, device=device) if param_wire == "bf16" else None
        else:
            self.own = n
        self.segments = [(o, m) for o, m, _ in segments] if segments else [(0, self.own)]
        self.base_lrs = [l for _, _, l in segments] if segments else [lr]
        # adamw: both moments; lion: the momentum; adafactor: the first moment only with beta1, factored second moments in the tables
        first = kind != "adafactor" or self.opt.get("beta1") is not None
        self.exp_avg = torch.zeros(self.own, dtype=torch.float32, device=device) if first else None
        self.exp_avg_sq = torch.zeros(self.own, dtype=torch.float32, device=device) if kind == "adamw" else None
        self.tables = []
        if kind == "adafactor":                          # one descriptor table per lr segment (offsets relative to the segment)
            assert not self.shard, "Adafactor factors whole tensors: not sharded"
            base = bucket.params.data_ptr()
            rows = sorted(((p.data_ptr() - base) // 4, name, p) for name, p in bucket.named_tensors())
            for o, m in self.segments:
                seg = [(name, off - o, p.shape, p.stride()) for off, name, p in rows if o <= off < o + m]
                assert seg and all(off + math.prod(sh) <= m for _, off, sh, _ in seg), "a tensor straddles two lr segments"
                self.tables.append(K.AdafactorTable(seg, device))
            assert sum(t.count for t in self.tables) == len(rows), "every tensor of the bucket belongs to one lr segment"
        self.lrs = [torch.full((1,), l, dtype=torch.float32, device=device) for l in self.base_lrs]
        # (the kernel advances its step counter per launch: one counter per segment / per chunk of a sharded bucket, in lockstep)
        self.steps = [torch.zeros(1, dtype=torch.int32, device=device) for _ in range(max(len(self.base_lrs), len(self.parts)))]
        self.step_count = self.steps[0]
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=device)
        # lion / adafactor: the norm is summed without atomics (K.sumsq_ordered), so the whole step is bit-reproducible; adamw keeps K.sumsq
        self.sumsq_part = torch.zeros(K.SUMSQ_PARTIALS, dtype=torch.float32, device=device) if kind != "adamw" else None

    def tensors(self):
        """Everything a step mutates besides the bucket itself (snapshot / restore around the graph warm-up)."""
        own = [t for t in (self.exp_avg, self.exp_avg_sq) if t is not None] + [x for t in self.tables for x in t.tensors()]
        return own + [self.sumsq] + self.lrs + self.steps + ([self.ema] if self.ema is not None else [])

    def accumulate_norm(self, g):                       # sumsq <- |g|^2: this bucket's share of the global gradient norm
        if self.sumsq_part is None:
            K.sumsq(g, self.sumsq)
        else:
            K.sumsq_ordered(g, self.sumsq, self.sumsq_part)

    def step(self, p, g, off, n, k, total, max_norm, world):
        """One fused clip + optimizer launch sequence over p / g; off, n: where their state lies in the flat buffers; k: the lr segment (its
        lr, step counter, Adafactor table) or the chunk of a sharded bucket (its step counter; one lr).  Outside the clip: the raw gradient."""
        o, lr_t, step_t = self.opt, self.lrs[0 if self.shard else k], self.steps[k]
        clip = dict(sumsq_t=total if self.clipped else None, grad_scale=1.0 / world, max_norm=max_norm if self.clipped else 0.0)
        m = self.exp_avg[off:off + n] if self.exp_avg is not None else None
        if o["type"] == "adamw":
            K.adamw_clip_fused(p, g, m, self.exp_avg_sq[off:off + n], lr_t, step_t, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                               weight_decay=self.weight_decay, **clip)
        elif o["type"] == "lion":
            K.lion_clip_fused(p, g, m, lr_t, step_t, beta1=o["betas"][0], beta2=o["betas"][1], weight_decay=self.weight_decay, **clip)
        else:
            K.adafactor_step(p, g, self.tables[k], lr_t, step_t, m=m, eps=o["eps"], clip_threshold=o["clip_threshold"],
                             decay_rate=o["decay_rate"], beta1=o["beta1"], weight_decay=self.weight_decay,
                             scale_parameter=o["scale_parameter"], relative_step=o["relative_step"], warmup_init=o["warmup_init"], **clip)


LION_DEFAULTS = dict(betas=(0.9, 0.99))                                         # lion_pytorch.Lion
ADAFACTOR_DEFAULTS = dict(eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, scale_parameter=True,
                          relative_step=True, warmup_init=False)                # transformers.optimization.Adafactor


def _optimizer_cfg(optimizer):
    """NativeTrainer's `optimizer=` argument -> {'type': ..., the class's keyword arguments with its defaults filled in}."""
    cfg = dict(optimizer or {"type": "adamw"})
    kind = cfg.get("type")
    known = {"adamw": {}, "lion": LION_DEFAULTS, "adafactor": ADAFACTOR_DEFAULTS}
    if kind not in known:
        raise ValueError(f"Unknown optimizer type {kind!r}: 'adamw', 'lion' or 'adafactor'")
    extra = set(cfg) - {"type", "weight_decay", "lr"} - set(known[kind])
    if extra:
        raise ValueError(f"optimizer type {kind!r} takes no {sorted(extra)}")
    cfg = {**known[kind], **cfg}
    if kind == "adafactor":
        if cfg.get("lr") is not None and cfg["relative_step"]:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if cfg["warmup_init"] and not cfg["relative_step"]:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
    return cfg


FP32_WIRE = 10      # chunk ids >= 10: parameters the kernels read as fp32 (biases, norm affine) — never rounded on the wire


def _bf16_consumed(model):
    """ids of the parameters the kernels consume as bf16 operands: the weights of HipLinear / HipConv2d (what HostBucket.layers packs).
    Everything else — biases, norm affine, embedding / positional tables, any non-Hip layer inside a plugin or text encoder — is read
    in fp32 by its module and must come back from the wire exact, or data-parallel replicas would compute with different values."""
    from .layers import HipConv2d, HipLinear
    return {id(m.weight) for m in model.modules() if isinstance(m, (HipLinear, HipConv2d))}


def _chunker(overlap, param_wire, unet_names=True, bf16_ids=None):
    """(name, parameter) -> chunk id of a sharded host bucket.  With overlap: the order backward finishes the gradients of a UNet —
    0 = up blocks + output head (first), 1 = mid block, 2 = everything else (down blocks, conv_in, time / class / addition embeddings:
    complete only when backward ends).  With param_wire='bf16': only the parameters in `bf16_ids` (`_bf16_consumed`: HipLinear /
    HipConv2d weights, consumed as bf16 operands anyway) travel as bf16; the rest (biases, GroupNorm / LayerNorm affine, tables of
    non-Hip layers — consumed in fp32) form a chunk of their own that always returns as fp32, so that every rank computes with the
    same values."""
    if not overlap and param_wire != "bf16":
        return None

    def chunk_of(name, p):
        if param_wire == "bf16" and (p.dim() <= 1 or (bf16_ids is not None and id(p) not in bf16_ids)):
            return FP32_WIRE + 2
        if not (overlap and unet_names):
            return 2
        if name.startswith(("up_blocks.", "conv_norm_out.", "conv_out.")):
            return 0
        return 1 if name.startswith("mid_block.") else 2
    return chunk_of


class _WarmupComm(NullComm):
    """Local stand-in for the communicator during a graph warm-up: same world / rank (slices keep their shapes), no traffic."""

    def __init__(self, real):
        self.world, self.rank = real.world, real.rank

    def reduce_scatter(self, send, recv):
        recv.copy_(send[self.rank * recv.numel():(self.rank + 1) * recv.numel()])
        return recv

    def all_gather(self, send, recv):
        recv[self.rank * send.numel():(self.rank + 1) * send.numel()].copy_(send)
        return recv
