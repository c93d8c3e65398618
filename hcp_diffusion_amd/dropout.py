"""Native LoRA dropout: the per-module switch, state tensor and layer numbering behind ``lora.LoraHipContainer._dropped``.

The reference drops the whole output of a LoRA'd layer with torch's dropout (lora_base_patch.py:74).  Natively the mask is a pure
function of (seed, forward count, layer id, element index) — csrc/dropout.hip — regenerated in the backward pass and never stored, and
everything that varies per step lives in a device int64[2] tensor ``(seed, calls)``, so a captured graph serves every step.

One :class:`NativeDropout` per top-level native module (UNet, CLIP text encoder, each member of the SDXL pair): the modules run their
backwards at different times and must not share a counter.  It is a plain attribute, not a buffer: ``state_dict`` and checkpoints are
unchanged, and a resumed run restarts the mask stream at ``calls = 0``.
"""
import torch

from . import kernels as K


def _wrap_i64(v):
    return ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)


class NativeDropout:
    def __init__(self, module, seed, index):
        self.seed, self.index = int(seed), int(index)
        self.name = f"{type(module).__name__} (module index {index})"
        self.state = K.dropout_state(_wrap_i64(self.seed + self.index), next(module.parameters()).device)
        self.gen = 0               # host-side twin of state[1]: what ops._DropoutResidualFn checks its backward against
        self.blocks = []           # blocks with p > 0 in named_modules order: layer_id = position
        self._lora = []            # every LoRA block of the module (their p values are part of the cache key)
        self._key = None

    def resolve(self, module):
        """Number the module's LoRA blocks with p > 0.  Blocks are wrapped after the module exists, so this runs lazily at the top-level
        forward; cached on the tell-tales of graphed.capturable_cached, the count of LoRA blocks ever constructed and the blocks' p values
        (a block going 0 -> p, `set_hyper_params`, renumbers at the next forward; under graph replay no Python runs: reset_hip_graph())."""
        from .lora import LoraHipLayer
        key = (module.training, len(module._forward_pre_hooks), len(module._forward_hooks), LoraHipLayer.constructed,
               tuple(b.dropout.p for b in self._lora))
        if key == self._key:
            return
        for b in self._lora:
            b._nd = None
        self._lora = [m for m in module.modules() if isinstance(m, LoraHipLayer)]
        self.blocks = [m for m in self._lora if m.dropout.p > 0]
        for i, b in enumerate(self.blocks):
            b._nd = (self, i)
        key = key[:4] + (tuple(b.dropout.p for b in self._lora),)
        dev = next(module.parameters()).device
        if self.state.device != dev:
            self.state = self.state.to(dev)
        self._key = key

    def release(self):
        for b in self._lora:
            b._nd = None
        self.blocks, self._lora, self._key = [], [], None

    def begin(self, module):
        """Top-level forward, before any layer runs: one more training forward -> state[1] += 1 (one tiny launch, captured with the
        forward when there is a graph).  Gradient-checkpoint recomputation goes through sub-module forwards only and so sees the same
        count and rebuilds the same mask."""
        self.resolve(module)
        if torch.is_grad_enabled() and any(b.training for b in self.blocks):
            K.dropout_advance(self.state)
            self.gen += 1

    def snapshot(self):
        return self.state.clone(), self.gen

    def restore(self, saved):
        self.state.copy_(saved[0])
        self.gen = saved[1]


class NativeDropoutMixin:
    """``enable_native_dropout(seed)`` / ``disable_native_dropout()`` of a top-level native module."""
    dropout_module_index = 0       # state = (seed + index, 0): UNet 0, text encoder 1 (SDXL pair: clip_B 1, clip_bigG 2)

    def enable_native_dropout(self, seed=0, module_index=None):
        """LoRA dropout of this module's blocks through csrc/dropout.hip instead of torch's dropout: capturable, no stored mask, the same
        bits eager and replayed.  The stream differs from torch's; two forwards before the first one's backward are refused.
        Blocks with p > 0 are numbered at the module's next forward and again whenever blocks are added or a block's p changes; a module
        that replays captured graphs runs no Python, so call reset_hip_graph() after such a change, as after any change of what trains.
        Under several ranks give every rank its own seed (NativeTrainer adds the rank itself)."""
        self.disable_native_dropout()
        self._hcp_dropout = NativeDropout(self, seed, self.dropout_module_index if module_index is None else module_index)
        self._hcp_capturable = None
        if getattr(self, "_hip_graphs", None):
            self._hip_graphs = {}
        return self

    def disable_native_dropout(self):
        nd = getattr(self, "_hcp_dropout", None)
        if nd is not None:
            nd.release()
        self._hcp_dropout = None
        self._hcp_capturable = None
        if getattr(self, "_hip_graphs", None):
            self._hip_graphs = {}
        return self

    def _native_dropout_begin(self):
        nd = getattr(self, "_hcp_dropout", None)
        if nd is not None:
            nd.begin(self)
