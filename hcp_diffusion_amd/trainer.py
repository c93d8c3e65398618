"""Native inner loop: the arithmetic of ``Trainer.train_one_step`` (reference hcpdiff/train_ac.py:467-504) for the
benchmark configuration (cached latents — the VAE encode "stays a one-off host call" —, eps-prediction loss, LoRA
on the UNet), restated step by step:

  make_noise   train_ac.py:437-447   torch RNG for noise/timesteps (kept for parity), add_noise = HIP kernel
  forward      train_ac.py:449-465   NativeUNet2DConditionModel (HIP kernels)
  get_loss     train_ac.py:506-515   masked MSE in fp32, one kernel producing loss AND d loss/d pred
  backward     train_ac.py:482       autograd over the native ops; LoRA grads land in one flat fp32 bucket
  DDP          accelerate/torch DDP  ONE all-reduce(SUM) of the flat bucket over RCCL (dist.py), 1/world folded
                                     into the optimizer kernel
  clip + step  train_ac.py:485-494   global-norm clip + AdamW + zero_grad = 3 launches (csrc/optim.hip)

Everything between two host interactions is stream-ordered device work with static shapes, so the whole step is
captured once into a hipGraph (two graphs around the all-reduce when world_size > 1) and replayed; the reference's
per-step ``loss.item()`` sync (train_ac.py:504) is deferred to whenever the caller reads the loss tensor.
"""
import contextlib
import random

import torch

from . import kernels as K
from . import ops
from .bucket_state import FP32_WIRE, _bf16_consumed, _chunker, _optimizer_cfg, _OptState, _WarmupComm
from .comm import AbiComm, NullComm, make_comm
from .fullft import HostBucket
from .lora import get_match_layers, make_lora
from .scheduler import NativeDDPMScheduler, NativeZeroTerminalScheduler, PyramidNoiseState, check_pyramid_args


def ddpm_alphas_cumprod(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, device="cpu"):
    """DDPMScheduler(beta_schedule='scaled_linear') table; constants as in the reference's
    loggers/preview/image_previewer.py:28."""
    return NativeDDPMScheduler(num_train_timesteps, beta_start, beta_end).alphas_cumprod.to(device)


def parse_cfg_scale(cfg_scale):
    """NativeTrainer's `cfg_scale=` -> None or (lo, hi, rate kind): the reference's ``train.cfg_scale`` text ('3.0', '1.0-3.0',
    '1.0-3.0:cos') read as utils.get_cfg_range reads it, or a plain number.  The reference `eval`s a rate it does not know
    (cfg_context.py:34); configuration text is not evaluated here: anything but 'ln', 'cos', 'cos2' raises."""
    if cfg_scale is None:
        return None
    kind = "ln"
    if isinstance(cfg_scale, str):
        text = cfg_scale
        if text.find(":") != -1:
            text, kind = text.split(":")
        if text.find("-") != -1:
            lo, hi = text.split("-")
            lo, hi = float(lo), float(hi)
        else:
            lo = hi = float(text)
    else:
        lo = hi = float(cfg_scale)
    if kind not in K.CFG_RATE_KINDS:
        raise ValueError(f"cfg_scale rate {kind!r}: one of 'ln', 'cos', 'cos2' (other rate expressions are not evaluated)")
    return lo, hi, kind


def parse_noise_cfg(noise_cfg):
    """NativeTrainer's `noise_cfg=` -> (None or the pyramid settings {level, discount, step_size, resize_mode}, zero_terminal flag)."""
    if noise_cfg is None:
        return None, False
    cfg = dict(noise_cfg)
    kind, zero_terminal = cfg.pop("type", None), bool(cfg.pop("zero_terminal", False))
    if kind not in (None, "pyramid"):
        raise ValueError(f"noise_cfg type {kind!r}: 'pyramid' (and / or zero_terminal=True)")
    extra = set(cfg) - ({"level", "discount", "step_size", "resize_mode"} if kind else set())
    if extra:
        raise ValueError(f"noise_cfg takes no {sorted(extra)}" + ("" if kind else " without type='pyramid'"))
    if kind is None:
        return None, zero_terminal
    pyr = {**dict(level=10, discount=0.9, step_size=2.0, resize_mode="bilinear"), **cfg}       # PyramidNoiseScheduler's defaults
    check_pyramid_args(pyr["level"], pyr["discount"], pyr["step_size"], pyr["resize_mode"])
    return pyr, zero_terminal


class NativeTrainer:
    def __init__(self, unet, lora_cfg=None, lr=1e-4, weight_decay=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0,
                 scale_lr_factor=1.0, process_group=None, use_graph=False, loss_weight=1.0, num_train_timesteps=1000,
                 overlap_wgrad=False, grouped_wgrad=True, train_cfg=None, plugins=None, ema=None, loss_cfg=None, text_encoder=None,
                 lora_te_cfg=None, comm=None, shard_optimizer=None, gradient_accumulation_steps=1, loss_type="eps",
                 overlap_exchange=False, grad_wire="fp32", param_wire="fp32", pt_cfg=None, pt_words=None, pt_weight_decay=5e-4,
                 optimizer=None, cfg_scale=None, noise_cfg=None, native_dropout=None):
        """lora_cfg: the reference's ``lora_unet`` list ({layers, rank, alpha, lr, ...}); train_cfg: its ``unet`` list
        ({layers, lr}) of host modules to fine-tune in full (DreamBooth.yaml:6-10 uses ``layers: ['']`` = everything);
        plugins: [(plugin module, lr)] — trainable hook plugins such as controlnet.ControlNetHipPlugin (make_plugin,
        cfg_net_tools.py:148-162: all of the plugin's parameters form one param group); ema: None or the ModelEMA arguments
        {decay_max, inv_gamma, power} (``model.ema``, train_ac.py:238-242): an EMA copy of every trainable bucket, updated by
        one kernel per bucket after the optimizer step (train_ac.py:503); loss_cfg: None = ``train.loss.criterion`` MSELoss
        (train_base.yaml), or {type: 'min_snr'|'soft_min_snr'|'kdiff_min_snr'|'edm', gamma} = the reference's timestep-aware
        criteria (hcpdiff/loss/min_snr_loss.py, selected through ``need_timesteps`` in train_ac.py:509-510); text_encoder: a
        text_encoder.NativeCLIPTextModel — batches may then carry ``prompt_ids`` [B,77] instead of ``encoder_hidden_states`` and the
        prompt is encoded inside the step (TEUnetWrapper.forward, models/wrapper.py:14-30); lora_te_cfg: the reference's
        ``lora_text_encoder`` list (lora_conventional.yaml:14-19) — its blocks form a second flat bucket that shares the step's
        single global-norm clip (train_ac.py:485-490 clips TE_unet.trainable_parameters() together).
        comm: a comm.AbiComm / TorchComm / NullComm (default: comm.make_comm over ``process_group``); shard_optimizer: None = shard
        the host-parameter buckets (full fine-tune, plugins) whenever world > 1 — reduce-scatter, AdamW on this rank's slice,
        all-gather — and keep the small LoRA buckets on one all-reduce; gradient_accumulation_steps: ``accelerator.accumulate``
        (train_ac.py:119,468): the exchange, clip and optimizer step run on every N-th call only, the loss gradients of the
        N micro-steps add up scaled by 1/N; loss_type: 'eps' | 'sample' (train_ac.py:458-465: target = noise, or the clean latents
        against x0 recovered from the prediction).
        Sharded buckets only — overlap_exchange: a full fine-tune's bucket is laid out as three chunks in the order backward completes
        them (up blocks + head | mid block | down blocks + embeddings) and the reduce-scatter of a chunk leaves on a side stream the moment
        backward has passed it, under the rest of backward (torch DDP overlaps its buckets the same way: reducer hooks, train_ac.py:117);
        grad_wire='bf16': gradients are rounded to bf16 for the reduce-scatter (DDP's bf16_compress_hook numerics); param_wire='bf16':
        the all-gather returns the updated parameters as bf16 — bit-identical bf16 operands on every rank, but the fp32 masters of a
        slice are then current on its owner only (`sync_masters()`, a collective, re-gathers them; save_model insists on it).
        Prompt tuning — pt_cfg: the reference's ``tokenizer_pt.train`` list ([{name, lr}]), pt_words: {name: Parameter} (its
        ``ex_words_emb``, every word registered in the ``emb_ex`` hook on ``text_encoder``): the trained words form one flat fp32 bucket
        with one lr segment per word (``scale_lr_pt``: the same scale_lr_factor), stepped by the fused AdamW with pt_weight_decay
        (train_base.yaml:42-55 ``optimizer_pt``).  They join the global-norm clip only when the text encoder trains too
        (TE_unet.trainable_parameters() then holds the hook's emb_train, train_ac.py:483-490); the exchange and the captured step
        cover them like every bucket.
        optimizer: None or {'type': 'adamw'} = the fused AdamW with this constructor's betas / eps / weight_decay; {'type': 'lion', 'betas':
        (0.9, 0.99)} = lion_pytorch.Lion (Lion_optimizer.yaml); {'type': 'adafactor', ...} with the keyword names and defaults of
        transformers.optimization.Adafactor (FT_sdxl.yaml: relative_step False, weight_decay 1e-3) — without relative_step the step size
        is each item's lr, with it the lrs are ignored as that class ignores them.  'weight_decay' in the dict overrides this
        constructor's.  The choice applies to EVERY bucket (LoRA, text-encoder LoRA, host buckets, plugins, words — those with
        pt_weight_decay).  Lion is elementwise and shards like AdamW; Adafactor needs whole tensors (row / column statistics), so its host
        buckets stay on the unsharded all-reduce path at world > 1 and an explicit shard_optimizer raises.
        DreamArtist — cfg_scale: None, a number or the reference's ``train.cfg_scale`` text ('3.0', '1.0-3.0', '1.0-3.0:cos'; rates ln, cos,
        cos2).  Active exactly when the upper value is not 1.0 (train_ac.py:83); otherwise the step is the one above, unchanged.  Active
        (DreamArtistPTContext, models/cfg_context.py:12-39): the noisy latents and timesteps of the B samples are repeated to 2B rows in
        (pn b) order, the text side of the batch (prompt_ids or encoder_hidden_states, attn_mask) carries 2B rows — the B negative prompts
        first, as pair_dataset.collate_fn stacks them (:141-142) —, and loss and top gradient come from one kernel on the [2B] prediction:
        e = u + s_b (c - u) against the B targets (K.cfg_mse_masked_mean; mask, Min-SNR weights and loss_weight / accum as without it).
        added_cond_kwargs / plugin_input are refused with an active scale: the reference hands their B-row tensors to the 2B UNet call.
        Noise — noise_cfg: None = today's step, bit for bit; {'type': 'pyramid', level, discount, step_size, resize_mode} = the reference's
        noise.PyramidNoiseScheduler around the step's scheduler, and / or {'zero_terminal': True} = its noise.ZeroTerminalScheduler.
        Pyramid noise: the level sizes are drawn on the host per step exactly as the reference draws them (the global ``random`` module) and
        reach the kernels as device data; level i's field is always drawn at its upper bound [B, C, int(h / step_size**i), int(w /
        step_size**i)] (one ``randn`` for all levels, in the graph), of which the kernel reads the leading B C hn wn values — one captured
        graph serves every draw.  As in the reference the eps target is the UNNORMALISED pyramid sum, the noisy latents come from the sum
        divided by its std.  Allowed under an active cfg_scale: the noise is made before the repeat.  Zero terminal SNR
        (alphas_cumprod[T - 1] = 0) is refused with loss_type='sample' and with an SNR-weighted loss_cfg: both divide by it.
        native_dropout: None = LoRA dropout through torch's op, today's step bit for bit; a seed = `enable_native_dropout(seed + rank)` on
        the UNet and the text encoder this trainer owns (csrc/dropout.hip: counter-based mask, nothing stored, the same bits eager and
        captured).  The mask stream is not part of a checkpoint: a resumed run restarts it."""
        self.noise_pyramid, self.noise_zero_terminal = parse_noise_cfg(noise_cfg)
        if self.noise_zero_terminal:
            if loss_type == "sample":
                raise ValueError("noise_cfg zero_terminal with loss_type='sample': x0 is recovered by dividing by sqrt(alphas_cumprod[t]), which "
                                 "is 0 at t = T - 1 on a zero-terminal-SNR table")
            if loss_cfg is not None and loss_cfg.get("type", "mse") != "mse":
                raise ValueError(f"noise_cfg zero_terminal with loss_cfg type {loss_cfg.get('type')!r}: the SNR-weighted criteria divide by "
                                 "snr = acp / (1 - acp), which is 0 at t = T - 1 on a zero-terminal-SNR table")
            # (an active cfg_scale reads no alphas_cumprod — its rates are functions of t / (T - 1) alone —, so it combines with this table)
        self.opt_cfg = _optimizer_cfg(optimizer)
        self.cfg_scale = parse_cfg_scale(cfg_scale)
        self.cfg_active = self.cfg_scale is not None and self.cfg_scale[1] != 1.0
        self.unet = unet
        self.device = next(unet.parameters()).device
        self.comm = comm if comm is not None else make_comm(self.device, process_group)
        self.world = self.comm.world
        shard = (self.world > 1) if shard_optimizer is None else bool(shard_optimizer and self.world > 1)
        if self.opt_cfg["type"] == "adafactor":
            if shard_optimizer:
                raise ValueError("shard_optimizer with Adafactor: its second moments are row / column statistics of WHOLE tensors, which "
                                 "a slice of the flat bucket does not hold; leave shard_optimizer unset (one all-reduce per bucket)")
            shard = False
        if shard_optimizer == "force":        # tests: the sharded code path (chunks, side stream, wire casts) on ONE rank
            shard = "force"
        if grad_wire not in ("fp32", "bf16") or param_wire not in ("fp32", "bf16"):
            raise ValueError("grad_wire / param_wire: 'fp32' or 'bf16'")
        if param_wire == "bf16" and ema is not None:
            raise ValueError("param_wire='bf16' leaves the fp32 masters of a slice on its owner: keep 'fp32' with an EMA model")
        self._overlap = bool(overlap_exchange and shard)
        self.weight_decay, self.betas, self.eps, self.max_grad_norm = weight_decay, betas, eps, max_grad_norm
        hyper = dict(opt=self.opt_cfg, betas=betas, eps=eps, default_wd=weight_decay)       # what every bucket's optimizer state is built with
        sharding = dict(comm=self.comm, shard=shard, **(dict(grad_wire=grad_wire, param_wire=param_wire) if shard else {}), **hyper)
        pad = self.world * 64 if shard else 1
        if loss_type not in ("eps", "sample"):
            raise ValueError(f"Unknown loss type {loss_type}")
        self.loss_type = loss_type
        self.accum, self._micro = max(1, int(gradient_accumulation_steps)), 0
        unet.requires_grad_(False)            # config_model(): freeze host, eval (train_ac.py:264-268)
        unet.eval()
        self.host_buckets = []
        named = dict(unet.named_modules())
        for item in (train_cfg or []):        # get_params_group (train_ac.py:280-296): matched modules' own parameters
            seen, params = set(), []
            for layer_name in get_match_layers(item["layers"], named):
                for n_, p_ in named[layer_name].named_parameters():
                    full = f"{layer_name}.{n_}" if layer_name else n_
                    if id(p_) not in seen and "lora_block_" not in full:
                        seen.add(id(p_)); params.append((full, p_))
            hb = HostBucket(unet, params, pad_multiple=pad, chunk_of=_chunker(self._overlap, param_wire, bf16_ids=_bf16_consumed(unet)) if shard else None)
            self.host_buckets.append(_OptState(hb, item.get("lr", lr) * scale_lr_factor, self.device, **sharding))
        self.plugins = []
        for plugin, plr in (plugins or []):
            plugin.train()
            hb = HostBucket(plugin, list(plugin.named_parameters()), pad_multiple=pad,
                            chunk_of=_chunker(False, param_wire, unet_names=False, bf16_ids=_bf16_consumed(plugin)) if shard else None)
            self.host_buckets.append(_OptState(hb, plr * scale_lr_factor, self.device, **sharding))
            self.plugins.append(plugin)
        self.param_groups, self.lora_group, self.bucket = make_lora(unet, lora_cfg) if lora_cfg else ([], None, None)
        assert self.bucket is not None or self.host_buckets or lora_te_cfg or pt_cfg, "nothing to train: no LoRA layer matched and no host group given"
        self._lora_state = (_OptState(self.bucket, lr * scale_lr_factor, self.device,
                                      segments=self._segments(self.param_groups, self.bucket, scale_lr_factor, lr), **hyper)
                            if self.bucket is not None else None)
        self.text_encoder, self.lora_te_group, self.te_bucket, self._te_state = text_encoder, None, None, None
        if text_encoder is not None:
            text_encoder.requires_grad_(False)
            text_encoder.eval()
            if lora_te_cfg:
                te_groups, self.lora_te_group, self.te_bucket = make_lora(text_encoder, lora_te_cfg)
                assert self.te_bucket is not None, "lora_text_encoder matched no layer"
                self._te_state = _OptState(self.te_bucket, lr * scale_lr_factor, self.device,
                                           segments=self._segments(te_groups, self.te_bucket, scale_lr_factor, lr), **hyper)
        elif lora_te_cfg:
            raise ValueError("lora_te_cfg needs the text_encoder module")
        self.pt_bucket, self._pt_state, self.pt_words, self.pt_hook = None, None, {}, None
        if pt_cfg:
            from .prompt_tuning import PTBucket, find_hook
            hook = find_hook(text_encoder) if text_encoder is not None else None
            if hook is None:
                raise ValueError("pt_cfg needs a text_encoder carrying an embedding hook (EmbeddingPTHook.hook)")
            words = []
            for item in pt_cfg:
                if item["name"] not in (pt_words or {}):
                    raise ValueError(f"pt_cfg word {item['name']!r} is not in pt_words")
                words.append((item["name"], pt_words[item["name"]], item.get("lr", lr) * scale_lr_factor))
            self.pt_bucket = PTBucket(hook, words)
            self.pt_words = dict(zip(self.pt_bucket.names, self.pt_bucket.words))
            self.pt_hook = hook
            self._pt_state = _OptState(self.pt_bucket, lr, self.device, segments=self.pt_bucket.segments, weight_decay=pt_weight_decay,
                                       clipped=self.te_bucket is not None, **hyper)
        self._dropout_modules = []
        if native_dropout is not None:
            for mod in (unet, text_encoder):
                if mod is not None:
                    mod.enable_native_dropout(int(native_dropout) + self.comm.rank)
                    self._dropout_modules += [getattr(mod, n) for n in mod.model_names] if hasattr(mod, "model_names") else [mod]
        self._state_list = [st for st in (self._lora_state, *self.host_buckets, self._te_state, self._pt_state) if st is not None]
        self.ema_cfg = None if ema is None else {**dict(decay_max=0.9997, inv_gamma=1.0, power=2.0 / 3.0), **ema}
        if ema is not None:
            for st in self._state_list:
                if st is not self._pt_state:                  # (ModelEMA covers the UNet / text encoder, not the words)
                    st.ema = st.bucket.params.clone()
        for st in self.host_buckets:
            st.bucket.refresh()
        self.loss_weight = loss_weight
        self.loss_kind, self.loss_gamma = None, 1.0
        if loss_cfg is not None and loss_cfg.get("type", "mse") != "mse":
            if loss_cfg["type"] not in K.SNR_LOSS_KINDS:
                raise ValueError(f"Unknown loss criterion {loss_cfg['type']}")
            self.loss_kind, self.loss_gamma = loss_cfg["type"], float(loss_cfg.get("gamma", 1.0))
        sched = NativeDDPMScheduler(num_train_timesteps)
        self.acp = (NativeZeroTerminalScheduler(sched) if self.noise_zero_terminal else sched).alphas_cumprod.to(self.device)
        self._pyramid = PyramidNoiseState(self.noise_pyramid, self.device) if self.noise_pyramid is not None else None
        self.num_train_timesteps = num_train_timesteps
        self._ctor_lr, self._scale_lr_factor = lr, scale_lr_factor
        self.use_graph = use_graph
        # measured on MI355X / ROCm 7.2: the side-stream (parallel graph branch) form is SLOWER (32.6 vs 30.0 ms/step:
        # every fork/join edge of the hipGraph costs more than the overlap buys); one grouped launch at the end wins.
        self.overlap_wgrad = overlap_wgrad and self.device.type == "cuda"
        self._wgrad_ctx = ops.WgradContext(grouped=grouped_wgrad, side_stream=self.overlap_wgrad)   # this trainer's own (no process-global switch)
        self._xstream = torch.cuda.Stream(self.device) if (self._overlap and self.device.type == "cuda") else None
        self._graph_cache = {}           # batch signature -> (forward/backward graph, static inputs, loss tensor), least recently used first
        self.max_graph_signatures = 32   # aspect-ratio buckets x context lengths kept captured (each holds its static inputs; the pool is shared)
        self._opt_graph, self._opt_graph_sent = None, ()
        self._sent, self._masters_stale, self._warned_evict = set(), False, False
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)

    @staticmethod
    def _segments(groups, bucket, scale, default_lr):
        """[(offset, numel, lr)] of the cfg items inside the flat LoRA bucket (make_lora appends blocks item by item)."""
        segs, off = [], 0
        for g in groups:
            n = sum(p.numel() for p in g["params"])
            if n:
                segs.append((off, n, g.get("lr", default_lr) * scale))
            off += n
        assert off == bucket.params.numel(), "LoRA cfg items must own disjoint layers (a layer matched by two items)"
        return segs

    # ---- the pieces of train_one_step
    def make_noise(self, latents):
        noise = torch.randn_like(latents)
        t = torch.randint(0, self.num_train_timesteps, (latents.shape[0],), device=latents.device).long()
        if self._pyramid is None:
            return K.add_noise(latents, noise, t, self.acp), noise, t
        return self._pyramid.add_noise(latents, noise, t, self.acp), noise, t

    def forward_backward(self, latents, encoder_hidden_states, mask=None, added_cond_kwargs=None, plugin_input=None, prompt_ids=None,
                         attn_mask=None, exchange=False):
        """attn_mask: the batch's ``attn_mask`` [B, L] (train_ac.py:473; wrapper.py:20,29 hands it to the text encoder as
        attention_mask and to the UNet as encoder_attention_mask).  exchange: this is the last backward before the optimizer step —
        with overlap_exchange the chunks of the sharded UNet buckets are reduce-scattered as backward completes them."""
        if self.cfg_active:
            self._check_cfg_batch(dict(latents=latents, encoder_hidden_states=encoder_hidden_states, prompt_ids=prompt_ids, attn_mask=attn_mask,
                                       added_cond_kwargs=added_cond_kwargs, plugin_input=plugin_input))
        noisy, noise, t_raw = self.make_noise(latents)                    # cfg_context.py:19-20: 'b c h w -> (pn b) c h w', timesteps.repeat(2)
        noisy, t = (noisy.repeat(2, 1, 1, 1), t_raw.repeat(2)) if self.cfg_active else (noisy, t_raw)
        self.unet._bwd_marks = ({"after_up": lambda g: self._exchange_early(0), "after_mid": lambda g: self._exchange_early(1)}
                                if (exchange and self._overlap) else None)
        self._sent = set()                   # chunk ids this backward reduce-scattered itself
        kw = {"encoder_attention_mask": attn_mask} if attn_mask is not None else {}
        wg = self._wgrad_ctx
        with ops.wgrad_context(wg):                                       # this step's autograd nodes report their LoRA weight gradients to `wg`
            if encoder_hidden_states is None:                             # wrapper.py:20: the prompt is encoded inside the step
                if self.text_encoder is None or prompt_ids is None:
                    raise ValueError("a batch needs encoder_hidden_states, or prompt_ids together with a text_encoder")
                with torch.set_grad_enabled(self.te_bucket is not None or self.pt_bucket is not None):
                    encoder_hidden_states = self.text_encoder(prompt_ids, attention_mask=attn_mask)
                if isinstance(encoder_hidden_states, tuple):              # the SDXL pair answers (states, [pooled_B, pooled_bigG]):
                    encoder_hidden_states, pooled = encoder_hidden_states  # wrapper.py:64-73 feeds pooled[-1] with the batch's crop_info
                    if not added_cond_kwargs or added_cond_kwargs.get("time_ids") is None:
                        raise ValueError("an SDXL text encoder needs the batch's added_cond_kwargs={'time_ids': ...}")
                    added_cond_kwargs = dict(added_cond_kwargs, text_embeds=pooled[-1])
            if plugin_input:                                              # wrapper.py:15,25-28: feeders see the batch dict
                for feeder in getattr(self.unet, "input_feeder", []):
                    feeder(dict(noisy_latents=noisy, timesteps=t, encoder_hidden_states=encoder_hidden_states, **plugin_input))
            if added_cond_kwargs:                                         # SDXL: wrapper.py:66-73
                kw["added_cond_kwargs"] = added_cond_kwargs
            pred = self.unet(noisy, t, encoder_hidden_states, **kw).sample          # wrapper.py:29
        loss, grad = self._loss_and_grad(pred.detach(), noise, t_raw, mask)  # the weights and the rate read the B raw timesteps (cfg_context.py:18,26)
        try:
            torch.autograd.backward(pred, grad)
            wg.flush()                           # all layers' LoRA weight gradients: one grouped launch
        finally:
            wg.items.clear()                     # (an exception mid-backward must not leak operands into the next step)
            wg.join()
            self.unet._bwd_marks = None
            if self._xstream is not None and exchange:
                torch.cuda.current_stream(self.device).wait_stream(self._xstream)      # join (inside the capture, when there is one)
        return loss

    def _loss_and_grad(self, pred, noise, t, mask):
        """'eps' (train_ac.py:458-459): target = noise.  'sample' (:460-463): MSE(x0_hat, x0) = (1-acp)/acp * MSE(eps, noise), a per-sample
        weight — under an active cfg_scale too (noise_scheduler.step is linear in the prediction), where the loss sits on e = u + s (c - u)."""
        sw = K.snr_loss_weight(t, self.acp, self.loss_kind, self.loss_gamma) if self.loss_kind else None
        lw = self.loss_weight / self.accum                                # accelerator.accumulate: micro-step losses average
        if self.loss_type == "sample":
            a = self.acp[t].view(-1)
            w_s = (1.0 - a) / a
            sw = w_s if sw is None else sw * w_s
        if self.cfg_active:
            return K.cfg_mse_masked_mean(pred, noise, t, self.cfg_scale, mask, weight=lw, sample_weight=sw, num_train_timesteps=self.num_train_timesteps)
        return K.mse_masked_mean(pred, noise, mask, weight=lw, sample_weight=sw)

    def _check_cfg_batch(self, b):
        """An active cfg_scale: the text side carries 2B rows (negatives first); inputs the reference does not define under it are refused."""
        B = b["latents"].shape[0]
        if b.get("added_cond_kwargs") or b.get("plugin_input"):
            raise ValueError("cfg_scale (DreamArtist) with added_cond_kwargs / plugin_input: the reference's SDXL wrapper and plugin feeders "
                             "hand their B-row tensors to the 2B-row UNet call; that combination is not defined")
        for key in ("prompt_ids", "encoder_hidden_states", "attn_mask"):
            v = b.get(key)
            if v is not None and v.shape[0] != 2 * B:
                raise ValueError(f"cfg_scale (DreamArtist): {key} has {v.shape[0]} rows for {B} latents; it needs 2B = {2 * B} rows, the B negative "
                                 "prompts first, then the B positive ones")

    # ---- the sharded exchange
    def _exchange_part(self, st, k):
        """Reduce-scatter chunk k of a sharded bucket: this rank receives the summed gradient of its slice of the chunk."""
        _, lo, hi, own, off = st.parts[k]
        g = st.bucket.grads[lo:hi]
        if st.gwire is not None:               # bf16 on the wire; the same pass clears the fp32 gradients (= zero_grad)
            K.cast_f32_bf16(g, st.gwire[lo:hi], scale=1.0, zero_src=True)
            self.comm.reduce_scatter(st.gwire[lo:hi], st.gshard_w[off:off + own])
        else:
            self.comm.reduce_scatter(g, st.gshard[off:off + own])

    def _exchange_early(self, cid):
        """Backward hook (unet._bwd_marks): every gradient of chunk `cid` is enqueued — send it from the side stream."""
        xs = self._xstream
        self._sent.add(cid)
        if xs is not None:
            xs.wait_stream(torch.cuda.current_stream(self.device))
        with (torch.cuda.stream(xs) if xs is not None else contextlib.nullcontext()):
            for st in self.host_buckets:
                for k, part in enumerate(st.parts):
                    if part[0] == cid:
                        self._exchange_part(st, k)

    def sync_masters(self):
        """param_wire='bf16': all-gather the fp32 masters of every sharded bucket (each rank holds fp32 truth for its own slices only).
        A COLLECTIVE: every rank must call it — save_model (which the reference's trainer runs on the main process only,
        train_ac.py:523) refuses to write rounded masters and asks for this call instead of issuing it behind one rank's back."""
        self._masters_stale = False
        for st in self.host_buckets:
            if st.shard and st.pwire is not None:
                for cid, lo, hi, own, _ in st.parts:
                    r = self.comm.rank
                    if cid < FP32_WIRE:
                        self.comm.all_gather(st.bucket.params[lo + r * own:lo + (r + 1) * own], st.bucket.params[lo:hi])

    def _states(self):                         # every bucket's optimizer state: LoRA, host buckets and plugins, text-encoder LoRA, words
        return self._state_list

    def _refresh_buckets(self):                # the bf16 operands of every bucket <- its fp32 masters, for the next forward
        for b in (self.bucket, self.te_bucket, *(st.bucket for st in self.host_buckets), self.pt_bucket):
            if b is not None:
                b.refresh()

    def all_reduce(self):
        """DDP's exchange for the buckets that are NOT sharded: one all-reduce(SUM) per flat gradient bucket (LoRA: 12 MB)."""
        if self.world > 1:
            for st in self._states():
                if not st.shard:
                    self.comm.all_reduce_(st.bucket.grads)

    def _reduce_sharded(self, st, early_sent):
        """Reduce-scatter what backward has not sent itself: this rank receives the summed gradient of its slices only; then their norm."""
        for k, part in enumerate(st.parts):
            if part[0] not in early_sent:
                self._exchange_part(st, k)
        if st.gshard_w is not None:
            K.cast_bf16_f32(st.gshard_w, st.gshard)
        st.accumulate_norm(st.gshard)

    def _step_sharded(self, st, total):
        """The optimizer on this rank's slice of every chunk, then the all-gather of the updated parameters (fp32, or bf16 on the wire)."""
        b, r = st.bucket, self.comm.rank
        for k, (cid, lo, hi, own, off) in enumerate(st.parts):
            mlo, mhi = lo + r * own, lo + (r + 1) * own
            mine = b.params[mlo:mhi]
            st.step(mine, st.gshard[off:off + own], off, own, k, total, self.max_grad_norm, self.world)
            if st.pwire is None or cid >= FP32_WIRE:
                self.comm.all_gather(mine, b.params[lo:hi])      # every rank holds the updated masters again
                continue
            self._masters_stale = True
            K.cast_f32_bf16(mine, st.pwire[mlo:mhi])             # bf16 on the wire: what the layers' operands are made of anyway
            self.comm.all_gather(st.pwire[mlo:mhi], st.pwire[lo:hi])
            if mlo > lo:                                          # the other ranks' slices: bf16 -> fp32 -> (repack) bf16 is exact
                K.cast_bf16_f32(st.pwire[lo:mlo], b.params[lo:mlo])
            if mhi < hi:
                K.cast_bf16_f32(st.pwire[mhi:hi], b.params[mhi:hi])
        if st.gwire is None:
            b.grads.zero_()                                       # zero_grad of the full bucket (the kernel cleared the slice copy only)

    def _step_flat(self, st, total):
        for k, (off, n) in enumerate(st.segments):            # one fused launch sequence per lr segment
            st.step(st.bucket.params[off:off + n], st.bucket.grads[off:off + n], off, n, k, total, self.max_grad_norm, self.world)

    def optimizer_step(self, early_sent=()):
        """early_sent: ids of the chunks the last backward already reduce-scattered (overlap_exchange)."""
        states = self._states()
        for st in states:
            if st.shard:
                self._reduce_sharded(st, early_sent)
            else:
                st.accumulate_norm(st.bucket.grads)
        # clip_grad_norm_ over ALL trainable parameters (train_ac.py:485-489): slices add up across ranks (one 4-byte all-reduce)
        total = None
        if any(st.shard for st in states):
            total = torch.stack([st.sumsq for st in states if st.shard]).sum(0)
            self.comm.all_reduce_(total)
        rest = [st.sumsq for st in states if not st.shard and st.clipped]
        if rest:
            r = rest[0] if len(rest) == 1 else torch.stack(rest).sum(0)
            total = r if total is None else total + r
        for st in states:
            (self._step_sharded if st.shard else self._step_flat)(st, total)
        if self.ema_cfg is not None:           # update_ema (train_ac.py:503,517-521)
            for st in states:
                if st.ema is not None:
                    K.ema_update(st.ema, st.bucket.params, st.step_count, **self.ema_cfg)
        self._refresh_buckets()

    def ema_state_dict(self):
        """{parameter name: EMA tensor} with the parameters' own shapes (what ModelEMA.state_dict() returns, utils/ema.py:46-47)."""
        out = {}
        ids = {id(p): n for n, p in self.unet.named_parameters()}
        if self.text_encoder is not None:
            ids.update({id(p): n for n, p in self.text_encoder.named_parameters()})
        for st in self._states():
            if st.ema is None:
                continue
            b = st.bucket
            base = b.params.data_ptr()
            for name, p in b.named_tensors():
                if b is self.bucket or b is self.te_bucket:       # LoRA factors: the model's names (the checkpoint keys)
                    name = ids.get(id(p), name)
                off = (p.data_ptr() - base) // 4
                out[name] = st.ema[off:off + p.numel()].as_strided(p.shape, p.stride())
        return out

    def save_model(self, ckpt_manager, step, name="unet"):
        """Trainer.save_model for the UNet half (train_ac.py:523-528): ``{name}-{step}`` with base / lora (+ _ema) sections and one
        ``{name}-{plugin}-{step}`` file per plugin, through a ckpt.CkptManagerNative (or the reference's own manager)."""
        from .ckpt import _EMAView
        from .patch_api import PluginGroup
        if self._masters_stale and self.world > 1:
            raise RuntimeError("param_wire='bf16': the fp32 masters of other ranks' slices are bf16-rounded here; call sync_masters() on "
                               "EVERY rank before save_model()")
        ema = _EMAView(self.ema_state_dict(), self.unet) if self.ema_cfg else None
        paths = [ckpt_manager.save_model_with_lora(self.unet, self.lora_group, name=name, step=step, model_ema=ema)]
        if self.lora_te_group is not None:     # train_ac.py:529-533: the text encoder's own file
            te_ema = _EMAView(self.ema_state_dict(), self.text_encoder) if self.ema_cfg else None
            paths.append(ckpt_manager.save_model_with_lora(self.text_encoder, self.lora_te_group, name="text_encoder", step=step, model_ema=te_ema,
                                                           exclude_key="emb_ex."))      # train_ac.py:531-533: the words have files of their own
        if self.pt_words:                      # train_ac.py:542: {word}-{step}.pt, the reference's save_emb layout
            paths += ckpt_manager.save_embedding(self.pt_words, step, False) or []
        for plugin in self.plugins:
            pema = None
            if ema is not None:             # EMA names of a plugin bucket are relative to the plugin; a whole-model plugin's
                pema = _EMAView({f".{plugin.name}.{k}": v for k, v in ema.state_dict().items()}, torch.nn.Module())   # block path is ''
            paths += ckpt_manager.save_plugins(self.unet, {plugin.name: PluginGroup({"": plugin})}, name=name, step=step, model_ema=pema)
        return paths

    def set_lr_factor(self, factor):
        """lr scheduler hook (LambdaLR semantics of the reference's get_scheduler): every param group's lr = its own base lr x factor."""
        for st in self._states():
            for lr_t, base in zip(st.lrs, st.base_lrs):
                lr_t.fill_(base * factor)

    def set_lr(self, lr):
        """Set the lr of the groups that were built with the constructor's `lr`; groups with their own lr keep their ratio to it
        (the constructor's ``scale_lr_factor`` stays applied, as the reference's scale_lr multiplies every group's lr once:
        train_ac.py:192-197)."""
        if self._ctor_lr == 0:                 # built with lr 0 (e.g. a warm-up that starts from zero): no ratio to keep
            for st in self._states():
                for lr_t in st.lrs:
                    lr_t.fill_(lr * self._scale_lr_factor)
            return
        self.set_lr_factor(lr / self._ctor_lr)

    # ---- one optimisation step
    def train_one_step(self, latents, encoder_hidden_states=None, mask=None, added_cond_kwargs=None, plugin_input=None, prompt_ids=None,
                       attn_mask=None):
        """latents [B,4,h,w] fp32 (cached VAE latents), encoder_hidden_states [B,L,D]; SDXL adds
        added_cond_kwargs={"text_embeds" [B,1280], "time_ids" [B,6]}; plugins read plugin_input (ControlNet: {"cond"});
        attn_mask [B,L]: the batch's ``attn_mask`` (text encoder attention_mask / UNet encoder_attention_mask, wrapper.py:20,29).
        Returns the loss as a device tensor (no host sync)."""
        return self.train_data_list([dict(latents=latents, encoder_hidden_states=encoder_hidden_states, mask=mask, attn_mask=attn_mask,
                                          added_cond_kwargs=added_cond_kwargs, plugin_input=plugin_input, prompt_ids=prompt_ids)])

    @staticmethod
    def _tensors(batch):
        """(path, tensor) for every tensor input of a batch dict (nested one level: added_cond_kwargs / plugin_input)."""
        for k, v in batch.items():
            if torch.is_tensor(v):
                yield (k,), v
            elif isinstance(v, dict):
                for k2, v2 in v.items():
                    if torch.is_tensor(v2):
                        yield (k, k2), v2

    def _run_all(self, data_list, exchange=False):
        K.wgrad_staging_begin_step()
        total = None
        for i, b in enumerate(data_list):
            keep, self.loss_weight = self.loss_weight, self.loss_weight * b.get("loss_weight", 1.0)
            if self._pyramid is not None:
                self._pyramid.idx = i              # (this batch's level table; None again below: forward_backward called on its own)
            try:
                l = self.forward_backward(b["latents"], b.get("encoder_hidden_states"), b.get("mask"), b.get("added_cond_kwargs"),
                                          b.get("plugin_input"), b.get("prompt_ids"), b.get("attn_mask"),
                                          exchange=exchange and i == len(data_list) - 1)
            finally:
                self.loss_weight = keep
                if self._pyramid is not None:
                    self._pyramid.idx = None
            total = l if total is None else total + l
        return total

    def train_data_list(self, data_list):
        """The reference's ``train_one_step(data_list)`` (train_ac.py:467-504): one batch per dataset (DreamBooth: instance +
        class images), each forward/backward accumulating into the same gradient buckets, then ONE clip + optimizer step.
        Per-dataset ``loss_weight`` (train_ac.py:481, get_loss_weights) scales that batch's loss and gradient.  Returns the
        summed loss (device tensor).  With gradient accumulation the exchange + optimizer step run on every N-th call."""
        data_list = [{**b, "latents": b["latents"].float().contiguous()} for b in data_list]     # the caller's dicts stay untouched
        if self.pt_bucket is not None:     # custom ids without a word: refused here while the batch is still on the host
            from .prompt_tuning import check_ids
            for b in data_list:
                if b.get("prompt_ids") is not None:
                    check_ids(self.pt_hook, b["prompt_ids"])
        if self.cfg_active:                 # refused before anything is enqueued or captured
            for b in data_list:
                self._check_cfg_batch(b)
        self._micro += 1
        sync = self._micro % self.accum == 0
        early = sync and self._overlap             # this backward sends the early chunks itself
        sent = ()
        if not self.use_graph:
            if self._pyramid is not None:
                self._pyramid.draw_levels(data_list)
            self.loss = self._run_all(data_list, exchange=early)
            sent = tuple(sorted(self._sent))
        else:
            sig = self._signature(data_list) + (early,)
            entry = self._graph_cache.pop(sig, None)
            if entry is None:                      # a new aspect-ratio bucket / context length: capture once, replay afterwards
                if len(self._graph_cache) >= self.max_graph_signatures:
                    self._graph_cache.pop(next(iter(self._graph_cache)))          # least recently used (dict order = use order)
                    if not self._warned_evict:
                        self._warned_evict = True
                        import warnings
                        warnings.warn(f"hcp_diffusion_amd: more than {self.max_graph_signatures} batch signatures: the least recently used step "
                                      "graph is dropped and re-captured on its next use (raise NativeTrainer.max_graph_signatures)")
                entry = self._capture(data_list, sig, early)
            self._graph_cache[sig] = entry         # most recently used last
            graph, static, loss, sent = entry
            for sb, b in zip(static, data_list):
                live = dict(self._tensors(b))
                for path, t in self._tensors(sb):
                    t.copy_(live[path])
            if self._pyramid is not None:
                self._pyramid.draw_levels(data_list)   # the level tables are static inputs too: this step's sizes, drawn as eager mode draws them
            graph.replay()
            self.loss = loss
        if sync:
            # param_wire='bf16': after this step the other ranks' slices of the fp32 masters are bf16-rounded here.  Set at the SYNC STEP,
            # not inside optimizer_step(): a captured optimizer step replays without running that Python.
            if any(st.shard and st.pwire is not None for st in self._states()):
                self._masters_stale = True
            self.all_reduce()
            if self._opt_graph is not None and self._opt_graph_sent == tuple(sent):
                self._opt_graph.replay()
            else:
                self.optimizer_step(early_sent=sent)
            ops.invalidate_merged_cache()      # the parameters moved (raw-pointer kernels, possibly a graph replay: no version counter saw it)
        return self.loss

    def _signature(self, data_list):
        """What a captured forward/backward graph is specialised to: shapes / dtypes of every tensor input, per dataset (the
        reference's aspect-ratio buckets hand every step ONE resolution, but a different one from step to step:
        data/bucket.py:167-204), plus the scalar settings baked into the kernels' arguments."""
        return tuple(tuple(sorted((path, tuple(t.shape), str(t.dtype)) for path, t in self._tensors(b))) + (b.get("loss_weight", 1.0),)
                     for b in data_list)

    def _snapshot(self):
        snap = [(st, [t.clone() for t in st.tensors()], st.bucket.params.clone(), st.bucket.grads.clone()) for st in self._states()]
        drop = [(m._hcp_dropout, m._hcp_dropout.snapshot()) for m in self._dropout_modules if m._hcp_dropout is not None]
        return snap, torch.get_rng_state(), (torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None), random.getstate(), drop

    def _restore(self, saved):
        snap, cpu_rng, dev_rng, host_rng, drop = saved
        random.setstate(host_rng)                  # (pyramid noise draws its level sizes from the global `random` module)
        for nd, saved_nd in drop:                  # native dropout: the warm-up steps advanced the modules' forward counts
            nd.restore(saved_nd)
        with torch.no_grad():
            for st, ts, p_, g_ in snap:
                for t, v in zip(st.tensors(), ts):
                    t.copy_(v)
                st.bucket.params.copy_(p_)
                st.bucket.grads.copy_(g_)
        torch.set_rng_state(cpu_rng)
        if dev_rng is not None:
            torch.cuda.set_rng_state(dev_rng, self.device)
        self._refresh_buckets()

    def _capture(self, data_list, sig, early=False):
        def clone(b):
            return {k: (v.clone() if torch.is_tensor(v) else {k2: v2.clone() for k2, v2 in v.items()} if isinstance(v, dict) else v)
                    for k, v in b.items() if v is not None}
        static = [clone(b) for b in data_list]
        # Warm-up on a side stream (allocator growth, lazy weight packing and autotuned workspaces must not happen inside the
        # capture).  It runs real steps, so every piece of training state it touches — parameters, gradients, AdamW moments,
        # step counters, EMA, the RNG streams (torch's and the host `random` module's) — is put back afterwards: the first captured step is the FIRST optimisation step,
        # as in eager mode and as in the reference.
        saved = self._snapshot()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        # The warm-up exchanges NOTHING: a rank that meets a new batch signature alone (a data pipeline that does not hand every rank
        # the same shape on the same step) must not issue collectives its peers do not — NullComm stands in while it runs.
        comm, self.comm = self.comm, _WarmupComm(self.comm)
        try:
            with torch.cuda.stream(side):
                for _ in range(2):
                    if self._pyramid is not None:
                        self._pyramid.draw_levels(static)
                    self._run_all(static, exchange=early)
                    self.all_reduce()
                    self.optimizer_step(early_sent=tuple(sorted(self._sent)))
        finally:
            self.comm = comm
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._restore(saved)
        torch.cuda.synchronize()
        pool = next(iter(self._graph_cache.values()))[0].pool() if self._graph_cache else None
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, pool=pool):
            loss = self._run_all(static, exchange=early)      # (the early chunks' reduce-scatters become a side branch of this graph)
        sent = tuple(sorted(self._sent))
        entry = (g1, static, loss, sent)
        self._graph_cache[sig] = entry
        sharded = any(st.shard for st in self._states())
        if self._opt_graph is None and (not sharded or isinstance(self.comm, (NullComm, AbiComm))):
            # the optimizer step is shape independent: captured once.  Sharded buckets interleave collectives with the kernels:
            # captured when they go through the C ABI (hcp_reduce_scatter_flat / hcp_allgather_flat are stream-ordered launches like any
            # kernel: tests/test_comm.py); torch.distributed collectives stay eager — some twenty launches.
            saved = self._snapshot()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, pool=g1.pool()):
                self.optimizer_step(early_sent=sent)
            self._opt_graph, self._opt_graph_sent = g2, sent
            self._restore(saved)              # capture does not execute, but keep the contract explicit
        return entry
