"""Inference over the native UNet: the classifier-free-guidance batched forward of the reference's pipeline
hook (utils/pipe_hook.py:120-140: ``torch.cat([latents] * 2)`` -> ONE UNet call -> ``uncond + scale (text - uncond)``) and a DDIM
(eta = 0) step, fused into one kernel per step (``hcp_cfg_ddim_step``).  This is what the in-training previewer
(loggers/preview/image_previewer.py:97-149) needs from the UNet side; the VAE decoder and the prompt pipeline stay the reference's.

``NativeDDIMSampler.sample`` runs the whole denoising loop on the device with no host synchronisation.

``NativeEulerSampler`` is the sampler the reference's inference and workflow configs name (diffusers EulerAncestralDiscreteScheduler;
``ancestral=False``: EulerDiscreteScheduler) over ``csrc/sampler.hip``: one launch per step does guidance, the update, the ancestral
noise, the legacy inpaint blend and the next UNet input, everything per-step is read from a device table through a device counter, and
``use_graph=True`` replays ONE captured graph {UNet forward, step, advance} for every step of every run of a signature."""
import math
import warnings

import torch

from . import kernels as K
from .trainer import ddpm_alphas_cumprod


def _cfg_inputs(B, cond, uncond, guidance_scale, encoder_attention_mask, added_cond_kwargs, uncond_added_cond_kwargs):
    """(guided, text states, UNet keyword arguments) of a sampling loop: [uncond ; cond] rows when guided, the key-mask row rules of the
    reference's previewer (image_previewer.py:133-135,147)."""
    guided = uncond is not None and guidance_scale != 1.0
    ehs = torch.cat([uncond, cond]) if guided else cond
    added = None
    if added_cond_kwargs is not None:
        u = uncond_added_cond_kwargs or added_cond_kwargs
        added = {k: torch.cat([u[k], v]) if guided else v for k, v in added_cond_kwargs.items()}
    mask = None
    if encoder_attention_mask is not None:
        rows = encoder_attention_mask.shape[0]
        if rows == 2 * B:                                      # reference order [negative prompts; prompts]
            mask = encoder_attention_mask if guided else encoder_attention_mask[B:]      # unguided: the prompts' rows only
        elif rows == B:
            mask = torch.cat([encoder_attention_mask] * 2) if guided else encoder_attention_mask
        else:
            raise ValueError(f"encoder_attention_mask has {rows} rows for a batch of {B}: expected [B, L] or [2B, L] "
                             "([negative prompts; prompts])")
    kw = {}
    if mask is not None:
        kw["encoder_attention_mask"] = mask
    if added is not None:
        kw["added_cond_kwargs"] = added
    return guided, ehs, kw


class NativeDDIMSampler:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1):
        self.acp = ddpm_alphas_cumprod(num_train_timesteps, beta_start, beta_end)       # host copy: the step coefficients are scalars
        self.num_train_timesteps, self.steps_offset = num_train_timesteps, steps_offset

    def timesteps(self, num_inference_steps):
        """Leading spacing with the Stable Diffusion offset (diffusers DDIMScheduler, timestep_spacing='leading', steps_offset=1)."""
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (torch.arange(num_inference_steps) * ratio).flip(0) + self.steps_offset
        return ts.clamp(max=self.num_train_timesteps - 1)

    @torch.no_grad()
    def sample(self, unet, latents, cond, uncond=None, guidance_scale=7.5, num_inference_steps=20, encoder_attention_mask=None,
               added_cond_kwargs=None, uncond_added_cond_kwargs=None):
        """latents [B,4,h,w] fp32 unit-variance noise; cond / uncond [B,L,D] text states.  encoder_attention_mask: [B,L] (the same key
        mask for both halves of the guided batch) or [2B,L] in the reference's order [negative prompts; prompts] — what the previewer
        hands the pipeline when ``encoder_attention_mask`` is on (image_previewer.py:133-135,147).  Returns the denoised latents."""
        dev = latents.device
        x = latents.float().contiguous().clone()
        guided, ehs, kw = _cfg_inputs(x.shape[0], cond, uncond, guidance_scale, encoder_attention_mask, added_cond_kwargs,
                                      uncond_added_cond_kwargs)
        ts = self.timesteps(num_inference_steps)
        ratio = self.num_train_timesteps // num_inference_steps
        for t in ts.tolist():
            xin = torch.cat([x, x]) if guided else x                      # pipe_hook.py:121
            tt = torch.full((xin.shape[0],), t, dtype=torch.long, device=dev)
            eps2 = unet(xin, tt, ehs, **kw).sample.float().contiguous()
            prev = t - ratio
            a_t = float(self.acp[t]); a_prev = float(self.acp[prev]) if prev >= 0 else float(self.acp[0])
            K.cfg_ddim_step(x, eps2, a_t, a_prev, guidance_scale, out=x)
        return x


class _GraphEntry:
    __slots__ = ("graph", "capacity", "x", "model_in", "t", "table", "state", "ehs", "kw", "init", "noise0", "mask")


class NativeEulerSampler:
    """Euler-ancestral (``ancestral=True``) or plain Euler sampling, epsilon prediction, in sigma space: sigma = sqrt((1 - acp) / acp) at
    the run's timesteps, x' = x + eps (sigma_down - sigma) + z sigma_up, the UNet sees x / sqrt(sigma^2 + 1).

    The ancestral noise is drawn in the step kernel from (seed, step, element) — Philox4x32-10 + Box-Muller, csrc/sampler.hip — so a run
    is a function of ``seed`` and its inputs, on any stream, eager or replayed.  It is NOT torch's generator stream: the same seed gives
    other numbers than diffusers' ``randn_tensor``.

    'leading' and 'trailing' spacings give integer timesteps.  'linspace' (diffusers' default for this scheduler) gives non-integer
    timesteps and interpolated sigmas, and the native UNet takes int64 timesteps: it is refused, not rounded."""

    def __init__(self, ancestral=True, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, timestep_spacing="leading",
                 steps_offset=1, seed=0):
        if timestep_spacing == "linspace":
            raise NotImplementedError("timestep_spacing='linspace' gives non-integer timesteps and interpolated sigmas; the native UNet "
                                      "takes int64 timesteps — use 'leading' or 'trailing' (nothing is rounded silently)")
        if timestep_spacing not in ("leading", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: 'leading' or 'trailing'")
        self.acp = ddpm_alphas_cumprod(num_train_timesteps, beta_start, beta_end)
        self.ancestral, self.num_train_timesteps, self.timestep_spacing, self.steps_offset = ancestral, num_train_timesteps, timestep_spacing, steps_offset
        self.seed = int(seed)
        self.captures = 0                       # graphs captured so far (a replayed run does not count)
        self._graphs = {}
        self._warned = False

    def timesteps(self, num_inference_steps):
        """int64 [n], descending (diffusers' set_timesteps for the two integer spacings)."""
        n, T = int(num_inference_steps), self.num_train_timesteps
        if n < 1:
            raise ValueError("num_inference_steps must be >= 1")
        if self.timestep_spacing == "leading":
            ts = (torch.arange(n) * (T // n)).flip(0) + self.steps_offset
        else:
            ts = torch.round(torch.arange(T, 0, -T / n, dtype=torch.float64)).long()[:n] - 1
        return ts.clamp(min=0, max=T - 1)

    def _sigma64(self, ts):
        a = self.acp.double()[ts]
        return ((1 - a) / a).sqrt()

    def sigmas(self, num_inference_steps):
        """float32 [n + 1]: sigma at the run's timesteps, then the terminal 0."""
        return torch.cat([self._sigma64(self.timesteps(num_inference_steps)), torch.zeros(1, dtype=torch.float64)]).float()

    def start_step(self, num_inference_steps, strength=None):
        """Row an img2img run starts at: steps - int(steps * strength) (``get_timesteps`` of the reference's pipelines)."""
        n = int(num_inference_steps)
        if strength is None:
            return 0
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"strength {strength!r}: in (0, 1]")
        run = min(int(n * strength), n)
        if run < 1:
            raise ValueError(f"strength {strength} leaves no step of {n}")
        return n - run

    def table(self, num_inference_steps, strength=None):
        """The step table of csrc/sampler.hip, float32 [n, 8], computed in float64 and rounded once: row i = (sigma_i, sigma_down_i,
        sigma_up_i, c_in_next_i, timestep_i, timestep_next_i, sigma_init_i, c_in_i).  Every row is filled; a run with ``strength``
        starts at row ``start_step(n, strength)``."""
        self.start_step(num_inference_steps, strength)
        ts = self.timesteps(num_inference_steps)
        s = self._sigma64(ts)
        nxt = torch.cat([s[1:], torch.zeros(1, dtype=torch.float64)])
        if self.ancestral:
            up = (nxt ** 2 * (s ** 2 - nxt ** 2) / s ** 2).clamp(min=0).sqrt()
            down = (nxt ** 2 - up ** 2).clamp(min=0).sqrt()
        else:
            up, down = torch.zeros_like(s), nxt
        t64 = ts.double()
        init = (s ** 2 + 1).sqrt() if self.timestep_spacing == "leading" else s        # diffusers' init_noise_sigma
        rows = [s, down, up, 1 / (nxt ** 2 + 1).sqrt(), t64, torch.cat([t64[1:], t64[-1:]]), init, 1 / (s ** 2 + 1).sqrt()]
        return torch.stack(rows, dim=1).float().contiguous()

    # ------------------------------------------------------------------------------------------------------------------ the loop
    @staticmethod
    def _body(unet, e, guidance, noise_i):
        eps2 = unet(e.model_in, e.t, e.ehs, **e.kw).sample.float().contiguous()
        K.euler_step(e.x, eps2, e.table, e.state, guidance, noise=noise_i, init=e.init if e.mask is not None else None, noise0=e.noise0,
                     mask=e.mask, out=e.x, model_in_next=e.model_in)
        K.sampler_advance(e.state, e.table, e.t)

    def _buffers(self, x, guided, ehs, kw, init, mask, capacity):
        e = _GraphEntry()
        dev, B = x.device, x.shape[0]
        rows = 2 * B if guided else B
        e.graph, e.capacity = None, capacity
        e.x = torch.empty_like(x)
        e.model_in = torch.empty((rows,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
        e.t = torch.zeros(rows, dtype=torch.int64, device=dev)
        e.table = torch.zeros(capacity, K.SAMPLER_ROW, dtype=torch.float32, device=dev)
        e.state = K.sampler_state(self.seed, dev)
        e.ehs = ehs.clone()
        e.kw = {k: ({a: b.clone() for a, b in v.items()} if isinstance(v, dict) else v.clone()) for k, v in kw.items()}
        e.init = torch.empty_like(x) if init is not None else None
        e.mask = torch.empty((B, 1) + tuple(x.shape[2:]), dtype=torch.float32, device=dev) if mask is not None else None
        e.noise0 = torch.empty_like(x) if mask is not None else None
        return e

    def _load(self, e, x, ehs, kw, init, mask, tab, start):
        """This run's inputs into the entry's buffers, then hcp_sampler_begin: nothing else happens on the host before the loop."""
        e.x.copy_(x)
        e.ehs.copy_(ehs)
        for k, v in kw.items():
            if isinstance(v, dict):
                for a, b in v.items():
                    e.kw[k][a].copy_(b)
            else:
                e.kw[k].copy_(v)
        if e.init is not None:
            e.init.copy_(init)
        if e.mask is not None:
            e.mask.copy_(mask)
            e.noise0.copy_(x)                       # the start noise: what the blend re-noises the kept region with
        n = tab.shape[0]
        full = torch.cat([tab, tab[-1:].expand(e.capacity - n, -1)]) if e.capacity > n else tab      # rows past the run repeat its final row
        e.table.copy_(full)
        e.state.copy_(torch.tensor([self.seed, 0], dtype=torch.int64))
        K.sampler_begin(e.state, e.table, e.x, e.t, start, model_in=e.model_in, noise=e.x, init=e.init)

    def _warn(self, msg):
        if not self._warned:
            self._warned = True
            warnings.warn("hcp_diffusion_amd: NativeEulerSampler(use_graph=True) runs eagerly: " + msg)

    @torch.no_grad()
    def sample(self, unet, latents, cond, uncond=None, guidance_scale=7.5, num_inference_steps=20, encoder_attention_mask=None,
               added_cond_kwargs=None, uncond_added_cond_kwargs=None, init_latents=None, strength=None, mask=None, noise=None,
               use_graph=False):
        """latents [B,4,h,w]: unit-variance noise (scaled here: text2img x = latents * init_noise_sigma; with ``init_latents``
        x = init_latents + latents * sigma_start).  cond / uncond / encoder_attention_mask / added_cond_kwargs as in
        ``NativeDDIMSampler.sample``.  ``strength`` (with ``init_latents``) starts at step ``steps - int(steps * strength)``.
        ``mask`` [B,1,h,w] (1 = keep ``init_latents``; needs them): the legacy inpaint blend, re-noised with ``latents``.
        ``noise`` [steps,B,4,h,w] replaces the in-kernel draw of step i by noise[i] (tests pin the arithmetic with it; such a run is
        eager).  ``use_graph=True``: one captured graph per signature, replayed once per step.  Returns the denoised latents."""
        x = latents.float().contiguous()
        dev, B = x.device, x.shape[0]
        guided, ehs, kw = _cfg_inputs(B, cond, uncond, guidance_scale, encoder_attention_mask, added_cond_kwargs, uncond_added_cond_kwargs)
        n = int(num_inference_steps)
        if strength is not None and init_latents is None:
            raise ValueError("strength needs init_latents")
        if mask is not None and init_latents is None:
            raise ValueError("mask needs init_latents")
        tab, start = self.table(n, strength), self.start_step(n, strength)
        init = init_latents.float().contiguous() if init_latents is not None else None
        if init is not None and init.shape != x.shape:
            raise ValueError(f"init_latents {tuple(init.shape)} for latents {tuple(x.shape)}")
        if mask is not None:
            mask = mask.to(dtype=torch.float32).expand(B, 1, *x.shape[2:]).contiguous()
        if noise is not None:
            if tuple(noise.shape) != (n,) + tuple(x.shape):
                raise ValueError(f"noise {tuple(noise.shape)}: expected {(n,) + tuple(x.shape)}")
            noise = noise.float().contiguous()
        g = float(guidance_scale) if guided else 1.0

        if use_graph:
            from . import graphed
            if not x.is_cuda:
                self._warn("graphs need the HIP device")
            elif noise is not None:
                self._warn("noise= is a per-step input")
            elif not graphed.capturable(unet):
                self._warn("the UNet is not capturable (active torch dropout, forward hooks, or nothing trainable)")
            else:
                return self._sample_graphed(unet, x, guided, g, ehs, kw, init, mask, tab, start)
        e = self._buffers(x, guided, ehs, kw, init, mask, n)
        self._load(e, x, ehs, kw, init, mask, tab, start)
        for i in range(start, n):
            self._body(unet, e, g, noise[i] if noise is not None else None)
        return e.x

    def _sample_graphed(self, unet, x, guided, g, ehs, kw, init, mask, tab, start):
        def sig(t):
            return (tuple(t.shape), t.dtype)
        key = (id(unet), x.device.index, tuple(x.shape), guided, g, init is not None, mask is not None, sig(ehs),
               tuple(sorted((k, tuple(sorted((a, sig(b)) for a, b in v.items())) if isinstance(v, dict) else sig(v)) for k, v in kw.items())))
        n = tab.shape[0]
        e = self._graphs.get(key)
        if e is None or e.capacity < n:
            e = self._buffers(x, guided, ehs, kw, init, mask, n)
            cur = torch.cuda.current_stream(x.device)
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._load(e, x, ehs, kw, init, mask, tab, start)
                self._body(unet, e, g, None)        # warm-up: lazy packing, workspaces — nothing may allocate or pack under capture
                e.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(e.graph, stream=side):
                    self._body(unet, e, g, None)
            cur.wait_stream(side)
            self.captures += 1
            self._graphs[key] = e
        self._load(e, x, ehs, kw, init, mask, tab, start)
        for _ in range(start, n):
            e.graph.replay()
        return e.x.clone()
