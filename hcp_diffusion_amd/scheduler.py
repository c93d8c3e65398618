"""Seam 4 (``model.noise_scheduler``, train_base.yaml:76 -> train_ac.py:211): the slice of diffusers' DDPMScheduler the training
step uses — ``config.num_train_timesteps`` and ``add_noise`` (train_ac.py:437-447) — over the native kernel.

``add_noise(x0, noise, t) = sqrt(acp_t) x0 + sqrt(1 - acp_t) noise`` with the scaled-linear beta schedule of Stable Diffusion
(constants as in the reference's loggers/preview/image_previewer.py:28).

The reference's ``hcpdiff.noise`` wrappers around that object have native counterparts here: ``NativePyramidNoiseScheduler``
(multi-resolution noise, two launches whatever the level count: csrc/noise.hip) and ``NativeZeroTerminalScheduler`` (betas rescaled to
zero terminal SNR).  Both delegate every other attribute to the scheduler they wrap and compose in either order."""
import random
from types import SimpleNamespace

import torch

from . import kernels as K


class NativeDDPMScheduler:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear"):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, prediction_type="epsilon")
        # the three schedules of diffusers' DDPMScheduler (published definitions; Stable Diffusion trains with 'scaled_linear')
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "squaredcos_cap_v2":         # Nichol & Dhariwal's cosine schedule, betas capped at 0.999
            import math
            bar = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
            betas = torch.tensor([min(1 - bar((i + 1) / num_train_timesteps) / bar(i / num_train_timesteps), 0.999)
                                  for i in range(num_train_timesteps)], dtype=torch.float32)
        else:
            raise NotImplementedError(f"beta_schedule {beta_schedule!r}: 'scaled_linear', 'linear' and 'squaredcos_cap_v2' exist")
        self.betas = betas                                 # (diffusers' attribute names: the zero-terminal wrapper replaces all three)
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self._acp_dev = {}

    def _acp(self, device):
        key = str(device)
        hit = self._acp_dev.get(key)
        if hit is None or hit[0] is not self.alphas_cumprod:       # (a wrapper replaced the table: the device copy follows)
            hit = self._acp_dev[key] = (self.alphas_cumprod, self.alphas_cumprod.to(device=device, dtype=torch.float32))
        return hit[1]

    def add_noise(self, original_samples, noise, timesteps):
        x0 = original_samples.float().contiguous()
        return K.add_noise(x0, noise.float().contiguous(), timesteps.long(), self._acp(x0.device)).to(original_samples.dtype)


class NativeNoiseBase:
    """A wrapper around a noise scheduler (the reference's noise/noise_base.py): attributes it does not define are the wrapped
    scheduler's, for reading AND for writing — ``wrapper.alphas_cumprod = table`` reaches the scheduler that owns the table through any
    number of wrappers, which is what lets the two wrappers below compose in either order."""

    def __init__(self, base_scheduler):
        object.__setattr__(self, "base_scheduler", base_scheduler)

    def __getattr__(self, item):                           # (only called when normal lookup fails)
        if item == "base_scheduler":
            raise AttributeError(item)
        return getattr(self.base_scheduler, item)

    def __setattr__(self, key, value):
        if key not in self.__dict__ and hasattr(self.base_scheduler, key):
            setattr(self.base_scheduler, key, value)
        else:
            object.__setattr__(self, key, value)


def _acp_on(scheduler, device):
    """The alphas_cumprod table of any (wrapped) scheduler as fp32 on `device`."""
    if hasattr(scheduler, "_acp"):
        return scheduler._acp(device)
    return scheduler.alphas_cumprod.to(device=device, dtype=torch.float32)


def pyramid_level_bounds(h, w, level, step_size):
    """[(hn, wn)] upper bounds of the level sizes: the reference's loop with the smallest ratio it can draw (r = step_size).  Every draw
    has r >= step_size, so level i is never larger than bound i and the loop never runs longer than this list."""
    out = []
    for i in range(1, level):
        r = step_size
        wn, hn = max(1, int(w / (r ** i))), max(1, int(h / (r ** i)))
        out.append((hn, wn))
        if wn == 1 or hn == 1:
            break
    return out


def pyramid_level_dims(h, w, level, step_size):
    """[(hn, wn)] of one draw — the host side of pyramid_noise.py:25-30: one ``random.random()`` of the global module per level,
    r = that * 2 + step_size, sizes max(1, int(. / r**i)), stop after the first level with a side of 1."""
    out = []
    for i in range(1, level):
        r = random.random() * 2 + step_size
        wn, hn = max(1, int(w / (r ** i))), max(1, int(h / (r ** i)))
        out.append((hn, wn))
        if wn == 1 or hn == 1:
            break
    return out


def check_pyramid_args(level, discount, step_size, resize_mode):
    if resize_mode not in K.PYRAMID_MODES:
        raise ValueError(f"pyramid noise resize_mode {resize_mode!r}: 'bilinear' or 'nearest'")
    if not (isinstance(level, int) and 1 <= level <= K.PYRAMID_MAX_LEVELS + 1):
        raise ValueError(f"pyramid noise level {level!r}: an int in [1, {K.PYRAMID_MAX_LEVELS + 1}] (level - 1 fields, one launch holds "
                         f"{K.PYRAMID_MAX_LEVELS})")
    if not step_size > 0:
        raise ValueError(f"pyramid noise step_size {step_size!r}: must be positive")
    float(discount)


class PyramidNoiseState:
    """Pyramid noise inside NativeTrainer's step: the settings, per position in the step's data list one device table [n_active, (hn, wn)
    x PYRAMID_MAX_LEVELS] — static inputs of the captured step, filled on the host before every step —, their pinned staging rings, the
    workspace of the ordered partial sums, and `idx`: the table of the batch being run (None: forward_backward called on its own)."""

    def __init__(self, settings, device):
        self.level, self.discount, self.step_size, self.resize_mode = (settings[k] for k in ("level", "discount", "step_size", "resize_mode"))
        self.device, self.tables, self.staging, self.ws, self.idx = device, {}, {}, None, None

    def table(self, idx):
        if idx not in self.tables:
            self.tables[idx] = torch.zeros(1 + 2 * K.PYRAMID_MAX_LEVELS, dtype=torch.int32, device=self.device)
        return self.tables[idx]

    def fill(self, idx, h, w):
        """One draw of the level sizes (the reference's host loop: one random.random() per level) into table `idx`; one small host-to-device
        copy, outside any capture.  On the GPU the copy is asynchronous, from a ring of pinned staging buffers: a copy from pageable memory
        returns only when the stream has drained, which would keep the host from enqueueing replay k + 1 while replay k runs.  Each slot
        carries the event of its last copy, waited for before the slot is written again (only a host eight steps ahead ever waits)."""
        dims = pyramid_level_dims(h, w, self.level, self.step_size)
        n = 1 + 2 * K.PYRAMID_MAX_LEVELS
        table = self.table(idx)
        if table.is_cuda:
            ring = self.staging.setdefault(idx, [[], 0])
            if len(ring[0]) < 8:
                ring[0].append((torch.zeros(n, dtype=torch.int32).pin_memory(), torch.cuda.Event()))
            host, done = ring[0][ring[1] % len(ring[0])]
            ring[1] += 1
            done.synchronize()
        else:
            host, done = torch.zeros(n, dtype=torch.int32), None
        host.zero_()
        host[0] = len(dims)
        host[1:1 + 2 * len(dims)] = torch.tensor(dims, dtype=torch.int32).flatten()
        table.copy_(host, non_blocking=True)
        if done is not None:
            done.record()
        return dims

    def draw_levels(self, data_list):
        """Before a step runs or replays: the level sizes of every dataset's batch, in order."""
        for i, b in enumerate(data_list):
            self.fill(i, b["latents"].shape[2], b["latents"].shape[3])

    def draw_fields(self, shape, device):
        """The level fields at their upper bounds (every draw of the sizes fits: r >= step_size): ONE randn, cut into the levels."""
        B, C, h, w = shape
        sizes = [B * C * hn * wn for hn, wn in pyramid_level_bounds(h, w, self.level, self.step_size)]
        flat = torch.randn(max(sum(sizes), 1), dtype=torch.float32, device=device)
        return list(flat.split(sizes)) if sizes else []

    def add_noise(self, latents, noise, t, acp):
        """PyramidNoiseScheduler.add_noise (noise/pyramid_noise.py:23-32): `noise` leaves as the unnormalised sum (the eps target, as in the
        reference, whose `noise += ...` writes into train_ac.make_noise's tensor while `noise / noise.std()` is a new one)."""
        idx = self.idx
        if idx is None:                                   # forward_backward called on its own (eager): this call's sizes are drawn here
            idx = 0
            self.fill(0, latents.shape[2], latents.shape[3])
        table = self.table(idx)
        fields = self.draw_fields(latents.shape, latents.device)
        if self.ws is None:
            self.ws = K.pyramid_noise_workspace(latents.device)
        K.pyramid_noise_accum(noise, fields, table[1:], table[:1], self.discount, self.resize_mode, self.ws)
        return K.pyramid_noise_finish(latents, noise, t, acp, self.ws)[0]


class NativePyramidNoiseScheduler(NativeNoiseBase):
    """PyramidNoiseScheduler (reference noise/pyramid_noise.py).  The host side of ``add_noise`` is the reference's loop (the global
    ``random`` module decides the level sizes); the level fields are drawn on the device, and all levels are resized, scaled and added
    by ONE launch, the std and the noisy latents by a second.

    As in the reference, ``noise`` is modified IN PLACE and is left holding the UNNORMALISED sum — the reference's ``noise += ...``
    writes into the caller's tensor, its ``noise = noise / noise.std()`` binds a new one — while the returned noisy latents are built
    from the sum divided by its std.  train_ac.make_noise hands that caller's tensor to the loss as the eps target."""

    def __init__(self, base_scheduler, level: int = 10, discount: float = 0.9, step_size: float = 2., resize_mode: str = 'bilinear'):
        super().__init__(base_scheduler)
        check_pyramid_args(level, discount, step_size, resize_mode)
        object.__setattr__(self, "level", level)
        object.__setattr__(self, "discount", discount)
        object.__setattr__(self, "step_size", step_size)
        object.__setattr__(self, "resize_mode", resize_mode)

    def add_noise(self, original_samples, noise, timesteps, fields=None):
        """fields: None (drawn here with torch.randn on noise's device) or a list of at least as many tensors as the draw has levels,
        field i holding at least B*C*hn_i*wn_i values (tests inject their draws)."""
        with torch.no_grad():
            b, c, h, w = noise.shape
            dims = pyramid_level_dims(h, w, self.level, self.step_size)
            dev = noise.device
            if fields is None:
                fields = [torch.randn(b, c, hn, wn, device=dev, dtype=torch.float32) for hn, wn in dims]
            if len(fields) < len(dims):
                raise ValueError(f"pyramid noise: {len(dims)} levels drawn, {len(fields)} fields given")
            fields = [f.to(device=dev, dtype=torch.float32).contiguous() for f in fields[:K.PYRAMID_MAX_LEVELS]]
            for f, (hn, wn) in zip(fields, dims):
                if f.numel() < b * c * hn * wn:
                    raise ValueError(f"pyramid noise: a field of {f.numel()} values for a level of {b}x{c}x{hn}x{wn}")
            table = torch.zeros(max(len(fields), 1), 2, dtype=torch.int32)
            for i, d in enumerate(dims):
                table[i, 0], table[i, 1] = d
            work = noise if (noise.dtype == torch.float32 and noise.is_contiguous()) else noise.float().contiguous()
            part = K.pyramid_noise_accum(work, fields, table.to(dev), torch.tensor([len(dims)], dtype=torch.int32).to(dev), self.discount,
                                         self.resize_mode)
            x0 = original_samples.float().contiguous()
            xt, _ = K.pyramid_noise_finish(x0, work, timesteps.long().contiguous(), _acp_on(self.base_scheduler, dev), part)
            if work is not noise:
                noise.copy_(work)                          # the caller's tensor carries the sum, in its own dtype
        return xt.to(original_samples.dtype)


def rescale_zero_terminal_snr(betas):
    """Algorithm 1 of Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed" (arXiv 2305.08891), in the fp32 torch
    operations and the operation order of the reference's noise/zero_terminal.py:21-42, so that the table carries the same bits: shift
    sqrt(alphas_cumprod) so that its last entry is 0, rescale so that its first entry is unchanged, and read the betas back."""
    abar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first, last = abar_sqrt[0].clone(), abar_sqrt[-1].clone()
    abar_sqrt -= last
    abar_sqrt *= first / (first - last)
    abar = abar_sqrt ** 2
    alphas = torch.cat([abar[0:1], abar[1:] / abar[:-1]])
    return 1 - alphas


class NativeZeroTerminalScheduler(NativeNoiseBase):
    """ZeroTerminalScheduler (reference noise/zero_terminal.py): replaces ``betas``, ``alphas`` and ``alphas_cumprod`` of the wrapped
    scheduler by the zero-terminal-SNR rescaling; ``add_noise`` is the wrapped scheduler's, on the new table.  alphas_cumprod[-1] is 0:
    anything that divides by it (the 'sample' loss, the SNR-weighted criteria, a DDIM-eps sampler) is not defined on this table."""

    def __init__(self, base_scheduler):
        super().__init__(base_scheduler)
        base_scheduler.betas = rescale_zero_terminal_snr(base_scheduler.betas)
        base_scheduler.alphas = 1.0 - base_scheduler.betas
        base_scheduler.alphas_cumprod = torch.cumprod(base_scheduler.alphas, dim=0)


class NativeEulerAncestralScheduler:
    """The method surface of diffusers' EulerAncestralDiscreteScheduler that the reference's pipelines (utils/pipe_hook.py HookPipe_T2I /
    _I2I / _inpaint) and its ImagePreviewer touch, over csrc/sampler.hip — for a caller that keeps its own denoising loop.
    ``NativeEulerSampler.sample`` is the same arithmetic with the loop on the device; given the same seed the two agree bit for bit.

    ``step`` is the unguided form of ``hcp_euler_step`` on the row found from ``t``.  The ancestral noise is drawn IN THE KERNEL from
    (seed, step, element): seeded from ``generator.initial_seed()`` when a generator is given, else from ``seed``.  It is not torch's
    random stream — the generator's state is neither read nor advanced, and the numbers are not those of diffusers' ``randn_tensor``.
    'linspace' spacing is refused (non-integer timesteps; sampler.NativeEulerSampler)."""
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 timestep_spacing="leading", steps_offset=1, prediction_type="epsilon", seed=0, ancestral=True):
        if beta_schedule != "scaled_linear" or prediction_type != "epsilon":
            raise NotImplementedError("NativeEulerAncestralScheduler: beta_schedule 'scaled_linear' and prediction_type 'epsilon' exist")
        from .sampler import NativeEulerSampler
        self._s = NativeEulerSampler(ancestral, num_train_timesteps, beta_start, beta_end, timestep_spacing, steps_offset, seed)
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      prediction_type=prediction_type)
        self.alphas_cumprod = self._s.acp
        self.timesteps = self.sigmas = None
        self._dev = {}

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = int(num_inference_steps)
        self.timesteps = self._s.timesteps(num_inference_steps)        # host int64: the loop's `t` indexes the table without a device read
        self.sigmas = self._s.sigmas(num_inference_steps)
        self._table = self._s.table(num_inference_steps)
        self._rows = {int(t): i for i, t in reversed(list(enumerate(self.timesteps.tolist())))}
        self._dev = {}

    @property
    def init_noise_sigma(self):
        if self.timesteps is None:
            self.set_timesteps(self.config.num_train_timesteps)
        return float(self._table[0, 6])

    def _on(self, device):
        """Per device: the step table, the same rows arranged so that a step is the identity and writes c_in x (scale_model_input),
        and the (seed, row) state with the host's record of the row it holds."""
        key = str(device)
        d = self._dev.get(key)
        if d is None:
            scale = self._table.clone()
            scale[:, 1], scale[:, 2], scale[:, 3] = self._table[:, 0], 0.0, self._table[:, 7]          # sigma_down = sigma, no noise, c_in
            d = self._dev[key] = dict(table=self._table.to(device), scale=scale.to(device), state=K.sampler_state(self._s.seed, device),
                                      seed=self._s.seed, row=0, scratch=torch.zeros(1, dtype=torch.int64, device=device))
        return d

    def _point(self, d, row, seed=None):
        seed = d["seed"] if seed is None else int(seed)
        if d["row"] != row or d["seed"] != seed:
            d["state"].copy_(torch.tensor([seed, row], dtype=torch.int64))
            d["row"], d["seed"] = row, seed

    def _row(self, t):
        if self.timesteps is None:
            raise RuntimeError("set_timesteps() first")
        t = int(t.reshape(-1)[0]) if torch.is_tensor(t) else int(t)
        if t not in self._rows:
            raise ValueError(f"timestep {t} is not one of this run's {self.timesteps.tolist()}")
        return self._rows[t]

    def scale_model_input(self, sample, timestep):
        """sample / sqrt(sigma_t^2 + 1), any leading batch (the pipelines hand [2B, ...] when guided)."""
        x = sample.float().contiguous()
        d = self._on(x.device)
        self._point(d, self._row(timestep))
        out = torch.empty_like(x)
        K.euler_step(x, x, d["scale"], d["state"], model_in_next=out)            # x' = x + eps * 0, model_in_next = c_in x' 
        return out.to(sample.dtype)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        x, eps = sample.float().contiguous(), model_output.float().contiguous()
        d = self._on(x.device)
        row = self._row(timestep)
        self._point(d, row, generator.initial_seed() if generator is not None else None)
        prev = K.euler_step(x, eps, d["table"], d["state"]).to(sample.dtype)
        K.sampler_advance(d["state"], d["table"], d["scratch"])            # the next step's row, without a host write
        d["row"] = min(row + 1, self._table.shape[0] - 1)
        return SimpleNamespace(prev_sample=prev) if return_dict else (prev,)

    def add_noise(self, original_samples, noise, timesteps):
        """Sigma space: original + noise * sigma_t (one timestep for the whole batch, as the pipelines call it)."""
        x0 = original_samples.float().contiguous()
        d = self._on(x0.device)
        out = noise.float().contiguous().clone()
        K.sampler_begin(d["state"], d["table"], out, d["scratch"], self._row(timesteps), noise=out, init=x0)
        d["row"] = self._row(timesteps)                                     # hcp_sampler_begin set state[1] to that row
        return out.to(original_samples.dtype)
