"""Pyramid noise and zero-terminal SNR on the native path: the two kernels of csrc/noise.hip against the float64 restatement of
tests/noise_ref.py, that restatement against the reference's own hcpdiff.noise classes, the seam classes of scheduler.py and
NativeTrainer(noise_cfg=...).

Tolerance of the kernel comparison (not fixed in advance): torch's own fp32 path (F.interpolate, *, +=, / std, the add_noise formula:
the reference's arithmetic) runs next to the float64 restatement on the same inputs and its max abs deviation e32 is the yardstick:
|kernel - f64| <= 2 e32 (the factor covers another summation order across the levels) and never above 1e-4 — for the sum left in `noise`, for xt and
for the std scalar alike.  Two routes to one LoRA gradient are compared with the gate
of tests/test_dreamartist.py's trainer test (cosine > 0.9999, norms within 1e-2)."""
import importlib
import os
import random
import sys
import types

import pytest
import torch

import cfg_ref
import noise_ref
from hcp_diffusion_amd import _lib
from hcp_diffusion_amd import kernels as K
from hcp_diffusion_amd import scheduler as S
from hcp_diffusion_amd.trainer import NativeTrainer
from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, seeded_init_

REF = "/root/reference/hcpdiff"
T = 1000
SHAPES = [(1, 4, 8, 8), (2, 4, 12, 20), (3, 4, 64, 64)]
TIMESTEPS = {1: [[0], [T - 1], [437]], 2: [[0, T - 1], [437, 0]], 3: [[0, T - 1, 437]]}
DISCOUNT = 0.9
PAD = 37                      # floats of NaN behind the used part of every field buffer


def level_sets(h, w):
    return {"1x1": [(1, 1)], "identity": [(h, w)], "3x2": [(3, 2)], "three": [(5, 7), (2, 3), (1, 1)], "none": []}


class TorchDDPM:
    """The slice of diffusers' DDPMScheduler the reference's wrappers touch, in torch, at the dtype of its inputs."""

    def __init__(self):
        self.betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)

    def add_noise(self, original_samples, noise, timesteps):
        a = self.alphas_cumprod.to(original_samples.dtype)[timesteps].view(-1, 1, 1, 1)
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise


# ------------------------------------------------------------------------------------------------ shared inputs and references
_DATA, _REFS = {}, {}


def _data(shape):
    """x0, base noise and, per level set, the field buffers (NaN behind the used part) of one shape: made once, never written to."""
    if shape not in _DATA:
        B, C, h, w = shape
        g = torch.Generator().manual_seed(B * 1000 + h * 10 + w)
        fields = {}
        for name, dims in level_sets(h, w).items():
            bufs = []
            for hn, wn in (dims or [(2, 2)]):                  # 'none': one buffer that no level reads — all NaN
                buf = torch.full((B * C * hn * wn + PAD,), float("nan"))
                if dims:
                    buf[:B * C * hn * wn] = torch.randn(B * C * hn * wn, generator=g)
                bufs.append(buf)
            fields[name] = bufs
        _DATA[shape] = dict(x0=torch.randn(shape, generator=g), noise=torch.randn(shape, generator=g), fields=fields,
                            acp=TorchDDPM().alphas_cumprod)
    return _DATA[shape]


def _reference(shape, mode, lname, ts):
    """((xt, sum, std) float64, the same from torch's fp32 path), computed once per case."""
    key = (shape, mode, lname, tuple(ts))
    if key not in _REFS:
        d = _data(shape)
        dims = level_sets(shape[2], shape[3])[lname]
        args = (d["x0"], d["noise"], d["fields"][lname], dims, DISCOUNT, mode, torch.tensor(ts), d["acp"])
        _REFS[key] = (noise_ref.pyramid_add_noise(*args), noise_ref.torch_fp32_path(*args))
    return _REFS[key]


def _run_kernels(backend, shape, mode, lname, ts, d=None):
    """(xt, sum, std) on the backend's device for one case."""
    d = d or _data(shape)
    dims = level_sets(shape[2], shape[3])[lname]
    fields = [backend.to(f) for f in d["fields"][lname]]
    table = torch.zeros(len(fields), 2, dtype=torch.int32)
    for i, hw in enumerate(dims):
        table[i, 0], table[i, 1] = hw
    noise = backend.to(d["noise"].clone())
    part = K.pyramid_noise_accum(noise, fields, backend.to(table), backend.to(torch.tensor([len(dims)], dtype=torch.int32)), DISCOUNT, mode)
    outs = []
    for t in ts:
        xt, std = K.pyramid_noise_finish(backend.to(d["x0"]), noise, backend.to(torch.tensor(t)), backend.to(d["acp"]), part)
        outs.append((xt.cpu(), std.cpu()))
    return outs, noise.cpu(), part.cpu()


def _record(line):
    """The observed (kernel, torch fp32) deviation pairs, printed and, where HCP_NOISE_ACCURACY_OUT names a file, appended to it."""
    print(line)
    path = os.environ.get("HCP_NOISE_ACCURACY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------ 1. the kernels against float64
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64(backend, shape, mode):
    """Every level set (a 1x1 level, the identity resize, 3x2, three levels, no level) with NaN behind the used part of every field
    buffer, timesteps 0 and T - 1 included: the sum left in `noise`, std and xt."""
    B = shape[0]
    worst = [0.0, 0.0, 0.0, 0.0]
    for lname in level_sets(shape[2], shape[3]):
        outs, ksum, _ = _run_kernels(backend, shape, mode, lname, TIMESTEPS[B])
        for ts, (xt, std) in zip(TIMESTEPS[B], outs):
            (xt64, s64, sd64), (xt32, s32, sd32) = _reference(shape, mode, lname, ts)
            what = f"{backend.name} {shape} {mode} levels={lname} t={ts}"
            assert torch.isfinite(ksum).all() and torch.isfinite(xt).all(), what
            k_sum, t_sum = float((ksum.double() - s64).abs().max()), float((s32.double() - s64).abs().max())
            k_xt, t_xt = float((xt.double() - xt64).abs().max()), float((xt32.double() - xt64).abs().max())
            k_sd = abs(float(std) - sd64)
            _record(f"{what}: sum kernel {k_sum:.3e} torch-fp32 {t_sum:.3e} | xt kernel {k_xt:.3e} torch-fp32 {t_xt:.3e} | "
                    f"std kernel {k_sd:.3e} torch-fp32 {abs(sd32 - sd64):.3e}")
            worst = [max(a, b) for a, b in zip(worst, (k_sum, t_sum, k_xt, t_xt))]
            assert k_sum <= 2 * t_sum and k_sum <= 1e-4, what + " sum"
            assert k_xt <= 2 * t_xt and k_xt <= 1e-4, what + " xt"
            assert k_sd <= 2 * abs(sd32 - sd64) and k_sd <= 1e-4, what + " std"
    _record(f"{backend.name} {shape} {mode} WORST: sum kernel {worst[0]:.3e} torch-fp32 {worst[1]:.3e} | xt kernel {worst[2]:.3e} "
            f"torch-fp32 {worst[3]:.3e}")
    d = _data(shape)
    assert all(torch.isnan(f[-PAD:]).all() for fs in d["fields"].values() for f in fs)         # the inputs stayed as they were made


def test_two_calls_give_the_same_bits(backend):
    shape = (3, 4, 64, 64)
    a = _run_kernels(backend, shape, "bilinear", "three", [[0, T - 1, 437]])
    b = _run_kernels(backend, shape, "bilinear", "three", [[0, T - 1, 437]])
    assert torch.equal(a[1], b[1])                                                              # the sum
    n_parts = 2 * 16 * 3                                                                        # 16 pixel blocks x 3 plane groups
    assert torch.equal(a[2][:n_parts], b[2][:n_parts]) and a[2][:n_parts].abs().sum() > 0       # the ordered partials
    assert torch.equal(a[0][0][1], b[0][0][1]) and torch.equal(a[0][0][0], b[0][0][0])          # std, xt


def test_kernels_refuse_bad_arguments(backend):
    d = _data((1, 4, 8, 8))
    noise, f = backend.to(d["noise"].clone()), [backend.to(d["fields"]["3x2"][0])]
    dims, n = backend.to(torch.tensor([[3, 2]], dtype=torch.int32)), backend.to(torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError, match="'bilinear' or 'nearest'"):
        K.pyramid_noise_accum(noise, f, dims, n, DISCOUNT, "bicubic")
    with pytest.raises(_lib.HcpError, match="resize mode 2"):
        K.pyramid_noise_accum(noise, f, dims, n, DISCOUNT, 2)
    with pytest.raises(AssertionError):
        K.pyramid_noise_accum(noise, f * (K.PYRAMID_MAX_LEVELS + 1), dims, n, DISCOUNT)
    with pytest.raises(AssertionError):
        K.pyramid_noise_accum(noise.double(), f, dims, n, DISCOUNT)
    assert torch.equal(noise.cpu(), d["noise"])                                                 # nothing ran


def test_a_size_table_the_buffers_cannot_serve_reads_nothing():
    """Interpreter only: sizes larger than the field buffer, a size of 0, a level count outside [0, n_max] — the guard in front of the
    loads leaves NaN in the result instead of reading past a buffer."""
    from conftest import emu_cdll
    K._set_backend_for_tests(emu_cdll())
    try:
        d = _data((1, 4, 8, 8))
        f = [d["fields"]["3x2"][0].clone()]
        for dims, n in ([[1000, 1000]], 1), ([[0, 2]], 1), ([[3, 2]], 2), ([[3, 2]], -1):
            noise = d["noise"].clone()
            part = K.pyramid_noise_accum(noise, f, torch.tensor(dims, dtype=torch.int32), torch.tensor([n], dtype=torch.int32), DISCOUNT)
            assert torch.isnan(noise).all(), (dims, n)
            xt, std = K.pyramid_noise_finish(d["x0"], noise, torch.tensor([5]), d["acp"], part)
            assert torch.isnan(xt).all() and torch.isnan(std).all()
    finally:
        K._set_backend_for_tests(None)


# ------------------------------------------------------------------------------------------------ 2. pinned to the reference
def _load_reference_noise(monkeypatch):
    """hcpdiff/noise as a package of its own (its files import only torch, random and diffusers' SchedulerMixin, for which a stand-in
    module serves where diffusers is absent — or is itself a bare stand-in that another test's loader left in sys.modules, without
    that name: whichever test ran before in this process must not decide)."""
    try:
        from diffusers import SchedulerMixin  # noqa: F401
    except ImportError:
        stub = types.ModuleType("diffusers")
        stub.__path__ = []
        stub.__dict__.update({k: v for k, v in vars(sys.modules.get("diffusers", stub)).items() if not k.startswith("__")})
        stub.SchedulerMixin = type("SchedulerMixin", (), {})
        monkeypatch.setitem(sys.modules, "diffusers", stub)            # (for this test only: put back at teardown)
    pkg = types.ModuleType("_ref_noise")
    pkg.__path__ = [os.path.join(REF, "noise")]
    monkeypatch.setitem(sys.modules, "_ref_noise", pkg)
    for sub in ("noise_base", "pyramid_noise", "zero_terminal"):                # (registered with monkeypatch: gone again at teardown)
        monkeypatch.setitem(sys.modules, f"_ref_noise.{sub}", pkg)
        del sys.modules[f"_ref_noise.{sub}"]
    pyr = importlib.import_module("_ref_noise.pyramid_noise")
    zt = importlib.import_module("_ref_noise.zero_terminal")
    return pyr.PyramidNoiseScheduler, zt.ZeroTerminalScheduler


DRAWS = [0.05, 0.1, 0.3, 0.61, 0.12, 0.77, 0.5, 0.2, 0.99]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_restatement_equals_the_reference(monkeypatch, mode):
    """noise_ref.pyramid_add_noise == PyramidNoiseScheduler.add_noise in float64 with random.random and torch.randn replaced by the
    test's draws: the returned xt, and the caller's `noise` tensor, which the reference leaves holding the UNNORMALISED sum.  The host
    loop of scheduler.pyramid_level_dims draws the same sizes from the same random.random values."""
    Pyramid, _ = _load_reference_noise(monkeypatch)
    B, C, h, w = 2, 4, 24, 40
    g = torch.Generator().manual_seed(3)
    x0, noise0 = torch.randn(B, C, h, w, generator=g, dtype=torch.float64), torch.randn(B, C, h, w, generator=g, dtype=torch.float64)
    t = torch.tensor([T - 1, 437])
    real_randn = torch.randn
    drawn = []

    def fake_randn(*shape, **kw):
        drawn.append(real_randn(*shape, generator=g, dtype=torch.float64))
        return drawn[-1]
    it = iter(DRAWS)
    monkeypatch.setattr(random, "random", lambda: next(it))
    monkeypatch.setattr(torch, "randn", fake_randn)
    noise = noise0.clone()
    sched = Pyramid(TorchDDPM(), level=10, discount=DISCOUNT, step_size=2.0, resize_mode=mode)
    xt_ref = sched.add_noise(x0, noise, t)
    monkeypatch.setattr(torch, "randn", real_randn)
    dims = [tuple(f.shape[2:]) for f in drawn]
    assert len(dims) >= 3 and (dims[-1][0] == 1 or dims[-1][1] == 1)
    it = iter(DRAWS)
    assert S.pyramid_level_dims(h, w, 10, 2.0) == dims
    bounds = S.pyramid_level_bounds(h, w, 10, 2.0)
    assert len(bounds) >= len(dims) and all(d[0] <= b[0] and d[1] <= b[1] for d, b in zip(dims, bounds))
    xt64, s64, sd64 = noise_ref.pyramid_add_noise(x0, noise0, drawn, dims, DISCOUNT, mode, t, TorchDDPM().alphas_cumprod)
    assert float((noise - s64).abs().max()) <= 1e-13 * float(s64.abs().max())           # the quirk: the sum, not sum / std
    assert abs(float(noise.std()) - sd64) <= 1e-13 * sd64 and abs(sd64 - 1.0) > 0.05
    assert float((xt_ref - xt64).abs().max()) <= 1e-13 * float(xt64.abs().max())


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
def test_zero_terminal_table_equals_the_reference_bits(monkeypatch):
    _, ZeroTerminal = _load_reference_noise(monkeypatch)
    base = TorchDDPM()
    ZeroTerminal(base)
    nat = S.NativeZeroTerminalScheduler(S.NativeDDPMScheduler())
    for name in ("betas", "alphas", "alphas_cumprod"):
        assert torch.equal(getattr(base, name), getattr(nat, name)), name
    assert nat.alphas_cumprod[-1].item() == 0.0 and nat.alphas_cumprod[0].item() == TorchDDPM().alphas_cumprod[0].item()
    b64, a64, acp64 = noise_ref.zero_terminal_table(TorchDDPM().betas)
    assert acp64[-1].item() == 0.0
    assert float((nat.alphas_cumprod.double() - acp64).abs().max()) <= 1e-6             # (fp32 cumprod of 1000 factors)


# ------------------------------------------------------------------------------------------------ 3. the seam classes
def test_seam_wrappers_delegate_compose_and_keep_dtype(backend, monkeypatch):
    dev = backend.device
    base = S.NativeDDPMScheduler()
    plain_table = base.alphas_cumprod.clone()
    pyr = S.NativePyramidNoiseScheduler(base, level=6, discount=0.8)
    assert pyr.config.num_train_timesteps == 1000 and pyr.level == 6 and pyr.base_scheduler is base
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(2, 4, 12, 20, generator=g).to(dev).to(torch.bfloat16)
    noise = torch.randn(2, 4, 12, 20, generator=g).to(dev).to(torch.bfloat16)
    t = torch.tensor([3, T - 1]).to(dev)
    want = base.add_noise(x0, noise, t)
    n0 = noise.clone()
    random.seed(4)
    got = pyr.add_noise(x0, noise, t)
    assert got.dtype == want.dtype == torch.bfloat16 and got.shape == want.shape and got.device == want.device
    assert not torch.equal(noise, n0) and torch.isfinite(got.float()).all()             # the caller's tensor now holds the sum
    # injected fields, fp32: the class is the two kernels on the host loop's sizes
    random.seed(4)
    dims = S.pyramid_level_dims(12, 20, 6, 2.0)
    fields = [torch.randn(2, 4, hn, wn, generator=g) for hn, wn in dims]
    x32, n32 = x0.float(), n0.float().clone()
    random.seed(4)
    xt = pyr.add_noise(x32, n32, t, fields=[backend.to(f) for f in fields])
    xt64, s64, _ = noise_ref.pyramid_add_noise(x32.cpu(), n0.float().cpu(), fields, dims, 0.8, "bilinear", t.cpu(), plain_table)
    assert float((n32.cpu().double() - s64).abs().max()) <= 1e-5 and float((xt.cpu().double() - xt64).abs().max()) <= 1e-5
    # composition in either order reaches the scheduler that owns the table
    a = S.NativeZeroTerminalScheduler(S.NativePyramidNoiseScheduler(S.NativeDDPMScheduler(), level=6, discount=0.8))
    b = S.NativePyramidNoiseScheduler(S.NativeZeroTerminalScheduler(S.NativeDDPMScheduler()), level=6, discount=0.8)
    assert torch.equal(a.alphas_cumprod, b.alphas_cumprod) and a.alphas_cumprod[-1].item() == 0.0
    assert torch.equal(a.base_scheduler.base_scheduler.alphas_cumprod, a.alphas_cumprod) and not torch.equal(a.alphas_cumprod, plain_table)
    for sched in (a, b):
        random.seed(4)
        n = n0.float().clone()
        out = sched.add_noise(x32, n, torch.tensor([T - 1, T - 1]).to(dev), fields=[backend.to(f) for f in fields])
        assert float((out.cpu().double() - s64 / noise_ref.std_unbiased(s64)).abs().max()) <= 1e-5     # acp[T - 1] = 0: pure noise
    with pytest.raises(ValueError, match="resize_mode"):
        S.NativePyramidNoiseScheduler(base, resize_mode="bicubic")
    with pytest.raises(ValueError, match="level"):
        S.NativePyramidNoiseScheduler(base, level=40)


# ------------------------------------------------------------------------------------------------ 4. the trainer
PATS_A, PATS_F = [r"re:.*\.attn.?$"], [r"re:.*\.ff$"]
PYR = dict(type="pyramid", level=10, discount=0.9, step_size=2.0, resize_mode="bilinear")


def _native(dev):
    torch.manual_seed(0)
    ora = seeded_init_(OracleUNet2DConditionModel(**MICRO_CONFIG), 1)
    nat = NativeUNet2DConditionModel(**MICRO_CONFIG)
    nat.load_state_dict(ora.state_dict())
    return nat.to(dev)


def _trainer(dev, lora_cfg=None, **kw):
    """As tests/test_trainer.py builds it: MICRO_CONFIG UNet, rank-4 LoRA on attention + feed-forward, seeded non-zero W_up."""
    tr = NativeTrainer(_native(dev), lora_cfg or [dict(layers=PATS_A + PATS_F, rank=4)], lr=kw.pop("lr", 1e-2), **kw)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for blk in tr.bucket.blocks:
            blk.layer.W_up.copy_((torch.randn(blk.layer.W_up.shape, generator=g) * 0.05).to(dev))
    tr.bucket.pack()
    return tr


def _batch(dev, seed=1, B=2, L=24, rows=None, hw=(8, 8)):
    g = torch.Generator().manual_seed(seed)
    return dict(latents=torch.randn(B, 4, *hw, generator=g).to(dev),
                encoder_hidden_states=torch.randn(B if rows is None else rows, L, 32, generator=g).to(dev))


def _one_wave_mask(dev, hw=(8, 8)):
    """The first 64 elements of the first channel: hcp_mse_masked_mean meets in an fp32 atomic per wave, and with a single non-zero wave
    sum the loss does not depend on the order of arrival — 'the same bits' is then a property of the code, not of a run."""
    mask = torch.zeros(2, 4, *hw)
    mask[0, 0].view(-1)[:64] = 1.0
    return mask.to(dev)


def test_no_noise_cfg_is_the_present_step_bit_for_bit(backend):
    """noise_cfg None: loss and bucket gradient carry the bits of a trainer built without the argument, and of the parent's make_noise —
    one randn_like, one randint, K.add_noise on the scaled-linear table — written out here."""
    dev = backend.device
    b, mask = _batch(dev), _one_wave_mask(dev)
    got = []
    for kw in ({}, dict(noise_cfg=None), "parent"):
        tr = _trainer(dev, **({} if kw == "parent" else kw))
        assert tr.noise_pyramid is None and not tr.noise_zero_terminal
        assert torch.equal(tr.acp.cpu(), TorchDDPM().alphas_cumprod)
        torch.manual_seed(77)
        if kw == "parent":
            noise = torch.randn_like(b["latents"])
            t = torch.randint(0, 1000, (2,), device=dev).long()
            tr.make_noise = lambda lat: (K.add_noise(lat, noise, t, tr.acp), noise, t)
        loss = tr.forward_backward(b["latents"], b["encoder_hidden_states"], mask=mask)
        got.append((loss.cpu().clone(), tr.bucket.grads.cpu().clone()))
    assert got[0][1].abs().max() > 0
    for loss, grads in got[1:]:
        assert torch.equal(loss, got[0][0]) and torch.equal(grads, got[0][1])


def test_trainer_pyramid_step_vs_float64_noise(backend, monkeypatch):
    """Pyramid noise with injected field draws: the noisy latents and the eps target of the step are the float64 restatement's — the
    target handed to the loss is the UNNORMALISED sum —, and loss and LoRA bucket gradient are those of an identically built plain
    trainer fed the restatement's noisy latents and target."""
    dev = backend.device
    b = _batch(dev)
    B, C, h, w = b["latents"].shape
    tr = _trainer(dev, noise_cfg=PYR)
    bounds = S.pyramid_level_bounds(h, w, 10, 2.0)
    assert bounds == [(4, 4), (2, 2), (1, 1)]
    g = torch.Generator().manual_seed(21)
    fields = [torch.randn(B * C * hn * wn, generator=g) for hn, wn in bounds]          # drawn at the upper bounds, as the step draws them
    tr._pyramid.draw_fields = lambda shape, device: [f.to(device) for f in fields]
    tr.optimizer_step = lambda *a, **k: None                                            # (keeps the bucket gradients)
    seen, targets = [], []
    real_make, real_mse = tr.make_noise, K.mse_masked_mean
    tr.make_noise = lambda lat: (seen.append(real_make(lat)), seen[-1])[1]
    monkeypatch.setattr(K, "mse_masked_mean", lambda pred, target, *a, **k: (targets.append(target), real_mse(pred, target, *a, **k))[1])
    preds = []
    tr.unet.register_forward_hook(lambda m, a, out: preds.append(out.sample.detach().cpu().clone()))
    random.seed(8)
    torch.manual_seed(31)
    loss = tr.train_data_list([dict(b)])
    # the step's draws again: level sizes from the host module, base noise and timesteps from torch's generator
    random.seed(8)
    dims = S.pyramid_level_dims(h, w, 10, 2.0)
    torch.manual_seed(31)
    n0 = torch.randn_like(b["latents"])
    t = torch.randint(0, 1000, (B,), device=dev).long()
    assert 1 <= len(dims) <= len(bounds) and int(tr._pyramid.tables[0][0]) == len(dims)
    assert tr._pyramid.tables[0][1:1 + 2 * len(dims)].cpu().tolist() == [v for d in dims for v in d]
    noisy, noise, t_step = seen[0]
    assert torch.equal(t_step, t) and targets[0] is noise
    xt64, s64, sd64 = noise_ref.pyramid_add_noise(b["latents"].cpu(), n0.cpu(), fields, dims, 0.9, "bilinear", t.cpu(), tr.acp.cpu())
    assert float((noise.cpu().double() - s64).abs().max()) <= 1e-5 and float((noisy.cpu().double() - xt64).abs().max()) <= 1e-5
    assert abs(float(noise.std()) - sd64) <= 1e-5 * sd64 and abs(sd64 - 1.0) > 0.05    # not normalised: the target is the sum
    # the returned loss is the plain MSE of the captured prediction against that target, under the gate of test_dreamartist.py's trainer test
    l64, _ = cfg_ref.mse_loss(preds[0].double(), noise.cpu())
    l32, _ = cfg_ref.mse_loss(preds[0], noise.cpu())
    cfg_ref.within(loss, l64, l32, "pyramid step loss")
    # the other route: the restatement's tensors through the same UNet
    monkeypatch.setattr(K, "mse_masked_mean", real_mse)
    tr2 = _trainer(dev)
    tr2.make_noise = lambda lat: (xt64.float().to(dev), s64.float().to(dev), t)
    tr2.optimizer_step = lambda *a, **k: None
    loss2 = tr2.train_data_list([dict(b)])
    g1, g2 = tr.bucket.grads, tr2.bucket.grads
    assert g1.abs().max().item() > 0 and abs(loss.item() / loss2.item() - 1) < 1e-2
    assert torch.nn.functional.cosine_similarity(g1, g2, dim=0).item() > 0.9999 and abs(g1.norm().item() / g2.norm().item() - 1) < 1e-2


def test_accumulation_ema_lion_two_datasets_and_cfg_run_under_it(backend):
    dev = backend.device
    tr = _trainer(dev, noise_cfg=dict(PYR, zero_terminal=True, resize_mode="nearest"), ema=dict(decay_max=0.99), optimizer=dict(type="lion"),
                  lr=1e-3, gradient_accumulation_steps=2)
    assert tr.acp[-1].item() == 0.0
    p0 = tr.bucket.params.clone()
    data = [_batch(dev, 1), dict(_batch(dev, 2), loss_weight=0.5)]
    random.seed(1)
    loss = tr.train_data_list(data)
    assert torch.isfinite(loss).all() and torch.equal(tr.bucket.params, p0) and tr.bucket.grads.abs().max().item() > 0
    assert sorted(tr._pyramid.tables) == [0, 1]
    loss = tr.train_data_list(data)
    assert torch.isfinite(loss).all() and not torch.equal(tr.bucket.params, p0) and tr.bucket.grads.abs().max().item() == 0.0
    assert not torch.equal(tr._lora_state.ema, p0)
    # under an active cfg_scale (DreamArtist): the noise is made before the repeat; zero terminal SNR combines with it too
    trc = _trainer(dev, noise_cfg=dict(PYR, zero_terminal=True), cfg_scale="1.0-3.0:cos")
    bc = _batch(dev, 3, rows=4)
    loss = trc.train_one_step(bc["latents"], bc["encoder_hidden_states"])
    assert torch.isfinite(loss).all()
    # forward_backward on its own draws its sizes itself
    random.seed(2)
    before = random.getstate()
    trc.forward_backward(bc["latents"], bc["encoder_hidden_states"])
    assert random.getstate() != before


def test_refusals(backend):
    dev = backend.device
    with pytest.raises(ValueError, match="zero_terminal with loss_type='sample'"):
        _trainer(dev, noise_cfg=dict(zero_terminal=True), loss_type="sample")
    for kind in ("min_snr", "soft_min_snr", "kdiff_min_snr", "edm"):
        with pytest.raises(ValueError, match="SNR-weighted"):
            _trainer(dev, noise_cfg=dict(PYR, zero_terminal=True), loss_cfg=dict(type=kind, gamma=5.0))
    _trainer(dev, noise_cfg=dict(zero_terminal=True), loss_cfg=dict(type="mse"))
    _trainer(dev, noise_cfg=PYR, loss_type="sample", loss_cfg=dict(type="min_snr", gamma=5.0))     # pyramid alone divides by nothing new
    with pytest.raises(ValueError, match="'pyramid'"):
        _trainer(dev, noise_cfg=dict(type="perlin"))
    with pytest.raises(ValueError, match="resize_mode"):
        _trainer(dev, noise_cfg=dict(PYR, resize_mode="bicubic"))
    with pytest.raises(ValueError, match="level"):
        _trainer(dev, noise_cfg=dict(PYR, level=18))
    with pytest.raises(ValueError, match="step_size"):
        _trainer(dev, noise_cfg=dict(PYR, step_size=0.0))
    with pytest.raises(ValueError, match="takes no"):
        _trainer(dev, noise_cfg=dict(PYR, octaves=3))
    with pytest.raises(ValueError, match="without type='pyramid'"):
        _trainer(dev, noise_cfg=dict(zero_terminal=True, level=4))


def test_warm_up_restore_puts_back_the_host_random_state(backend):
    """What a capture's warm-up runs between _snapshot and _restore draws level sizes from the global `random` module: its state is part
    of what is put back."""
    tr = _trainer(backend.device, noise_cfg=PYR)
    random.seed(5)
    state = random.getstate()
    saved = tr._snapshot()
    tr._pyramid.draw_levels([_batch(backend.device)])
    assert random.getstate() != state
    tr._restore(saved)
    assert random.getstate() == state


# ------------------------------------------------------------------------------------------------ 5. the captured step (GPU)
GRAPH_SEED, GRAPH_STEPS = 3, 6


GRAPH_HW = (16, 16)             # (at 8 x 8 every draw has two levels: int(8 / r**2) is 1 for every r in (2, 4))


def _level_counts(seed, steps, h=16, w=16):
    random.seed(seed)
    return [len(S.pyramid_level_dims(h, w, 10, 2.0)) for _ in range(steps)]


def test_the_graph_test_seed_draws_more_than_one_level_count():
    assert len(set(_level_counts(GRAPH_SEED, GRAPH_STEPS))) >= 2


@pytest.mark.gpu
def test_graph_pyramid_step_equals_eager():
    """use_graph=True against eager, six steps from the same host and torch seeds, Lion (ordered norm) and a one-wave mask (ordered loss):
    every loss and the final LoRA parameters carry the same bits, with at least two different level counts among the steps — a level
    table frozen at capture, or host draws the warm-up did not put back, fail here."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    K._set_backend_for_tests(None)
    dev = torch.device("cuda:0")
    b, mask = _batch(dev, hw=GRAPH_HW), _one_wave_mask(dev, GRAPH_HW)
    counts = _level_counts(GRAPH_SEED, GRAPH_STEPS)
    assert len(set(counts)) >= 2
    res = []
    for use_graph in (False, True):
        tr = _trainer(dev, [dict(layers=PATS_A + PATS_F, rank=4, dropout=0.0)], use_graph=use_graph, noise_cfg=PYR, optimizer=dict(type="lion"),
                      lr=1e-3)
        random.seed(GRAPH_SEED)
        torch.manual_seed(123); torch.cuda.manual_seed(123)
        losses, seen = [], []
        for step in range(GRAPH_STEPS):
            losses.append(tr.train_one_step(b["latents"], b["encoder_hidden_states"], mask=mask).clone())
            seen.append(int(tr._pyramid.tables[0][0]))
        torch.cuda.synchronize()
        assert seen == counts
        if use_graph:
            assert len(tr._graph_cache) == 1
        res.append((losses, tr.bucket.params.clone(), random.random()))
    (le, pe, re_), (lg, pg, rg) = res
    assert re_ == rg                                                                    # same position in the host random stream
    assert all(torch.isfinite(l).all() and l.item() > 0 for l in le) and len({l.item() for l in le}) == GRAPH_STEPS
    for a, b_ in zip(le, lg):
        assert torch.equal(a, b_)
    assert torch.equal(pe, pg)
