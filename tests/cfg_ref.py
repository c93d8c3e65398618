"""Restatement of the DreamArtist loss (reference hcpdiff/models/cfg_context.py:12-39 DreamArtistPTContext.pre / post followed by
train_ac.py:506-515 ``(MSELoss(reduction='none')(e, target) * mask).mean()``) in whatever dtype the prediction carries: float64 is the
oracle of tests/test_dreamartist.py, float32 the yardstick of fp32 rounding.  The gradient is the closed form of the issue, pinned to
the reference's autograd in that file.  Nothing here reads outside the repository."""
import math

import torch


def ulp32(x):
    x = float(x)
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


def scale_per_sample(t, cfg, num_train_timesteps, dtype, B):
    """s_b = (hi - lo) rate_b + lo (cfg_context.py:25-38); rate is 1 and unused with a fixed scale."""
    lo, hi, kind = cfg
    if lo == hi:
        return torch.full((B,), hi, dtype=dtype)
    rate = t.to(dtype) / (num_train_timesteps - 1)
    if kind == "cos":
        rate = torch.cos((rate - 1) * math.pi / 2)
    elif kind == "cos2":
        rate = 1 - torch.cos(rate * math.pi / 2)
    elif kind != "ln":
        raise ValueError(kind)
    return (hi - lo) * rate + lo


def weights(target, mask, sample_weight):
    """mask (1 or C channels) times sample_weight[b], broadcast to target's shape and dtype."""
    w = torch.ones_like(target)
    if mask is not None:
        w = w * mask.to(target.dtype)
    if sample_weight is not None:
        w = w * sample_weight.to(target.dtype).view(-1, *([1] * (target.dim() - 1)))
    return w


def cfg_loss(pred2, target, t, cfg, num_train_timesteps=1000, mask=None, sample_weight=None, weight=1.0):
    """(loss, grad2) in pred2's dtype.  pred2 [2B, ...]: negative rows first; target [B, ...]."""
    B = target.shape[0]
    u, c = pred2.chunk(2)
    target = target.to(pred2.dtype)
    s = scale_per_sample(t, cfg, num_train_timesteps, pred2.dtype, B).view(-1, *([1] * (target.dim() - 1)))
    e = u + s * (c - u)
    w = weights(target, mask, sample_weight)
    loss = ((e - target) ** 2 * w).mean() * weight
    g = 2 * weight / target.numel() * (e - target) * w
    return loss, torch.cat([(1 - s) * g, s * g])


def mse_loss(pred, target, mask=None, sample_weight=None, weight=1.0):
    """The plain masked MSE of K.mse_masked_mean: (loss, grad)."""
    target = target.to(pred.dtype)
    w = weights(target, mask, sample_weight)
    return ((pred - target) ** 2 * w).mean() * weight, 2 * weight / target.numel() * (pred - target) * w


def within(got, want64, got32, what=""):
    """The gate of tests/test_optim_family.py: |got - f64| <= 4 e32 + ulp32(max|x|), e32 = the fp32 restatement's own max error."""
    want64 = torch.as_tensor(want64, dtype=torch.float64).reshape(-1)
    e32 = float((torch.as_tensor(got32).double().reshape(-1) - want64).abs().max())
    err = float((torch.as_tensor(got).detach().cpu().double().reshape(-1) - want64).abs().max())
    bound = 4 * e32 + ulp32(want64.abs().max())
    print(f"{what}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{what}: err {err:.3e} > 4 * e32 ({e32:.3e}) + ulp32 = {bound:.3e}"
