"""Restatements of the two optimizer rules the fused kernels implement, in whatever dtype the tensors carry (float64: the oracle;
float32: the yardstick of fp32 rounding, and what is pinned bit for bit against the installed transformers class).

adafactor_step is transformers.optimization.Adafactor.step for one tensor (same operations in the same order); lion_step is
lion_pytorch.Lion's update_fn.  Nothing here reads outside the repository."""
import math

import torch


def adafactor_step(p, g, st, *, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                   scale_parameter=True, relative_step=True, warmup_init=False):
    """One step on tensor p with gradient g; st: the per-parameter state dict of the installed class ({} before the first step)."""
    factored = g.dim() >= 2
    if not st:
        st["step"] = 0
        if beta1 is not None:
            st["exp_avg"] = torch.zeros_like(g)
        if factored:
            st["exp_avg_sq_row"] = torch.zeros(g.shape[:-1]).to(g)
            st["exp_avg_sq_col"] = torch.zeros(g.shape[:-2] + g.shape[-1:]).to(g)
        else:
            st["exp_avg_sq"] = torch.zeros_like(g)
    st["step"] += 1
    st["RMS"] = p.norm(2) / (p.numel() ** 0.5)
    rel = lr
    if relative_step:
        rel = min(1e-6 * st["step"] if warmup_init else 1e-2, 1.0 / math.sqrt(st["step"]))
    lr_t = (max(eps[1], st["RMS"]) if scale_parameter else 1.0) * rel
    beta2t = 1.0 - math.pow(st["step"], decay_rate)
    update = (g ** 2) + eps[0]
    if factored:
        row, col = st["exp_avg_sq_row"], st["exp_avg_sq_col"]
        row.mul_(beta2t).add_(update.mean(dim=-1), alpha=(1.0 - beta2t))
        col.mul_(beta2t).add_(update.mean(dim=-2), alpha=(1.0 - beta2t))
        r_factor = (row / row.mean(dim=-1, keepdim=True)).rsqrt_().unsqueeze(-1)
        update = torch.mul(r_factor, col.unsqueeze(-2).rsqrt()).mul_(g)
    else:
        st["exp_avg_sq"].mul_(beta2t).add_(update, alpha=(1.0 - beta2t))
        update = st["exp_avg_sq"].rsqrt().mul_(g)
    update.div_(((update.norm(2) / (update.numel() ** 0.5)) / clip_threshold).clamp_(min=1.0))
    update.mul_(lr_t)
    if beta1 is not None:
        st["exp_avg"].mul_(beta1).add_(update, alpha=(1 - beta1))
        update = st["exp_avg"]
    if weight_decay != 0:
        p.add_(p, alpha=(-weight_decay * lr_t))
    p.add_(-update)


def lion_step(p, g, m, lr, beta1=0.9, beta2=0.99, weight_decay=0.0):
    """Returns the sign argument (the rule is discontinuous where it is ~0)."""
    p.mul_(1 - lr * weight_decay)
    arg = m * beta1 + g * (1 - beta1)
    p.add_(arg.sign(), alpha=-lr)
    m.mul_(beta2).add_(g, alpha=1 - beta2)
    return arg


def clip_factor(gs, grad_scale, max_norm):
    """The kernels' shared prologue in float64: g * grad_scale, then the global-norm clip over all of gs."""
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs)) * grad_scale
    c = max_norm / (norm + 1e-6)
    return grad_scale * min(c, 1.0)


def clip_factor32(gs, grad_scale, max_norm):
    """The same prologue as an fp32 program (sum of squares, sqrt, divide: each rounds): the factor the fp32 yardstick runs with."""
    ss = torch.zeros((), dtype=torch.float32)
    for g in gs:
        ss = ss + (g.float() * g.float()).sum()
    norm = ss.sqrt() * torch.tensor(grad_scale, dtype=torch.float32)
    c = torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
    return torch.tensor(grad_scale, dtype=torch.float32) * torch.clamp(c, max=1.0)
