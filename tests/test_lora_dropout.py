"""Native LoRA dropout (csrc/dropout.hip, dropout.py, lora.LoraHipContainer._dropped): the counter-based mask against a numpy
restatement of Philox4x32-10, the values and gradients against float64, the bookkeeping of the per-module state tensor, capture, the
trainer switch and the ABI.

Tolerances.  A kept element is bf16(y * scale (+ residual)) from fp32 arithmetic: one bf16 rounding (2^-9 relative to the result) plus the
fp32 roundings of the scale, the product and the sum (each 2^-24 relative to its operands) — asserted as 2^-8 |exact| + 2^-22 (|y scale| +
|residual|), which is 2^-8 relative wherever the sum does not cancel.  Dropped elements are exact.  Layer outputs and gradients of W_down /
W_up / the input use the gates of the LoRA layer tests in tests/test_model.py for the same quantities (max abs error / max abs value
< 2e-2; 3e-2 for the factors of the DAPP and merged forms)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from hcp_diffusion_amd import _lib
from hcp_diffusion_amd import kernels as K
from hcp_diffusion_amd import ops
from hcp_diffusion_amd.dropout import NativeDropoutMixin
from hcp_diffusion_amd.lora import DAPPHipLayer, LoraHipLayer, make_lora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the restatement
def philox4x32_10(c, k):
    """c: four, k: two arrays (or ints) of 32-bit values -> four uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in c)
    k0, k1 = (np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in k)
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def threshold(p):
    return 65536 if p >= 1 else int(round(p * 65536))


def scale_of(p):
    t = threshold(p)
    return 0.0 if t >= 65536 else 1.0 / (1.0 - t / 65536.0)


def keep_mask(n, seed, calls, layer_id, group_base, p):
    """bool [n]: element i is kept.  Group g = i // 8 draws one Philox block; element 8g + 2j takes the low half of word j, 8g + 2j + 1 the
    high half; keep iff that 16-bit value >= round(p * 65536)."""
    groups = n // 8
    ctr = [(group_base + g) % (1 << 64) for g in (0, groups - 1)]
    assert ctr[1] - ctr[0] == groups - 1                             # (no wrap of the 64-bit counter inside a test's range)
    g = np.uint64(ctr[0]) + np.arange(groups, dtype=np.uint64)
    s = seed % (1 << 64)
    w = philox4x32_10((g & M32, g >> np.uint64(32), layer_id, calls % (1 << 32)), (s & 0xFFFFFFFF, s >> 32))
    lanes = np.empty((groups, 8), dtype=np.uint64)
    for j in range(4):
        lanes[:, 2 * j] = w[j] & np.uint64(0xFFFF)
        lanes[:, 2 * j + 1] = w[j] >> np.uint64(16)
    return (lanes >= np.uint64(threshold(p))).reshape(-1)


def _state(dev, seed, calls):
    return torch.tensor([seed, calls], dtype=torch.int64).to(dev)


def test_restatement_known_answers():
    hexs = lambda w: " ".join(f"{int(v[0]):08x}" for v in w)
    assert hexs(philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert hexs(philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexs(philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


# ------------------------------------------------------------------------------------------------ the mask
SEEDS = [1234, (1 << 32) + 77, -987654321012345]
BASES = [0, 15, (1 << 32) + 3]
CALLS = [0, 1, (1 << 32) + 1]


def _kernel_mask(dev, n, seed, calls, layer_id, group_base, p):
    out = K.dropout_residual_fwd(torch.ones(n, dtype=BF16, device=dev), None, _state(dev, seed, calls), layer_id, group_base, p)
    return (out.float().cpu().numpy() != 0)


@pytest.mark.parametrize("shape", [(8,), (3, 40), (5, 320), (2, 1280)], ids=lambda s: "x".join(map(str, s)))
def test_mask_is_the_restatement_bit_for_bit(backend, shape):
    dev = backend.device
    n = math.prod(shape)
    seen = {}
    for seed in SEEDS:
        for gb in BASES:
            for lid in (0, 7):
                for calls in CALLS:
                    for p in (0.1, 0.5, 1.0):
                        got = _kernel_mask(dev, n, seed, calls, lid, gb, p)
                        assert np.array_equal(got, keep_mask(n, seed, calls, lid, gb, p)), (seed, gb, lid, calls, p)
                        seen[(seed, gb, lid, calls, p)] = got
    for seed in SEEDS:
        for gb in BASES:
            for lid in (0, 7):
                for p in (0.1, 0.5, 1.0):
                    assert np.array_equal(seen[(seed, gb, lid, 1, p)], seen[(seed, gb, lid, (1 << 32) + 1, p)])     # calls enters with 32 bits (documented wrap)
    if n >= 120:                                          # neighbouring calls / layer_id / group_base: another mask (n = 8 at p = 0.5 can collide by chance)
        s = SEEDS[0]
        base = _kernel_mask(dev, n, s, 5, 3, 9, 0.5)
        for other in ((s, 6, 3, 9), (s, 5, 4, 9), (s, 5, 3, 10)):
            assert not np.array_equal(base, _kernel_mask(dev, n, *other, 0.5)), other
    assert not seen[(SEEDS[0], 0, 0, 0, 1.0)].any()


def test_mask_when_the_grid_stride_loop_turns_over(backend):
    """More groups than the largest launch has threads (kernels.DROPOUT_MAX_THREADS = drop_grid's 2048 blocks x 256): the first 261
    threads of the grid take a second trip."""
    groups = K.DROPOUT_MAX_THREADS + 261
    n = 8 * groups
    got = _kernel_mask(backend.device, n, SEEDS[1], 1, 7, BASES[2], 0.1)
    assert np.array_equal(got, keep_mask(n, SEEDS[1], 1, 7, BASES[2], 0.1))


# ------------------------------------------------------------------------------------------------ values
def _bound(exact, ys, res):
    return 2.0 ** -8 * np.abs(exact) + 2.0 ** -22 * (np.abs(ys) + np.abs(res))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_values_forward_and_backward_vs_float64(backend, with_res, inplace, p):
    dev = backend.device
    g = torch.Generator().manual_seed(3)
    shape, seed, calls, lid, gb = (5, 320), 99, 4, 2, 15
    n = math.prod(shape)
    y = torch.randn(shape, generator=g).to(BF16)
    res = torch.randn(shape, generator=g).to(BF16) if with_res else None
    dy = torch.randn(shape, generator=g).to(BF16)
    keep = keep_mask(n, seed, calls, lid, gb, p).reshape(shape)
    sc = scale_of(p)
    st = _state(dev, seed, calls)
    yd = backend.to(y.clone())
    out = K.dropout_residual_fwd(yd, None if res is None else backend.to(res), st, lid, gb, p, out=yd if inplace else None)
    assert (out.data_ptr() == yd.data_ptr()) == inplace
    o = out.float().cpu().numpy().astype(np.float64)
    y64, r64 = y.double().numpy(), (res.double().numpy() if with_res else np.zeros(shape))
    exact = np.where(keep, y64 * sc, 0.0) + r64
    assert np.array_equal(o[~keep], r64[~keep])                       # dropped: exactly 0 (+ residual)
    assert (np.abs(o - exact) <= _bound(exact, y64 * sc, r64))[keep].all()
    dd = backend.to(dy.clone())
    dx = K.dropout_bwd(dd, st, lid, gb, p, out=dd if inplace else None)
    d = dx.float().cpu().numpy().astype(np.float64)
    d64 = dy.double().numpy()
    assert np.array_equal(d[~keep], np.zeros_like(d[~keep]))
    assert (np.abs(d - d64 * sc) <= _bound(d64 * sc, d64 * sc, 0.0))[keep].all()
    if not with_res:                                                  # the zero patterns of forward and backward are the same one
        nz = (y64 != 0) & (d64 != 0)
        assert np.array_equal((o != 0)[nz], (d != 0)[nz])


def test_autograd_function_saves_nothing_and_passes_dy_to_the_residual(backend):
    dev = backend.device
    g = torch.Generator().manual_seed(4)
    y = backend.to(torch.randn(3, 40, generator=g).to(BF16)).requires_grad_(True)
    r = backend.to(torch.randn(3, 40, generator=g).to(BF16)).requires_grad_(True)
    dy = backend.to(torch.randn(3, 40, generator=g).to(BF16))
    st = _state(dev, 5, 2)
    out = ops.dropout_residual(y, r, st, 1, 0, 0.5)
    assert out.grad_fn.saved_tensors == ()
    out.backward(dy)
    keep = torch.from_numpy(keep_mask(120, 5, 2, 1, 0, 0.5).reshape(3, 40))
    assert torch.equal(r.grad.cpu(), dy.cpu())
    assert torch.equal(y.grad.cpu() != 0, keep & (dy.cpu() != 0))


def test_refused_arguments(backend):
    dev = backend.device
    st = _state(dev, 0, 0)
    with pytest.raises(_lib.HcpError, match="multiple of 8"):
        K.dropout_residual_fwd(torch.ones(12, dtype=BF16, device=dev), None, st, 0, 0, 0.1)
    with pytest.raises(_lib.HcpError, match="p must be"):
        K.dropout_bwd(torch.ones(16, dtype=BF16, device=dev), st, 0, 0, -0.5)


# ------------------------------------------------------------------------------------------------ keep rate
_RATE = {}


def _rate_seed():
    """The first seed whose restatement mask lies within the bound (chosen on the CPU; the kernel must then reproduce that mask)."""
    if not _RATE:
        n, p = 1 << 20, 0.1
        tol = 5.0 * math.sqrt(p * (1 - p) / n)
        for seed in range(100):
            m = keep_mask(n, seed, 1, 0, 0, p)
            if abs(m.mean() - (1 - 6554 / 65536)) <= tol:
                _RATE.update(seed=seed, mask=m, tol=tol)
                break
    return _RATE


def test_keep_rate(backend):
    r = _rate_seed()
    n = 1 << 20
    got = _kernel_mask(backend.device, n, r["seed"], 1, 0, 0, 0.1)
    rate = got.mean()
    print(f"keep rate {rate:.6f} (expected {1 - 6554 / 65536:.6f}, bound {r['tol']:.6f}, seed {r['seed']})")
    assert abs(rate - (1 - 6554 / 65536)) <= r["tol"]
    assert np.array_equal(got, r["mask"])


# ------------------------------------------------------------------------------------------------ layers
class Top(NativeDropoutMixin, torch.nn.Module):
    """A top-level native module around one host layer: its forward opens the native-dropout forward as the UNet's does."""

    def __init__(self, host):
        super().__init__()
        self.host = host

    def forward(self, *a, **k):
        self._native_dropout_begin()
        return self.host(*a, **k)


SEED = 21


def _rel(a, b):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
    return ((a - b).abs().max() / b.abs().max()).item()


def _check_layer(backend, top, blocks, drop_blk, x, res, dy, ref_fn, p=0.5, tol_f=2e-2, expect_id=0, nchw_in=False):
    """Train-mode output of `top(x, residual=res)` against (the same call with p = 0, no residual) x mask x scale (+ res); gradients against
    float64 autograd of `ref_fn(x64, factors64) -> pre-dropout output in the layout of the native output`."""
    dev = backend.device
    top.train()
    drop_blk.dropout.p = 0.0
    kw = {} if res is None else dict(residual=backend.to(res))
    with torch.no_grad():
        y0 = top(backend.to(x)).detach().cpu()
    assert top._hcp_dropout.state[1].item() == 0                      # no grad: no forward counted
    drop_blk.dropout.p = p                                            # p changed 0 -> p: the next forward renumbers
    xn = backend.to(x).clone().requires_grad_(not nchw_in)
    y = top(xn, **kw)
    assert top._hcp_dropout.state[1].item() == 1 and drop_blk._nd[1] == expect_id
    n = y.numel()
    keep = torch.from_numpy(keep_mask(n, SEED + top._hcp_dropout.index, 1, expect_id, 0, p).reshape(y.shape))
    sc = scale_of(p)
    r64 = res.double() if res is not None else torch.zeros(y.shape, dtype=torch.float64)
    exact = torch.where(keep, y0.double() * sc, torch.zeros((), dtype=torch.float64)) + r64
    o = y.detach().double().cpu()
    assert torch.equal(o[~keep], r64[~keep])
    bound = torch.from_numpy(_bound(exact.numpy(), (y0.double() * sc).numpy(), r64.numpy()))
    assert ((o - exact).abs() <= bound)[keep].all()
    y.backward(backend.to(dy))
    x64 = x.detach().double().requires_grad_(not nchw_in)
    fac = [(b.layer.W_down.detach().double().cpu().requires_grad_(True), b.layer.W_up.detach().double().cpu().requires_grad_(True)) for b in blocks]
    yr = ref_fn(x64, fac) * keep.double() * sc + r64
    yr.backward(dy.double())
    assert _rel(y, yr.detach()) < 2e-2
    if not nchw_in:
        assert _rel(xn.grad, x64.grad) < 2e-2
    for b, (wd, wu) in zip(blocks, fac):
        assert wd.grad.abs().max() > 0 and wu.grad.abs().max() > 0
        assert _rel(b.layer.W_down.grad, wd.grad) < tol_f and _rel(b.layer.W_up.grad, wu.grad) < tol_f
    top.eval()                                                        # eval mode: the identity
    with torch.no_grad():
        assert torch.equal(top(backend.to(x)).cpu(), y0)
    return keep


def _w_up(blocks, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for b in blocks:
            b.layer.W_up.copy_((torch.randn(b.layer.W_up.shape, generator=g) * 0.1).to(b.layer.W_up.device))


def test_linear_host(backend):
    from hcp_diffusion_amd.layers import HipLinear
    torch.manual_seed(1)
    top = Top(HipLinear(64, 48).to(backend.device)); top.requires_grad_(False)
    blk = LoraHipLayer.wrap_model(0, top.host, parent_block=top, host_name="host", rank=4, alpha=2.0, dropout=0.5)[""]
    _w_up([blk])
    top.enable_native_dropout(SEED)
    h = top.host._host
    W, b = h.weight.detach().double().cpu(), h.bias.detach().double().cpu()
    ref = lambda x, fac: x @ (W + float(blk.alpha) * (fac[0][1] @ fac[0][0])).T + b
    x = torch.randn(5, 7, 64).to(BF16); res = torch.randn(5, 7, 48).to(BF16); dy = torch.randn(5, 7, 48).to(BF16)
    _check_layer(backend, top, [blk], blk, x, res, dy, ref)


def test_conv3x3_host(backend):
    from hcp_diffusion_amd.layers import HipConv2d
    torch.manual_seed(2)
    top = Top(HipConv2d(16, 24, 3, padding=1).to(backend.device)); top.requires_grad_(False)
    blk = LoraHipLayer.wrap_model(0, top.host, parent_block=top, host_name="host", rank=4, alpha=2.0, dropout=0.5)[""]
    _w_up([blk])
    top.enable_native_dropout(SEED)
    h = top.host._host
    W, b = h.weight.detach().double().cpu(), h.bias.detach().double().cpu()

    def ref(x, fac):
        w = W + float(blk.alpha) * torch.einsum("or,rikl->oikl", fac[0][1][:, :, 0, 0], fac[0][0])
        return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
    x = torch.randn(2, 6, 5, 16).to(BF16); res = torch.randn(2, 6, 5, 24).to(BF16); dy = torch.randn(2, 6, 5, 24).to(BF16)
    _check_layer(backend, top, [blk], blk, x, res, dy, ref)


def test_two_blocks_on_one_host_use_the_last_blocks_layer_id(backend):
    from hcp_diffusion_amd.layers import HipLinear
    torch.manual_seed(3)
    top = Top(HipLinear(64, 48).to(backend.device)); top.requires_grad_(False)
    b0 = LoraHipLayer.wrap_model(0, top.host, parent_block=top, host_name="host", rank=4, alpha=1.0, dropout=0.5)[""]
    b1 = LoraHipLayer.wrap_model(1, top.host, parent_block=top, host_name="host", rank=8, alpha=4.0, dropout=0.5)[""]
    _w_up([b0, b1])
    top.enable_native_dropout(SEED)
    h = top.host._host
    W, b = h.weight.detach().double().cpu(), h.bias.detach().double().cpu()
    ref = lambda x, fac: x @ (W + float(b0.alpha) * (fac[0][1] @ fac[0][0]) + float(b1.alpha) * (fac[1][1] @ fac[1][0])).T + b
    x = torch.randn(5, 7, 64).to(BF16); dy = torch.randn(5, 7, 48).to(BF16)
    _check_layer(backend, top, [b0, b1], b1, x, None, dy, ref, expect_id=1)      # b0 (p > 0) is layer 0, the acting last block layer 1
    assert b0._nd[1] == 0


def test_merged_form_conv_in(backend):
    from hcp_diffusion_amd.layers import HipConvIn
    torch.manual_seed(4)
    top = Top(HipConvIn(4, 16, 3, 1, 1).to(backend.device)); top.requires_grad_(False)
    blk = LoraHipLayer.wrap_model(0, top.host, parent_block=top, host_name="host", rank=4, alpha=2.0, dropout=0.5)[""]
    assert blk.merged
    _w_up([blk])
    top.enable_native_dropout(SEED)
    h = top.host._host
    W, b = h.weight.detach().double().cpu(), h.bias.detach().double().cpu()

    def ref(x, fac):
        w = W + float(blk.alpha) * torch.einsum("or,rikl->oikl", fac[0][1][:, :, 0, 0], fac[0][0])
        return torch.nn.functional.conv2d(x.to(BF16).double(), w, b, padding=1).permute(0, 2, 3, 1)
    x = torch.randn(2, 4, 8, 8); dy = torch.randn(2, 8, 8, 16).to(BF16)
    _check_layer(backend, top, [blk], blk, x, None, dy, ref, tol_f=3e-2, nchw_in=True)


def test_dapp_halves_use_different_masks(backend):
    from hcp_diffusion_amd.layers import HipLinear
    torch.manual_seed(5)
    top = Top(HipLinear(64, 48).to(backend.device)); top.requires_grad_(False)
    bp = DAPPHipLayer.wrap_model(0, top.host, parent_block=top, host_name="host", rank=4, alpha=1.0, branch="p", dropout=0.5)[""]
    bn = DAPPHipLayer.wrap_model(1, top.host, parent_block=top, host_name="host", rank=8, alpha=2.0, branch="n", dropout=0.5)[""]
    _w_up([bp, bn])
    top.enable_native_dropout(SEED)
    h = top.host._host
    W, b = h.weight.detach().double().cpu(), h.bias.detach().double().cpu()
    w_of = lambda blk, f: W + float(blk.alpha) * (f[1] @ f[0])
    ref = lambda x, fac: torch.cat([x[:3] @ w_of(bn, fac[1]).T, x[3:] @ w_of(bp, fac[0]).T]) + b
    x = torch.randn(6, 7, 64).to(BF16); res = torch.randn(6, 7, 48).to(BF16); dy = torch.randn(6, 7, 48).to(BF16)
    # the acting block is the container's LAST plugin (bn, layer id 1); the second half continues the first half's groups, so the mask of
    # the concatenated output is the restatement's over all its elements from group 0
    keep = _check_layer(backend, top, [bp, bn], bn, x, res, dy, ref, tol_f=3e-2, expect_id=1)
    assert not torch.equal(keep[:3], keep[3:])


def test_never_enabled_or_p_zero_is_todays_output(backend):
    """Not enabled: torch's dropout, bit-equal to the op itself on the layer's p = 0 output under the same torch seed.  Enabled with p = 0:
    the fused-residual call of today, bit for bit, and no forward is counted."""
    from hcp_diffusion_amd.layers import HipLinear
    dev = backend.device
    torch.manual_seed(6)
    top = Top(HipLinear(64, 48).to(dev)); top.requires_grad_(False)
    blk = LoraHipLayer.wrap_model(0, top.host, parent_block=top, host_name="host", rank=4, alpha=2.0, dropout=0.0)[""]
    _w_up([blk])
    top.train()
    x = backend.to(torch.randn(5, 7, 64).to(BF16)); res = backend.to(torch.randn(5, 7, 48).to(BF16))
    y_plain = top(x, residual=res).detach().clone()
    y_nores = top(x).detach().clone()
    blk.dropout.p = 0.5
    torch.manual_seed(77)
    y_torch = top(x, residual=res).detach().clone()
    assert blk._nd is None and getattr(top, "_hcp_dropout", None) is None
    torch.manual_seed(77)
    assert torch.equal(y_torch, K.add(torch.nn.functional.dropout(y_nores, 0.5, True), res))
    blk.dropout.p = 0.0
    top.enable_native_dropout(SEED)
    assert torch.equal(top(x, residual=res).detach(), y_plain)
    assert blk._nd is None and top._hcp_dropout.state.tolist() == [SEED, 0]
    top.disable_native_dropout()
    assert top._hcp_dropout is None


# ------------------------------------------------------------------------------------------------ bookkeeping on the UNet
PATS = [r"re:.*\.attn.?$", r"re:.*\.ff$"]


def _unet(dev, dropout=0.1, native=SEED):
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, seeded_init_
    torch.manual_seed(0)
    nat = NativeUNet2DConditionModel(**MICRO_CONFIG)
    nat.load_state_dict(seeded_init_(OracleUNet2DConditionModel(**MICRO_CONFIG), 1).state_dict())
    nat.to(dev)
    nat.requires_grad_(False)
    _, _, bucket = make_lora(nat, [dict(layers=PATS, rank=4, dropout=dropout)])
    _w_up(bucket.blocks, 5)
    bucket.pack()
    if native is not None:
        nat.enable_native_dropout(native)
    return nat, bucket


def _unet_data(dev, n=1):
    g = torch.Generator().manual_seed(7)
    return [(torch.randn(2, 4, 8, 8, generator=g).to(dev), torch.randint(0, 1000, (2,), generator=g).to(dev),
             torch.randn(2, 9, 32, generator=g).to(BF16).to(dev), torch.randn(2, 4, 8, 8, generator=g).to(dev)) for _ in range(n)]


def _fwd_bwd(nat, batch):
    """One forward / backward with the LoRA weight gradients as ONE grouped launch at the end of backward — the form graphed.capture
    records, so that eager and replayed steps run the same kernels."""
    x, t, ehs, target = batch
    wg = ops.WgradContext(grouped=True)
    K.wgrad_staging_begin_step()
    with ops.wgrad_context(wg):
        pred = nat(x, t, ehs).sample
        loss = torch.nn.functional.mse_loss(pred.float(), target)
        loss.backward()
        wg.flush()
    return loss


def test_state_counts_training_forwards_and_checkpointing_rebuilds_the_mask(backend):
    dev = backend.device
    (batch,) = _unet_data(dev)
    grads = []
    for ckpt in (False, True):
        nat, bucket = _unet(dev, native=None)
        keys = set(nat.state_dict())                                   # before enabling
        nat.enable_native_dropout(SEED)
        assert set(nat.state_dict()) == keys and not any(b is nat._hcp_dropout.state for b in nat.buffers())
        if ckpt:
            nat.enable_gradient_checkpointing()
        nd = nat._hcp_dropout
        assert nd.state.tolist() == [SEED, 0]
        for k in range(1, 3):
            bucket.grads.zero_()
            _fwd_bwd(nat, batch)
            assert nd.state.tolist() == [SEED, k] and nd.gen == k
        with torch.no_grad():
            nat(*batch[:3])
        assert nd.state[1].item() == 2                                 # grad disabled: not a training forward
        assert [b._nd[1] for b in nd.blocks] == list(range(len(bucket.blocks))) and len(nd.blocks) > 4
        assert set(nat.state_dict()) == keys
        grads.append(bucket.grads.cpu().clone())
    assert grads[0].abs().max() > 0 and torch.equal(grads[0], grads[1])
    nat0, bucket0 = _unet(dev, dropout=0.0)                            # the masks act: another gradient than without dropout
    _fwd_bwd(nat0, batch); bucket0.grads.zero_(); _fwd_bwd(nat0, batch)
    assert not torch.equal(bucket0.grads.cpu(), grads[0])


def test_backward_of_a_stale_forward_is_refused(backend):
    dev = backend.device
    (batch,) = _unet_data(dev)
    nat, _ = _unet(dev)
    x, t, ehs, _ = batch
    first = nat(x, t, ehs).sample
    nat(x, t, ehs).sample
    with pytest.raises(RuntimeError, match="NativeUNet2DConditionModel.*torch dropout"):
        first.float().mean().backward()


# ------------------------------------------------------------------------------------------------ capture
def test_capturable_with_native_dropout_only(backend):
    from hcp_diffusion_amd import graphed
    nat, _ = _unet(backend.device)
    assert graphed.capturable(nat) is True
    nat.disable_native_dropout()
    assert graphed.capturable(nat) is False                            # the same module on torch dropout
    nat.enable_native_dropout(SEED)
    assert graphed.capturable_cached(nat)[0] is True


def test_module_graph_replays_and_equals_eager_bit_for_bit(backend):
    """Three optimizer steps with the module replaying its captured pair (recorded callables on the CPU, hipGraphs on the GPU) against
    three eager steps from the same seed: the same parameters, bit for bit."""
    dev = backend.device
    data = _unet_data(dev, 3)
    res = {}
    for graph in (False, True):
        nat, bucket = _unet(dev)
        params = [p for blk in bucket.blocks for p in (blk.layer.W_down, blk.layer.W_up)]
        if graph:
            nat.enable_hip_graph(True, _recorded_on_cpu=not backend.is_gpu)
        opt = torch.optim.SGD(params, lr=1e-2)
        for batch in data:
            x, t, ehs, target = batch
            if graph:
                pred = nat(x, t, ehs).sample
                assert type(pred.grad_fn).__name__ == "_GraphedFnBackward"      # replayed, not the eager fallback
                torch.nn.functional.mse_loss(pred.float(), target).backward()
            else:
                _fwd_bwd(nat, batch)
            opt.step()
            opt.zero_grad(set_to_none=False)
        if graph:
            assert len(nat._hip_graphs) == 1
        assert nat._hcp_dropout.state.tolist() == [SEED, 3]
        res[graph] = bucket.params.detach().cpu().clone()
    assert torch.equal(res[False], res[True])


# ------------------------------------------------------------------------------------------------ trainer
def _dapp_trainer(dev, native, dropout=0.1, use_graph=False):
    """(Lion: the optimizer whose whole step is summed without atomics — bucket_state.py: AdamW's global-norm clip adds its partial sums
    with fp32 atomics in arrival order, so no AdamW run on the GPU repeats its own bits, with or without dropout.)"""
    from hcp_diffusion_amd.text_encoder import NativeCLIPTextModel
    from hcp_diffusion_amd.trainer import NativeTrainer
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    from oracle.clip_ref import OracleCLIPTextModel
    from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, seeded_init_
    tcfg = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=77)
    ucfg = dict(MICRO_CONFIG, cross_attention_dim=64)
    torch.manual_seed(0)
    nu = NativeUNet2DConditionModel(**ucfg); nu.load_state_dict(seeded_init_(OracleUNet2DConditionModel(**ucfg), 1).state_dict()); nu.to(dev)
    nt = NativeCLIPTextModel(**tcfg); nt.load_state_dict(seeded_init_(OracleCLIPTextModel(**tcfg), 2).state_dict()); nt.to(dev)
    dapp = lambda layers: [dict(layers=layers, rank=4, type="dapp_hip", branch=br, dropout=dropout) for br in "pn"]
    tr = NativeTrainer(nu, dapp(PATS), lr=1e-3, text_encoder=nt, lora_te_cfg=dapp([r"re:.*self_attn$", r"re:.*mlp$"]), cfg_scale="3.0",
                       native_dropout=native, use_graph=use_graph, optimizer=dict(type="lion"))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for bk in (tr.bucket, tr.te_bucket):
            for blk in bk.blocks:
                blk.layer.W_up.copy_((torch.randn(blk.layer.W_up.shape, generator=g) * 0.05).to(dev))
            bk.pack()
    return tr


def _trainer_run(dev, native, dropout=0.1, use_graph=False, steps=3):
    tr = _dapp_trainer(dev, native, dropout, use_graph)
    g = torch.Generator().manual_seed(9)
    B = 2
    ids = torch.randint(0, 98, (2 * B, 77), generator=g); ids[:, 0] = 98; ids[:, 40:] = 99
    lat = torch.randn(B, 4, 8, 8, generator=g).to(dev)
    noise, t = torch.randn(B, 4, 8, 8, generator=g).to(dev), torch.tensor([100, 800]).to(dev)
    tr.make_noise = lambda l: (K.add_noise(l, noise, t, tr.acp), noise, t)
    snaps = []                                                         # after every step: bucket parameters, then the optimizer moments
    for _ in range(steps):
        tr.train_one_step(lat, prompt_ids=ids.to(dev))
        if dev.type == "cuda":
            torch.cuda.synchronize()
        out = [tr.bucket.params, tr.te_bucket.params] + [x for st in (tr._lora_state, tr._te_state) for x in st.tensors()]
        snaps.append([x.detach().cpu().clone() for x in out])
    return tr, snaps


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def test_trainer_native_dropout_is_reproducible_and_seeded(backend):
    """Three steps twice: the same bits.  Another seed, and dropout 0.0, differ from the first step on (one step each is enough to see it)."""
    dev = backend.device
    tr, base = _trainer_run(dev, 11)
    assert tr.unet._hcp_dropout.state.tolist() == [11, 3] and tr.text_encoder._hcp_dropout.state.tolist() == [12, 3]
    assert len(tr.unet._hcp_dropout.blocks) > 4 and len(tr.text_encoder._hcp_dropout.blocks) > 4
    assert _same(base, _trainer_run(dev, 11)[1])
    assert not _same(base[:1], _trainer_run(dev, 12, steps=1)[1])
    assert not _same(base[:1], _trainer_run(dev, 11, dropout=0.0, steps=1)[1])
    tr0 = _dapp_trainer(dev, None)                                     # native_dropout=None: torch's path, no state tensor on the modules
    assert getattr(tr0.unet, "_hcp_dropout", None) is None and getattr(tr0.text_encoder, "_hcp_dropout", None) is None
    assert all(b._nd is None for b in tr0.bucket.blocks + tr0.te_bucket.blocks)


@pytest.mark.gpu
def test_trainer_captured_step_equals_eager_bit_for_bit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    K._set_backend_for_tests(None)
    dev = torch.device("cuda:0")
    _, eager = _trainer_run(dev, 11, use_graph=False)
    tr, graph = _trainer_run(dev, 11, use_graph=True)
    assert len(tr._graph_cache) == 1
    assert tr.unet._hcp_dropout.state.tolist() == [11, 3]
    assert _same(eager, graph)
    assert _same(graph, _trainer_run(dev, 11, use_graph=True)[1])


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_of_the_dropout_entry_points():
    names = ["hcp_dropout_residual_fwd", "hcp_dropout_bwd", "hcp_dropout_advance"]
    header = open(os.path.join(ROOT, "include", "hcp_mi355x.h")).read()
    from hcp_diffusion_amd.build import SOURCES, build_product
    assert "dropout.hip" in SOURCES
    lib = ctypes.CDLL(str(build_product()))
    for n in names:
        assert re.search(rf"\bint {n}\s*\(", header) and n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n), n
    # the argument counts of header and binding agree
    for n in names:
        args = re.search(rf"\bint {n}\s*\((.*?)\);", header, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._PROTOTYPES[n][1]), n
    assert _lib.ABI_VERSION >= 8 and f"#define HCP_ABI_VERSION {_lib.ABI_VERSION}" in header
    bound = _lib.load()
    assert bound.hcp_dropout_advance(None, None) < 0 and b"null state" in bound.hcp_last_error()
    assert bound.hcp_dropout_residual_fwd(None, None, None, 7, None, 0, 0, 0.1, None) < 0
    assert bound.hcp_dropout_bwd(None, None, 8, None, 0, 0, 0.1, None) < 0
