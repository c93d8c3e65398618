"""Folded upsampler convolutions (csrc/gemm_pp.hip MODE 4 / 5, csrc/pack.hip conv_fold_pack_kernel): behind a nearest-2x upsample a 3x3
convolution reads a 2x2 neighbourhood of the low-resolution source per output parity, so the frozen upsampler convs run as four 2x2
convolutions (forward) and one 4x4 stride-2 convolution over dY (data gradient) on weights folded once from the fp32 master.

  * the folding kernel alone: equality with fp32 sums of the master taps (ascending (ky, kx) order), rounded once
  * forward and data gradient element-wise against float64 of the operands the kernel was given (bf16 input, bf16 folded images), with the
    per-element bound rule of gemm_check (accumulation + epilogue + output rounding)
  * Upsample2D end to end: folded against unfolded, both against float64 F.interpolate + F.conv2d from the fp32 master
  * the fall-backs (trainable weight, LoRA-wrapped conv, Cin = 72) never enter the folded entry point and compute what they computed
  * module-level graph capture on the two-level miniature UNet

Cases (batch, source Hs x Ws, Cin -> Cout): (2, 3x5, 64 -> 160) ragged M tile, Ws no power of two, every pixel on a border; (1, 1x1, 64 ->
160) all taps but one invalid; (2, 4x4, 128 -> 320) two N tiles per parity, two channel chunks per tap, bias, split-K 2 on the data gradient."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_check as GC
from hcp_diffusion_amd import kernels as K

BF = torch.bfloat16
CASES = [(2, 3, 5, 64, 160), (1, 1, 1, 64, 160), (2, 4, 4, 128, 320)]
IDS = ["b2_3x5_c64_160", "b1_1x1_c64_160", "b2_4x4_c128_320"]

YS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}          # forward: kernel rows behind tap ty = 0 | 1 of output parity py
AS = ((2,), (1, 2), (0, 1), (0,))                   # data gradient: kernel rows behind tap ay = 0 .. 3


def _master(cout, cin, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cout, 3, 3, cin, generator=g) / math.sqrt(9 * cin) * torch.exp2(torch.rand(cout, generator=g) * 4 - 2)[:, None, None, None]


def _sum_taps(w, kys, kxs):
    """fp32 sum of master taps in ascending (ky, kx) order: w [Cout][3][3][Cin] -> [Cout][Cin]"""
    acc = None
    for ky in kys:
        for kx in kxs:
            acc = w[:, ky, kx, :].clone() if acc is None else acc + w[:, ky, kx, :]
    return acc


def _fold_ref(w):
    cout, _, _, cin = w.shape
    wf = torch.empty(2, 2, cout, 2, 2, cin)
    wdf = torch.empty(cin, 4, 4, cout)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    wf[py, px, :, ty, tx, :] = _sum_taps(w, YS[py][ty], YS[px][tx])
    for ay in range(4):
        for ax in range(4):
            wdf[:, ay, ax, :] = _sum_taps(w, AS[ay], AS[ax]).T
    return wf.to(BF), wdf.to(BF)


def _pack(w, to):
    cout, _, _, cin = w.shape
    wf = to(torch.full((2, 2, cout, 2, 2, cin), float("nan"), dtype=BF)); wdf = to(torch.full((cin, 4, 4, K.fold_cout_pad(cout)), float("nan"), dtype=BF))
    K.conv_fold_pack(to(w.contiguous()), wf, wdf)
    return wf, wdf


@pytest.mark.parametrize("cin,cout", [(64, 160), (128, 320)])
def test_fold_pack_equals_fp32_tap_sums(tbackend, cin, cout):
    w = _master(cout, cin, 11 + cin)
    wf, wdf = _pack(w, tbackend.to)
    rf, rdf = _fold_ref(w)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    assert torch.equal(wf.cpu()[py, px, :, ty, tx, :], rf[py, px, :, ty, tx, :]), (py, px, ty, tx)
    for ay in range(4):
        for ax in range(4):
            assert torch.equal(wdf.cpu()[:, ay, ax, :cout], rdf[:, ay, ax, :]), (ay, ax)
    assert not wdf.cpu()[..., cout:].float().any()                          # the K padding of the data-gradient image is zero


def _fwd_items(x, wf, bias, y):
    """float64 reference of the folded forward from the kernel's own operands, per output parity."""
    B, Hs, Ws, cin = x.shape
    cout = wf.shape[2]
    Xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    W = wf.double()
    ref = torch.zeros(B, 2 * Hs, 2 * Ws, cout, dtype=torch.float64, device=x.device)
    pre = torch.zeros_like(ref)
    for py in range(2):
        for px in range(2):
            acc = accabs = 0
            for ty in range(2):
                for tx in range(2):
                    xs = Xp[:, ty + py:ty + py + Hs, tx + px:tx + px + Ws, :].reshape(-1, cin)
                    acc = acc + xs @ W[py, px, :, ty, tx, :].T
                    accabs = accabs + xs.abs() @ W[py, px, :, ty, tx, :].abs().T
            r, epi = GC._epilogue(acc, accabs, 1.0, [bias.double()[None, :]] if bias is not None else [])
            ref[:, py::2, px::2, :] = r.view(B, Hs, Ws, cout)
            pre[:, py::2, px::2, :] = (GC.gamma(4 * cin) * accabs + epi).view(B, Hs, Ws, cout)
    return [GC._rounded("y", y.double().reshape(-1, cout), ref.reshape(-1, cout), pre.reshape(-1, cout), "bf16")]


def _dgrad_items(dy, wdf, dx):
    B, H2, W2, cout = dy.shape
    Hs, Ws, cin = H2 // 2, W2 // 2, wdf.shape[0]
    Yp = F.pad(dy.double(), (0, 0, 1, 1, 1, 1))
    W = wdf.double()[..., :cout]
    acc = accabs = 0
    for ay in range(4):
        for ax in range(4):
            ys = Yp[:, ay:ay + 2 * Hs:2, ax:ax + 2 * Ws:2, :].reshape(-1, cout)
            acc = acc + ys @ W[:, ay, ax, :].T
            accabs = accabs + ys.abs() @ W[:, ay, ax, :].abs().T
    ref, epi = GC._epilogue(acc, accabs, 1.0, [])
    return [GC._rounded("dx", dx.double().reshape(-1, cin), ref, GC.gamma(16 * cout) * accabs + epi, "bf16")]


def _acts(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, C, generator=g) * torch.exp2(torch.rand(B, H, W, 1, generator=g) * 8 - 4)).to(BF)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_folded_kernels_against_float64(tbackend, case):
    B, Hs, Ws, cin, cout = case
    to = tbackend.to
    L = K.lib()
    w = _master(cout, cin, 3)
    wf, wdf = _pack(w, to)
    wp = to(w.to(BF).contiguous())
    wd = to(w.permute(3, 1, 2, 0).to(BF).contiguous())
    x = to(_acts(B, Hs, Ws, cin, 5)); dy = to(_acts(B, 2 * Hs, 2 * Ws, cout, 6))
    big = cin == 128
    bias = to(torch.randn(cout, generator=torch.Generator().manual_seed(8))) if big else None
    desc = dict(kind="conv_fold", case=list(case))
    try:
        y = K.conv3x3(x, wp, cout, upsample=True, bias=bias, fold=wf)
        assert tuple(y.shape) == (B, 2 * Hs, 2 * Ws, cout)
        r1 = GC.compare(desc, _fwd_items(x, wf, bias, y))
        splits = (1, 2) if big else (1,)
        for split in splits:
            if split > 1:
                L.hcp_debug_set_gemm_config(1024 + 4 + 64 * split)      # tile id 4 (64 x 160), split-K forced
            dx = K.conv3x3(dy, wd, cin, mode=1, out_hw=(2 * Hs, 2 * Ws), fold=wdf)
            assert tuple(dx.shape) == (B, Hs, Ws, cin)
            r2 = GC.compare(desc, _dgrad_items(dy, wdf, dx))
            print(f"\n{IDS[CASES.index(case)]} split {split}: worst err / bound forward {r1:.3g}, data gradient {r2:.3g}")
    finally:
        L.hcp_debug_set_gemm_config(-1)


def _upsampler(cin, cout, dev, seed=21):
    from hcp_diffusion_amd.layers import HipConv2d
    from hcp_diffusion_amd.unet import Upsample2D
    m = Upsample2D(cin)
    m.conv = HipConv2d(cin, cout, 3, 1, 1)
    w = _master(cout, cin, seed)
    with torch.no_grad():
        m.conv.weight.copy_(w.permute(0, 3, 1, 2))
        m.conv.bias.copy_(torch.randn(cout, generator=torch.Generator().manual_seed(seed + 1)) * 0.1)
    m.to(dev)
    m.requires_grad_(False)
    return m


def _run_module(m, x, dy):
    xi = x.clone().requires_grad_(True)
    K.LAUNCHES = []
    try:
        y = m(xi)
        y.backward(dy)
        trace = [k for k in map(K.trace_key, K.LAUNCHES) if k is not None]
    finally:
        K.LAUNCHES = None
    return y.detach().cpu(), xi.grad.detach().cpu(), trace


class _Count:
    """Calls of the folded entry point (kernels._conv3x3_fold) while the context is open."""
    def __enter__(self):
        self.n, self.orig = 0, K._conv3x3_fold

        def counted(*a, **k):
            self.n += 1
            return self.orig(*a, **k)
        K._conv3x3_fold = counted
        return self

    def __exit__(self, *exc):
        K._conv3x3_fold = self.orig


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_upsample2d_folded_against_unfolded(tbackend, case):
    """Folded and unfolded module, forward and dX, against float64 F.interpolate + F.conv2d of the fp32 master: the folded path's maximum
    error may exceed the unfolded path's by at most one bf16 spacing at the largest output (one rounding per folded weight instead of up
    to four independent ones: the error against the exact convolution does not grow).
    Both errors are printed on every run; on the interpreter (LAB_NOTEBOOK round 8): y 0.156 vs 0.161, 0.0049 vs 0.0029, 0.265 vs 0.270;
    dX 0.325 vs 0.502, 0.074 vs 0.068, 0.253 vs 0.409 (folded vs unfolded, the three cases in order)."""
    B, Hs, Ws, cin, cout = case
    dev = tbackend.device
    L = K.lib()
    m = _upsampler(cin, cout, dev)
    x = _acts(B, Hs, Ws, cin, 31).to(dev); dy = _acts(B, 2 * Hs, 2 * Ws, cout, 32).to(dev)
    w64 = m.conv.weight.detach().double().cpu(); b64 = m.conv.bias.detach().double().cpu()
    xr = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.conv2d(F.interpolate(xr, scale_factor=2.0, mode="nearest"), w64, b64, padding=1)
    yr.backward(dy.double().cpu().permute(0, 3, 1, 2))
    yr = yr.detach().permute(0, 2, 3, 1); dxr = xr.grad.permute(0, 2, 3, 1)
    try:
        with _Count() as c:
            yf, dxf, tf = _run_module(m, x, dy)
        assert c.n == 2                                                   # forward and data gradient both took the folded entry point
        L.hcp_debug_set_conv_fold(0)
        yu, dxu, tu = _run_module(m, x, dy)
    finally:
        L.hcp_debug_set_conv_fold(1)
    assert tf == tu                                                       # the folded operands are not part of the trace
    for name, f, u, r in (("y", yf, yu, yr), ("dx", dxf, dxu, dxr)):
        ef, eu = (f.double() - r).abs().max().item(), (u.double() - r).abs().max().item()
        ulp = 2.0 ** (math.floor(math.log2(r.abs().max().item())) - 7)
        print(f"\n{IDS[CASES.index(case)]} {name}: max |err| folded {ef:.4g}, unfolded {eu:.4g}, bf16 spacing at max |ref| {ulp:.4g}")
        assert ef <= eu + ulp, (name, ef, eu, ulp)


@pytest.mark.parametrize("which", ["trainable", "lora", "cin72"])
def test_fallbacks_keep_the_unfolded_kernels(tbackend, which):
    """A weight that requires grad, a LoRA-wrapped conv and Cin = 72 never reach the folded entry point: same trace and same bits with
    the switch on and off."""
    dev = tbackend.device
    L = K.lib()
    cin = 72 if which == "cin72" else 64
    m = _upsampler(cin, 160, dev)
    params = []
    if which == "trainable":
        m.conv.weight.requires_grad_(True)
        params = [m.conv.weight]
    elif which == "lora":
        from hcp_diffusion_amd.lora import make_lora
        _, _, bucket = make_lora(m, [dict(layers=["conv"], rank=4)])
        with torch.no_grad():
            for blk in bucket.blocks:
                blk.layer.W_up.copy_(torch.randn(blk.layer.W_up.shape, generator=torch.Generator().manual_seed(9)).to(dev) * 0.05)
        bucket.pack()
    x = _acts(2, 3, 5, cin, 41).to(dev); dy = _acts(2, 6, 10, 160, 42).to(dev)
    res = []
    try:
        for on in (1, 0):
            L.hcp_debug_set_conv_fold(on)
            for p in params:
                p.grad = None
            with _Count() as c:
                res.append(_run_module(m, x, dy))
            assert c.n == 0, which
    finally:
        L.hcp_debug_set_conv_fold(1)
    (y1, dx1, t1), (y0, dx0, t0) = res
    assert t1 == t0 and any(t[0] == "conv" and t[9] == 1 for t in t1)     # the upsample=1 launch is there, unchanged
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)


def _mini_unet(dev, channels):
    from hcp_diffusion_amd.lora import make_lora
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, seeded_init_
    cfg = dict(MICRO_CONFIG, block_out_channels=channels, num_attention_heads=channels[0] // 40)      # head dims 40 / 80
    torch.manual_seed(0)
    nat = NativeUNet2DConditionModel(**cfg)
    nat.load_state_dict(seeded_init_(OracleUNet2DConditionModel(**cfg), 1).state_dict())
    nat.to(dev)
    nat.requires_grad_(False)
    _, _, bucket = make_lora(nat, [dict(layers=[r"re:.*\.attn.?$", r"re:.*\.ff$"], rank=4)])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for blk in bucket.blocks:
            blk.layer.W_up.copy_(torch.randn(blk.layer.W_up.shape, generator=g).to(dev) * 0.05)
    bucket.pack()
    return nat, [p for blk in bucket.blocks for p in (blk.layer.W_down, blk.layer.W_up)]


def _graph_vs_eager(dev, is_gpu, channels, folds):
    g = torch.Generator().manual_seed(7)
    data = [(torch.randn(2, 4, 8, 8, generator=g).to(dev), torch.randint(0, 1000, (2,), generator=g).to(dev),
             torch.randn(2, 9, 32, generator=g).to(BF).to(dev), torch.randn(2, 4, 8, 8, generator=g).to(dev)) for _ in range(2)]
    losses = {}
    for graph in (False, True):
        nat, params = _mini_unet(dev, channels)
        if graph:
            nat.enable_hip_graph(True, _recorded_on_cpu=not is_gpu)
        opt = torch.optim.AdamW(params, lr=1e-2, weight_decay=1e-3)
        out = []
        with _Count() as c:
            for x, t, ehs, target in data:
                loss = F.mse_loss(nat(x, t, ehs).sample.float(), target)
                loss.backward()
                opt.step(); opt.zero_grad(set_to_none=True)
                out.append(loss.item())
        if not graph:
            assert (c.n > 0) == folds
        losses[graph] = out
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), losses


def test_graph_capture_equals_eager(tbackend):
    """unet.enable_hip_graph() on the two-level miniature UNet of bench.py's emulator configuration (its C80 upsampler keeps the 3x3
    gather): graph losses = eager losses, as test_graphed.py asks."""
    _graph_vs_eager(tbackend.device, tbackend.is_gpu, (40, 80), folds=False)


@pytest.mark.gpu
def test_graph_capture_equals_eager_with_a_folded_upsampler():
    """The same miniature at (160, 320) channels, whose C320 upsampler runs folded inside the captured graph (GPU only: two minutes on
    the interpreter)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    K._set_backend_for_tests(None)
    try:
        _graph_vs_eager(torch.device("cuda:0"), True, (160, 320), folds=True)
    finally:
        K._set_backend_for_tests(None)
