"""The narrow ping-pong tile (csrc/gemm_pp.hip, tile id 16 = 32 x 160): one 16-row block per compute wave, so after the groups' exchange
a wave finishes part of its 16-column blocks (group 0 three, group 1 two) instead of half of its row blocks.  Forced through the tuning
hooks (hcp_debug_set_gemm_config(1024 + id + 64 * split), loaders = 8 + ring) and checked against fp32: plain GEMM with K-extension,
bias, residual and ragged M / N, split-K, the fused-LoRA GEMM (Y and T), the tile epilogue, and the GEGLU-forward fallback (the narrow
tile has no pairing epilogue: the caller's own kernels run and the stand-alone GEGLU pass follows)."""
import pytest
import torch
import torch.nn.functional as F

import gemm_check as GC
from hcp_diffusion_amd import kernels as K

BF = torch.bfloat16
NARROW = 16


def relerr(a, b):
    a = a.float().cpu(); b = b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def rnd(*shape):
    return torch.randn(*shape).to(BF)


def t_full(t):
    t = t.float().cpu()
    return t[:, :32] + t[:, 32:] if t.shape[1] == 64 else t


def force(cfg, split=1):
    return 1024 + cfg + 64 * split


def _reset(L):
    L.hcp_debug_set_gemm_config(-1); L.hcp_debug_set_gemm_loaders(-1); L.hcp_debug_set_gemm_epilogue(-1)


@pytest.mark.parametrize("ring", [2, 3, 4])
def test_narrow_tile_plain_gemm(tbackend, ring):
    to = tbackend.to
    L = K.lib()
    torch.manual_seed(300 + ring)
    M, N, Kd = (70, 304, 192) if not tbackend.is_gpu else (1000, 1264, 1280)      # ragged M (not a multiple of 32) and N (not of 160)
    a, b, a2, b2 = rnd(M, Kd), rnd(N, Kd), rnd(M, 32), rnd(N, 32)
    bias, res = torch.randn(N), rnd(M, N)
    ref = a.float() @ b.float().T + a2.float() @ b2.float().T + bias + res.float()
    try:
        L.hcp_debug_set_gemm_loaders(8 + ring)
        for split in (1, 2):
            L.hcp_debug_set_gemm_config(force(NARROW, split))
            out = K.gemm(to(a), to(b), a2=to(a2), b2=to(b2), bias=to(bias), residual=to(res))
            assert relerr(out, ref) < 1e-2, split
            ops = dict(a=to(a), b=to(b), a2=to(a2), b2=to(b2), bias=to(bias), residual=to(res))
            GC.check(GC.desc("gemm", M=M, N=N, K=Kd, K2=32, bias=True, residual=True), ops, {"out": out})
            o32 = K.gemm(to(a), to(b), bias=to(bias), out_f32=True)
            assert relerr(o32, a.float() @ b.float().T + bias) < 1e-5, split
            GC.check(GC.desc("gemm", M=M, N=N, K=Kd, bias=True, out_f32=True), ops, {"out": o32})
    finally:
        _reset(L)


@pytest.mark.parametrize("ring", [2, 3, 4])
def test_narrow_tile_fused_lora(tbackend, ring):
    to = tbackend.to
    L = K.lib()
    torch.manual_seed(310 + ring)
    M, N, Kd = (70, 304, 192) if not tbackend.is_gpu else (1000, 1264, 1280)
    a, b = rnd(M, Kd), rnd(N, Kd)
    l, e = (torch.randn(32, Kd) * 0.2).to(BF), (torch.randn(N, 32) * 0.2).to(BF)
    bias, res = torch.randn(N), rnd(M, N)
    t_ref = a.float() @ l.float().T
    ref = a.float() @ b.float().T + t_ref.to(BF).float() @ e.float().T + bias + res.float()
    try:
        L.hcp_debug_set_gemm_loaders(8 + ring)
        L.hcp_debug_set_gemm_config(force(NARROW))
        out, t = K.gemm_lora(to(a), to(b), to(l), to(e), bias=to(bias), residual=to(res))
        assert relerr(out, ref) < 1e-2
        assert relerr(t_full(t), t_ref) < (1e-4 if K.T_SPLIT else 1e-2)
        GC.check(GC.desc("gemm_lora", M=M, N=N, K=Kd, ldt=t.shape[1], bias=True, residual=True),
                 dict(a=to(a), b=to(b), l=to(l), e=to(e), bias=to(bias), residual=to(res)), {"out": out, "t": t})
    finally:
        _reset(L)


def _split_hi_lo(x):
    hi = x.to(BF)
    return hi, (x - hi.float()).to(BF)


def test_narrow_tile_epilogues_agree(tbackend):
    """Tile epilogue (16-byte row pieces through LDS) and lane-layout epilogue give the same bits on the narrow tile: row bias, alpha,
    the (hi | lo) residual stream, the fused-LoRA tail."""
    to = tbackend.to
    L = K.lib()
    torch.manual_seed(320)
    M, N, Kd = (70, 304, 192) if not tbackend.is_gpu else (1000, 1264, 1280)
    a, b, a2, b2 = rnd(M, Kd), (torch.randn(N, Kd) * 0.1).to(BF), rnd(M, 32), (torch.randn(N, 32) * 0.1).to(BF)
    bias = torch.randn(N); rpg = max(1, M // 4); rb = torch.randn((M + rpg - 1) // rpg, N)
    hi, lo = _split_hi_lo(torch.randn(M, N) * 4)
    l, e = (torch.randn(32, Kd) * 0.2).to(BF), (torch.randn(N, 32) * 0.2).to(BF)

    def run():
        o1 = K.gemm(to(a), to(b), a2=to(a2), b2=to(b2), bias=to(bias), rowbias=to(rb), rows_per_group=rpg, residual=to(hi), alpha=0.5)
        o2, o2l = K.gemm(to(a), to(b), bias=to(bias), residual=to(hi), residual_lo=to(lo), want_lo=True)
        (o3, o3l), t = K.gemm_lora(to(a), to(b), to(l), to(e), bias=to(bias), residual=to(hi), residual_lo=to(lo), want_lo=True)
        return [x.cpu().clone() for x in (o1, o2, o2l, o3, o3l, t)]
    try:
        L.hcp_debug_set_gemm_loaders(8 + 3); L.hcp_debug_set_gemm_config(force(NARROW))
        L.hcp_debug_set_gemm_epilogue(0)
        lane = run()
        L.hcp_debug_set_gemm_epilogue(1)
        tile = run()
    finally:
        _reset(L)
    for x, y in zip(lane, tile):
        assert torch.equal(x, y)
    ref = 0.5 * (a.float() @ b.float().T + a2.float() @ b2.float().T) + bias + rb.repeat_interleave(rpg, 0)[:M] + hi.float()
    assert relerr(tile[0], ref) < 1e-2
    assert relerr(tile[1].float() + tile[2].float(), a.float() @ b.float().T + bias + hi.float() + lo.float()) < 1e-4
    ops = dict(a=a, b=b, a2=a2, b2=b2, bias=bias, rowbias=rb, residual=hi, residual_lo=lo, l=l, e=e)
    GC.check(GC.desc("gemm", M=M, N=N, K=Kd, K2=32, bias=True, rowbias=True, rows_per_group=rpg, residual=True, alpha=0.5), ops, {"out": tile[0]})
    GC.check(GC.desc("gemm", M=M, N=N, K=Kd, bias=True, residual=True, residual_lo=True, want_lo=True), ops, {"out": tile[1], "out_lo": tile[2]})
    GC.check(GC.desc("gemm_lora", M=M, N=N, K=Kd, ldt=tile[5].shape[1], bias=True, residual=True, residual_lo=True, want_lo=True), ops,
             {"out": tile[3], "out_lo": tile[4], "t": tile[5]})


@pytest.mark.parametrize("lora", [False, True])
def test_narrow_tile_geglu_falls_back(tbackend, lora):
    """The narrow tile refuses the GEGLU-forward pairing epilogue: the GEMM runs on id 16's fallback kernels and the stand-alone GEGLU
    pass computes gact from the rounded (h | g)."""
    to = tbackend.to
    L = K.lib()
    torch.manual_seed(330)
    M, Fd, Kd = (70, 160, 192) if not tbackend.is_gpu else (1000, 1280, 640)
    a, b = rnd(M, Kd), (torch.randn(2 * Fd, Kd) * 0.1).to(BF)
    bias = torch.randn(2 * Fd)
    l, e = (torch.randn(32, Kd) * 0.2).to(BF), (torch.randn(2 * Fd, 32) * 0.2).to(BF)
    hg = a.float() @ b.float().T + bias
    if lora:
        hg = hg + (a.float() @ l.float().T).to(BF).float() @ e.float().T
    try:
        L.hcp_debug_set_gemm_loaders(8 + 3); L.hcp_debug_set_gemm_config(force(NARROW))
        if lora:
            (o, ga), t = K.gemm_lora(to(a), to(b), to(l), to(e), bias=to(bias), want_gact=True)
        else:
            o, ga = K.gemm(to(a), to(b), bias=to(bias), want_gact=True)
    finally:
        _reset(L)
    assert relerr(o, hg) < 1e-2
    two_pass = F.gelu(o.float().cpu()[:, Fd:]) * o.float().cpu()[:, :Fd]
    assert relerr(ga, two_pass) < 1e-2
    ops = dict(a=to(a), b=to(b), l=to(l), e=to(e), bias=to(bias))
    if lora:
        GC.check(GC.desc("gemm_lora", M=M, N=2 * Fd, K=Kd, ldt=t.shape[1], bias=True, gact=True), ops, {"out": o, "gact": ga, "t": t})
    else:
        GC.check(GC.desc("gemm", M=M, N=2 * Fd, K=Kd, bias=True, gact=True), ops, {"out": o, "gact": ga})


# the SD1.5 shapes (batch 4) whose dispatch-table entries moved to the narrow tile: (fused-LoRA?, M, N, K, K2)
RETUNED = [(True, 1024, 1280, 1280, 0), (False, 1024, 1280, 1280, 32), (False, 1024, 1280, 1280, 0), (False, 256, 1280, 1280, 0)]


@pytest.mark.parametrize("lora,M,N,Kd,K2", RETUNED)
def test_retuned_shapes_match_previous_tile(tbackend, lora, M, N, Kd, K2):
    """The dispatched result of every retuned shape equals the 64 x 160 ping-pong tile it replaced to within bf16 rounding (on the
    interpreter at a reduced size: the same comparison, outside the table)."""
    to = tbackend.to
    L = K.lib()
    torch.manual_seed(340 + M + Kd)
    if not tbackend.is_gpu:
        M, N, Kd = M // 16 + 6, N // 4, Kd // 10
    a, b = rnd(M, Kd), (torch.randn(N, Kd) * 0.1).to(BF)
    a2, b2 = (rnd(M, K2), rnd(N, K2)) if K2 else (None, None)
    l, e = (torch.randn(32, Kd) * 0.2).to(BF), (torch.randn(N, 32) * 0.2).to(BF)
    bias, res = torch.randn(N), rnd(M, N)

    def run():
        if lora:
            return K.gemm_lora(to(a), to(b), to(l), to(e), bias=to(bias), residual=to(res))[0].cpu().clone()
        return K.gemm(to(a), to(b), a2=None if a2 is None else to(a2), b2=None if b2 is None else to(b2), bias=to(bias),
                      residual=to(res)).cpu().clone()
    try:
        _reset(L)
        got = run()
        L.hcp_debug_set_gemm_loaders(8 + 4); L.hcp_debug_set_gemm_config(force(14))
        prev = run()
    finally:
        _reset(L)
    assert relerr(got, prev) < 1e-2
