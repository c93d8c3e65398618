"""TEST HELPER: element-wise float64 check of one GEMM-family launch (kernels.gemm / gemm_lora / gemm_geglu_bwd / conv3x3 /
wgrad_linear / wgrad_conv3x3), described by the plain dict that kernels.LAUNCHES records.

    ops = make_operands(desc, device)          # seeded from a hash of the descriptor
    outs = run(desc, ops)                      # the wrapper, into NaN-poisoned outputs (gap columns hold a sentinel)
    ratio = check(desc, ops, outs)             # |out - ref| <= bound at every element, else AssertionError; returns max err / bound

The reference and the bound are computed in float64 with torch on the operands' device.  The bound is a sum of named terms:

  accumulation  GAMMA * sqrt(K_total) * 2^-24 * sum_k |a_ik| |b_jk|  over every reduced product (K-extension and LoRA path included; the
                split-K slab sums are part of the same reduction).  GAMMA = 2: fp32-accumulate MFMA measures 1e-7 ... 3.5e-7 of
                sum |ab| for K <= 4096, i.e. 1.7 ... 6 ulps, against >= 16 ulps allowed here at K >= 64.
  epilogue      2^-24 |term| for each fp32 addition of the epilogue (alpha, bias, row bias, residual, residual_lo, split-K slabs)
  output        2^-8 |ref| for a bf16 output (the round-to-nearest bound: one half-ulp at the bottom of a binade); 2^-17 |ref| for a
                (hi | lo) pair out + out_lo; 0 for fp32

Measured on MI355X over every launch of the four benchmark workloads and every table entry at its key (tests/test_gemm_launches.py),
worst err / bound: gemm 0.996, gemm_lora 0.996, gemm_geglu_bwd 0.991, conv3x3 0.996 (bf16 outputs: the rounding term itself, an output
one half-ulp off at the bottom of its binade), wgrad_linear 0.458, wgrad_conv3x3 0.222 (fp32 outputs: the accumulation term).  GAMMA = 2
as first set.
  fused LoRA    the reference's LoRA term uses the kernel's own returned T (a legitimate one-ulp flip of T must not fail D); T itself
                is checked against float64 A L^T with its own bound
  GEGLU         the h / g errors (accumulation + epilogue + the bf16 rounding the stand-alone pass reads) propagated through gelu,
                gelu' and gelu'' (|gelu''| <= 0.8), plus PHI_ERR absolute on the Abramowitz-Stegun Phi; the GEGLU-backward epilogue
                rounds dY_ff to bf16 before it multiplies (csrc/gemm_params.h: the values of the two-kernel form)

Operands: activations N(0,1) with per-row scales 2^U(-4,4), weights N(0,1/K) with per-output-channel scales 2^U(-2,2) — an error in a
small row cannot hide behind the largest row."""
import hashlib
import json
import math
import re
from pathlib import Path

import torch
import torch.nn.functional as F

BF = torch.bfloat16
U = 2.0 ** -24
GAMMA = 2.0
PHI_ERR = 3e-7 + 16 * U                # Abramowitz-Stegun Phi (3e-7) + its fp32 evaluation
SENTINEL16 = 0x7FA5                    # bit patterns left in the gap columns of a strided output (ldd > N)
SENTINEL32 = 0x7FA5A5A5

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hcp_diffusion_amd" / "csrc"


def gamma(k_total):
    return GAMMA * math.sqrt(max(k_total, 1)) * U


# ---------------------------------------------------------------- operands

def seed_of(desc):
    return int(hashlib.sha256(json.dumps(desc, sort_keys=True).encode()).hexdigest()[:12], 16)


class _Gen:
    def __init__(self, desc, device):
        self.dev = torch.device(device)
        self.g = torch.Generator(device=self.dev).manual_seed(seed_of(desc))

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.g, device=self.dev, dtype=torch.float32)

    def scales(self, n, lo, hi):
        return torch.exp2(torch.rand(n, generator=self.g, device=self.dev) * (hi - lo) + lo)

    def act(self, rows, cols):
        return (self.randn(rows, cols) * self.scales(rows, -4, 4)[:, None]).to(BF)

    def wt(self, rows, cols, k=None):
        return (self.randn(rows, cols) / math.sqrt(k or cols) * self.scales(rows, -2, 2)[:, None]).to(BF)


def _strided(t, ld):
    """t [R, C] as a view with row stride ld >= C (the columns beyond C hold other data: here zeros)."""
    if ld == t.shape[1]:
        return t.contiguous()
    base = torch.zeros(t.shape[0], ld, dtype=t.dtype, device=t.device)
    base[:, :t.shape[1]] = t
    return base[:, :t.shape[1]]


def make_operands(desc, device):
    d = desc
    g = _Gen(d, device)
    o = {}
    kind = d["kind"]
    if kind == "gemm":
        M, N, K, K2 = d["M"], d["N"], d["K"], d["K2"]
        o["a"] = _strided(g.act(M, K), d["lda"]); o["b"] = _strided(g.wt(N, K), d["ldb"])
        if K2:
            o["a2"] = _strided(g.act(M, K2), d["lda2"]); o["b2"] = _strided(g.wt(N, K2), d["ldb2"])
        if d["bias"]:
            o["bias"] = g.randn(N)
        if d["rowbias"]:
            o["rowbias"] = g.randn((M + d["rows_per_group"] - 1) // d["rows_per_group"], N)
        if d["residual"]:
            o["residual"] = _strided(g.act(M, N), d["ldr"])
            if d["residual_lo"]:
                o["residual_lo"] = _strided((o["residual"].float() * g.randn(M, N) * 2.0 ** -9).to(BF), d["ldr"])
    elif kind == "gemm_lora":
        M, N, K = d["M"], d["N"], d["K"]
        o["a"] = _strided(g.act(M, K), d["lda"]); o["b"] = _strided(g.wt(N, K), d["ldb"])
        o["l"] = g.wt(32, K); o["e"] = g.wt(N, 32)
        if d["bias"]:
            o["bias"] = g.randn(N)
        if d["residual"]:
            o["residual"] = _strided(g.act(M, N), d["ldr"])
            if d["residual_lo"]:
                o["residual_lo"] = _strided((o["residual"].float() * g.randn(M, N) * 2.0 ** -9).to(BF), d["ldr"])
    elif kind == "gemm_geglu_bwd":
        M, Fd, C = d["M"], d["N"], d["K"]
        o["dy"] = _strided(g.act(M, C), d["lda"]); o["wt"] = _strided(g.wt(Fd, C), d["ldb"])
        o["hg"] = g.act(M, 2 * Fd)
        if d["lora"]:
            o["l"] = g.wt(32, C); o["e"] = g.wt(Fd, 32)
    elif kind == "conv3x3":
        B, Hs, Ws, C1, C2 = d["B"], d["Hs"], d["Ws"], d["C1"], d["C2"]
        M, N, Ctot = d["M"], d["N"], C1 + C2
        o["x1"] = g.act(B * Hs * Ws, C1).view(B, Hs, Ws, C1)
        if C2:
            o["x2"] = g.act(B * Hs * Ws, C2).view(B, Hs, Ws, C2)
        o["wp"] = g.wt(N, 9 * Ctot).view(N, 3, 3, Ctot)
        if d["K2"]:
            o["a2"] = g.act(M, 32); o["b2"] = g.wt(N, 32)
        if d["bias"]:
            o["bias"] = g.randn(N)
        if d["rowbias"]:
            o["rowbias"] = g.randn(B, N)
        if d["residual"]:
            o["residual"] = g.act(M, N).view(B, d["Ho"], d["Wo"], N)
    elif kind == "wgrad_linear":
        M, N, K = d["M"], d["N"], d["K"]
        o["dy"] = _strided(g.act(M, N), d["ldy"]); o["x"] = _strided(g.act(M, K), d["ldx"])
        o["dw0"] = _strided(g.randn(N, K), d["ldw"])
    elif kind == "wgrad_conv3x3":
        B, Hs, Ws, C1, C2 = d["B"], d["Hs"], d["Ws"], d["C1"], d["C2"]
        o["x1"] = g.act(B * Hs * Ws, C1).view(B, Hs, Ws, C1)
        if C2:
            o["x2"] = g.act(B * Hs * Ws, C2).view(B, Hs, Ws, C2)
        dy = g.act(d["M"], d["ldy"])
        c_end, c_pad = d["col0"] + d["Cout"], min(d["ldy"], d["col0"] + (d["Cout"] + 7) // 8 * 8)
        dy[:, c_end:c_pad] = 0                                             # the documented contract: padded columns of the piece are zero
        o["dy"] = dy.view(B, d["Ho"], d["Wo"], d["ldy"])
        o["dw0"] = g.randn(d["Cout"], 3, 3, d["Cw"])
    else:
        raise ValueError(f"unknown launch kind {kind}")
    return o


# ---------------------------------------------------------------- running the wrapper

def _poisoned(shape, ld, dtype, device, fill):
    """A [rows, cols] output with row stride ld: the columns are `fill`, the gap columns (ld > cols) the sentinel bit pattern."""
    rows, cols = shape
    base = torch.empty(rows, ld, dtype=dtype, device=device)
    if ld > cols:
        iv = base.view(torch.int16 if dtype == BF else torch.int32)
        iv.fill_(SENTINEL16 if dtype == BF else SENTINEL32)
    base[:, :cols].fill_(fill)
    return base


def _fill_like(t, fill):
    t.fill_(fill)
    return t


def run(desc, ops, fill=float("nan")):
    """Call the wrapper the descriptor names on `ops`; outputs that the wrapper allocates itself are poisoned through a patched
    torch.empty of this call only (the wrappers take the buffers they return from torch.empty)."""
    from hcp_diffusion_amd import kernels as K
    d = desc
    kind = d["kind"]
    dev = next(iter(ops.values())).device
    outs = {}
    real_empty = torch.empty

    def poisoned_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return _fill_like(t, fill) if t.is_floating_point() else t
    if kind == "gemm":
        dt = torch.float32 if d["out_f32"] else BF
        base = _poisoned((d["M"], d["N"]), d["ldd"], dt, dev, fill)
        outs["base"] = base
        K.torch.empty = poisoned_empty
        try:
            r = K.gemm(ops["a"], ops["b"], a2=ops.get("a2"), b2=ops.get("b2"), bias=ops.get("bias"), rowbias=ops.get("rowbias"),
                       rows_per_group=d["rows_per_group"] or 1, residual=ops.get("residual"), alpha=d["alpha"], out_f32=d["out_f32"],
                       out=base[:, :d["N"]], residual_lo=ops.get("residual_lo"), want_lo=d["want_lo"], want_gact=d["gact"])
        finally:
            K.torch.empty = real_empty
        if d["gact"]:
            outs["out"], outs["gact"] = r
        elif d["want_lo"]:
            outs["out"], outs["out_lo"] = r
        else:
            outs["out"] = r
    elif kind == "gemm_lora":
        K.torch.empty = poisoned_empty
        try:
            r, t = K.gemm_lora(ops["a"], ops["b"], ops["l"], ops["e"], bias=ops.get("bias"), residual=ops.get("residual"), want_t=True,
                               residual_lo=ops.get("residual_lo"), want_lo=d["want_lo"], want_gact=d["gact"])
        finally:
            K.torch.empty = real_empty
        outs["t"] = t
        if d["gact"]:
            outs["out"], outs["gact"] = r
        elif d["want_lo"]:
            outs["out"], outs["out_lo"] = r
        else:
            outs["out"] = r
    elif kind == "gemm_geglu_bwd":
        K.torch.empty = poisoned_empty
        try:
            outs["out"], u = K.gemm_geglu_bwd(ops["dy"], ops["wt"], ops["hg"], l=ops.get("l"), e=ops.get("e"), want_t=True)
        finally:
            K.torch.empty = real_empty
        if u is not None:
            outs["t"] = u
    elif kind == "conv3x3":
        dt = torch.float32 if d["out_f32"] else BF
        out = torch.full((d["B"], d["Ho"], d["Wo"], d["N"]), fill, dtype=dt, device=dev)
        outs["out"] = K.conv3x3(ops["x1"], ops["wp"], d["N"], x2=ops.get("x2"), stride=d["stride"], upsample=bool(d["upsample"]),
                                mode=d["mode"], out_hw=(d["Ho"], d["Wo"]), bias=ops.get("bias"), rowbias=ops.get("rowbias"),
                                residual=ops.get("residual"), out_f32=d["out_f32"], a2=ops.get("a2"), b2=ops.get("b2"), pad=d["pad"], out=out)
    elif kind == "wgrad_linear":
        base = ops["dw0"]._base if ops["dw0"]._base is not None else ops["dw0"]
        base = base.clone()
        if d["ldw"] > d["K"]:
            base[:, d["K"]:].view(torch.int32).fill_(SENTINEL32)
        outs["base"] = base
        outs["out"] = base[:, :d["K"]]
        K.wgrad_linear(ops["dy"], ops["x"], outs["out"])
    elif kind == "wgrad_conv3x3":
        outs["out"] = ops["dw0"].clone()
        K.wgrad_conv3x3(ops["dy"], ops["x1"], outs["out"], x2=ops.get("x2"), stride=d["stride"], upsample=bool(d["upsample"]),
                        cout=d["Cout"], col0=d["col0"])
    return outs


# ---------------------------------------------------------------- float64 references

def _d(t):
    return t.double()


def _gelu_parts(x):
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    cdf = 0.5 * (1 + torch.special.erf(x / math.sqrt(2)))
    return x * cdf, cdf + x * phi, phi          # gelu, gelu', phi


def _epilogue(acc, accabs, alpha, extras):
    """ref and pre-output-rounding bound of alpha * acc + sum(extras): one 2^-24 |term| per fp32 operation (and one for the split-K
    slab sums, whose magnitudes add up to at most sum |ab|)."""
    ref = alpha * acc
    absum = abs(alpha) * accabs
    n = 2 + (1 if alpha != 1.0 else 0)
    for t in extras:
        ref = ref + t
        absum = absum + t.abs()
        n += 1
    return ref, U * n * absum


def _rowbias_rows(rb, M, rpg):
    idx = torch.arange(M, device=rb.device) // rpg
    return rb[idx]


def _conv_taps(X, s, up, pad, Ho, Wo):
    """the 9 shifted NHWC slices [B*Ho*Wo, C] of the forward gather (nearest-2x upsample, zero padding 1 or the asymmetric pad 0)."""
    if up:
        X = X.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    Xp = F.pad(X, (0, 0, 1, 1, 1, 1)) if pad else F.pad(X, (0, 0, 0, 1, 0, 1))
    C = X.shape[3]
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, Xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :].reshape(-1, C)


def conv_forward_ref(x1, x2, wp, s, up, pad, Ho, Wo):
    """(acc, accabs) [B*Ho*Wo, Cout] of the 3x3 forward convolution: the sum of 9 shifted products."""
    X = _d(x1) if x2 is None else torch.cat([_d(x1), _d(x2)], 3)
    W = _d(wp)
    acc = accabs = 0
    for ky, kx, Xs in _conv_taps(X, s, up, pad, Ho, Wo):
        w = W[:, ky, kx, :]
        acc = acc + Xs @ w.T
        accabs = accabs + Xs.abs() @ w.abs().T
    return acc, accabs


def conv_dgrad_ref(dy, wp, s, Ho, Wo):
    """(acc, accabs) [B*Ho*Wo, Cin]: the adjoint of the forward sum — dX[iy, ix] += dY[oy, ox] W[tap] with iy = s oy + ky - 1."""
    B, Hs, Ws, C1 = dy.shape
    cin = wp.shape[0]
    Y = _d(dy).reshape(-1, C1)
    W = _d(wp)
    acc = torch.zeros(B, Ho + 2, Wo + 2, cin, dtype=torch.float64, device=dy.device)
    accabs = torch.zeros_like(acc)
    for ky in range(3):
        for kx in range(3):
            w = W[:, ky, kx, :]
            acc[:, ky:ky + s * (Hs - 1) + 1:s, kx:kx + s * (Ws - 1) + 1:s, :] += (Y @ w.T).view(B, Hs, Ws, cin)
            accabs[:, ky:ky + s * (Hs - 1) + 1:s, kx:kx + s * (Ws - 1) + 1:s, :] += (Y.abs() @ w.abs().T).view(B, Hs, Ws, cin)
    return acc[:, 1:Ho + 1, 1:Wo + 1].reshape(-1, cin), accabs[:, 1:Ho + 1, 1:Wo + 1].reshape(-1, cin)


class Item:
    """one compared output: got / ref / bound (float64, same shape)."""
    def __init__(self, name, got, ref, bound):
        self.name, self.got, self.ref, self.bound = name, got, ref, bound


def _rounded(name, got, ref, pre, out_kind):
    rnd = {"bf16": 2.0 ** -8, "hilo": 2.0 ** -17, "f32": 0.0}[out_kind]
    return Item(name, got, ref, pre + rnd * (ref.abs() + pre))


def _t_items(t, A, L, ldt, two_launch):
    """the fused-LoRA T / U: (the T the product used, its check against float64 A L^T)."""
    tr = _d(t[:, :32]) + (_d(t[:, 32:64]) if ldt == 64 else 0)
    ref = A @ L.T
    pre = gamma(A.shape[1]) * (A.abs() @ L.abs().T)
    kind = "hilo" if (ldt == 64 and not two_launch) else "bf16"
    items = [_rounded("T", tr, ref, pre, kind)]
    if ldt == 64 and two_launch:                     # the two-launch form keeps the bf16-rounded T and zeroes the residual half
        items.append(Item("T_lo", _d(t[:, 32:64]), torch.zeros_like(ref), torch.zeros_like(ref)))
    return tr, items


def _gact_item(ref, pre, got):
    """GEGLU forward: gact = bf16(h gelu(g)) of (h | g) = ref; the h / g the pass used are within pre + 2^-8 |ref| of the reference
    (the fused epilogue's fp32 values, or the bf16 (h | g) the stand-alone pass reads)."""
    Fh = ref.shape[1] // 2
    h, gg = ref[:, :Fh], ref[:, Fh:]
    e = pre + 2.0 ** -8 * ref.abs()
    eh, eg = e[:, :Fh], e[:, Fh:]
    G, G1, _ = _gelu_parts(gg)
    y = h * G
    dg = G1.abs() * eg + 0.4 * eg * eg                  # |gelu(g + dg) - gelu(g)| <= |gelu'| dg + max|gelu''| / 2 dg^2
    err = eh * (G.abs() + dg) + h.abs() * dg + h.abs() * gg.abs() * PHI_ERR + 4 * U * y.abs()
    return Item("gact", _d(got), y, err + 2.0 ** -8 * (y.abs() + err))


def two_launch_lora(M, N, K, tables=None):
    """launch_lora_dispatched's choice of the two-launch form (T GEMM + K-extension GEMM) for a fused-LoRA problem."""
    e = lookup(tables or load_tables(), (3, M, N, K, 1, 1, 0))
    if e is not None:
        return e["cfg"] == -1
    return K >= 4096 and M <= 4096


def references(desc, ops, outs):
    d = desc
    kind = d["kind"]
    items = []
    if kind in ("gemm", "gemm_lora"):
        M, N = d["M"], d["N"]
        A, B = _d(ops["a"]), _d(ops["b"])
        acc, accabs, kt = A @ B.T, A.abs() @ B.abs().T, d["K"]
        if kind == "gemm" and d["K2"]:
            A2, B2 = _d(ops["a2"]), _d(ops["b2"])
            acc, accabs, kt = acc + A2 @ B2.T, accabs + A2.abs() @ B2.abs().T, kt + d["K2"]
        if kind == "gemm_lora":
            tr, t_items = _t_items(outs["t"], A, _d(ops["l"]), d["ldt"], two_launch_lora(M, N, d["K"]))
            items += t_items
            E = _d(ops["e"])
            acc, accabs, kt = acc + tr @ E.T, accabs + tr.abs() @ E.abs().T, kt + (64 if d["ldt"] == 64 else 32)
        extras = []
        if d["bias"]:
            extras.append(_d(ops["bias"])[None, :])
        if d.get("rowbias"):
            extras.append(_rowbias_rows(_d(ops["rowbias"]), M, d["rows_per_group"]))
        if d["residual"]:
            extras.append(_d(ops["residual"]))
            if d["residual_lo"]:
                extras.append(_d(ops["residual_lo"]))
        ref, epi = _epilogue(acc, accabs, d.get("alpha", 1.0), extras)
        pre = gamma(kt) * abs(d.get("alpha", 1.0)) * accabs + epi
        if d["want_lo"]:
            items.append(_rounded("out+out_lo", _d(outs["out"]) + _d(outs["out_lo"]), ref, pre, "hilo"))
        else:
            items.append(_rounded("out", _d(outs["out"]), ref, pre, "f32" if d.get("out_f32") else "bf16"))
        if d["gact"]:
            items.append(_gact_item(ref, pre, outs["gact"]))
    elif kind == "gemm_geglu_bwd":
        Fd = d["N"]
        Y, W = _d(ops["dy"]), _d(ops["wt"])
        acc, accabs, kt = Y @ W.T, Y.abs() @ W.abs().T, d["K"]
        if d["lora"]:
            tr, t_items = _t_items(outs["t"], Y, _d(ops["l"]), d["ldt"], two_launch_lora(d["M"], Fd, d["K"]))
            items += t_items
            E = _d(ops["e"])
            acc, accabs, kt = acc + tr @ E.T, accabs + tr.abs() @ E.abs().T, kt + (64 if d["ldt"] == 64 else 32)
        ed = gamma(kt) * accabs + 2 * U * accabs
        ed = ed + 2.0 ** -8 * (acc.abs() + ed)          # the epilogue rounds dY_ff to bf16 first (the two-kernel form's values)
        hg = _d(ops["hg"])
        h, g = hg[:, :Fd], hg[:, Fd:]
        G, G1, phi = _gelu_parts(g)
        r1 = acc * G
        e1 = ed * G.abs() + acc.abs() * g.abs() * PHI_ERR + 4 * U * r1.abs()
        r2 = acc * h * G1
        e2 = ed * (h * G1).abs() + (acc * h).abs() * (PHI_ERR * (1 + g.abs()) + 8 * U * (1 + g.abs() * phi)) + 4 * U * r2.abs()
        got = _d(outs["out"])
        items.append(_rounded("dh", got[:, :Fd], r1, e1, "bf16"))
        items.append(_rounded("dg", got[:, Fd:], r2, e2, "bf16"))
    elif kind == "conv3x3":
        M, N = d["M"], d["N"]
        if d["mode"] == 0:
            acc, accabs = conv_forward_ref(ops["x1"], ops.get("x2"), ops["wp"], d["stride"], d["upsample"], d["pad"], d["Ho"], d["Wo"])
        else:
            acc, accabs = conv_dgrad_ref(ops["x1"], ops["wp"], d["stride"], d["Ho"], d["Wo"])
        kt = d["K"]
        if d["K2"]:
            A2, B2 = _d(ops["a2"]), _d(ops["b2"])
            acc, accabs, kt = acc + A2 @ B2.T, accabs + A2.abs() @ B2.abs().T, kt + 32
        extras = []
        if d["bias"]:
            extras.append(_d(ops["bias"])[None, :])
        if d["rowbias"]:
            extras.append(_rowbias_rows(_d(ops["rowbias"]), M, d["Ho"] * d["Wo"]))
        if d["residual"]:
            extras.append(_d(ops["residual"]).reshape(M, N))
        ref, epi = _epilogue(acc, accabs, 1.0, extras)
        items.append(_rounded("out", _d(outs["out"]).reshape(M, N), ref, gamma(kt) * accabs + epi, "f32" if d["out_f32"] else "bf16"))
    elif kind == "wgrad_linear":
        Y, X = _d(ops["dy"]), _d(ops["x"])
        dw0 = _d(ops["dw0"])
        ref, epi = _epilogue(Y.T @ X, Y.T.abs() @ X.abs(), 1.0, [dw0])
        items.append(Item("dw", _d(outs["out"]), ref, gamma(d["M"]) * (Y.T.abs() @ X.abs()) + epi))
    elif kind == "wgrad_conv3x3":
        Cout, Cw, c0 = d["Cout"], d["Cw"], d["col0"]
        Y = _d(ops["dy"]).reshape(d["M"], d["ldy"])[:, c0:c0 + Cout]
        X = _d(ops["x1"]) if "x2" not in ops else torch.cat([_d(ops["x1"]), _d(ops["x2"])], 3)
        acc = torch.zeros(Cout, 3, 3, Cw, dtype=torch.float64, device=Y.device)
        accabs = torch.zeros_like(acc)
        for ky, kx, Xs in _conv_taps(X, d["stride"], d["upsample"], 1, d["Ho"], d["Wo"]):
            acc[:, ky, kx, :] = Y.T @ Xs[:, :Cw]
            accabs[:, ky, kx, :] = Y.T.abs() @ Xs[:, :Cw].abs()
        ref, epi = _epilogue(acc, accabs, 1.0, [_d(ops["dw0"])])
        items.append(Item("dw", _d(outs["out"]), ref, gamma(d["M"]) * accabs + epi))
    return items


def describe(desc):
    return json.dumps({k: v for k, v in desc.items() if v not in (False, 0) or k in ("M", "N", "K")}, sort_keys=True)


def compare(desc, items, base=None, cols=None, describe=describe):
    """|got - ref| <= bound at every element (NaN fails); the gap columns of `base` beyond `cols` still hold the sentinel.
    Returns the worst err / bound; raises AssertionError naming the descriptor and the worst element (row / col, or the axes an item
    names in `dims`: tests/attn_check.py gives batch / row / head / col)."""
    worst = 0.0
    for it in items:
        err = (it.got - it.ref).abs()
        bad = ~(err <= it.bound)                     # NaN compares False: an unwritten (poisoned) element fails
        ratio = torch.where(it.bound > 0, err / it.bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        flat = ratio.reshape(-1)
        i = int(torch.argmax(flat))
        r = float(flat[i])
        if bool(bad.any()):
            ncols = it.ref.shape[-1]
            row, col = divmod(i, ncols) if it.ref.dim() == 2 else (i // ncols, i % ncols)
            where = f"row {row} col {col}"
            if getattr(it, "dims", None):
                idx = [int(x) for x in torch.unravel_index(torch.tensor(i), it.ref.shape)]
                where = " ".join(f"{n} {x}" for n, x in zip(it.dims, idx))
            g, rf, b = float(it.got.reshape(-1)[i]), float(it.ref.reshape(-1)[i]), float(it.bound.reshape(-1)[i])
            raise AssertionError(f"{it.name} of {describe(desc)}: {int(bad.sum())} elements outside the float64 bound; worst at {where}"
                                 f": got {g:.9g} ref {rf:.9g} err {abs(g - rf):.3g} bound {b:.3g} (ratio {r:.3g})")
        worst = max(worst, r)
    if base is not None and base.shape[1] > cols:
        gap = base[:, cols:]
        iv = gap.view(torch.int16) if gap.dtype == BF else gap.view(torch.int32)
        want = SENTINEL16 if gap.dtype == BF else SENTINEL32
        bad = iv != want
        if bool(bad.any()):
            i = int(torch.argmax(bad.reshape(-1).int()))
            row, col = divmod(i, gap.shape[1])
            raise AssertionError(f"gap column written by {describe(desc)}: row {row} col {cols + col} (ldd {base.shape[1]}, N {cols})")
    return worst


def check(desc, ops, outs):
    cols = desc["K"] if desc["kind"] == "wgrad_linear" else desc["N"]
    return compare(desc, references(desc, ops, outs), outs.get("base"), cols)


# ---------------------------------------------------------------- the dispatch tables (csrc/gemm_tuned_loaders.inc, csrc/gemm_tuned.inc)

_ENTRY = re.compile(r"^\{([-\d,\s]+)\},?\s*(?://\s*(.*))?$")
_TABLES = None


def load_tables():
    """Both tables as data, in lookup_tuned's order (the loader table first): dicts with the key, the choice and the comment."""
    global _TABLES
    if _TABLES is None:
        out = []
        for name in ("gemm_tuned_loaders.inc", "gemm_tuned.inc"):
            for ln, line in enumerate((CSRC / name).read_text().splitlines(), 1):
                m = _ENTRY.match(line.strip())
                if not m:
                    continue
                v = [int(x) for x in m.group(1).split(",") if x.strip()]
                assert len(v) in (9, 10), f"{name}:{ln}: {line}"
                keys = ("mode", "M", "N", "K", "has_k2", "stride", "up", "cfg", "split", "loaders")
                e = dict(zip(keys, v + [0] * (10 - len(v))))
                e.update(table=name, line=ln, comment=(m.group(2) or "").strip())
                out.append(e)
        _TABLES = out
    return _TABLES


def entry_key(e):
    return (e["mode"], e["M"], e["N"], e["K"], e["has_k2"], e["stride"], e["up"])


def lookup(tables, key):
    """lookup_tuned: the first entry whose (mode, M, N, K, has_K2) match — and, for the conv modes 1 / 2, stride and upsample."""
    mode, M, N, K, k2, s, up = key
    for e in tables:
        if e["mode"] == mode and e["M"] == M and e["N"] == N and e["K"] == K and e["has_k2"] == k2 and \
                (mode in (0, 3) or (e["stride"] == s and e["up"] == up)):
            return e
    return None


def dispatch_keys(desc, tables=None):
    """The lookup_tuned keys one launch consults (a fused-LoRA problem in its two-launch form consults three)."""
    d = desc
    kind = d["kind"]
    if kind == "gemm":
        return [(0, d["M"], d["N"], d["K"], 1 if d["K2"] else 0, 1, 0)]
    if kind == "conv3x3":
        return [(1 if d["mode"] == 0 else 2, d["M"], d["N"], d["K"], 1 if d["K2"] else 0, d["stride"], d["upsample"])]
    if kind == "gemm_geglu_bwd" and not d["lora"]:
        return [(0, d["M"], d["N"], d["K"], 0, 1, 0)]
    if kind in ("gemm_lora", "gemm_geglu_bwd"):
        keys = [(3, d["M"], d["N"], d["K"], 1, 1, 0)]
        if two_launch_lora(d["M"], d["N"], d["K"], tables):
            keys += [(0, d["M"], 32, d["K"], 0, 1, 0), (0, d["M"], d["N"], d["K"], 1, 1, 0)]
        return keys
    return []                                   # the weight gradients have their own launch rule (csrc/wgrad.hip)


_CONV_COMMENT = re.compile(r"conv C(\d+)\+(\d+) H(\d+) Cout(\d+) s(\d) up(\d)")
_DGRAD_COMMENT = re.compile(r"dgrad C(\d+) H(\d+) Cout(\d+) s(\d)")


def _square_geometry(M):
    """(B, Ho) with B * Ho^2 == M: two or more images where possible (a batch edge to cross), else one."""
    for B in (2, 4, 8, 3, 6, 1):
        if M % B == 0:
            h = math.isqrt(M // B)
            if h * h * B == M:
                return B, h
    raise ValueError(f"no square conv geometry for M={M}")


def synth_descriptor(e):
    """A launch that reaches table entry e at its key: plain GEMM (bias + residual), fused-LoRA GEMM, forward conv (the geometry its
    comment names, else one source with C = K / 9 and a square image consistent with M), or data-gradient conv."""
    mode, M, N, K, k2, s, up = entry_key(e)
    if mode == 0:
        return dict(kind="gemm", M=M, N=N, K=K, K2=32 if k2 else 0, lda=K, ldb=K, ldd=N, lda2=32 if k2 else 0, ldb2=32 if k2 else 0,
                    ldr=N, bias=True, rowbias=False, rows_per_group=0, residual=True, residual_lo=False, want_lo=False, gact=False,
                    alpha=1.0, out_f32=False)
    if mode == 3:
        return dict(kind="gemm_lora", M=M, N=N, K=K, lda=K, ldb=K, ldd=N, ldt=32, want_t=True, ldr=N, bias=True, residual=True,
                    residual_lo=False, want_lo=False, gact=False)
    m = _CONV_COMMENT.search(e["comment"]) if mode == 1 else _DGRAD_COMMENT.search(e["comment"])
    if mode == 1:
        if m and int(m.group(5)) == s and int(m.group(6)) == up and 9 * (int(m.group(1)) + int(m.group(2))) == K:
            C1, C2, Hs = int(m.group(1)), int(m.group(2)), int(m.group(3))
            Ho = (Hs * (2 if up else 1) - 1) // s + 1
            B = M // (Ho * Ho)
        else:
            C1, C2 = K // 9, 0
            B, Ho = _square_geometry(M)
            Hs = Ho * s // (2 if up else 1)
        assert B * Ho * Ho == M and (Hs * (2 if up else 1) - 1) // s + 1 == Ho, e
        return dict(kind="conv3x3", M=M, N=N, K=K, K2=32 if k2 else 0, mode=0, B=B, Hs=Hs, Ws=Hs, C1=C1, C2=C2, Cout=N, stride=s,
                    upsample=up, pad=1, Ho=Ho, Wo=Ho, ldd=N, ldr=N, bias=True, rowbias=True, rows_per_group=Ho * Ho, residual=True,
                    out_f32=False)
    if m and int(m.group(4)) == s and int(m.group(1)) == N and 9 * int(m.group(3)) == K:
        Ho = int(m.group(2))
        B = M // (Ho * Ho)
    else:
        B, Ho = _square_geometry(M)
    Hs = (Ho - 1) // s + 1
    assert B * Ho * Ho == M, e
    return dict(kind="conv3x3", M=M, N=N, K=K, K2=32 if k2 else 0, mode=1, B=B, Hs=Hs, Ws=Hs, C1=K // 9, C2=0, Cout=N, stride=s,
                upsample=0, pad=1, Ho=Ho, Wo=Ho, ldd=N, ldr=N, bias=False, rowbias=False, rows_per_group=0, residual=True, out_f32=False)


# ---------------------------------------------------------------- element-wise checks of hand-built calls (tests/test_kernels.py, ...)

_DEFAULTS = {
    "gemm": dict(K2=0, bias=False, rowbias=False, rows_per_group=0, residual=False, residual_lo=False, want_lo=False, gact=False, alpha=1.0,
                 out_f32=False),
    "gemm_lora": dict(ldt=32, bias=False, residual=False, residual_lo=False, want_lo=False, gact=False),
    "conv3x3": dict(K2=0, mode=0, C2=0, stride=1, upsample=0, pad=1, bias=False, rowbias=False, residual=False, out_f32=False),
    "wgrad_linear": {},
    "wgrad_conv3x3": dict(C2=0, stride=1, upsample=0, col0=0),
}


def desc(kind, **kw):
    """a descriptor for references() / check() with the flags a hand-built call leaves at their defaults; conv sizes are derived."""
    d = dict(_DEFAULTS[kind], kind=kind)
    d.update(kw)
    if kind in ("conv3x3", "wgrad_conv3x3"):
        d.setdefault("M", d["B"] * d["Ho"] * d["Wo"])
        d.setdefault("K", 9 * (d["C1"] + d["C2"]))
        d.setdefault("N", d["Cout"])
    return d
