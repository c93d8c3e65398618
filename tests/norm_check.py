"""TEST HELPER: element-wise float64 check of one norm launch (csrc/norm.hip through kernels.groupnorm_fwd / groupnorm_bwd /
groupnorm_affine_grad / layernorm_fwd / layernorm_bwd / layernorm_affine_grad), described by a plain dict:

    kind  gn_fwd | gn_bwd | gn_affine    B, HW, C, G, silu, eps, addend; slab (False: the two-launch row-chunk path, through
                                         hcp_debug_set_gn_target(-1)), target (workgroups a row-chunk launch aims at, default 512)
    kind  ln_fwd | ln_bwd | ln_affine    M, C, eps, addend, x_lo, addend_lo, want_lo

    ops = make_operands(desc, device)          # seeded from a hash of the descriptor
    outs = run(desc, ops)                      # the wrappers, every buffer they allocate NaN-poisoned (the GroupNorm workspace too)
    ratio = check(desc, ops, outs)             # |out - ref| <= bound at every element, else AssertionError; returns max err / bound

Operands.  GroupNorm x: every (sample, group) has its own standard deviation 2^U(-4,4) and its own mean, 0 to 40 standard deviations
(40 rand^2, either sign), so a wrong quiet group cannot hide behind a loud one and the one-pass sums cancel.  LayerNorm rows alike.
gamma N(1, 0.5) with a random sign and every 7th channel scaled by 2^-10; beta N(0, 0.3) with every 5th channel moved by -4 (SiLU's
negative tail, where silu' changes sign).  dy and the addend N(0,1) with per-row scales 2^U(-4,4).  (hi | lo) operands are the two
bf16 images of ONE fp32 tensor (hi = bf16(v), lo = bf16(v - hi)).  dgamma / dbeta start from N(0,1): the kernel accumulates.

Running.  torch.empty / torch.empty_like are patched for the call: y, stats, dx, dx_lo and the GroupNorm workspace start as NaN, so an
element that is never written, or a workspace partial that is read before it is written, fails.  Every input is compared bit for bit with
a copy taken before the call.  run() sets the descriptor's slab / target through the debug hook and restores the defaults in a finally.

Reference.  float64 torch from the bf16 inputs as given.  The forward statistics (mean, rstd per (sample, group) / per row) are their
own item, against the float64 statistics of x.  Everything downstream — y, dx, dgamma / dbeta, the row-chunk path's backward partial
sums — is referred to the kernel's OWN stats (as the attention backward is to its own lse): a legitimate last-bit difference of the
statistics does not fail them, and their bounds stay tight where the statistics' bound is loose.  The row-chunk path leaves its partials
in the workspace: forward (mean_c, M2_c) and backward (S1_c, S2_c) per (sample, chunk, group) are items ("ws_*").

Bound per element, a sum of named terms (U = 2^-24; g(n) = NG GAMMA sqrt(n) U, the fp32 accumulation of n terms, gemm_check.gamma
times the one free constant NG; every sum below is over the elements actually summed together: a group's n = HW Cg, a chunk's n_c,
a row's C):
  mean          g(n) sum|x| / n + 2 U |mean|                                   (row-chunk: + g(nchunk) sum|x| / n for the merge)
  M2 two-pass   (g(n) + 4 U) M2 + n e_mean^2                                   (slab kernels and LayerNorm: sum (x - mean)^2 from registers)
  M2 one-pass   per chunk (3 g(n_c) + 6 U) sum_c x^2: m2 = sum x^2 - (sum x)^2 / n_c cancels to M2_c out of sum x^2, so at
                |mean| = m std the chunk's relative error is (1 + m^2) times the accumulation error — carried as it is; the merge
                adds (g(nchunk) + 4 U)(M2 + 2 S2) + 4 sum_c n_c |mean_c - K| (e_mean_c + e_mean_0), S2 = sum_c n_c (mean_c - K)^2
  rstd          rstd (e_M2 / (2 (M2 + n eps)) + 4 U)                           (division, sqrt, reciprocal)
  y             4 U (|x a| + |mean a| + |beta|), a = rstd gamma: y = x a + (beta - mean a) cancels to z; LayerNorm (x - mean) rstd
                gamma + beta: 4 U (|xh gamma| + |beta|) (+ U |x| rstd |gamma| for the fp32 add of hi + lo)
  SiLU          sigmoid on the hardware exp2 and rcp: relative e_s = (1 - s)(EXP_REL + 2 U |z|) + 2 U (EXP_REL of attn_check; the
                fp32 multiply of z by -log2 e in front).  silu: |silu'| e_z + |silu| (e_s + 2 U).  silu' = s (1 + z (1 - s)):
                e_z / 2 (|silu''| <= 1/2) + e_s s (1 + |z|) + 4 U (s + |z| s (1 - s))
  xh, dxh       e_xh = 3 U |xh|;  e_dxh = |dy gamma| e_silu' + 2 U |dxh|
  S1, S2        sum e_dxh + g(n) sum|dxh|;  sum (e_dxh |xh| + |dxh| e_xh) + g(n) sum|dxh xh|      (row-chunk: per chunk, n_c)
  c1, c2        e_S / n + g(nchunk) sum|.| / n + 2 U |c|
  dx            rstd (e_dxh + e_c1 + |xh| e_c2 + |c2| e_xh + 3 U (|dxh| + |c1| + |xh c2|)) + 2 U |rstd t| + U (|addend| + |addend_lo|
                + |dx|): the last bracket of the first term is the cancellation in t = dxh - c1 - xh c2
  dgamma/dbeta  sum (e_dz |xh| + |dz| e_xh) + g(rows) sum|dz xh| + U nblocks (|start| + sum|dz xh|): one fp32 atomic add per
                (row block, sample) slab onto the starting value
  output        2^-8 |ref| for a bf16 output, 2^-17 |ref| for the pair dx + dx_lo, 0 for fp32 (stats, workspace, dgamma / dbeta)

NG is the one free constant: sqrt(n) is the typical size of an accumulated rounding error, not its maximum.  It scales only the
accumulation terms.  The items whose bound is made of them are the statistics and the workspace partials (mean, rstd, ws_mean, ws_M2,
ws_S1, ws_S2): the 0.5 rule is applied to these.  A bf16 output (y, dx, the pair dx + dx_lo) reaches err / bound ~ 1 whatever NG
is — the rounding term itself, an output half an ulp off at the bottom of its binade, as in gemm_check — and so do dgamma / dbeta
where one row is summed (M = 1: the bound is the rounding of the one fp32 atomic add onto the starting value); they are reported and
held to 1 (dgamma / dbeta over several rows are accumulation items, held to 0.5).  Measured on MI355X, product library (the row-chunk cases: the tuning build of the same sources) against this float64
reference over every descriptor of tests/test_norm_launches.py (its GPU report test prints these figures at every run), worst
err / bound with NG = 1:
  slab GroupNorm       mean 0.035  rstd 0.091  y 0.996  dx 0.995  dgamma 0.161  dbeta 0.041
  row-chunk GroupNorm  mean 0.040  rstd 0.061  ws_mean 0.094  ws_M2 0.043  ws_S1 0.139  ws_S2 0.140  y 0.996  dx 0.996
  LayerNorm            mean 0.135  rstd 0.346  y 0.996  dx 0.995  dx+dx_lo 0.968  dgamma 0.192  dbeta 0.045; one row: 0.950, 0.972
The worst accumulation item with NG = 1, 1/2, 1/4, 1/8: 0.346, 0.412, 0.456 (LayerNorm rstd), 0.611 (ws_S1).  NG = 1/4 is the
smallest power of two that leaves the worst ratio at or below 0.5 — with it, over the same descriptors:
  slab GroupNorm       mean 0.113  rstd 0.192  dgamma 0.338  dbeta 0.073
  row-chunk GroupNorm  mean 0.127  rstd 0.145  ws_mean 0.279  ws_M2 0.133  ws_S1 0.412  ws_S2 0.304
  LayerNorm            mean 0.264  rstd 0.456  dgamma 0.424  dbeta 0.150  (y, dx, dx + dx_lo, one-row dgamma / dbeta: 0.954 .. 0.996)
The interpreter passes under the same NG.  Nothing failed its bound — the one-pass m2 of gn_fwd_partial at |mean| up to 40 std, and
mean8 / rstd8 of a straddling affine-gradient thread, included: no kernel was changed.

Mutation test (tests/test_norm_launches.py::test_mutations_are_caught): a torch model of the blocked algorithms with twelve faults —
ragged_last_row_dropped, straddling_thread_group_off_by_one, stats_of_neighbouring_sample, c2_omitted,
silu_grad_omitted_in_quietest_group, addend_dropped_in_last_chunk, dead_slab_chunk_not_masked, magic_row_division_off_by_one,
affine_tail_rows_dropped, dbeta_channel_doubled, ln_padding_lane_in_variance, dx_lo_from_unrounded — every one is caught under NG = 1/4.
The old gates (tensor-maximum relerr < 1e-2 for y / dx, < 2e-3 for dgamma / dbeta, the group means to 1e-4 of the largest, dx + dx_lo
to 1e-4) are applied by the same test to the faulty model run on operands as tests/test_kernels.py drew them (_old_operands there: one
scale per tensor; GroupNorm at 1021 rows, LayerNorm at 5): they pass c2_omitted.  With one scale per tensor there is no quiet group, so
the SiLU fault shows; the others they would have caught only on the code paths they ran — the slab classes <8,2> at 1024 threads,
<4,2>, <32,2>, the R = 1 row-chunk geometries and the second merge round were run by no test."""
import json
import math

import torch
import torch.nn.functional as F

import gemm_check as GC
from attn_check import EXP_REL
from gemm_check import BF, U, Item

NG = 0.25

GN_KINDS = ("gn_fwd", "gn_bwd", "gn_affine")
LN_KINDS = ("ln_fwd", "ln_bwd", "ln_affine")
_DEFAULTS = dict(eps=1e-5, silu=False, addend=False, slab=True, target=512, x_lo=False, addend_lo=False, want_lo=False)


def desc(kind, **kw):
    assert kind in GN_KINDS + LN_KINDS, kind
    d = dict(_DEFAULTS, kind=kind)
    d.update(kw)
    if kind in GN_KINDS:
        d.setdefault("G", 32)
        assert d["C"] % d["G"] == 0 and d["C"] % 8 == 0
    else:
        assert not d["addend_lo"] or d["addend"], "addend_lo needs addend (the wrapper's contract)"
    return d


def describe(d):
    return json.dumps({k: v for k, v in d.items() if v not in (False, 0) and _DEFAULTS.get(k, None) != v}, sort_keys=True)


def gm(n):
    """fp32 accumulation of n terms (n: a number or a tensor of counts)."""
    if torch.is_tensor(n):
        return NG * GC.GAMMA * U * torch.sqrt(n.double().clamp_min(1.0))
    return NG * GC.gamma(n)


# ---------------------------------------------------------------- the dispatch rules of csrc/norm.hip as data

def gn_geom(B, HW, C, target=512):
    """GNGeom gn_geom(B, HW, C) with g_gn_target_wgs = target."""
    TX = C // 8
    R = max(256 // TX, 1)
    rows = (HW * B + target - 1) // target
    rows = (rows + R - 1) // R * R
    rows = max(rows, 4 * R)
    return dict(TX=TX, R=R, threads=TX * R, nchunk=(HW + rows - 1) // rows, rows_per_chunk=rows)


def gn_slab_geom(HW, C, G):
    """GNSlab gn_slab_geom: None where the two-launch path runs."""
    Cg = C // G
    if Cg % 2:
        return None
    ce = 4 if Cg % 4 == 0 else 2
    if HW * Cg > 65536 or Cg > 2048:
        return None
    if ce == 2 and HW > 1024:
        return None
    total = HW * (Cg // ce)
    cpr = Cg // ce
    nt = 256 if total <= 256 * 8 else 1024
    nch = 1
    while nch * nt < total:
        nch *= 2
    return dict(nt=nt, nch=nch, ce=ce, cpr=cpr, magic=0 if cpr == 1 else ((1 << 32) + cpr - 1) // cpr, total=total)


def gn_workspace_bytes(B, HW, C, G, target=512):
    return (B * gn_geom(B, HW, C, target)["nchunk"] * G * 2 + B * G * 2) * 4


def affine_grad_blocks(rows, col_tiles, groups):
    """(row blocks, rows_per_block) of affine_grad_blocks."""
    cdiv = lambda a, b: (a + b - 1) // b
    splits = max(1, min(cdiv(1024, col_tiles * groups), cdiv(rows, 128)))
    rpb = cdiv(cdiv(rows, splits), 32) * 32
    return cdiv(rows, rpb), rpb


def ln_nv(C):
    return 1 if C <= 512 else 2 if C <= 1024 else 4 if C <= 2048 else 8


def uses_slab(d):
    return bool(d["slab"]) and gn_slab_geom(d["HW"], d["C"], d["G"]) is not None


def selected(d):
    """the kernel instantiation (and workgroup size) a descriptor launches."""
    k = d["kind"]
    if k in ("gn_fwd", "gn_bwd"):
        if uses_slab(d):
            s = gn_slab_geom(d["HW"], d["C"], d["G"])
            return ("gn_slab_" + k[3:], s["nch"], s["ce"], s["nt"])
        return ("gn_chunk_" + k[3:],)
    if k == "gn_affine":
        return ("affine", True)
    if k == "ln_affine":
        return ("affine", False)
    hl = d["x_lo"] if k == "ln_fwd" else (d["x_lo"] or d["addend_lo"] or d["want_lo"])
    return (k, ln_nv(d["C"]), bool(hl))


def all_instantiations():
    """every (kernel, template arguments, workgroup size) the entry points of csrc/norm.hip can launch: HCP_GN_SLAB_SWITCH x the two
    workgroup sizes gn_slab_geom picks (256 threads: up to 8 chunks; 1024: from 4 up), the HCP_LN_* macros, the row-chunk pairs, the
    affine-gradient kernel in both forms."""
    out = {("gn_chunk_fwd",), ("gn_chunk_bwd",), ("affine", True), ("affine", False)}
    for k in ("gn_slab_fwd", "gn_slab_bwd"):
        for ce, top in ((4, 16), (2, 32)):
            out |= {(k, nch, ce, 256) for nch in (1, 2, 4, 8)}
            out |= {(k, nch, ce, 1024) for nch in (4, 8, 16, 32) if nch <= top}
    for k in ("ln_fwd", "ln_bwd"):
        out |= {(k, nv, hl) for nv in (1, 2, 4, 8) for hl in (False, True)}
    return out


# ---------------------------------------------------------------- operands

def _affine_params(g, C):
    ga = g.randn(C) * 0.5 + 1.0
    ga = ga * (torch.rand(C, generator=g.g, device=g.dev) < 0.5).float().mul(2).sub(1)
    ga[3::7] *= 2.0 ** -10
    be = g.randn(C) * 0.3
    be[1::5] -= 4.0
    return ga, be


def _rows(g, *shape):
    """N(0,1) with one scale 2^U(-4,4) per row (all axes but the last)."""
    n = math.prod(shape[:-1])
    return (g.randn(*shape) * g.scales(n, -4, 4).view(*shape[:-1], 1)).to(BF)


def _spread(g, n):
    """(std, mean) of n populations: std 2^U(-4,4), mean 0 .. 40 std of either sign."""
    std = g.scales(n, -4, 4)
    m = torch.rand(n, generator=g.g, device=g.dev) ** 2 * 40.0
    sign = (torch.rand(n, generator=g.g, device=g.dev) < 0.5).float() * 2 - 1
    return std, std * m * sign


def split_hi_lo(v):
    hi = v.to(BF)
    return hi, (v - hi.float()).to(BF)


def make_operands(d, device):
    g = GC._Gen(d, device)
    o = {}
    if d["kind"] in GN_KINDS:
        B, HW, C, G = d["B"], d["HW"], d["C"], d["G"]
        std, mean = _spread(g, B * G)
        o["x"] = (g.randn(B, HW, G, C // G) * std.view(B, 1, G, 1) + mean.view(B, 1, G, 1)).view(B, HW, C).to(BF)
        o["gamma"], o["beta"] = _affine_params(g, C)
        if d["kind"] != "gn_fwd":
            o["dy"] = _rows(g, B, HW, C)
        if d["kind"] == "gn_bwd" and d["addend"]:
            o["addend"] = _rows(g, B, HW, C)
    else:
        M, C = d["M"], d["C"]
        std, mean = _spread(g, M)
        v = g.randn(M, C) * std.view(M, 1) + mean.view(M, 1)
        if d["x_lo"]:
            o["x"], o["x_lo"] = split_hi_lo(v)
        else:
            o["x"] = v.to(BF)
        o["gamma"], o["beta"] = _affine_params(g, C)
        if d["kind"] != "ln_fwd":
            o["dy"] = _rows(g, M, C)
        if d["kind"] == "ln_bwd" and d["addend"]:
            a = g.randn(M, C) * g.scales(M, -4, 4).view(M, 1)
            if d["addend_lo"]:
                o["addend"], o["addend_lo"] = split_hi_lo(a)
            else:
                o["addend"] = a.to(BF)
    if d["kind"] in ("gn_affine", "ln_affine"):
        o["dg0"], o["db0"] = g.randn(d["C"]), g.randn(d["C"])
    return o


# ---------------------------------------------------------------- running the wrappers

def run(d, ops):
    from hcp_diffusion_amd import kernels as K
    kind = d["kind"]
    hooks = kind in GN_KINDS and (not d["slab"] or d["target"] != 512)
    before = {k: v.clone() for k, v in ops.items()}
    real_empty, real_empty_like = torch.empty, torch.empty_like
    taken = []

    def poisoned_empty(*a, **kw):
        t = real_empty(*a, **kw)
        taken.append(t)
        return t.fill_(fill) if t.is_floating_point() else t

    def poisoned_empty_like(t, **kw):
        return real_empty_like(t, **kw).fill_(fill)
    fill = float("nan")
    outs = {}

    def workspace():
        """the GroupNorm workspace among the buffers taken so far: the last flat fp32 one of exactly the workspace's size."""
        n = max(gn_workspace_bytes(d["B"], d["HW"], d["C"], d["G"], d["target"]), 4) // 4
        ws = [t for t in taken if t.dtype == torch.float32 and t.dim() == 1 and t.numel() == n]
        assert ws, f"{describe(d)}: the wrapper took no workspace of {n} floats"
        return ws[-1]
    K.torch.empty, K.torch.empty_like = poisoned_empty, poisoned_empty_like
    try:
        if hooks:
            if not d["slab"]:
                K.lib().hcp_debug_set_gn_target(-1)
            K.lib().hcp_debug_set_gn_target(d["target"])
        if kind in GN_KINDS:
            outs["y"], outs["stats"] = K.groupnorm_fwd(ops["x"], ops["gamma"], ops["beta"], d["G"], d["eps"], d["silu"])
            outs["ws_fwd"] = workspace()
            del taken[:]
            if kind == "gn_bwd":
                outs["dx"] = K.groupnorm_bwd(ops["x"], ops["dy"], ops["gamma"], ops["beta"], outs["stats"], d["G"], d["silu"],
                                             addend=ops.get("addend"))
                outs["ws_bwd"] = workspace()
            elif kind == "gn_affine":
                outs["dgamma"], outs["dbeta"] = ops["dg0"].clone(), ops["db0"].clone()
                K.groupnorm_affine_grad(ops["x"], ops["dy"], ops["gamma"], ops["beta"], outs["stats"], d["G"], d["silu"],
                                        outs["dgamma"], outs["dbeta"])
        else:
            outs["y"], outs["stats"] = K.layernorm_fwd(ops["x"], ops["gamma"], ops["beta"], d["eps"], x_lo=ops.get("x_lo"))
            if kind == "ln_bwd":
                r = K.layernorm_bwd(ops["x"], ops["dy"], ops["gamma"], outs["stats"], addend=ops.get("addend"), x_lo=ops.get("x_lo"),
                                    addend_lo=ops.get("addend_lo"), want_lo=d["want_lo"])
                outs["dx"], outs["dx_lo"] = r if d["want_lo"] else (r, None)
            elif kind == "ln_affine":
                outs["dgamma"], outs["dbeta"] = ops["dg0"].clone(), ops["db0"].clone()
                K.layernorm_affine_grad(ops["x"], ops["dy"], outs["stats"], outs["dgamma"], outs["dbeta"])
    finally:
        K.torch.empty, K.torch.empty_like = real_empty, real_empty_like
        if hooks:
            K.lib().hcp_debug_set_gn_target(-2)
            K.lib().hcp_debug_set_gn_target(512)
    for k, v in ops.items():
        same = torch.equal(v.view(torch.int16 if v.dtype == BF else torch.int32), before[k].view(torch.int16 if v.dtype == BF else torch.int32))
        assert same, f"{describe(d)}: the launch changed its input {k}"
    return outs


# ---------------------------------------------------------------- float64 references and bounds

def _sigmoid(z):
    s = torch.sigmoid(z)
    return s, (1 - s) * (EXP_REL + 2 * U * z.abs()) + 2 * U


def _silu(z, e_z):
    s, es = _sigmoid(z)
    sp = s * (1 + z * (1 - s))
    ref = z * s
    return ref, sp.abs() * e_z + ref.abs() * (es + 2 * U)


def _silu_grad(z, e_z):
    s, es = _sigmoid(z)
    sp = s * (1 + z * (1 - s))
    return sp, 0.5 * e_z + es * s * (1 + z.abs()) + 4 * U * (s + z.abs() * s * (1 - s))


def _dz(d, xh, e_xh, ga, be, dy):
    """(dz, e_dz) = dy [silu'(xh gamma + beta)] from xh and its error."""
    if not d["silu"]:
        return dy, torch.zeros_like(dy)
    z = xh * ga + be
    e_z = 3 * U * ((xh * ga).abs() + be.abs()) + ga.abs() * e_xh
    sp, e_sp = _silu_grad(z, e_z)
    dz = dy * sp
    return dz, dy.abs() * e_sp + U * dz.abs()


def _bf16(name, got, ref, pre, dims):
    it = Item(name, got.double().reshape(ref.shape), ref, pre + 2.0 ** -8 * (ref.abs() + pre))
    it.dims = dims
    return it


def _f32(name, got, ref, bound, dims):
    it = Item(name, got.double().reshape(ref.shape), ref, bound)
    it.dims = dims
    return it


def _chunks(d, t4):
    """[B, HW, G, Cg] -> ([B, nchunk, rows_per_chunk, G, Cg] zero-padded, counts [1, nchunk, 1] of live elements per (chunk, group))."""
    B, HW, G, Cg = t4.shape
    ge = gn_geom(B, HW, d["C"], d["target"])
    nc, rpc = ge["nchunk"], ge["rows_per_chunk"]
    t = F.pad(t4, (0, 0, 0, 0, 0, nc * rpc - HW)).view(B, nc, rpc, G, Cg)
    rows = torch.tensor([min(rpc, HW - c * rpc) for c in range(nc)], dtype=torch.float64, device=t4.device)
    return t, (rows * Cg).view(1, nc, 1)


GN_DIMS = ("batch", "row", "group", "channel_in_group")
WS_DIMS = ("batch", "chunk", "group")


def _gn_fwd_items(d, ops, outs):
    B, HW, C, G, eps = d["B"], d["HW"], d["C"], d["G"], d["eps"]
    Cg, n = C // G, HW * (C // G)
    x = ops["x"].double().view(B, HW, G, Cg)
    ga, be = ops["gamma"].double().view(1, 1, G, Cg), ops["beta"].double().view(1, 1, G, Cg)
    mean = x.mean((1, 3))
    M2 = ((x - mean.view(B, 1, G, 1)) ** 2).sum((1, 3))
    A1 = x.abs().sum((1, 3))
    items = []
    if uses_slab(d):
        e_mean = gm(n) * A1 / n + 2 * U * mean.abs()
        e_M2 = (gm(n) + 4 * U) * M2 + n * e_mean ** 2
    else:
        xc, cnt = _chunks(d, x)
        nc = xc.shape[1]
        live = (torch.arange(xc.shape[2], device=x.device).view(1, 1, -1) * Cg < cnt).double().view(1, nc, -1, 1, 1)
        mean_c = xc.sum((2, 4)) / cnt
        M2_c = (((xc - mean_c.view(B, nc, 1, G, 1)) ** 2) * live).sum((2, 4))
        e_mean_c = gm(cnt) * xc.abs().sum((2, 4)) / cnt + 2 * U * mean_c.abs()
        e_M2_c = (3 * gm(cnt) + 6 * U) * (xc ** 2).sum((2, 4))
        ws = outs["ws_fwd"][:B * nc * G * 2].double().view(B, nc, G, 2)
        items += [_f32("ws_mean", ws[..., 0], mean_c, e_mean_c, WS_DIMS), _f32("ws_M2", ws[..., 1], M2_c, e_M2_c, WS_DIMS)]
        dk = (mean_c - mean_c[:, :1]).abs()
        e_mean = (gm(n) + gm(nc)) * A1 / n + 2 * U * mean.abs()
        e_M2 = e_M2_c.sum(1) + (gm(nc) + 4 * U) * (M2 + 2 * (cnt * dk * dk).sum(1)) + 4 * (cnt * dk * (e_mean_c + e_mean_c[:, :1])).sum(1) \
            + n * e_mean ** 2
    rstd = (M2 / n + eps) ** -0.5
    e_rstd = rstd * (0.5 * e_M2 / (M2 + n * eps) + 4 * U)
    st = outs["stats"].double()
    items += [_f32("mean", st[..., 0], mean, e_mean, ("batch", "group")), _f32("rstd", st[..., 1], rstd, e_rstd, ("batch", "group"))]
    mk, rk = st[..., 0].view(B, 1, G, 1), st[..., 1].view(B, 1, G, 1)
    a = rk * ga
    z = x * a + (be - mk * a)
    pre = 4 * U * ((x * a).abs() + (mk * a).abs() + be.abs())
    if d["silu"]:
        z, pre = _silu(z, pre)
    items.append(_bf16("y", outs["y"], z, pre, GN_DIMS))
    return items


def _gn_xh(d, ops, outs):
    B, HW, C, G = d["B"], d["HW"], d["C"], d["G"]
    Cg = C // G
    st = outs["stats"].double()
    x = ops["x"].double().view(B, HW, G, Cg)
    xh = (x - st[..., 0].view(B, 1, G, 1)) * st[..., 1].view(B, 1, G, 1)
    return xh, 3 * U * xh.abs(), st[..., 1].view(B, 1, G, 1)


def _gn_bwd_items(d, ops, outs):
    B, HW, C, G = d["B"], d["HW"], d["C"], d["G"]
    Cg, n = C // G, HW * (C // G)
    ga, be = ops["gamma"].double().view(1, 1, G, Cg), ops["beta"].double().view(1, 1, G, Cg)
    xh, e_xh, rstd = _gn_xh(d, ops, outs)
    dy = ops["dy"].double().view(B, HW, G, Cg)
    dz, e_dz = _dz(d, xh, e_xh, ga, be, dy)
    dxh = dz * ga
    e_dxh = e_dz * ga.abs() + 2 * U * dxh.abs()
    p2 = dxh * xh
    e_p2 = e_dxh * xh.abs() + dxh.abs() * e_xh + U * p2.abs()
    items = []
    nc = 1
    if not uses_slab(d):
        (c1p, cnt), (c2p, _) = _chunks(d, dxh), _chunks(d, p2)
        nc = c1p.shape[1]
        sums = lambda t: _chunks(d, t)[0].sum((2, 4))
        ws = outs["ws_bwd"][:B * nc * G * 2].double().view(B, nc, G, 2)
        items += [_f32("ws_S1", ws[..., 0], c1p.sum((2, 4)), sums(e_dxh) + gm(cnt) * sums(dxh.abs()), WS_DIMS),
                  _f32("ws_S2", ws[..., 1], c2p.sum((2, 4)), sums(e_p2) + gm(cnt) * sums(p2.abs()), WS_DIMS)]
    acc = gm(n) + gm(nc)
    c1 = dxh.sum((1, 3), keepdim=True) / n
    c2 = p2.sum((1, 3), keepdim=True) / n
    e_c1 = (e_dxh.sum((1, 3), keepdim=True) + acc * dxh.abs().sum((1, 3), keepdim=True)) / n + 2 * U * c1.abs()
    e_c2 = (e_p2.sum((1, 3), keepdim=True) + acc * p2.abs().sum((1, 3), keepdim=True)) / n + 2 * U * c2.abs()
    t = dxh - c1 - xh * c2
    e_t = e_dxh + e_c1 + xh.abs() * e_c2 + c2.abs() * e_xh + 3 * U * (dxh.abs() + c1.abs() + (xh * c2).abs())
    ref = rstd * t
    pre = rstd * e_t + 2 * U * ref.abs()
    if d["addend"]:
        ad = ops["addend"].double().view(B, HW, G, Cg)
        ref = ref + ad
        pre = pre + U * (ad.abs() + ref.abs())
    items.append(_bf16("dx", outs["dx"], ref, pre, GN_DIMS))
    return items


def _affine_items(d, ops, outs, xh, e_xh, dz, e_dz, rows, nblocks):
    """dgamma / dbeta over every axis but the last of [.., C]-shaped xh / dz."""
    C = d["C"]
    flat = lambda t: t.reshape(-1, C)
    p = flat(dz * xh)
    e_p = flat(e_dz * xh.abs() + dz.abs() * e_xh) + U * p.abs()
    dg0, db0 = ops["dg0"].double(), ops["db0"].double()
    acc = gm(rows) + U * nblocks
    return [_f32("dgamma", outs["dgamma"], dg0 + p.sum(0), e_p.sum(0) + acc * p.abs().sum(0) + U * nblocks * dg0.abs(), ("channel",)),
            _f32("dbeta", outs["dbeta"], db0 + flat(dz).sum(0), flat(e_dz).sum(0) + acc * flat(dz).abs().sum(0) + U * nblocks * db0.abs(),
                 ("channel",))]


def _gn_affine_items(d, ops, outs):
    B, HW, C, G = d["B"], d["HW"], d["C"], d["G"]
    Cg = C // G
    ga, be = ops["gamma"].double().view(1, 1, G, Cg), ops["beta"].double().view(1, 1, G, Cg)
    xh, e_xh, _ = _gn_xh(d, ops, outs)
    dz, e_dz = _dz(d, xh, e_xh, ga, be, ops["dy"].double().view(B, HW, G, Cg))
    splits, _ = affine_grad_blocks(HW, (C + 63) // 64, B)
    v = lambda t: t.reshape(B, HW, C)
    return _affine_items(d, ops, outs, v(xh), v(e_xh), v(dz), v(e_dz), B * HW, splits * B)


def _ln_x(ops):
    x = ops["x"].double()
    if "x_lo" in ops:
        return x + ops["x_lo"].double(), U * x.abs()
    return x, torch.zeros_like(x)


def _ln_fwd_items(d, ops, outs):
    M, C, eps = d["M"], d["C"], d["eps"]
    x, e_x = _ln_x(ops)
    ga, be = ops["gamma"].double(), ops["beta"].double()
    mean = x.mean(1)
    M2 = ((x - mean[:, None]) ** 2).sum(1)
    e_mean = gm(C) * x.abs().sum(1) / C + 2 * U * mean.abs() + e_x.sum(1) / C
    e_M2 = (gm(C) + 4 * U) * M2 + C * e_mean ** 2 + 2 * ((x - mean[:, None]).abs() * e_x).sum(1)
    rstd = (M2 / C + eps) ** -0.5
    e_rstd = rstd * (0.5 * e_M2 / (M2 + C * eps) + 4 * U)
    st = outs["stats"].double()
    items = [_f32("mean", st[:, 0], mean, e_mean, ("row",)), _f32("rstd", st[:, 1], rstd, e_rstd, ("row",))]
    xh = (x - st[:, :1]) * st[:, 1:]
    ref = xh * ga + be
    pre = 4 * U * ((xh * ga).abs() + be.abs()) + e_x * st[:, 1:] * ga.abs()
    items.append(_bf16("y", outs["y"], ref, pre, ("row", "channel")))
    return items


def _ln_xh(ops, outs):
    x, e_x = _ln_x(ops)
    st = outs["stats"].double()
    xh = (x - st[:, :1]) * st[:, 1:]
    return xh, 3 * U * xh.abs() + e_x * st[:, 1:], st[:, 1:]


def _ln_bwd_items(d, ops, outs):
    C = d["C"]
    xh, e_xh, rstd = _ln_xh(ops, outs)
    dxh = ops["dy"].double() * ops["gamma"].double()
    e_dxh = U * dxh.abs()
    p2 = dxh * xh
    e_p2 = e_dxh * xh.abs() + dxh.abs() * e_xh + U * p2.abs()
    c1, c2 = dxh.mean(1, keepdim=True), p2.mean(1, keepdim=True)
    e_c1 = (e_dxh.sum(1, keepdim=True) + gm(C) * dxh.abs().sum(1, keepdim=True)) / C + 2 * U * c1.abs()
    e_c2 = (e_p2.sum(1, keepdim=True) + gm(C) * p2.abs().sum(1, keepdim=True)) / C + 2 * U * c2.abs()
    t = dxh - c1 - xh * c2
    e_t = e_dxh + e_c1 + xh.abs() * e_c2 + c2.abs() * e_xh + 3 * U * (dxh.abs() + c1.abs() + (xh * c2).abs())
    ref = rstd * t
    pre = rstd * e_t + 2 * U * ref.abs()
    for k in ("addend", "addend_lo"):
        if k in ops:
            ref = ref + ops[k].double()
            pre = pre + U * (ops[k].double().abs() + ref.abs())
    dims = ("row", "channel")
    items = [_bf16("dx", outs["dx"], ref, pre, dims)]
    if d["want_lo"]:
        hi, lo = outs["dx"].double(), outs["dx_lo"].double()
        items.append(_f32("dx+dx_lo", hi + lo, ref, pre + 2.0 ** -17 * (ref.abs() + pre), dims))
        items.append(_f32("|dx_lo| beyond half an ulp of dx", (lo.abs() - 2.0 ** -8 * hi.abs()).clamp_min(0), torch.zeros_like(ref),
                          torch.zeros_like(ref), dims))
    return items


def _ln_affine_items(d, ops, outs):
    M, C = d["M"], d["C"]
    xh, e_xh, _ = _ln_xh(ops, outs)
    dz = ops["dy"].double()
    splits, _ = affine_grad_blocks(M, (C + 63) // 64, 1)
    return _affine_items(d, ops, outs, xh, e_xh, dz, torch.zeros_like(dz), M, splits)


def references(d, ops, outs):
    """the compared items.  A backward / affine-gradient descriptor also carries its forward's items (the launch that made its stats)."""
    k = d["kind"]
    if k in GN_KINDS:
        items = _gn_fwd_items(d, ops, outs)
        return items + (_gn_bwd_items(d, ops, outs) if k == "gn_bwd" else _gn_affine_items(d, ops, outs) if k == "gn_affine" else [])
    items = _ln_fwd_items(d, ops, outs)
    return items + (_ln_bwd_items(d, ops, outs) if k == "ln_bwd" else _ln_affine_items(d, ops, outs) if k == "ln_affine" else [])


def _ratio(it):
    err = (it.got - it.ref).abs()
    r = torch.where(it.bound > 0, err / it.bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r).max())


def measure(d, ops, outs, g=1.0):
    """{item: worst err / bound} with NG = g, without asserting (NaN counts as infinite)."""
    global NG
    keep, NG = NG, g
    try:
        return {it.name: _ratio(it) for it in references(d, ops, outs)}
    finally:
        NG = keep


def check(d, ops, outs, ratios=None):
    """every element of every item within its bound, else AssertionError naming the worst element; returns the worst err / bound
    (`ratios`: a dict that collects the worst per item)."""
    worst = 0.0
    for it in references(d, ops, outs):
        r = GC.compare(d, [it], describe=describe)
        if ratios is not None:
            ratios[it.name] = max(ratios.get(it.name, 0.0), r)
        worst = max(worst, r)
    return worst
