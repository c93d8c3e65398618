"""TEST HELPER: element-wise float64 check of one attention launch (kernels.attention_fwd / attention_bwd), described by the plain dict
that kernels.LAUNCHES records (kind attn_fwd | attn_bwd; B, H, Nq, Nk, D; batch and row strides of q, k, v — the gradients share them;
layout separate | qkv | q+kv; key_bias and its batch stride; causal; prescaled; scale, 0 = the default D^-0.5).

    ops = make_operands(desc, device)          # seeded from a hash of the descriptor
    outs = run(desc, ops)                      # the wrapper, into NaN-poisoned outputs inside sentinel-filled buffers
    ratio = check(desc, ops, outs)             # |out - ref| <= bound at every element, else AssertionError; returns max err / bound

Operands.  q and k rows N(0,1) with per-row scales 2^U(-2,2); q also carries a per-head scale 2^[-3, 0] (evenly spaced over the heads,
shuffled), so the score spread of a (row, head) runs from ~2^-7 (a flat softmax) to ~16 (one key holds > 0.9 of the row): an error in a
quiet head or row cannot hide behind a loud one.  v and dO rows N(0,1) with per-row scales 2^U(-4,4).  A key bias is 0 / -10000 in a
pattern that differs per batch row, masks the end of the ragged last key tile and never key 0.  q | k | v that share a buffer are
slices of ONE buffer whose other columns hold random data; so does the bias buffer beyond Nk.  make_operands asserts from the float64
scores that no row's maximum is more than 70 nats above the maximum of its first 64 keys: the plain d = 40 forward then never takes its
exp2-overflow re-run (that path has its own directed test, test_attention_lsum_overflow_rerun, which calls check on its operands).

Running.  Every buffer the wrapper takes from torch.empty / torch.empty_like (o, lse, delta; dq / dk / dv of the out=None form, which
run(wrapper_alloc=True) uses for contiguous operands) is NaN-poisoned through patched allocators; otherwise dq / dk / dv are
slices of buffers laid out like the inputs', NaN inside the slices and the sentinel bit pattern everywhere else (the neighbouring
columns = another layer's gradient in the joint buffer, the rows between batch strides, one trailing guard row), which must be intact
afterwards; the shared workspace holds NaN bit patterns before each backward.

Reference.  float64 torch on the operands' device, one (batch, head) at a time, from the bf16 inputs as given (prescaled: from the
scaled bf16 tensor; dQ is the gradient with respect to that tensor).  The backward reference uses the kernel's own o and lse where the
kernel reads them — delta = rowsum(dO o), P = exp(S - lse) — so a legitimate last-bit difference of the forward does not fail the
backward; o and lse themselves are the forward's items.  delta is scratch the wrapper does not return: a wrong delta shows in dQ and dK.

Bound per element, a sum of named terms (U = 2^-24, gamma(n) = GAMMA sqrt(n) U of gemm_check; p = the exact probabilities):
  scores        E_qk = gamma(D) sum_d |q||k| scale  +  4 U (|S| + |max_k S| + 16 + |lse|)  +  2^-22: the fp32 MFMA accumulation of q.k, the
                fp32 subtraction of the reference maximum / lse and the multiply in front of the exponential, and one hardware exp2
                (v_exp_f32: 1 ulp, csrc/hcp_device.h "v_exp_f32 and v_rcp_f32 (1 ulp each)"; 2^-22 allows 2).  E is a relative error
                of the unnormalised p; through the softmax: lse  sum_k p E,   o  sum_k p E |v| + |o| sum_k p E.
  P rounding    P enters the PV MFMA as bf16: G 2^-8 sqrt(sum_k (p v)^2) on o.  At d = 40 the row sum comes out of that same MFMA
                (VAR_ONES): G 2^-8 sqrt(sum_k p^2) on lse and |o| times that on o.  Root-sum-square, not sum_k p |v|: at Nk = 4096 the
                worst-case sum is as large as a dropped key tile.
  PV            gamma(Nk) sum_k p |v|  (fp32 accumulation, rescales included);  lse arithmetic 4 U (|max S| + 16 + |lse| + 1)
  backward      P: E (with the kernel's lse).  dP - delta: gamma(D) (sum |dO||v| + sum |dO||o|) + 2 U (|dP| + |delta|)  =: e_dp.
                dS = P (dP - delta): |dS| (E + U) + P e_dp  =: e_dS.   dV: sum_q P E |dO| + G 2^-8 sqrt(sum_q (P dO)^2) + gamma(Nq) sum P |dO|;
                dQ: c (sum_k e_dS |k| + G 2^-8 sqrt(sum_k (dS k)^2) + gamma(Nk) sum |dS||k|) + U |dQ|, c = scale (ln 2 for prescaled q);
                dK alike over q, gamma(Nq).  The query-split dK / dV: U ceil(Nq / 64) sum |.| for the fp32 slab additions (at most one
                slab per query tile).
  output        2^-8 |ref| for the bf16 outputs, 0 for lse.

G is the one free constant (a root-sum-square is a typical size, not a maximum: 2^-8 sqrt(sum x^2) is about 2.5 standard deviations
of a sum of round-to-nearest bf16 errors, and the largest of 10^7 elements sits above 5).  Measured on MI355X, kernel against this float64
reference, over the 72 recorded launches of tests/golden/attention_launches.json and the 24 synthesized ones (measure(g=1); the GPU report test of
tests/test_attention_launches.py prints these figures at every run), worst err / bound with G = 1: o 1.85, lse 1.98,
dq 1.87, dk 1.76, dv 1.94 (every launch between 1.3 and 2.0, whatever its head dim, layout or mask: the rounding statistic, no outlier).
G = 8 is the smallest power of two that leaves the worst ratio at or below 0.5 — with it, over the recorded and the synthesized
launches: o 0.406, lse 0.252, dq 0.406, dk 0.372, dv 0.379 (the terms G does not scale keep G = 4 above 0.5: 0.406 at G = 8 means ~0.8).
The interpreter passes under the same G.  Mutation test (tests/test_attention_launches.py): every listed fault is caught with G = 8; the
old gates (tensor-max relerr < 1e-2 / 2e-2, lse within 2e-2) pass last_key_of_ragged_tile_dropped, delta_from_wrong_row and
dk_missing_ln2_in_quietest_head."""
import math

import torch

import gemm_check as GC
from gemm_check import BF, U, Item, gamma

G = 8.0
EXP_REL = 2.0 ** -22
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
OVERFLOW_MARGIN = 70.0           # nats; exp2 overflows 88 nats above the first tile's maximum (row sums of 4096 keys: ~80)
REF_SLACK = 16.0                 # nats the forward's reference may lag behind the row maximum (lazy rescale: 2^6, row sums up to 2^20)


def scale_of(d):
    return d["scale"] if d.get("scale") else d["D"] ** -0.5


_DEFAULTS = dict(layout="separate", key_bias=False, kb_bs=0, causal=False, prescaled=False, scale=0.0)


def desc(kind, **kw):
    """a descriptor with the flags a hand-built call leaves at their defaults and contiguous strides."""
    d = dict(_DEFAULTS, kind=kind)
    d.update(kw)
    C = d["H"] * d["D"]
    for t, n in (("q", d["Nq"]), ("k", d["Nk"]), ("v", d["Nk"])):
        d.setdefault(t + "_rs", C)
        d.setdefault(t + "_bs", n * d[t + "_rs"])
    if d["key_bias"] and not d["kb_bs"]:
        d["kb_bs"] = d["Nk"]
    return d


def describe(d):
    return GC.json.dumps({k: v for k, v in d.items() if v not in (False, 0, 0.0)}, sort_keys=True)


# ---------------------------------------------------------------- operands

class Slab:
    """One flat bf16 buffer holding [B, N, width] views with batch stride bs and row stride rs, plus one trailing guard row."""
    def __init__(self, B, N, bs, rs, device):
        assert bs >= N * rs and rs % 8 == 0 and bs % 8 == 0, (B, N, bs, rs)
        self.B, self.N, self.bs, self.rs = B, N, bs, rs
        self.flat = torch.empty(B * bs + rs, dtype=BF, device=device)
        self.owned = torch.zeros(B * bs + rs, dtype=torch.bool, device=device)

    def view(self, off, width):
        assert off + width <= self.rs
        self.owned.as_strided((self.B, self.N, width), (self.bs, self.rs, 1), off).fill_(True)
        return self.flat.as_strided((self.B, self.N, width), (self.bs, self.rs, 1), off)

    def poison(self, fill):
        self.flat.view(torch.int16).fill_(GC.SENTINEL16)
        self.flat[self.owned] = fill

    def intact(self):
        """index of the first element outside the owned views that no longer holds the sentinel, or None."""
        bad = (self.flat.view(torch.int16) != GC.SENTINEL16) & ~self.owned
        if not bool(bad.any()):
            return None
        i = int(torch.nonzero(bad)[0])
        b, r = divmod(i, self.bs)
        return dict(batch=b, row=r // self.rs, col=r % self.rs) if b < self.B else dict(guard_row_col=i - self.B * self.bs)


def _slabs(d, device):
    """(slabs, (q, k, v) views) laid out as the descriptor says: qkv = the column thirds of one buffer, q+kv = k | v neighbours in one
    buffer (centred in the row: the joint K/V projection has other layers' columns on both sides), separate = three buffers."""
    B, Nq, Nk, C = d["B"], d["Nq"], d["Nk"], d["H"] * d["D"]
    if d["layout"] == "qkv":
        assert Nq == Nk and d["q_rs"] == d["k_rs"] == d["v_rs"] >= 3 * C and d["q_bs"] == d["k_bs"] == d["v_bs"], d
        s = Slab(B, Nq, d["q_bs"], d["q_rs"], device)
        off = (d["q_rs"] - 3 * C) // 16 * 8
        return [s], (s.view(off, C), s.view(off + C, C), s.view(off + 2 * C, C))
    sq = Slab(B, Nq, d["q_bs"], d["q_rs"], device)
    q = sq.view((d["q_rs"] - C) // 16 * 8, C)
    if d["layout"] == "q+kv":
        assert d["k_rs"] == d["v_rs"] >= 2 * C and d["k_bs"] == d["v_bs"], d
        s = Slab(B, Nk, d["k_bs"], d["k_rs"], device)
        off = (d["k_rs"] - 2 * C) // 16 * 8
        return [sq, s], (q, s.view(off, C), s.view(off + C, C))
    sk, sv = Slab(B, Nk, d["k_bs"], d["k_rs"], device), Slab(B, Nk, d["v_bs"], d["v_rs"], device)
    return [sq, sk, sv], (q, sk.view((d["k_rs"] - C) // 16 * 8, C), sv.view((d["v_rs"] - C) // 16 * 8, C))


def key_bias_of(d, g):
    """fp32 [B, Nk] view (batch stride kb_bs) of 0 / -10000: a pattern per batch row, the end of the last key tile masked, key 0 never."""
    B, Nk = d["B"], d["Nk"]
    base = g.randn(B, max(d["kb_bs"], Nk)) * 5.0              # beyond Nk: values that would visibly change a row that read them
    j = torch.arange(Nk, device=g.dev)[None, :]
    b = torch.arange(B, device=g.dev)[:, None]
    masked = ((j * 7 + b * 3) % 5 == 2) | (j >= Nk - 2 - b % 4)
    masked[:, 0] = False
    base[:, :Nk] = masked.float() * -10000.0
    return base[:, :Nk]


def masked_scores(d, q, k, bias_row):
    """float64 (S, sum_d |q||k| in S's units) of one (batch, head): natural-log scores with bias and causal mask applied."""
    if d["prescaled"]:
        c = LN2
    else:
        c = scale_of(d)
    S = c * (q @ k.T)
    sabs = c * (q.abs() @ k.abs().T)
    if bias_row is not None:
        S = S + bias_row[None, :]
    if d["causal"]:
        n = S.shape[0]
        S = S.masked_fill(torch.ones(n, n, dtype=torch.bool, device=S.device).triu(1), -math.inf)
    return S, sabs


def _pairs(d):
    return [(b, h) for b in range(d["B"]) for h in range(d["H"])]


def _head(t, b, h, D):
    return t[b, :, h * D:(h + 1) * D].double()


def make_operands(d, device):
    g = GC._Gen(d, device)
    B, H, Nq, Nk, D = d["B"], d["H"], d["Nq"], d["Nk"], d["D"]
    C = H * D
    assert not d["causal"] or Nq == Nk
    slabs, (q, k, v) = _slabs(d, device)
    for s in slabs:
        s.flat.copy_(g.randn(s.flat.numel()).to(BF))
    hs = torch.exp2(torch.linspace(-3.0, 0.0, H, device=g.dev) if H > 1 else torch.full((1,), -1.0, device=g.dev))
    hs = hs[torch.randperm(H, generator=g.g, device=g.dev)]
    qf = g.randn(B, Nq, H, D) * g.scales(B * Nq, -2, 2).view(B, Nq, 1, 1) * hs.view(1, 1, H, 1)
    if d["prescaled"]:
        qf = qf * (scale_of(d) * LOG2E)
    q.copy_(qf.view(B, Nq, C).to(BF))
    k.copy_((g.randn(B, Nk, H, D) * g.scales(B * Nk, -2, 2).view(B, Nk, 1, 1)).view(B, Nk, C).to(BF))
    v.copy_((g.randn(B, Nk, C) * g.scales(B * Nk, -4, 4).view(B, Nk, 1)).to(BF))
    o = dict(q=q, k=k, v=v)
    if d["kind"] == "attn_bwd":
        o["do"] = (g.randn(B, Nq, C) * g.scales(B * Nq, -4, 4).view(B, Nq, 1)).to(BF)
    if d["key_bias"]:
        o["key_bias"] = key_bias_of(d, g)
    if not (d["key_bias"] or d["causal"]):                    # the plain forward must stay off its overflow re-run
        worst = 0.0
        for b, h in _pairs(d):
            S, _ = masked_scores(d, _head(q, b, h, D), _head(k, b, h, D), None)
            worst = max(worst, float((S.amax(1) - S[:, :64].amax(1)).max()))
        assert worst < OVERFLOW_MARGIN, f"operands of {describe(d)} would take the exp2-overflow re-run ({worst:.1f} nats above the first tile)"
    return o


# ---------------------------------------------------------------- running the wrapper

def run(d, ops, fill=float("nan"), wrapper_alloc=False):
    """wrapper_alloc: a backward whose q / k / v are contiguous is called with out=None, the form the unpacked attention module uses
    (ops._AttentionFn): dq / dk / dv then come from the wrapper's own torch.empty_like, poisoned like the other allocations."""
    from hcp_diffusion_amd import kernels as K
    dev = ops["q"].device
    H = d["H"]
    real_empty = torch.empty

    def poisoned_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(fill) if t.is_floating_point() else t
    kw = dict(scale=scale_of(d), key_bias=ops.get("key_bias"), causal=d["causal"], q_prescaled=d["prescaled"])
    outs = {}
    real_empty_like = torch.empty_like
    K.torch.empty = poisoned_empty
    K.torch.empty_like = lambda t, **k2: real_empty_like(t, **k2).fill_(fill)
    try:
        outs["o"], outs["lse"] = K.attention_fwd(ops["q"], ops["k"], ops["v"], H, **kw)
        if d["kind"] == "attn_bwd" and wrapper_alloc and all(ops[n].is_contiguous() for n in "qkv"):
            K._workspace(ops["q"]).view(torch.int32).fill_(-1)
            outs["dq"], outs["dk"], outs["dv"] = K.attention_bwd(ops["q"], ops["k"], ops["v"], outs["o"], ops["do"], outs["lse"], H, **kw)
        elif d["kind"] == "attn_bwd":
            slabs, grads = _slabs(d, dev)
            for s in slabs:
                s.poison(fill)
            K._workspace(ops["q"]).view(torch.int32).fill_(-1)                  # 0xFFFFFFFF: NaN as fp32
            outs["dq"], outs["dk"], outs["dv"] = K.attention_bwd(ops["q"], ops["k"], ops["v"], outs["o"], ops["do"], outs["lse"], H,
                                                                 out=grads, **kw)
            outs["slabs"] = slabs
    finally:
        K.torch.empty = real_empty
        K.torch.empty_like = real_empty_like
    return outs


def workspace_written(t):
    """True when the launch before left values in the head of the shared workspace that run() filled with NaN bit patterns: the
    query-split dK / dV pass stores its first fp32 slab there, no other attention kernel touches it."""
    from hcp_diffusion_amd import kernels as K
    return bool((K._workspace(t).view(torch.int32)[:4096] != -1).any())


# ---------------------------------------------------------------- float64 references and bounds

def _finite_abs(S):
    return torch.where(torch.isfinite(S), S.abs(), torch.zeros_like(S))


def forward_pair(d, q, k, v, bias_row):
    """(o_ref, o_pre, lse_ref, lse_bound) of one (batch, head); o_pre is the bound before the output rounding."""
    D, Nk = d["D"], k.shape[0]
    S, sabs = masked_scores(d, q, k, bias_row)
    lse = torch.logsumexp(S, 1)
    P = torch.exp(S - lse[:, None])
    o = P @ v
    sa = _finite_abs(S)
    smax = S.amax(1).abs() + REF_SLACK
    E = gamma(D) * sabs + 4 * U * (sa + (smax + lse.abs())[:, None]) + EXP_REL
    W = P * E
    wsum = W.sum(1)
    p2 = (P * P).sum(1).sqrt()
    ones = 1.0 if D == 40 else 0.0                            # the row sum rides on the PV MFMA (bf16 P) at d = 40 only
    lse_b = wsum + ones * G * 2.0 ** -8 * p2 + 4 * U * (smax + lse.abs() + 1.0)
    o_pre = W @ v.abs() + wsum[:, None] * o.abs() + G * 2.0 ** -8 * (((P * P) @ (v * v)).sqrt() + ones * o.abs() * p2[:, None]) \
        + (gamma(Nk) + 4 * U) * (P @ v.abs())
    return o, o_pre, lse, lse_b


def backward_pair(d, q, k, v, do, o_k, lse_k, bias_row):
    """((dq, pre), (dk, pre), (dv, pre)) of one (batch, head) from the kernel's own o and lse."""
    D, Nq, Nk = d["D"], q.shape[0], k.shape[0]
    c = LN2 if d["prescaled"] else scale_of(d)
    S, sabs = masked_scores(d, q, k, bias_row)
    P = torch.exp(S - lse_k[:, None])
    sa = _finite_abs(S)
    E = gamma(D) * sabs + 4 * U * (sa + (S.amax(1).abs() + REF_SLACK + lse_k.abs())[:, None]) + EXP_REL
    dP = do @ v.T
    delta = (do * o_k).sum(1)
    e_dp = gamma(D) * (do.abs() @ v.abs().T + (do.abs() * o_k.abs()).sum(1)[:, None]) + 2 * U * (dP.abs() + delta.abs()[:, None])
    dS = P * (dP - delta[:, None])
    e_dS = dS.abs() * (E + U) + P * e_dp
    slab = U * ((Nq + 63) // 64)
    r = G * 2.0 ** -8
    dv = P.T @ do
    pd = P.T @ do.abs()
    dv_pre = (P * E).T @ do.abs() + r * ((P * P).T @ (do * do)).sqrt() + (gamma(Nq) + slab) * pd
    dq = c * (dS @ k)
    dq_pre = c * (e_dS @ k.abs() + r * ((dS * dS) @ (k * k)).sqrt() + gamma(Nk) * (dS.abs() @ k.abs())) + U * dq.abs()
    dk = c * (dS.T @ q)
    dk_pre = c * (e_dS.T @ q.abs() + r * ((dS * dS).T @ (q * q)).sqrt() + (gamma(Nq) + slab) * (dS.abs().T @ q.abs())) + U * dk.abs()
    return (dq, dq_pre), (dk, dk_pre), (dv, dv_pre)


DIMS = ("batch", "row", "head", "col")


def _bf16_item(name, got, ref, pre, B, H, D):
    it = Item(name, got.double().reshape(B, -1, H, D), ref, pre + 2.0 ** -8 * (ref.abs() + pre))
    it.dims = DIMS
    return it


def references(d, ops, outs, pairs=None):
    """the compared items; `pairs`: a subset of (batch, head) to check (the others' elements are compared with an infinite bound)."""
    B, H, Nq, Nk, D = d["B"], d["H"], d["Nq"], d["Nk"], d["D"]
    dev = ops["q"].device
    full = pairs is None
    pairs = _pairs(d) if full else pairs

    def buf(n, *tail):
        ref = torch.zeros(B, n, *tail, dtype=torch.float64, device=dev)
        return ref, torch.zeros_like(ref) if full else torch.full_like(ref, math.inf)
    bias = ops.get("key_bias")
    if d["kind"] == "attn_fwd":
        (o_r, o_b), (l_r, l_b) = buf(Nq, H, D), buf(H, Nq)
        l_r, l_b = l_r.view(B, H, Nq), l_b.view(B, H, Nq)
        for b, h in pairs:
            o, op, l, lb = forward_pair(d, _head(ops["q"], b, h, D), _head(ops["k"], b, h, D), _head(ops["v"], b, h, D),
                                        bias[b].double() if bias is not None else None)
            o_r[b, :, h], o_b[b, :, h], l_r[b, h], l_b[b, h] = o, op, l, lb
        lse = Item("lse", outs["lse"].double(), l_r, l_b)
        lse.dims = ("batch", "head", "row")
        return [_bf16_item("o", outs["o"], o_r, o_b, B, H, D), lse]
    (q_r, q_b), (k_r, k_b), (v_r, v_b) = buf(Nq, H, D), buf(Nk, H, D), buf(Nk, H, D)
    for b, h in pairs:
        (dq, dqp), (dk, dkp), (dv, dvp) = backward_pair(
            d, _head(ops["q"], b, h, D), _head(ops["k"], b, h, D), _head(ops["v"], b, h, D), _head(ops["do"], b, h, D),
            _head(outs["o"], b, h, D), outs["lse"][b, h].double(), bias[b].double() if bias is not None else None)
        q_r[b, :, h], q_b[b, :, h], k_r[b, :, h], k_b[b, :, h], v_r[b, :, h], v_b[b, :, h] = dq, dqp, dk, dkp, dv, dvp
    return [_bf16_item("dq", outs["dq"], q_r, q_b, B, H, D), _bf16_item("dk", outs["dk"], k_r, k_b, B, H, D),
            _bf16_item("dv", outs["dv"], v_r, v_b, B, H, D)]


def measure(d, ops, outs, pairs=None, g=1.0):
    """{output: worst err / bound} with G = g, without asserting (NaN counts as infinite): how the G = 1 figures of the docstring
    are recorded (tests/test_attention_launches.py prints them next to the ratios under the module's G)."""
    global G
    out = {}
    keep, G = G, g
    try:
        items = references(d, ops, outs, pairs)
    finally:
        G = keep
    for it in items:
        err = (it.got - it.ref).abs()
        r = torch.where(it.bound > 0, err / it.bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        out[it.name] = float(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r).max())
    return out


def check(d, ops, outs, pairs=None, ratios=None):
    """every element within its bound and every sentinel intact, else AssertionError naming batch / head / row / column of the worst
    element; returns the worst err / bound (`ratios`: a dict that collects the worst per output)."""
    worst = 0.0
    for it in references(d, ops, outs, pairs):
        r = GC.compare(d, [it], describe=describe)
        if ratios is not None:
            ratios[it.name] = max(ratios.get(it.name, 0.0), r)
        worst = max(worst, r)
    for s in outs.get("slabs", ()):
        bad = s.intact()
        assert bad is None, f"{describe(d)}: an element outside dq / dk / dv was written (row stride {s.rs}, batch stride {s.bs}): {bad}"
    return worst
