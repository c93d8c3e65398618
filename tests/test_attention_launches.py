"""Every attention launch of the benchmark workloads, the CLIP text encoders and the masked steps, element-wise against float64
(tests/attn_check.py).

CPU: the checker catches each injected fault of a small blocked flash-attention model (mutation test) and the old gates
(tensor-max relerr < 1e-2 / 2e-2, lse within 2e-2) pass several of them; every instantiation the dispatch of csrc/attention.hip can
select runs through the interpreter at a reduced, ragged shape in each layout; the fixture tests/golden/attention_launches.json is
consistent.
GPU: each recorded descriptor at its real shape through the product library's own dispatch, twice with identical bits; one synthesized
descriptor per instantiation no recorded launch selects; a fresh trace equal to the fixture (tools/trace_attention_launches.py)."""
import json
import math
import sys
from pathlib import Path

import pytest
import torch

import attn_check as AC
from hcp_diffusion_amd import kernels as K

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "attention_launches.json"
BF = torch.bfloat16
NAMES = {"sd15", "dreambooth", "controlnet", "sdxl", "clip_l", "clip_bigg", "sd15_masked", "sdxl_masked"}


def load_fixture():
    return json.loads(FIXTURE.read_text()) if FIXTURE.exists() else []


def relerr(a, b):
    a = a.float().cpu(); b = b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# ---------------------------------------------------------------- the dispatch rules of csrc/attention.hip, as data

def cdiv(a, b):
    return (a + b - 1) // b


def variant_of(d):
    return "masked" if (d["key_bias"] or d["causal"]) else "prescaled" if d["prescaled"] else "plain"


def fwd_shapes(D):
    """(rows per wave / 16, waves) pairs run_fwd can launch."""
    return {40: [(1, 4), (2, 4), (1, 8), (2, 8)], 64: [(1, 4), (2, 4)], 80: [(1, 4), (1, 8)], 160: [(1, 4)]}[D]


def bwd_shapes(D):
    """(dQ rows per wave / 16, dK/dV rows per wave / 16) pairs run_bwd can launch."""
    return [(a, b) for a in (1, 2) for b in (1, 2)] if D <= 64 else [(1, 1)]


def selected(d):
    """the instantiations the unforced heuristic picks for a descriptor: run_fwd, or run_bwd + plan_dkv (split: more than one slab)."""
    B, H, Nq, Nk, D = d["B"], d["H"], d["Nq"], d["Nk"], d["D"]
    bh, var = B * H, variant_of(d)
    if d["kind"] == "attn_fwd":
        wide = D <= 64 and bh * cdiv(Nq, 128) >= 512
        w8 = D in (40, 80) and bh * cdiv(Nq, 256 if D == 40 else 128) >= 256
        return [("fwd", D, var, 2 if wide else 1, 8 if w8 else 4)]
    wq = D <= 64 and bh * cdiv(Nq, 128) >= 512
    wk = D <= 64 and bh * cdiv(Nk, 128) >= 512
    base, nqt = cdiv(Nk, 128 if wk else 64) * bh, cdiv(Nq, 64)
    qsplit = 1
    if base < 256 and nqt >= 8:
        qsplit = min(cdiv(256, base), nqt // 16)
    return [("dq", D, var, 2 if wq else 1), ("dkv", D, var, 2 if wk else 1, qsplit >= 2)]


def all_instantiations():
    out = []
    for D in (40, 64, 80, 160):
        for var in ("plain", "prescaled", "masked"):
            out += [("fwd", D, var, qt, nw) for qt, nw in fwd_shapes(D)]
            out += [("dq", D, var, qt) for qt in sorted({a for a, _ in bwd_shapes(D)})]
            out += [("dkv", D, var, kt, sp) for kt in sorted({b for _, b in bwd_shapes(D)}) for sp in (False, True)]
    return out


def synth_descriptor(kind, D, var, H, Nq, Nk):
    """B 2; the packed layout the product would use (q | k | v of one buffer for self-attention, k | v inside a wider joint buffer for
    cross-attention) with a gap row between the batch rows; masked: a key bias whose batch stride exceeds Nk, plus the causal mask on
    every self-attention shape with an odd log2(H) (so both masked forms meet the wide kernels)."""
    C = H * D
    kw = dict(key_bias=var == "masked", prescaled=var == "prescaled")
    if Nq == Nk:
        rs = 3 * C + 8
        kw.update(layout="qkv", q_rs=rs, k_rs=rs, v_rs=rs, q_bs=(Nq + 1) * rs, k_bs=(Nq + 1) * rs, v_bs=(Nq + 1) * rs)
        kw["causal"] = var == "masked" and H.bit_length() % 2 == 0
    else:
        rs = 2 * C + 2 * 320
        kw.update(layout="q+kv", k_rs=rs, v_rs=rs, k_bs=(Nk + 1) * rs, v_bs=(Nk + 1) * rs)
    if kw["key_bias"]:
        kw["kb_bs"] = Nk + 19
    return AC.desc(kind, B=2, H=H, Nq=Nq, Nk=Nk, D=D, **kw)


def synthesized():
    """[(id, descriptor)]: for each instantiation no recorded launch selects, the smallest (by scores computed) descriptor of a small
    search grid that makes the unforced heuristic select it; second value: the instantiations the heuristic cannot select at all
    (e.g. a query-split dK/dV at 32 rows per wave: the split needs < 256 workgroups, 32 rows >= 512; or d = 40 with 32 rows per wave in a 4-wave workgroup: 512 such workgroups always mean >= 256 8-wave ones)."""
    reached = {i for it in load_fixture() for i in selected(it["desc"])}
    want = [i for i in all_instantiations() if i not in reached]
    best = {}
    for kind in ("attn_fwd", "attn_bwd"):
        for D in (40, 64, 80, 160):
            for var in ("plain", "prescaled", "masked"):
                for H in (1, 2, 4, 8, 16, 32, 64, 128, 256):
                    for Nq in (77, 125, 253, 1021, 2045, 4093):
                        for Nk in (77, Nq):
                            d = synth_descriptor(kind, D, var, H, Nq, Nk)
                            cost = 2 * H * Nq * Nk * (D + 64)
                            for i in selected(d):
                                if i in want and cost < best.get(i, (math.inf, None))[0] and cost < 2 ** 34:
                                    best[i] = (cost, d)
    out, seen = [], set()
    for i in want:
        if i in best:
            key = json.dumps(best[i][1], sort_keys=True)
            if key not in seen:
                seen.add(key)
                out.append(("_".join(str(x) for x in i), best[i][1]))
    return out, [i for i in want if i not in best]


# ---------------------------------------------------------------- CPU: a blocked flash-attention model with injectable faults

T = 64
MUT = dict(B=2, H=3, Nq=200, Nk=269, D=64)
MUT_DESCS = {
    "plain_fwd": AC.desc("attn_fwd", **MUT), "plain_bwd": AC.desc("attn_bwd", layout="q+kv", k_rs=2 * 192 + 64, v_rs=2 * 192 + 64,
                                                                  k_bs=270 * 448, v_bs=270 * 448, **MUT),
    "bias_fwd": AC.desc("attn_fwd", key_bias=True, kb_bs=272, **MUT),
    "causal_fwd": AC.desc("attn_fwd", causal=True, **dict(MUT, Nk=200)),
    "pre_bwd": AC.desc("attn_bwd", prescaled=True, **MUT),
}
FAULTS = {   # fault -> descriptor it is injected into
    "interior_key_tile_dropped": "plain_fwd", "last_key_of_ragged_tile_dropped": "plain_fwd", "ragged_tail_reads_next_batch_row": "plain_fwd",
    "stale_accumulator_after_max_update": "plain_fwd", "lse_without_last_tile": "plain_fwd", "head_written_to_neighbour_head": "plain_fwd",
    "ragged_query_tail_unwritten": "plain_fwd", "bias_of_batch0_on_batch1": "bias_fwd", "causal_boundary_off_by_one": "causal_fwd",
    "slab_not_added": "plain_bwd", "slab_added_twice": "plain_bwd", "delta_from_wrong_row": "plain_bwd",
    "neighbour_column_overwritten": "plain_bwd", "dk_missing_ln2_in_quietest_head": "pre_bwd",
}
PAIR = (1, 1)                    # the (batch, head) most faults are confined to


def _quietest_head(d, ops):
    D = d["D"]
    return int(torch.stack([ops["q"][:, :, h * D:(h + 1) * D].float().abs().mean() for h in range(d["H"])]).argmin())


def _model_scores(d, ops, b, h, fault):
    D = d["D"]
    q, k = ops["q"][b, :, h * D:(h + 1) * D].float(), ops["k"][b, :, h * D:(h + 1) * D].float()
    if fault == "ragged_tail_reads_next_batch_row" and b == 0:       # the last tile runs on into batch row 1's keys
        pad = cdiv(d["Nk"], T) * T - d["Nk"]
        k = torch.cat([k, ops["k"][1, :pad, h * D:(h + 1) * D].float()])
    S = (q @ k.T) * (AC.LN2 if d["prescaled"] else AC.scale_of(d))
    if d["key_bias"]:
        kb = ops["key_bias"][0 if fault == "bias_of_batch0_on_batch1" else b]
        S = S + kb[None, :]
    if d["causal"]:
        n = S.shape[0]
        S = S.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(0 if fault == "causal_boundary_off_by_one" and (b, h) == PAIR else 1), -math.inf)
        if fault == "causal_boundary_off_by_one" and (b, h) == PAIR:
            S[0, 0] = q[0] @ k[0] * AC.scale_of(d)                    # (row 0 keeps its only key: the fault is the boundary of the others)
    return S


def model_forward(d, ops, fault=None):
    """online softmax over 64-key tiles: fp32 running max / sum / accumulator, bf16 P into the PV product; into NaN-poisoned outputs."""
    B, H, Nq, D = d["B"], d["H"], d["Nq"], d["D"]
    o = torch.full((B, Nq, H * D), math.nan)
    lse = torch.full((B, H, Nq), math.nan)
    for b in range(B):
        for h in range(H):
            here = (b, h) == PAIR
            S = _model_scores(d, ops, b, h, fault)
            v = ops["v"][b, :, h * D:(h + 1) * D].float()
            if S.shape[1] > v.shape[0]:
                v = torch.cat([v, ops["v"][1, :S.shape[1] - v.shape[0], h * D:(h + 1) * D].float()])
            if fault == "last_key_of_ragged_tile_dropped" and here:
                S, v = S[:, :-1], v[:-1]
            m = torch.full((Nq,), -math.inf); l = torch.zeros(Nq); acc = torch.zeros(Nq, D)
            nt = cdiv(S.shape[1], T)
            stale_row = int(S[:, T:].amax(1).sub(S[:, :T].amax(1)).argmax())          # a row whose maximum moves after the first tile
            for t in range(nt):
                if fault == "interior_key_tile_dropped" and here and t == 1:
                    continue
                s = S[:, t * T:(t + 1) * T]
                m_new = torch.maximum(m, s.amax(1))
                alpha = torch.exp(m - m_new)
                p = torch.exp(s - m_new[:, None])
                if fault == "lse_without_last_tile" and here and t == nt - 1:
                    l_before, m_before = l.clone(), m.clone()
                l = l * alpha + p.sum(1)
                keep = acc[stale_row].clone()
                acc = acc * alpha[:, None] + p.to(BF).float() @ v[t * T:(t + 1) * T]
                if fault == "stale_accumulator_after_max_update" and here and t >= 1:
                    acc[stale_row] = keep + (p.to(BF).float() @ v[t * T:(t + 1) * T])[stale_row]
                m = m_new
            hh = h
            if fault == "head_written_to_neighbour_head" and b == 1 and h == 0:
                hh = 1
            if not (fault == "head_written_to_neighbour_head" and b == 1 and h == 1):
                o[b, :, hh * D:(hh + 1) * D] = acc / l[:, None]
            lse[b, h] = m + torch.log(l)
            if fault == "lse_without_last_tile" and here:
                lse[b, h] = m_before + torch.log(l_before)
    if fault == "ragged_query_tail_unwritten":
        o[1, Nq // T * T:, -D:] = math.nan
    return {"o": o.to(BF), "lse": lse}


def model_backward(d, ops, fault=None):
    """dQ / dK / dV from the clean forward's o and lse: bf16 P and dS into the products, the query loop of dK / dV split into two fp32
    slabs added in order; written into sentinel-filled buffers laid out as the descriptor says."""
    B, H, Nq, Nk, D = d["B"], d["H"], d["Nq"], d["Nk"], d["D"]
    outs = model_forward(d, ops)
    slabs, (dq, dk, dv) = AC._slabs(d, "cpu")
    for s in slabs:
        s.poison(math.nan)
    c = AC.LN2 if d["prescaled"] else AC.scale_of(d)
    quiet = _quietest_head(d, ops)
    for b in range(B):
        for h in range(H):
            here = (b, h) == PAIR
            sl = slice(h * D, (h + 1) * D)
            S = _model_scores(d, ops, b, h, None)
            q, k, v, do = (ops[n][b, :, sl].float() for n in ("q", "k", "v", "do"))
            P = torch.exp(S - outs["lse"][b, h][:, None])
            delta = (do * outs["o"][b, :, sl].float()).sum(1)
            if fault == "delta_from_wrong_row" and here:
                delta[17] = delta[18]
            dS = (P * (do @ v.T - delta[:, None])).to(BF).float()
            P16 = P.to(BF).float()
            half = Nq // 2 // T * T
            parts = [(slice(0, half)), (slice(half, Nq))]
            kv = [(dS[p].T @ q[p] * c, P16[p].T @ do[p]) for p in parts]
            if fault == "slab_not_added" and here:
                kv = kv[:1]
            if fault == "slab_added_twice" and here:
                kv = kv + kv[1:]
            dkk = sum(x for x, _ in kv)
            if fault == "dk_missing_ln2_in_quietest_head" and h == quiet and b == 1:
                dkk = dkk / c
            dq[b, :, sl] = (dS @ k * c).to(BF); dk[b, :, sl] = dkk.to(BF); dv[b, :, sl] = sum(x for _, x in kv).to(BF)
    if fault == "neighbour_column_overwritten":
        s = slabs[1]
        i = int(torch.nonzero(~s.owned)[5])
        s.flat[i] = 0.0
    outs.update(dq=dq, dk=dk, dv=dv, slabs=slabs)
    return outs


def _old_gates_pass(d, ops, got):
    """the gates of tests/test_kernels.py before this checker: tensor-max relative error and an absolute lse tolerance."""
    items = {it.name: it for it in AC.references(d, ops, got)}
    ok = True
    for name, it in items.items():
        if name == "lse":
            ok = ok and bool(((it.got - it.ref).abs().max() < 2e-2))
        else:
            ok = ok and relerr(it.got, it.ref) < (1e-2 if name == "o" else 2e-2)
    return ok


def test_checker_catches_every_injected_fault():
    passed_by_old_gates = []
    clean = {}
    for name, d in MUT_DESCS.items():
        ops = AC.make_operands(d, "cpu")
        model = model_forward if d["kind"] == "attn_fwd" else model_backward
        r = AC.check(d, ops, model(d, ops))
        assert r <= 1.0
        clean[name] = (d, ops, model, r)
    for fault, name in FAULTS.items():
        d, ops, model, _ = clean[name]
        got = model(d, ops, fault)
        with pytest.raises(AssertionError):
            AC.check(d, ops, got)
        if fault != "neighbour_column_overwritten" and _old_gates_pass(d, ops, got):
            passed_by_old_gates.append(fault)
    print(f"clean model, worst err / bound: {({k: round(v[3], 3) for k, v in clean.items()})}")
    print(f"faults the old gates (relerr < 1e-2 / 2e-2, lse within 2e-2) pass: {passed_by_old_gates}")
    assert passed_by_old_gates, "the element-wise check is meant to catch faults that the tensor-max gates cannot see"


def test_checker_message_names_batch_head_row_and_column():
    d, ops = MUT_DESCS["plain_fwd"], AC.make_operands(MUT_DESCS["plain_fwd"], "cpu")
    got = model_forward(d, ops, "ragged_query_tail_unwritten")
    with pytest.raises(AssertionError, match=r"o of .*worst at batch 1 row 192 head 2 col 0: got nan"):
        AC.check(d, ops, got)


# ---------------------------------------------------------------- CPU: every selectable instantiation on the interpreter

VARIANTS = {"plain": {}, "prescaled": dict(prescaled=True), "bias": dict(key_bias=True), "causal": dict(causal=True),
            "causal_bias": dict(causal=True, key_bias=True)}
LAYOUTS = ("separate", "qkv", "q+kv")
SPLIT_BITS = (2 << 8) | (1 << 16)          # tools bits 8-19: >= 2 query tiles per split, 256 target workgroups


def runs_of(D):
    """forced hcp_debug_set_attention_config values that between them select every forward (bit 0: 32 rows per wave, bit 3: 8 waves)
    and every backward (bit 1: dQ, bit 2: dK/dV at 32 rows per wave) shape of head dim D: one run exercises one forward and one
    backward shape, so max(len(fwd_shapes), len(bwd_shapes)) runs are enough."""
    f, b = fwd_shapes(D), bwd_shapes(D)
    out = []
    for i in range(max(len(f), len(b))):
        (qt, nw), (wq, wk) = f[i % len(f)], b[i % len(b)]
        out.append((1 if qt == 2 else 0) | (8 if nw == 8 else 0) | (2 if wq == 2 else 0) | (4 if wk == 2 else 0))
    return out


def reduced_descriptor(kind, D, variant, layout, split):
    """B 2, H 2, ragged (Nq, Nk not multiples of 64 or of each other), batch strides with a gap row (more where the query split needs
    >= 8 query tiles); self-attention sizes where the layout or the causal mask need Nq == Nk."""
    H, B = 2, 2
    C = H * D
    Nq = 520 if split else 150
    Nk = Nq if (layout == "qkv" or "causal" in variant) else 77
    kw = dict(VARIANTS[variant])
    if layout == "qkv":
        rs = 3 * C + 16
        kw.update(q_rs=rs, k_rs=rs, v_rs=rs, q_bs=(Nq + 2) * rs, k_bs=(Nq + 2) * rs, v_bs=(Nq + 2) * rs)
    elif layout == "q+kv":
        rs = 2 * C + 48
        kw.update(q_bs=(Nq + 1) * C, k_rs=rs, v_rs=rs, k_bs=(Nk + 3) * rs, v_bs=(Nk + 3) * rs)
    else:
        kw.update(q_rs=C + 8, q_bs=(Nq + 1) * (C + 8), k_bs=(Nk + 2) * C, v_rs=C + 24, v_bs=Nk * (C + 24))
    if kw.get("key_bias"):
        kw["kb_bs"] = Nk + 11
    return AC.desc(kind, B=B, H=H, Nq=Nq, Nk=Nk, D=D, layout=layout, **kw)


def count_instantiation_layout_combinations():
    """per (variant, layout): sum over D of [forward shapes + dQ shapes x dK/dV shapes x {one slab, query split}]
    = (4 + 4*2) + (2 + 4*2) + (2 + 1*2) + (1 + 1*2) = 29;  x 5 variants x 3 layouts = 435.  (pre-scaled Q with a mask is rejected by
    the entry points' HCP_REQUIRE: the five variants are the admissible ones.)"""
    return sum(len(fwd_shapes(D)) + 2 * len(bwd_shapes(D)) for D in (40, 64, 80, 160)) * len(VARIANTS) * len(LAYOUTS)


def test_instantiation_count():
    n = count_instantiation_layout_combinations()
    runs = sum(2 * len(runs_of(D)) for D in (40, 64, 80, 160)) * len(VARIANTS) * len(LAYOUTS)
    print(f"{n} instantiation x layout combinations, covered by {runs} interpreter runs (one forward + one backward shape per run)")
    assert n == 435
    for D in (40, 64, 80, 160):
        cfgs = runs_of(D)
        assert {(2 if c & 1 else 1, 8 if c & 8 else 4) for c in cfgs} == set(fwd_shapes(D))
        assert {(2 if c & 2 else 1, 2 if c & 4 else 1) for c in cfgs} == set(bwd_shapes(D))


@pytest.fixture
def emu_tools():
    from conftest import emu_cdll
    K._set_backend_for_tests(emu_cdll())
    yield K.lib()
    K.lib().hcp_debug_set_attention_config(-1)
    K._set_backend_for_tests(None)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_every_instantiation_on_the_interpreter(emu_tools, D, variant, layout):
    L = emu_tools
    for split in (False, True):
        d = reduced_descriptor("attn_bwd", D, variant, layout, split)
        if split:
            assert not selected(d)[1][4], "the reduced shape must need the forced split"
        ops = AC.make_operands(d, "cpu")
        for cfg in runs_of(D):
            L.hcp_debug_set_attention_config(cfg | (SPLIT_BITS if split else 0))
            try:
                outs = AC.run(d, ops)
            finally:
                L.hcp_debug_set_attention_config(-1)
            assert AC.workspace_written(ops["q"]) == split, "forced query split: the dK / dV pass must leave slabs in the workspace (and only then)"
            AC.check(dict(d, kind="attn_fwd"), ops, outs)
            AC.check(d, ops, outs)


# ---------------------------------------------------------------- CPU: the fixture

def test_fixture_is_consistent():
    fx = load_fixture()
    assert fx and fx == sorted(fx, key=lambda x: json.dumps(x["desc"], sort_keys=True))
    seen = set()
    for item in fx:
        d = item["desc"]
        key = json.dumps(d, sort_keys=True)
        assert key not in seen
        seen.add(key)
        assert set(item["count"]) <= NAMES and all(n > 0 for n in item["count"].values())
        assert d["kind"] in ("attn_fwd", "attn_bwd") and d["D"] in (40, 64, 80, 160) and d["layout"] in LAYOUTS
        C = d["H"] * d["D"]
        for t, n in (("q", d["Nq"]), ("k", d["Nk"]), ("v", d["Nk"])):
            assert d[t + "_rs"] % 8 == 0 and d[t + "_bs"] % 8 == 0 and d[t + "_rs"] >= C and d[t + "_bs"] >= n * d[t + "_rs"], d
        if d["layout"] == "qkv":
            assert d["q_rs"] == d["k_rs"] == d["v_rs"] >= 3 * C and d["Nq"] == d["Nk"], d          # three slices of C columns: no overlap
        if d["layout"] == "q+kv":
            assert d["k_rs"] == d["v_rs"] >= 2 * C, d
        assert not d["causal"] or d["Nq"] == d["Nk"], d
        assert not d["prescaled"] or not (d["causal"] or d["key_bias"]), d
        assert d["key_bias"] == (d["kb_bs"] > 0) and (not d["key_bias"] or d["kb_bs"] >= d["Nk"]), d
    syn, never = synthesized()
    print(f"{len(fx)} descriptors select {len({i for it in fx for i in selected(it['desc'])})} of {len(all_instantiations())} instantiations; "
          f"{len(syn)} descriptors are synthesized; the unforced heuristic cannot select {never}")
    for name, d in syn:
        assert any("_".join(str(x) for x in i) == name for i in selected(d))


# ---------------------------------------------------------------- GPU: real shapes, the product library's dispatch

WORST = {}
WORST_G1 = {}


@pytest.fixture(scope="module")
def product():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from conftest import gpu_box_check
    gpu_box_check()
    K._set_backend_for_tests(None)
    assert K.lib().hcp_is_emulated() == 0
    yield torch.device("cuda:0")
    K._set_backend_for_tests(None)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _check_twice(d, dev):
    """check at the real shape, every (batch, head); a second run into differently poisoned buffers gives identical bits (the query-split
    dK / dV sums ordered slabs: no fp32 atomics in this family)."""
    ops = AC.make_operands(d, dev)
    outs = AC.run(d, ops)
    if d["kind"] == "attn_bwd":            # ties selected() to the library: plan_dkv split exactly where the restated rule says
        assert AC.workspace_written(ops["q"]) == selected(d)[1][4], f"query split of {AC.describe(d)} differs from the restated plan_dkv rule"
    AC.check(d, ops, outs, ratios=WORST)
    for k, v in AC.measure(d, ops, outs, g=1.0).items():
        WORST_G1[k] = max(WORST_G1.get(k, 0.0), v)
    again = AC.run(d, ops, fill=float("inf"), wrapper_alloc=True)       # contiguous q / k / v: the out=None form, same bits
    for name, t in outs.items():
        if name != "slabs" and (d["kind"] == "attn_bwd" or name in ("o", "lse")):
            assert torch.equal(_bits(t), _bits(again[name])), f"{name} of {AC.describe(d)} differs between two runs"
    del ops, outs, again


def _fixture_ids():
    return [(f"{i:03d}_{it['desc']['kind']}", it["desc"]) for i, it in enumerate(load_fixture())]


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [d for _, d in _fixture_ids()], ids=[i for i, _ in _fixture_ids()])
def test_recorded_launch_against_float64(product, desc):
    _check_twice(desc, product)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [d for _, d in synthesized()[0]], ids=[i for i, _ in synthesized()[0]])
def test_unreached_instantiation_against_float64(product, desc):
    _check_twice(desc, product)


@pytest.mark.gpu
def test_fresh_trace_equals_fixture(product):
    sys.path.insert(0, str(ROOT / "tools"))
    import trace_attention_launches as TA
    fresh = TA.dumps(TA.trace_all())
    assert fresh == FIXTURE.read_text(), "the attention launches changed: re-run `python tools/trace_attention_launches.py` on the GPU"


@pytest.mark.gpu
def test_report_worst_ratio_per_output(product):
    print("\nworst err / bound per output: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    print(f"the same with G = 1 (attn_check.G = {AC.G:g} is set from these): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST_G1.items())))
    assert WORST and all(v <= 1.0 for v in WORST.values())
