"""Every LoRA weight-gradient and pack launch (csrc/lora.hip) element-wise against float64 (tests/lora_check.py): the single, pair and
grouped entry points over every code path their launch rules select — direct add / vector reduce / scalar reduce, both output layouts,
with and without the residual half of a split T / U — at the smallest shapes that select them, interpreted on the CPU and, under -m gpu,
on the product library; hcp_lora_pack and hcp_split_hi_lo_bf16 bit for bit against torch's rounding; and the grouped launches of the
sd15 / sdxl workloads at their real shapes (tests/golden/lora_launches.json, tools/trace_lora_launches.py).

The mutation test runs a torch model of the blocked algorithm with the fourteen faults of FAULTS: the checker raises on every one; the
old gate (tests/test_kernels.py: tensor-maximum relerr < 2e-2 on operands of one scale) passes those of OLD_GATE_PASSES."""
import ctypes
import json
import math
import sys
from pathlib import Path

import pytest
import torch

import gemm_check as GC
import lora_check as LC
from hcp_diffusion_amd import kernels as K

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "lora_launches.json"
BF = torch.bfloat16
D, lay = LC.desc, LC.layer

# ---------------------------------------------------------------- the case list

# (M, r, grad_offset) that select: the direct add (one token range, two row blocks, the second ragged), the vector reduce (P % 4 == 0,
# aligned views) and the scalar reduce (P = 5 and views misaligned by one float: both conditions off for grad_up, the alignment for grad_down)
PATHS = {"direct": (100, 4, 0), "vector": (600, 4, 0), "scalar": (700, 5, 1)}


def _base_cases():
    out = []
    for lo in (False, True):
        for M, r, off in PATHS.values():
            kw = dict(u_split=lo, t_split=lo, grad_offset=off)
            out += [D("lora_wgrad", M, 136, 72, r, transpose_out=False, **kw), D("lora_wgrad", M, 136, 72, r, transpose_out=True, **kw),
                    D("lora_wgrad_pair", M, 136, 72, r, **kw),
                    D("lora_wgrad_grouped", layers=[lay(M, 136, 72, r, u_split=lo, t_split=lo)], grad_offset=off, grid_blocks=16)]
    return out


def _one(l, **kw):
    return D("lora_wgrad_grouped", layers=[l], **dict(dict(grid_blocks=16), **kw))


MIXED_LAYERS = [lay(700, 136, 264, 1, slot0=31), lay(100, 72, 8, 4, slot0=8, scale=-0.25), lay(1000, 264, 136, 5, slot0=27, t_split=True),
                lay(40, 8, 72, 8, slot0=24), lay(1, 136, 72, 16, slot0=16, u_split=True), lay(600, 72, 72, 4, slot0=3, ldu=96, ldt=192, t_split=True),
                lay(2100, 8, 136, 16, slot0=0, scale=2.0), lay(300, 320, 40, 2, slot0=5, ldy=56, ldx=328), lay(4200, 72, 8, 32),
                lay(130, 40, 328, 8, u_split=True, t_split=True, ldu=192, ldt=192), lay(900, 136, 136, 3, slot0=13),
                lay(64, 264, 8, 32), lay(520, 8, 8, 8, slot0=8, ldy=24)]
MIXED = D("lora_wgrad_grouped", layers=MIXED_LAYERS, grid_blocks=16 * len(MIXED_LAYERS), grad_offset=3)
MIXED_HALF = dict(MIXED, ws_bytes=LC.ws_need(MIXED) * 4 // 2 // 512 * 512)
TWICE = D("lora_wgrad_grouped", grid_blocks=32, layers=[lay(600, 136, 72, 4), lay(100, 72, 136, 5), lay(600, 136, 72, 4, same_as=0, scale=-1.5)])

EXTRA = [
    # splits >= 3 with two column tiles, ragged last range; M < 64; M = 1; Q = 8
    D("lora_wgrad", 300, 136, 72, 1), D("lora_wgrad", 300, 72, 264, 1, transpose_out=True),
    D("lora_wgrad", 40, 8, 8, 8), D("lora_wgrad", 1, 8, 8, 8, transpose_out=True, t_split=True), D("lora_wgrad_pair", 1, 72, 8, 5, u_split=True),
    # ranks 16, 32 with several ranges; one lo side only; different numbers of column tiles in both directions; column-slice x / dy
    D("lora_wgrad_pair", 2100, 8, 136, 16, t_split=True), D("lora_wgrad_pair", 4200, 264, 72, 32, u_split=True),
    D("lora_wgrad_pair", 600, 72, 264, 4, ldx=88, ldy=272), D("lora_wgrad_pair", 600, 264, 72, 4, grad_offset=2),
    # the single form behind a column-offset view of T / U (ops._lora_grads_wide: slot0 a multiple of 8), slices of a 32 G-wide T_all / U_all
    D("lora_wgrad", 600, 72, 72, 4, slot0=8), D("lora_wgrad", 100, 72, 72, 8, slot0=24, transpose_out=True),
    D("lora_wgrad", 600, 72, 72, 4, ldu=96), D("lora_wgrad", 600, 72, 72, 8, transpose_out=True, t_split=True, ldt=192),
    # rank 40 / 38 through ops._lora_grads_wide: out_col0 = 0 and 32; ldo = 38 switches the vector reduce off at P = 32
    D("lora_wgrad", 4200, 72, 136, 40, wide=True, ldu=64, ldt=64), D("lora_wgrad", 4200, 72, 136, 38, wide=True, ldu=64, ldt=64, slot0=8),
    D("lora_wgrad", 100, 72, 136, 40, wide=True, ldu=64, ldt=64, slot0=24),
    # grouped: every rank and slot, pcol0 + P == 32 with pcol0 off the 8-column pieces, gradient views misaligned by 1, 2, 3 floats
    _one(lay(300, 136, 72, 1, slot0=31)), _one(lay(700, 72, 136, 5, slot0=27, u_split=True), grad_offset=2),
    _one(lay(700, 72, 136, 5, slot0=3, t_split=True), grad_offset=3), _one(lay(1100, 8, 72, 8, slot0=8)), _one(lay(1100, 72, 8, 8, slot0=24)),
    _one(lay(2100, 72, 72, 16, slot0=16)), _one(lay(4200, 136, 8, 32)), _one(lay(40, 72, 72, 4, slot0=28)),
    _one(lay(600, 72, 136, 4, ldu=96, ldt=96, ldy=272, slot0=3)), _one(lay(600, 72, 136, 4, u_split=True, t_split=True, ldu=192, ldt=192)),
    MIXED, MIXED_HALF, TWICE,
]
CASES = _base_cases() + EXTRA

PACK_CASES = [D("lora_pack", Ntot=N, bu_ld=0, descs=[dict(K=Kd, N=N, r=r, alpha=1.0 / 3, slot0=0, n0=0)])
              for Kd, N, r in ((8, 24, 1), (24, 320, 5), (320, 8, 32), (8, 8, 5), (320, 320, 32), (24, 24, 1))] + [
    D("lora_pack", Ntot=344, bu_ld=64, descs=[dict(K=24, N=24, r=5, alpha=0.2, slot0=0, n0=0), dict(K=24, N=320, r=8, alpha=-1.7, slot0=8, n0=24)]),
    D("lora_pack", Ntot=32, bu_ld=64, descs=[dict(K=8, N=24, r=5, alpha=0.7, slot0=27, n0=8, null=True)])]
SPLIT_CASES = [D("split_hi_lo", M=M, C=C) for M, C in ((5, 4), (37, 32), (130, 96), (16385, 128))]


def classes(d):
    """the (entry point, reduce path, transposed, residual half) classes a descriptor's launches fall into, by the mirrored rules."""
    k = d["kind"]
    layout, _ = LC.grad_layout(d)
    out = set()
    if k == "lora_wgrad":
        od, ou, w = layout[0]
        for which, P, j, col0, tr in LC.problems(d):
            Q = d["N"] if tr else d["K"]
            s = LC.wgrad_launch(Q, Q, 1, d["M"], P)[1]
            vec = LC.reduce_is_vector(P, w if tr else d["K"], tr, (ou + col0) if tr else od + j * d["K"])
            out.add(("single", "direct" if s == 1 else "vector" if vec else "scalar", tr, bool(d["t_split"] if tr else d["u_split"])))
        return out
    if k == "lora_wgrad_pair":
        od, ou, w = layout[0]
        s = LC.wgrad_launch(d["K"], d["N"], 2, d["M"], d["r"])[1]
        for tr in (False, True):
            vec = LC.reduce_is_vector(d["r"], w if tr else d["K"], tr, ou if tr else od)
            out.add(("pair", "direct" if s == 1 else "vector" if vec else "scalar", tr, bool(d["t_split"] if tr else d["u_split"])))
        return out
    for p in LC.passes_of(d):
        ls = [d["layers"][i] for i in p]
        _, plan, _, _, _ = LC.group_plan(ls, d["grid_blocks"], d["ws_bytes"] or (1 << 40))
        for i, l, g in zip(p, ls, plan):
            od, ou, w = layout[i]
            for tr in (False, True):
                vec = LC.reduce_is_vector(l["r"], w if tr else l["K"], tr, ou if tr else od)
                out.add(("grouped", "direct" if g["splits"] == 1 else "vector" if vec else "scalar", tr, bool(l["t_split"] if tr else l["u_split"])))
    return out


ALL_CLASSES = {(e, p, tr, lo) for e in ("single", "pair", "grouped") for p in ("direct", "vector", "scalar") for tr in (False, True)
               for lo in (False, True)}


def test_every_class_has_a_case():
    """no case is skipped on either backend, so the classes of CASES are the classes that run; they are all the rules can select."""
    ran = set()
    for d in CASES:
        ran |= classes(d)
    assert ran == ALL_CLASSES, (ALL_CLASSES - ran, ran - ALL_CLASSES)


def _splits(d):
    if d["kind"] == "lora_wgrad":
        return [LC.wgrad_launch(d["N"] if tr else d["K"], 0, 1, d["M"], P)[:2] for _, P, _, _, tr in LC.problems(d)]
    if d["kind"] == "lora_wgrad_pair":
        return [LC.wgrad_launch(d["K"], d["N"], 2, d["M"], d["r"])[:2]]
    return [(max(g["qt0"], g["qt1"]), g["splits"]) for p in LC.passes_of(d)
            for g in LC.group_plan([d["layers"][i] for i in p], d["grid_blocks"], d["ws_bytes"] or (1 << 40))[1]]


def test_cases_cover_what_they_claim():
    L = [(d["kind"], l) for d in CASES for l in LC.layers_of(d)]
    assert {l["r"] for _, l in L} >= {1, 4, 5, 8, 16, 32}
    assert {l["slot0"] for k, l in L if k == "lora_wgrad_grouped"} >= {0, 3, 8, 24, 27, 28, 31}
    assert any(l["slot0"] + l["r"] == 32 and l["slot0"] % 8 for k, l in L if k == "lora_wgrad_grouped")
    assert {l["M"] for _, l in L} >= {1, 40} and any(l["M"] % 64 for _, l in L)
    assert any(l["K"] == 8 for _, l in L) and any(l["N"] == 8 for _, l in L) and any(l["K"] % 128 for _, l in L)
    sp = [x for d in CASES for x in _splits(d)]
    assert {min(s, 3) for _, s in sp} == {1, 2, 3} and any(s >= 3 and qt >= 2 for qt, s in sp)
    pairs = [d for d in CASES if d["kind"] == "lora_wgrad_pair" and LC.wgrad_launch(d["K"], d["N"], 2, d["M"], d["r"])[1] > 1]
    assert any(LC.cdiv(d["K"], 128) > LC.cdiv(d["N"], 128) for d in pairs) and any(LC.cdiv(d["K"], 128) < LC.cdiv(d["N"], 128) for d in pairs)
    assert {(l["u_split"], l["t_split"]) for k, l in L if k != "lora_wgrad"} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(l["ldy"] > l["N"] for _, l in L) and any(l["ldx"] > l["K"] for _, l in L)
    assert any(l["ldu"] == 96 for _, l in L) and any(l["ldt"] == 192 and l["t_split"] for _, l in L)
    assert {d["grad_offset"] % 4 for d in CASES} == {0, 1, 2, 3}
    assert any(d.get("wide") and d["r"] == 40 for d in CASES)
    mixed = [g["splits"] for g in LC.group_plan(MIXED_LAYERS, MIXED["grid_blocks"], 1 << 40)[1]]
    assert len(MIXED_LAYERS) >= 12 and 1 in mixed and max(mixed) > 1 and len({l["r"] for l in MIXED_LAYERS}) >= 6
    full, half = LC.group_plan(MIXED_LAYERS, MIXED["grid_blocks"], 1 << 40), LC.group_plan(MIXED_LAYERS, MIXED["grid_blocks"], MIXED_HALF["ws_bytes"])
    assert half[0] < full[0] and half[4] * 512 <= MIXED_HALF["ws_bytes"] < full[4] * 512, "the halved workspace makes the wrapper lower its target"
    assert len(LC.passes_of(TWICE)) == 2


def test_group_geometry_mirror_matches_the_library(backend):
    qt0, qt1, sp, rows = (ctypes.c_int() for _ in range(4))
    shapes = {(l["M"], l["K"], l["N"], l["r"]) for d in CASES for l in LC.layers_of(d) if l["r"] <= 32}
    shapes |= {(M, Kd, N, r) for M in (1, 63, 64, 65, 255, 257, 4096, 16384) for Kd, N in ((8, 8), (320, 2560), (1280, 136)) for r in (1, 5, 16, 32)}
    for M, Kd, N, r in sorted(shapes):
        for target in (1, 2, 8, 13, 102, 256, 0):
            nb = K.lib().hcp_lora_wgrad_group_geometry(M, Kd, N, r, target, ctypes.byref(qt0), ctypes.byref(qt1), ctypes.byref(sp), ctypes.byref(rows))
            assert (nb, qt0.value, qt1.value, sp.value, rows.value) == LC.group_geometry(M, Kd, N, r, target), (M, Kd, N, r, target)


# ---------------------------------------------------------------- running

MEASURED_NL = (1.0, 0.5, 0.25, 0.125, 0.0625)
RATIOS_AT = {g: {} for g in MEASURED_NL}       # NL -> kind -> worst err / bound over what this session ran on the GPU
RATIOS = {}                                    # the same under the module's NL, from check()


def run_check(d, be, kind=None):
    ops = LC.make_operands(d, be.device)
    outs = LC.run(d, ops)
    items = LC.references(d, ops, outs) if d["kind"] in LC.WGRAD_KINDS else None       # computed once: check and every NL below share them
    r = LC.check(d, ops, outs, items)
    if be.is_gpu and d["kind"] in LC.WGRAD_KINDS:
        kind = kind or d["kind"]
        RATIOS[kind] = max(RATIOS.get(kind, 0.0), r)
        for g, into in RATIOS_AT.items():
            into[kind] = max(into.get(kind, 0.0), LC.measure(items, g))
        del items
        again = LC.run(d, ops)
        assert torch.equal(outs["bucket"].view(torch.int32), again["bucket"].view(torch.int32)), f"{LC.describe(d)}: two runs differ in bits"
    return ops, outs


@pytest.mark.parametrize("i", range(len(CASES)))
def test_wgrad_case(backend, i):
    run_check(CASES[i], backend)


def test_halved_workspace_lowers_the_target(backend, monkeypatch):
    """the fit loop of kernels.lora_wgrad_grouped, observed through the launch record."""
    monkeypatch.setattr(K, "LAUNCHES", [])
    run_check(MIXED_HALF, backend)
    rec = [r for r in K.LAUNCHES if r["kind"] == "lora_wgrad_grouped"]
    natural = max(8, min(256, MIXED["grid_blocks"] // len(MIXED_LAYERS)))
    assert rec[0]["target"] == LC.group_plan(MIXED_LAYERS, MIXED["grid_blocks"], MIXED_HALF["ws_bytes"])[0] < natural
    assert [l["splits"] for l in rec[0]["layers"]] == [g["splits"] for g in LC.group_plan(MIXED_LAYERS, MIXED["grid_blocks"], MIXED_HALF["ws_bytes"])[1]]


@pytest.mark.parametrize("i", range(len(PACK_CASES)))
def test_pack_case(backend, i):
    run_check(PACK_CASES[i], backend)


@pytest.mark.parametrize("i", range(len(SPLIT_CASES)))
def test_split_hi_lo_case(backend, i):
    d = SPLIT_CASES[i]
    assert (d["M"] * d["C"] // 4 > 2048 * 256) == (i == len(SPLIT_CASES) - 1), "the last case takes the grid-stride loop's second trip"
    ops, outs = run_check(d, backend)
    lo = outs["dst"][:, d["C"]:].float()
    assert bool((lo[0] == 0).all()) and bool((lo[d["M"] // 2] != 0).any()), "exact bf16 values give lo == 0; the subnormal differences survive"


# ---------------------------------------------------------------- hardening of the grouped wrapper

def _items(M=70, Kd=72, N=40, r=4, slot0=0):
    z = lambda *s: torch.zeros(*s, dtype=BF)
    return [z(M, 32), z(M, Kd), torch.zeros(r, Kd), z(M, 32), z(M, N), torch.zeros(N, r), r, 1.0, slot0]


@pytest.mark.parametrize("what", ["K % 8", "N % 8", "x stride", "dy stride", "r = 0", "r = 33", "slot0 + r > 32", "grad_down shape", "grad_up dtype",
                                  "grad_up not contiguous"])
def test_grouped_wrapper_refuses(what, monkeypatch):
    """the arguments hcp_lora_wgrad / hcp_lora_wgrad_pair refuse are refused by the grouped wrapper before it binds a library, takes the
    workspace or launches anything (neither is there to be had in this test)."""
    def unreachable(*a):
        raise RuntimeError("the wrapper went on past its argument checks")
    monkeypatch.setattr(K, "lib", unreachable)
    monkeypatch.setattr(K, "_workspace", unreachable)
    it = _items()
    good = [tuple(_items()), None]
    if what == "K % 8":
        it[1], it[2] = torch.zeros(70, 80, dtype=BF)[:, :76], torch.zeros(4, 76)
    elif what == "N % 8":
        it[4], it[5] = torch.zeros(70, 48, dtype=BF)[:, :44], torch.zeros(44, 4)
    elif what == "x stride":
        it[1] = torch.zeros(70, 76, dtype=BF)[:, :72]
    elif what == "dy stride":
        it[4] = torch.zeros(70, 44, dtype=BF)[:, :40]
    elif what == "r = 0":
        it[2], it[5], it[6] = torch.zeros(0, 72), torch.zeros(40, 0), 0
    elif what == "r = 33":
        it[2], it[5], it[6] = torch.zeros(33, 72), torch.zeros(40, 33), 33
    elif what == "slot0 + r > 32":
        it[8] = 29
    elif what == "grad_down shape":
        it[2] = torch.zeros(72, 4)
    elif what == "grad_up dtype":
        it[5] = torch.zeros(40, 4, dtype=torch.float64)
    else:
        it[5] = torch.zeros(40, 8)[:, :4]
    good[1] = tuple(it)
    with pytest.raises(AssertionError, match="layer 1"):
        K.lora_wgrad_grouped(good)


# ---------------------------------------------------------------- mutation test: a torch model of the blocked algorithm with faults

FAULTS = ["last_slab_dropped", "slab_added_twice", "slab_stride_of_the_other_problem", "ragged_row_block_dropped", "lo_half_dropped",
          "pcol0_off_by_one", "store_instead_of_add", "scale_twice_on_the_direct_path", "transposed_index_swapped", "q_tail_tile_unwritten",
          "write_to_rank_row_P", "neighbouring_bucket_word_touched", "one_slab_too_many", "slab_q_tail_written"]
# the last two leave every gradient element right: only the workspace check (written floats == the mirrored rule) sees them, and
# q_tail_tile_unwritten — the producer leaves the last column tile's slabs NaN — is seen by it first
WORKSPACE_FAULTS = ("q_tail_tile_unwritten", "one_slab_too_many", "slab_q_tail_written")
# the faults the old gate (tensor-maximum relerr < 2e-2, or 2e-4 with split T / U; operands of one scale, gradients from zero, no
# sentinel around them) passes at these shapes (asserted below): from zero a store is an add, and nothing looked beside the gradients
# or into the workspace
OLD_GATE_PASSES = {"store_instead_of_add", "neighbouring_bucket_word_touched", "one_slab_too_many", "slab_q_tail_written"}
MUT_SLABS = _one(lay(1000, 136, 264, 5, slot0=3, t_split=True, u_split=True))        # three token ranges of 384, 384, 232 rows; qt 2 and 3
MUT_DIRECT = _one(lay(100, 136, 264, 5, slot0=3, t_split=True, u_split=True))        # one range: rows 64 + 36


def model(d, ops, fault=None):
    """fp32 model of lora_wgrad_grouped_kernel + its reduce for a one-layer call: 64-row tiles accumulated per token range, the ranges'
    [P x 128] slabs in a NaN workspace, the ordered reduce (one range: the direct add); returns run()'s dict."""
    l, o = d["layers"][0], ops[0]
    M, r, s0, scale = l["M"], l["r"], l["slot0"], l["scale"]
    _, plan, _, _, units = LC.group_plan(d["layers"], d["grid_blocks"], 1 << 40)
    g = plan[0]
    splits, rows = g["splits"], g["rows"]
    bucket = ops["bucket0"].clone()
    gd, gu = LC.grad_views(d, bucket)[0]
    ws = torch.full((units * 128 + 4096,), LC.NAN)
    pc = s0 + (1 if fault == "pcol0_off_by_one" else 0)
    begin = 0
    for z, (Lv, lo, R, Q, qt, qt_other) in enumerate(((o["U"], o["ulo"], o["x"], l["K"], g["qt0"], g["qt1"]),
                                                      (o["T"], o["tlo"], o["dy"], l["N"], g["qt1"], g["qt0"]))):
        Lc = LC._cols(Lv, pc, r) + (0 if fault == "lo_half_dropped" or not lo else LC._cols(Lv, lo + pc, r))
        Rd = R.double()
        part = []
        for s in range(splits):
            acc = torch.zeros(r, Q)
            me = min(M, (s + 1) * rows)
            for m0 in range(s * rows, me, 64):
                m1 = min(me, m0 + 64)
                if fault == "ragged_row_block_dropped" and m1 - m0 < 64:
                    continue
                acc = acc + (Lc[m0:m1].T @ Rd[m0:m1]).float()
            part.append(acc)
        out = gd if z == 0 else gu.T
        if splits == 1:
            v = part[0] * scale * (scale if fault == "scale_twice_on_the_direct_path" else 1.0)
            out[:] = v if fault == "store_instead_of_add" else out + v
        else:
            tile = r * 128
            slabs = ws[begin:begin + splits * qt * tile].view(splits, qt, tile)
            for s in range(splits):
                for t in range(qt):
                    w = min(128, Q - t * 128)
                    blk = part[s][:, t * 128:t * 128 + w]
                    if fault == "q_tail_tile_unwritten" and z == 1 and t == qt - 1:
                        continue                                                   # the producing workgroups of the last column tile never store
                    if fault == "slab_q_tail_written" and w < 128:
                        slabs[s, t] = 0.0                                          # the q >= Q tail stored too (zeros: no gradient changes)
                    if z == 0:
                        slabs[s, t].view(r, 128)[:, :w] = blk
                    else:
                        slabs[s, t].view(128, r)[:w] = blk.T
            flat = ws[begin:]
            sstride = (qt_other if fault == "slab_stride_of_the_other_problem" else qt) * tile
            for t in range(qt):
                w = min(128, Q - t * 128)
                order = list(range(splits - 1 if fault == "last_slab_dropped" else splits)) + ([1] if fault == "slab_added_twice" else [])
                a = None
                for s in order:
                    e = flat[s * sstride + t * tile:s * sstride + (t + 1) * tile]
                    if z == 0 or (fault == "transposed_index_swapped"):
                        e = e.view(r, 128)[:, :w]
                    else:
                        e = e.view(128, r)[:w].T
                    a = e.clone() if a is None else a + e
                cur = out[:, t * 128:t * 128 + w]
                out[:, t * 128:t * 128 + w] = a * scale if fault == "store_instead_of_add" else cur + a * scale
            begin += splits * qt * tile
            if fault == "one_slab_too_many" and z == 1:
                ws[begin:begin + tile] = 0.0                                       # a workgroup past the grid's end stores its (empty) tile
        if fault == "write_to_rank_row_P" and z == 0:
            row = (LC._cols(Lv, s0 + r, 1).T @ Rd).float().view(-1) * scale              # accumulator row P, stored one row below grad_down
            od = LC.grad_layout(d)[0][0][0]
            bucket[od + r * Q:od + (r + 1) * Q] += row
    if fault == "neighbouring_bucket_word_touched":
        bucket[LC.grad_layout(d)[0][0][0] - 1] = 0.0
    return dict(bucket=bucket, ws=ws, grads=[(gd, gu)])


def _old_operands(d):
    """operands as tests/test_kernels.py drew them: one scale per tensor, random values in every column of T / U, gradients from zero."""
    ops = LC.make_operands(d, "cpu")
    g = torch.Generator().manual_seed(GC.seed_of(d))
    for name, base in ops["_bases"].items():
        base.copy_(torch.randn(base.shape, generator=g).to(BF))
        if name[0] in "UT" and d["layers"][0][name[0].lower() + "_split"]:
            base[:, base.shape[1] // 2:] *= 2.0 ** -8
    ops["bucket0"][LC.HEAD:-LC.TAIL] = 0
    return ops


def _old_gate_passes(d, ops, outs):
    good = model(d, ops)
    relerr = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12))
    tol = 2e-4 if d["layers"][0]["t_split"] else 2e-2
    return all(relerr(a, b) < tol for a, b in zip(outs["grads"][0], good["grads"][0]))


def test_mutations_are_caught():
    passed_old = set()
    ran = set()
    for d in (MUT_SLABS, MUT_DIRECT):
        ops = LC.make_operands(d, "cpu")
        assert LC.check(d, ops, model(d, ops)) <= 1.0                            # the model itself is within the bound
        on_direct = ("scale_twice_on_the_direct_path", "store_instead_of_add", "ragged_row_block_dropped")
        for f in (on_direct if d is MUT_DIRECT else [f for f in FAULTS if f != "scale_twice_on_the_direct_path"]):
            ran.add(f)
            with pytest.raises(AssertionError, match="workspace floats were written" if f in WORKSPACE_FAULTS else None):
                LC.check(d, ops, model(d, ops, f))
            for tsplit in (True, False):
                do = _one(dict(d["layers"][0], t_split=tsplit, u_split=tsplit, ldu=64 if tsplit else 32, ldt=64 if tsplit else 32))
                old = _old_operands(do)
                if f == "lo_half_dropped" and not tsplit:
                    continue
                if _old_gate_passes(do, old, model(do, old, f)):
                    passed_old.add(f)
    assert ran == set(FAULTS)
    print("old gate passes:", sorted(passed_old))
    assert passed_old, "the element-wise check is meant to catch faults that a tensor-maximum relative error cannot see"
    assert passed_old == OLD_GATE_PASSES


def test_checker_message_names_the_element():
    d = MUT_SLABS
    ops = LC.make_operands(d, "cpu")
    with pytest.raises(AssertionError, match=r"layer 0 grad_down of \{.*\"kind\": \"lora_wgrad_grouped\".*p \d+ q \d+: got .* ref .* err .* bound"):
        LC.check(d, ops, model(d, ops, "last_slab_dropped"))


# ---------------------------------------------------------------- the recorded launches of the workloads

def load_fixture():
    return json.loads(FIXTURE.read_text())


def _layer_of(geo):
    l = lay(geo["M"], geo["K"], geo["N"], geo["r"], slot0=geo["slot0"], u_split=bool(geo["u_lo"]), t_split=bool(geo["t_lo"]),
            ldx=geo["ldx"], ldy=geo["ldy"], ldu=geo["ldu"], ldt=geo["ldt"])
    assert (geo["u_lo"] in (0, geo["ldu"] // 2)) and (geo["t_lo"] in (0, geo["ldt"] // 2)), geo
    return l


def test_fixture_is_sorted_and_agrees_with_the_mirror():
    fx = load_fixture()
    geos = fx["geometries"]
    keys = [json.dumps(g["geo"], sort_keys=True) for g in geos]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for g in geos:
        geo = g["geo"]
        assert geo["splits"] == LC.group_geometry(geo["M"], geo["K"], geo["N"], geo["r"], geo["target"])[3], geo
        assert all(n > 0 for n in g["count"].values()) and set(g["count"]) <= {"sd15", "sdxl"}
    assert sorted(fx["calls"]) == ["sd15", "sdxl"]
    for w, calls in fx["calls"].items():
        for c in calls:
            assert all(0 <= i < len(geos) and geos[i]["geo"]["target"] == c["target"] for i in c["layers"]), w


def _fixture_geometries():
    return [g["geo"] for g in load_fixture()["geometries"]] if FIXTURE.exists() else []


@pytest.fixture(scope="module")
def product():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from conftest import Backend, gpu_box_check
    gpu_box_check()
    K._set_backend_for_tests(None)
    assert K.lib().hcp_is_emulated() == 0
    yield Backend("gpu")
    K._set_backend_for_tests(None)
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("geo", _fixture_geometries(), ids=lambda g: "M{M}_K{K}_N{N}_r{r}_s{slot0}_t{target}".format(**g))
def test_recorded_geometry_at_its_real_shape(product, geo):
    d = D("lora_wgrad_grouped", layers=[_layer_of(geo)], grid_blocks=geo["target"])
    target, plan, *_ = LC.group_plan(d["layers"], d["grid_blocks"], 1 << 40)
    assert target == geo["target"] and plan[0]["splits"] == geo["splits"]
    run_check(d, product, "recorded geometry")


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["sd15", "sdxl"])
def test_recorded_grouped_call(product, workload):
    fx = load_fixture()
    call = max(fx["calls"][workload], key=lambda c: len(c["layers"]))
    layers = [_layer_of(fx["geometries"][i]["geo"]) for i in call["layers"]]
    d = D("lora_wgrad_grouped", layers=layers, grid_blocks=K.WGRAD_GRID_BLOCKS, ws_bytes=K._WS_BYTES)      # the workspace the workload ran with
    assert LC.group_plan(layers, d["grid_blocks"], d["ws_bytes"])[0] == call["target"]
    run_check(d, product, "recorded call")


@pytest.mark.gpu
def test_fresh_trace_equals_fixture(product, tmp_path):
    """the trace tool, as the command it is, in a process of its own: the two full-size trainers it builds (tens of GiB on the device)
    are gone with it, whatever would keep them alive here."""
    import subprocess
    torch.cuda.empty_cache()                          # what this process only caches is free for the tool
    out = tmp_path / "lora_launches.json"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "trace_lora_launches.py"), str(out)], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert out.read_text() == FIXTURE.read_text(), "the LoRA launches of the workloads changed: re-run `python tools/trace_lora_launches.py` on the GPU"


@pytest.mark.gpu
def test_report(product):
    """worst err / bound per kind over what this session ran (alone: over the base cases), at each NL of MEASURED_NL and under the module's."""
    if not RATIOS:
        for d in _base_cases():
            run_check(d, product)
    for k in sorted(RATIOS):
        print(f"[lora_check] {k:22s} " + "  ".join(f"NL={g:g}: {RATIOS_AT[g][k]:.3f}" for g in MEASURED_NL) + f"   module NL={LC.NL:g}: {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS_AT[1.0].values()) and all(v <= 0.5 for v in RATIOS.values()), RATIOS
    assert math.isfinite(max(RATIOS_AT[1.0].values()))
