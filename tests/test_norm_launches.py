"""Every norm launch (csrc/norm.hip) element-wise against float64 (tests/norm_check.py): every instantiation of the one-launch slab
kernels at both workgroup sizes, the row-chunk path in every (TX, R) geometry the models launch, every LayerNorm NV x HL class, the
affine-gradient kernel in both forms — interpreted on the CPU and, under -m gpu, on the product library (the row-chunk cases on the
tuning build, through hcp_debug_set_gn_target).

The mutation test shows what the checker sees that the older gates (tests/test_kernels.py: tensor-maximum relerr < 1e-2 for y / dx,
< 2e-3 for dgamma / dbeta, the group means to 1e-4) do not: of the twelve faults of FAULTS, run on operands as those tests drew them (one scale per tensor;
1021 rows for GroupNorm), the old gates pass those of OLD_GATES_PASS."""
import math

import pytest
import torch

import gemm_check as GC
import norm_check as NC
from hcp_diffusion_amd import kernels as K

BF = torch.bfloat16

# ---------------------------------------------------------------- the dispatch rules as data


def test_all_instantiations_counts():
    inst = NC.all_instantiations()
    slab = {i[1:3] for i in inst if i[0] == "gn_slab_fwd"}
    assert len(slab) == 11, "HCP_GN_SLAB_SWITCH has 11 arms"
    assert len([i for i in inst if i[0] == "gn_slab_fwd"]) == 15 and len([i for i in inst if i[0].startswith("ln_")]) == 16


def test_slab_switch_arms_match_the_source():
    """the (NCH, CE) pairs of HCP_GN_SLAB_SWITCH, read from the source, are the mirror's."""
    import re
    src = (GC.CSRC / "norm.hip").read_text()
    arms = {(int(a), int(b)) for a, b in re.findall(r"HCP_LAUNCH\(\(KERNEL<(\d+), (\d+)>\)", src)}
    assert arms == {i[1:3] for i in NC.all_instantiations() if i[0] == "gn_slab_fwd"}
    assert {(int(a), b == "true") for a, b in re.findall(r"HCP_LN_FWD\((\d), (true|false)\)", src)} == \
        {i[1:3] for i in NC.all_instantiations() if i[0] == "ln_fwd"}


def test_gn_geom_mirror_matches_the_library(tbackend):
    """hcp_groupnorm_workspace_bytes exposes nchunk: the mirror agrees over a grid of shapes, at the default target and at others."""
    L = K.lib()
    try:
        for target in (512, 65536, 5):
            L.hcp_debug_set_gn_target(target)
            for B in (1, 2, 4):
                for HW in (1, 5, 37, 64, 100, 1021, 1024, 4096, 16384):
                    for C in (8, 40, 128, 320, 512, 960, 1280, 2560, 8192):
                        G = 4 if C < 128 else 32
                        assert L.hcp_groupnorm_workspace_bytes(B, HW, C, G) == NC.gn_workspace_bytes(B, HW, C, G, target), (target, B, HW, C)
    finally:
        L.hcp_debug_set_gn_target(512)


def test_affine_grad_blocks_mirror_never_launches_an_empty_block():
    """affine_grad_blocks returns cdiv(rows, rows_per_block) as the grid's row blocks, so a launch with several splits and an empty last
    block cannot occur: the kernel's `mb < me` guard is never taken by any launch, and no case here can exercise it.  This holds for the
    mirror (compared by reading with csrc/norm.hip affine_grad_blocks: the library exports nothing that exposes it)."""
    for rows in (1, 31, 32, 33, 45, 129, 300, 769, 1025, 4096):
        for ct in (1, 2, 5, 40, 171, 1024):
            for groups in (1, 2, 4):
                blocks, rpb = NC.affine_grad_blocks(rows, ct, groups)
                assert rpb % 32 == 0 and blocks * rpb >= rows > (blocks - 1) * rpb


# ---------------------------------------------------------------- running and collecting

MEASURED_NG = (1.0, 0.5, 0.25, 0.125)
RATIOS_AT = {g: {} for g in MEASURED_NG}        # NG -> item -> worst err / bound over the cases this session ran on the GPU
RATIOS = {}                                     # the same under the module's NG, from check()


def _collect(d, ops, outs, be):
    kind = d["kind"]
    into = RATIOS if be.is_gpu else {}
    pre = kind[:2] + ("_chunk" if kind in NC.GN_KINDS and not NC.uses_slab(d) else "") + "."
    one_row = kind == "ln_affine" and d["M"] == 1 or kind == "gn_affine" and d["B"] * d["HW"] == 1
    name = lambda k: pre + k + ("[one row]" if one_row and k in ("dgamma", "dbeta") else "")
    r = {}
    worst = NC.check(d, ops, outs, ratios=r)
    for k, v in r.items():
        into[name(k)] = max(into.get(name(k), 0.0), v)
    if be.is_gpu:
        for g, into_g in RATIOS_AT.items():
            for k, v in NC.measure(d, ops, outs, g=g).items():
                into_g[name(k)] = max(into_g.get(name(k), 0.0), v)
    return r


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def run_check(d, be):
    ops = NC.make_operands(d, be.device)
    outs = NC.run(d, ops)
    outs["ratios"] = _collect(d, ops, outs, be)
    if be.is_gpu and d["kind"] not in ("gn_affine", "ln_affine"):            # no atomics in these kernels: identical bits
        again = NC.run(d, ops)
        for k in ("y", "stats", "dx", "dx_lo"):
            if outs.get(k) is not None:
                assert torch.equal(_bits(outs[k]), _bits(again[k])), f"{NC.describe(d)}: {k} differs between two runs"
    return outs


# ---------------------------------------------------------------- every slab instantiation at the smallest shape that selects it

# (C, HW, NCH, CE, threads) with G = 4: odd HW so dead chunks exist; Cg = 10 / 30 / 34 straddle an 8-channel thread of the other kernels;
# C = 8 and 16 are the magic == 0 arm (one chunk per row) of CE = 2 and 4
SLAB_CASES = [(40, 37, 1, 2, 256), (40, 101, 2, 2, 256), (40, 203, 4, 2, 256), (40, 409, 8, 2, 256), (40, 700, 4, 2, 1024),
              (40, 1021, 8, 2, 1024), (120, 601, 16, 2, 1024), (136, 1000, 32, 2, 1024),
              (8, 61, 1, 2, 256), (8, 300, 2, 2, 256), (8, 1021, 4, 2, 256),
              (16, 50, 1, 4, 256), (16, 509, 2, 4, 256), (16, 1021, 4, 4, 256), (16, 2045, 8, 4, 256), (16, 4093, 4, 4, 1024),
              (32, 511, 4, 4, 256), (32, 1023, 8, 4, 256), (32, 2047, 4, 4, 1024), (32, 4095, 8, 4, 1024), (32, 8191, 16, 4, 1024)]
FLAGS = [(True, True), (True, False), (False, True), (False, False)]     # (silu, addend); a backward descriptor runs and checks its forward too


def slab_descs(C, HW, emu):
    B = 1 if emu and HW * C > 100000 else 2      # the interpreter's run time; no case is skipped
    return [NC.desc("gn_bwd", B=B, HW=HW, C=C, G=4, silu=s, addend=a) for s, a in FLAGS]


def launched(d):
    """the instantiations a descriptor's run launches (a backward / affine descriptor runs its forward first)."""
    fwd = dict(d, kind=d["kind"][:2] + "_fwd")
    return {NC.selected(fwd), NC.selected(d)}


@pytest.mark.parametrize("C,HW,nch,ce,nt", SLAB_CASES)
def test_groupnorm_slab_instantiation(backend, C, HW, nch, ce, nt):
    for d in slab_descs(C, HW, not backend.is_gpu):
        assert NC.selected(d) == ("gn_slab_bwd", nch, ce, nt), NC.selected(d)
        assert NC.gn_slab_geom(HW, C, 4)["total"] < nch * nt, "dead chunks exist"
        outs = run_check(d, backend)
        assert bool(torch.isnan(outs["ws_fwd"]).all()) and bool(torch.isnan(outs["ws_bwd"]).all()), "the slab kernels leave the workspace alone"


# ---------------------------------------------------------------- the row-chunk path

def _target_for(B, HW, C, k):
    """a workgroup target under which rows_per_chunk = k R."""
    R = NC.gn_geom(B, HW, C)["R"]
    for t in list(range(1, 600)) + [65536]:
        if NC.gn_geom(B, HW, C, t)["rows_per_chunk"] == k * R:
            return t
    raise ValueError((B, HW, C, k))


def chunk_cases(gpu):
    """(B, HW, C, rows_per_chunk / R): every (TX, R) the models launch (C = 320 / 960: Cg = 10 / 30 straddle), each with the shortest
    chunk (4 R: a ragged last chunk of fewer than R rows) and with 7 R (one 4-row batch + 3, three 2-row batches + 1, per thread);
    nchunk = 1; nchunk > 8 J (C = 1280: J = 5, 42 chunks; C = 320: J = 7, 58); SDXL's C = 2560 at nchunk = 256 (GPU only: run time)."""
    out = []
    for C in (128, 256, 512, 320, 640, 960, 1280, 1920, 2560, 8192):
        R = max(256 // (C // 8), 1)
        out.append((2, 8 * R + max(R - 1, 1), C, 4))
        if C <= 1280:
            out.append((1, 14 * R - 1, C, 7))
    out += [(2, 5, 640, 4), (1, 165, 1280, 4), (1, 24 * 57 + 5, 320, 4)]
    if gpu:
        out.append((1, 1021, 2560, 4))
    return out


CHUNK_CASES = chunk_cases(True)


def chunk_descs(B, HW, C, k):
    t = _target_for(B, HW, C, k)
    return [NC.desc("gn_bwd", B=B, HW=HW, C=C, G=32, silu=s, addend=a, slab=False, target=t) for s, a in FLAGS]


@pytest.mark.parametrize("B,HW,C,k", CHUNK_CASES)
def test_groupnorm_row_chunk_path(tbackend, B, HW, C, k):
    if not tbackend.is_gpu and (B, HW, C, k) not in chunk_cases(False):
        pytest.skip("interpreter run time (2.6 M elements); the geometry class R = 1 / 320 threads runs at HW = 9")
    for d in chunk_descs(B, HW, C, k):
        ge = NC.gn_geom(B, HW, C, d["target"])
        assert ge["rows_per_chunk"] == k * ge["R"] and NC.selected(d) == ("gn_chunk_bwd",)
        r = run_check(d, tbackend)["ratios"]
        assert {"ws_mean", "ws_M2", "ws_S1", "ws_S2"} <= set(r), "the workspace partials are items on this path"


def test_row_chunk_cases_cover_what_they_claim():
    geoms = {C: NC.gn_geom(B, HW, C, _target_for(B, HW, C, k)) for B, HW, C, k in CHUNK_CASES if k == 4}
    assert {(g["TX"], g["R"]) for g in geoms.values()} == {(16, 16), (32, 8), (64, 4), (40, 6), (80, 3), (120, 2), (160, 1), (240, 1),
                                                            (320, 1), (1024, 1)}
    seen = set()
    for B, HW, C, k in CHUNK_CASES:
        g = NC.gn_geom(B, HW, C, _target_for(B, HW, C, k))
        tail = HW - (g["nchunk"] - 1) * g["rows_per_chunk"]
        seen |= {"ragged<R"} if tail < g["R"] or g["R"] == 1 and tail < g["rows_per_chunk"] else set()
        seen |= {"nchunk=1"} if g["nchunk"] == 1 else set()
        seen |= {"second merge round"} if g["nchunk"] > 8 * (g["threads"] // 32) else set()
        seen |= {"4+3 / 2+2+2+1"} if k == 7 else set()
    assert seen == {"ragged<R", "nchunk=1", "second merge round", "4+3 / 2+2+2+1"}


# ---------------------------------------------------------------- LayerNorm: every NV x HL

LN_C = (8, 320, 512, 520, 1024, 1032, 2048, 2560, 4096)
LN_M = (1, 3, 4, 9)
LN_FLAGS = [dict(x_lo=x, addend=a, addend_lo=al, want_lo=w) for x in (False, True) for a, al in ((False, False), (True, False), (True, True))
            for w in (False, True)]


def ln_descs(C):
    return [NC.desc("ln_bwd", M=M, C=C, **f) for M in LN_M for f in LN_FLAGS]


@pytest.mark.parametrize("C", LN_C)
def test_layernorm_every_class(backend, C):
    for d in ln_descs(C):
        run_check(d, backend)


# ---------------------------------------------------------------- affine gradients

AFFINE = [NC.desc("gn_affine", B=2, HW=300, C=40, G=4, silu=True), NC.desc("gn_affine", B=3, HW=45, C=320, G=32, silu=True),
          NC.desc("gn_affine", B=1, HW=33, C=8, G=4), NC.desc("gn_affine", B=2, HW=130, C=128, G=32, silu=True),
          NC.desc("gn_affine", B=2, HW=257, C=960, G=32),
          NC.desc("ln_affine", M=300, C=40), NC.desc("ln_affine", M=45, C=320), NC.desc("ln_affine", M=33, C=8),
          NC.desc("ln_affine", M=257, C=128), NC.desc("ln_affine", M=1, C=4096)]


@pytest.mark.parametrize("i", range(len(AFFINE)))
def test_affine_gradients(backend, i):
    d = AFFINE[i]
    rows = d.get("HW") or d["M"]
    blocks, rpb = NC.affine_grad_blocks(rows, (d["C"] + 63) // 64, d.get("B", 1))
    run_check(d, backend)
    assert rows % 32 or rows == 1 or blocks > 1


def test_affine_cases_cover_what_they_claim():
    geo = [(d.get("HW") or d["M"], NC.affine_grad_blocks(d.get("HW") or d["M"], (d["C"] + 63) // 64, d.get("B", 1))) for d in AFFINE]
    assert any(b > 1 and rows % rpb and rows % 32 for rows, (b, rpb) in geo), "several row blocks with a ragged last one"
    assert {8, 40, 320} <= {d["C"] for d in AFFINE}


# ---------------------------------------------------------------- the set that runs is the set that exists

def test_every_instantiation_has_a_case():
    for emu in (True, False):
        ran = set()
        for C, HW, *_ in SLAB_CASES:
            for d in slab_descs(C, HW, emu):
                ran |= launched(d)
        for c in chunk_cases(not emu):
            for d in chunk_descs(*c):
                ran |= launched(d)
        for C in LN_C:
            for d in ln_descs(C):
                ran |= launched(d)
        for d in AFFINE:
            ran |= launched(d)
        assert NC.all_instantiations() - ran == set() and ran - NC.all_instantiations() == set()


# ---------------------------------------------------------------- mutation test: a torch model of the blocked algorithms with faults

FAULTS = ["ragged_last_row_dropped", "straddling_thread_group_off_by_one", "stats_of_neighbouring_sample", "c2_omitted",
          "silu_grad_omitted_in_quietest_group", "addend_dropped_in_last_chunk", "dead_slab_chunk_not_masked",
          "magic_row_division_off_by_one", "affine_tail_rows_dropped", "dbeta_channel_doubled", "ln_padding_lane_in_variance",
          "dx_lo_from_unrounded"]
# which of them the old gates pass when the faulty model runs on operands as tests/test_kernels.py drew them (_old_operands: one scale
# per tensor) at 1021 rows for GroupNorm, 5 rows for LayerNorm (asserted below; tests/norm_check.py's docstring records the same set)
OLD_GATES_PASS = {"c2_omitted"}


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def model_gn(d, ops, fault=None):
    """float64 model of GroupNorm forward + backward (+ affine gradients) as the kernels block it, returning run()'s dict."""
    B, HW, C, G, eps = d["B"], d["HW"], d["C"], d["G"], d["eps"]
    Cg, n = C // G, HW * (C // G)
    x = ops["x"].double()
    ga, be = ops["gamma"].double(), ops["beta"].double()
    ge = NC.gn_geom(B, HW, C, d["target"])
    nc, rpc = ge["nchunk"], ge["rows_per_chunk"]
    last0 = (nc - 1) * rpc
    xs = x.clone()
    if fault == "ragged_last_row_dropped":
        xs[:, HW - 1] = 0                                                  # the row adds nothing; the count stays
    x4 = xs.view(B, HW, G, Cg)
    s = x4.sum((1, 3))
    if fault == "dead_slab_chunk_not_masked":
        sl = NC.gn_slab_geom(HW, C, G)
        s = s + (sl["nch"] * sl["nt"] - sl["total"]) * x4[:, 0, :, :sl["ce"]].sum(-1)
    mean = s / n
    M2 = ((x4 - mean.view(B, 1, G, 1)) ** 2).sum((1, 3))
    if fault == "ragged_last_row_dropped":
        M2 = M2 - mean ** 2 * Cg                                           # (the zeroed row's share)
    stats = torch.stack([mean, (M2 / n + eps) ** -0.5], -1).float()
    outs = dict(stats=stats)
    xc, cnt = NC._chunks(d, x4)
    mean_c = xc.sum((2, 4)) / cnt
    live = (torch.arange(rpc).view(1, 1, -1) * Cg < cnt).double().view(1, nc, rpc, 1, 1)
    M2_c = (((xc - mean_c.view(B, nc, 1, G, 1)) ** 2) * live).sum((2, 4))
    if fault == "ragged_last_row_dropped":
        M2_c[:, -1] -= mean_c[:, -1] ** 2 * Cg

    def ws_of(a, b):
        w = torch.full((B * nc * G * 2 + B * G * 2,), float("nan"))
        w[:B * nc * G * 2] = torch.stack([a, b], -1).float().flatten()
        return w
    outs["ws_fwd"] = ws_of(mean_c, M2_c)
    gi = torch.arange(C) // Cg
    if fault == "straddling_thread_group_off_by_one":
        gi = (torch.arange(C) // 8 * 8) // Cg                              # the thread's 8 channels all take its first channel's group
    st = stats.double()
    if fault == "stats_of_neighbouring_sample":
        st = st.roll(1, 0)
    mk, rk = st[:, gi, 0].view(B, 1, C), st[:, gi, 1].view(B, 1, C)
    xh = (x - mk) * rk
    z = xh * ga + be
    y = z * torch.sigmoid(z) if d["silu"] else z
    if fault == "magic_row_division_off_by_one":
        ce = NC.gn_slab_geom(HW, C, G)["ce"]
        r = HW - 1                                                         # chunk r * cpr lands on row r - 1, channel Cg: the next group's first chunk
        y[0, r - 1, Cg:Cg + ce] = ((x[0, r - 1, Cg:Cg + ce] - st[0, 0, 0]) * st[0, 0, 1]) * ga[:ce] + be[:ce]
        y[0, r, :ce] = 0.0                                                 # never written
    outs["y"] = y.to(BF)
    if d["kind"] == "gn_fwd":
        return outs
    st = outs["stats"].double()
    mk, rk = st[:, gi, 0].view(B, 1, C), st[:, gi, 1].view(B, 1, C)
    xh = (x - mk) * rk
    dy = ops["dy"].double()
    sp = _silu_grad(xh * ga + be) if d["silu"] else torch.ones_like(xh)
    if fault == "silu_grad_omitted_in_quietest_group":
        q = int(st[0, :, 1].argmin())
        sp[0, :, q * Cg:(q + 1) * Cg] = 1.0
    dz = dy * sp
    if d["kind"] == "gn_affine":
        keep = torch.ones(HW, 1)
        if fault == "affine_tail_rows_dropped":
            keep[HW // 32 * 32:] = 0
        outs["dgamma"] = (ops["dg0"].double() + (dz * xh * keep).sum((0, 1))).float()
        db = (dz * keep).sum((0, 1))
        if fault == "dbeta_channel_doubled":
            db[C // 2 + 1] *= 2
        outs["dbeta"] = (ops["db0"].double() + db).float()
        return outs
    dxh = dz * ga
    d4, p4 = dxh.view(B, HW, G, Cg), (dxh * xh).view(B, HW, G, Cg)
    outs["ws_bwd"] = ws_of(NC._chunks(d, d4)[0].sum((2, 4)), NC._chunks(d, p4)[0].sum((2, 4)))
    c1 = (d4.sum((1, 3)) / n)[:, gi].view(B, 1, C)
    c2 = (p4.sum((1, 3)) / n)[:, gi].view(B, 1, C)
    if fault == "c2_omitted":
        c2 = c2 * 0
    dx = rk * (dxh - c1 - xh * c2)
    if d["addend"]:
        ad = ops["addend"].double().clone()
        if fault == "addend_dropped_in_last_chunk":
            ad[:, last0:] = 0
        dx = dx + ad
    outs["dx"] = dx.to(BF)
    return outs


def model_ln(d, ops, fault=None):
    M, C, eps = d["M"], d["C"], d["eps"]
    x = ops["x"].double() + (ops["x_lo"].double() if "x_lo" in ops else 0)
    ga, be = ops["gamma"].double(), ops["beta"].double()
    mean = x.mean(1)
    M2 = ((x - mean[:, None]) ** 2).sum(1)
    if fault == "ln_padding_lane_in_variance":
        M2 = M2 + (NC.ln_nv(C) * 512 - C) * mean ** 2
    stats = torch.stack([mean, (M2 / C + eps) ** -0.5], -1).float()
    st = stats.double()
    xh = (x - st[:, :1]) * st[:, 1:]
    outs = dict(stats=stats, y=(xh * ga + be).to(BF))
    dxh = ops["dy"].double() * ga
    g = st[:, 1:] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    for k in ("addend", "addend_lo"):
        if k in ops:
            g = g + ops[k].double()
    outs["dx"] = g.to(BF)
    hi = outs["dx"].double()
    if fault == "dx_lo_from_unrounded":
        hi = (g.float().view(torch.int32) & -65536).view(torch.float32).double()      # the residual of the truncated, not the rounded, dx
    outs["dx_lo"] = (g - hi).to(BF) if d["want_lo"] else None
    return outs


def _old_gates_pass(d, outs, good):
    """the assertions tests/test_kernels.py made of these outputs, `good` standing for their float32 torch reference."""
    def relerr(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12))
    ok = True
    for k, tol in (("y", 1e-2), ("dx", 1e-2)):
        if outs.get(k) is not None:
            ok &= relerr(outs[k], good[k]) < tol
    if d["kind"] in NC.GN_KINDS:
        ok &= relerr(outs["stats"][..., 0], good["stats"][..., 0]) < 1e-4
    if outs.get("dgamma") is not None:
        ok &= relerr(outs["dgamma"], good["dgamma"]) < 2e-3 and relerr(outs["dbeta"], good["dbeta"]) < 2e-3
    if outs.get("dx_lo") is not None:
        ok &= relerr(outs["dx"].double() + outs["dx_lo"].double(), good["dx"].double() + good["dx_lo"].double()) < 1e-4
    return ok


def _old_operands(d):
    """operands as tests/test_kernels.py drew them: one scale for the whole tensor."""
    g = torch.Generator().manual_seed(GC.seed_of(d))
    rn = lambda *s: torch.randn(*s, generator=g)
    C = d["C"]
    o = dict(gamma=rn(C) * 0.5 + 1, beta=rn(C) * 0.3, dg0=rn(C), db0=rn(C))
    if d["kind"] in NC.GN_KINDS:
        shape = (d["B"], d["HW"], C)
        o["x"] = (rn(*shape) * 2 + 0.7).to(BF)
        o["addend"] = rn(*shape).to(BF)
    else:
        shape = (d["M"], C)
        o["x"], o["x_lo"] = NC.split_hi_lo(rn(*shape) * 3 + 1)
        o["addend"], o["addend_lo"] = NC.split_hi_lo(rn(*shape))
    o["dy"] = rn(*shape).to(BF)
    return o


def test_mutations_are_caught():
    chunk = NC.desc("gn_bwd", B=2, HW=53, C=320, G=32, silu=True, addend=True, slab=False, target=65536)     # chunks of 24, 24, 5 rows (R = 6)
    slab = dict(chunk, slab=True, target=512)                                                                # <2,2> @ 256, 247 dead chunks
    aff = NC.desc("gn_affine", B=2, HW=53, C=320, G=32, silu=True)
    ln = NC.desc("ln_bwd", M=5, C=520, x_lo=True, addend=True, addend_lo=True, want_lo=True)                 # NV = 2: 504 padding elements
    which = {"dead_slab_chunk_not_masked": slab, "magic_row_division_off_by_one": slab, "affine_tail_rows_dropped": aff,
             "dbeta_channel_doubled": aff, "ln_padding_lane_in_variance": ln, "dx_lo_from_unrounded": ln}
    passed_old = set()
    for d in (chunk, slab, aff, ln):
        model = model_ln if d["kind"] in NC.LN_KINDS else model_gn
        ops = NC.make_operands(d, "cpu")
        good = model(d, ops)
        assert NC.check(d, ops, good) <= 1.0                               # the model itself is within the bound
        for f in FAULTS:
            if which.get(f, chunk) is not d:
                continue
            bad = model(d, ops, f)
            with pytest.raises(AssertionError):
                NC.check(d, ops, bad)
            do = dict(d, HW=1021) if d["kind"] in NC.GN_KINDS else d          # the old gates on operands as they were used with: one
            old = _old_operands(do)                                            # scale per tensor, 32x32-sized (their GPU shapes)
            if _old_gates_pass(do, model(do, old, f), model(do, old)):
                passed_old.add(f)
    print("old gates pass:", sorted(passed_old))
    assert passed_old == OLD_GATES_PASS


# ---------------------------------------------------------------- GPU report

ACCUMULATION_ITEMS = ("mean", "rstd", "ws_mean", "ws_M2", "ws_S1", "ws_S2", "dgamma", "dbeta")      # ("dgamma[one row]" is not one)


@pytest.mark.gpu
def test_report():
    """worst err / bound per item over what this session ran (alone: over one case of each family), at NG = 1 and under the module's NG.
    The items bounded by accumulation terms (dgamma / dbeta over several rows among them) stay at or below 0.5 under the module's NG; a
    bf16 output, and dgamma / dbeta of a single row, sit at their rounding term (<= 1) whatever NG is (tests/norm_check.py)."""
    from conftest import Backend, gpu_box_check
    from hcp_diffusion_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    gpu_box_check()
    K._set_backend_for_tests(_lib.load_tools())
    try:
        if not RATIOS:
            be = Backend("gpu")
            for d in slab_descs(40, 409, False) + chunk_descs(2, 53, 320, 4) + ln_descs(520)[:12] + AFFINE[:1] + AFFINE[-2:]:
                run_check(d, be)
    finally:
        K._set_backend_for_tests(None)
    for k in sorted(RATIOS):
        print(f"[norm_check] {k:36s} " + "  ".join(f"NG={g:g}: {RATIOS_AT[g][k]:.3f}" for g in MEASURED_NG) + f"   module NG={NC.NG:g}: {RATIOS[k]:.3f}")
    for k, v in RATIOS.items():
        assert v <= (0.5 if k.split(".")[1] in ACCUMULATION_ITEMS else 1.0), (k, v)
    assert math.isfinite(max(RATIOS_AT[1.0].values()))
