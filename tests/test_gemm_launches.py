"""Every GEMM-family launch of the benchmark workloads, element-wise against float64 (tests/gemm_check.py).

CPU: the checker itself catches each injected fault (mutation test), the fixture tests/golden/gemm_launches.json is consistent with the
dispatch tables (csrc/gemm_tuned_loaders.inc, csrc/gemm_tuned.inc), and every (mode, tile id, split-K, loaders) combination the tables
can select runs through the interpreter at a reduced, ragged shape.
GPU: each recorded descriptor at its real shape through the product library's own dispatch, each table entry no recorded launch reaches
at its key, bit-identical reruns, and a fresh trace of the four workloads equal to the fixture (tools/trace_gemm_launches.py)."""
import json
import math
import sys
from pathlib import Path

import pytest
import torch

import gemm_check as GC
from hcp_diffusion_amd import kernels as K

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "gemm_launches.json"
BF = torch.bfloat16


def load_fixture():
    return json.loads(FIXTURE.read_text())


def relerr(a, b):
    a = a.float().cpu(); b = b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# ---------------------------------------------------------------- CPU: the checker catches what relerr misses

MUT_GEMM = dict(kind="gemm", M=70, N=48, K=256, K2=0, lda=256, ldb=256, ldd=56, lda2=0, ldb2=0, ldr=48, bias=True, rowbias=True,
                rows_per_group=16, residual=True, residual_lo=False, want_lo=False, gact=False, alpha=1.0, out_f32=False)
MUT_CONV = dict(kind="conv3x3", M=72, N=16, K=144, K2=0, mode=0, B=2, Hs=6, Ws=6, C1=16, C2=0, Cout=16, stride=1, upsample=0, pad=1,
                Ho=6, Wo=6, ldd=16, ldr=0, bias=False, rowbias=False, rows_per_group=0, residual=False, out_f32=False)
TM, TN, TK = 32, 16, 64          # output tile and K tile of the blocked model; two split-K slabs of two K tiles each


def _blocked_gemm(ops, fault=None):
    """fp32 blocked accumulation of MUT_GEMM, written into a NaN-poisoned [M, ldd] buffer, with one optional injected fault."""
    d = MUT_GEMM
    M, N, Kd = d["M"], d["N"], d["K"]
    A, B = ops["a"].float(), ops["b"].float()
    if fault == "ragged_row_from_above":
        A = A.clone(); A[M - 1] = A[M - 2]
    parts = [A[:, t:t + TK] @ B[:, t:t + TK].T for t in range(0, Kd, TK)]
    slabs = [parts[0] + parts[1], parts[2] + parts[3]]
    acc = slabs[0] + slabs[1]
    rows, cols = slice(TM, 2 * TM), slice(TN, 2 * TN)
    if fault == "dropped_k_tile":
        acc[rows, cols] -= parts[1][rows, cols]
    if fault == "slab_twice":
        acc[rows, cols] += slabs[1][rows, cols]
    if fault == "dropped_k_tile_small_row":           # the same fault confined to the row of smallest scale (~50x below the largest)
        r = int(A.abs().amax(1).argmin())
        acc[r, cols] -= parts[1][r, cols]
    bias = ops["bias"].clone()
    if fault == "bias_column":
        bias[int(bias.abs().argmax())] = 0
    grp = torch.arange(M) // d["rows_per_group"]
    if fault == "rowbias_group":
        grp[d["rows_per_group"]] -= 1
    v = acc + bias + ops["rowbias"][grp] + ops["residual"].float()
    base = GC._poisoned((M, N), d["ldd"], BF, "cpu", float("nan"))
    base[:, :N] = v.to(BF)
    if fault == "gap_written":
        base[5, N + 2] = 0
    if fault == "ragged_tail_unwritten":
        base[2 * TM:, 2 * TN:N] = float("nan")
    return {"base": base, "out": base[:, :N]}


def _conv_with_edge_fault(ops, fault):
    d = MUT_CONV
    acc, _ = GC.conv_forward_ref(ops["x1"], None, ops["wp"], 1, 0, 1, d["Ho"], d["Wo"])
    out = acc.float().view(d["B"], d["Ho"], d["Wo"], d["N"])
    if fault:                     # output pixel (b 1, y 0, x 0), tap (ky 1, kx 0): reads image 0's last pixel instead of the zero pad
        out[1, 0, 0] += ops["wp"][:, 1, 0, :].float() @ ops["x1"][0, -1, -1].float()
    return {"out": out.to(BF)}


GEMM_FAULTS = ["dropped_k_tile", "dropped_k_tile_small_row", "slab_twice", "bias_column", "rowbias_group", "ragged_row_from_above", "gap_written", "ragged_tail_unwritten"]


def test_checker_catches_every_injected_fault():
    ops = GC.make_operands(MUT_GEMM, "cpu")
    clean = _blocked_gemm(ops)
    assert GC.check(MUT_GEMM, ops, clean) <= 1.0
    ref = GC.references(MUT_GEMM, ops, clean)[0].ref
    missed_by_relerr = []
    for fault in GEMM_FAULTS:
        got = _blocked_gemm(ops, fault)
        with pytest.raises(AssertionError):
            GC.check(MUT_GEMM, ops, got)
        if fault != "gap_written" and relerr(got["out"], ref) < 1e-2:
            missed_by_relerr.append(fault)
    cops = GC.make_operands(MUT_CONV, "cpu")
    assert GC.check(MUT_CONV, cops, _conv_with_edge_fault(cops, False)) <= 1.0
    got = _conv_with_edge_fault(cops, True)
    with pytest.raises(AssertionError, match="row 36 col"):
        GC.check(MUT_CONV, cops, got)
    cref = GC.references(MUT_CONV, cops, got)[0].ref
    if relerr(got["out"].view(-1, MUT_CONV["N"]), cref) < 1e-2:
        missed_by_relerr.append("conv_edge_tap")
    print(f"faults the old relerr < 1e-2 gate passes: {missed_by_relerr}")
    assert missed_by_relerr, "the element-wise check is meant to catch faults that a tensor-max relative error cannot see"


def test_checker_message_names_the_worst_element():
    ops = GC.make_operands(MUT_GEMM, "cpu")
    got = _blocked_gemm(ops, "bias_column")
    col = int(ops["bias"].abs().argmax())
    with pytest.raises(AssertionError, match=rf"out of .*\"M\": 70.*col {col}: got .* ref .* err .* bound"):
        GC.check(MUT_GEMM, ops, got)


# ---------------------------------------------------------------- CPU: the tables and the fixture

def _count_entries(name):
    return sum(1 for ln in (GC.CSRC / name).read_text().splitlines() if ln.startswith("{"))


def test_tables_parse_and_fixture_is_consistent():
    tables = GC.load_tables()
    assert len(tables) == _count_entries("gemm_tuned_loaders.inc") + _count_entries("gemm_tuned.inc")
    for e in tables:
        assert e["mode"] in (0, 1, 2, 3) and 0 <= e["cfg"] <= 16 or (e["mode"] == 3 and e["cfg"] == -1), e
        assert e["split"] in (1, 2, 4, 8, 16) and e["loaders"] in (0, 1, 3, 4, 10, 11, 12), e
        assert e["mode"] != 3 or e["has_k2"] == 1, f"fused-LoRA keys carry has_K2 = 1: {e}"
    fx = load_fixture()
    assert fx and fx == sorted(fx, key=lambda x: json.dumps(x["desc"], sort_keys=True))
    seen = set()
    for item in fx:
        d = item["desc"]
        key = json.dumps(d, sort_keys=True)
        assert key not in seen
        seen.add(key)
        assert set(item["count"]) <= {"sd15", "dreambooth", "controlnet", "sdxl"} and all(n > 0 for n in item["count"].values())
        if d["kind"] in ("conv3x3", "wgrad_conv3x3"):
            assert d["M"] == d["B"] * d["Ho"] * d["Wo"] and d["K"] == 9 * (d["C1"] + d["C2"]), d
            if d["kind"] == "conv3x3" and d["mode"] == 0:
                up = 2 if d["upsample"] else 1
                assert d["Ho"] == (d["Hs"] * up + (2 if d["pad"] else 1) - 3) // d["stride"] + 1, d
            if d["kind"] == "conv3x3" and d["mode"] == 1:
                assert d["Hs"] == (d["Ho"] - 1) // d["stride"] + 1 and d["C1"] == d["K"] // 9, d
        if d["kind"] in ("gemm", "gemm_lora", "gemm_geglu_bwd"):
            assert d["lda"] >= d["K"] and d["ldb"] >= d["K"] and d["ldd"] >= d["N"] * (2 if d["kind"] == "gemm_geglu_bwd" else 1), d
        if d["kind"] == "wgrad_linear":
            assert d["ldy"] >= d["N"] and d["ldx"] >= d["K"] and d["ldw"] >= d["K"], d
    reached = reached_entries(fx)
    unreached = [e for e in tables if id(e) not in reached]
    print(f"{len(fx)} descriptors reach {len(reached)} of {len(tables)} table entries; {len(unreached)} are synthesized at their key")
    for e in unreached:
        d = GC.synth_descriptor(e)
        hit = [GC.lookup(tables, k) for k in GC.dispatch_keys(d, tables)]
        assert GC.lookup(tables, GC.entry_key(e)) in hit, e


def reached_entries(fx):
    tables = GC.load_tables()
    reached = set()
    for item in fx:
        for key in GC.dispatch_keys(item["desc"], tables):
            e = GC.lookup(tables, key)
            if e is not None:
                reached.add(id(e))
    return reached


def unreached_descriptors():
    tables = GC.load_tables()
    if not FIXTURE.exists():
        return []
    reached = reached_entries(load_fixture())
    out = []
    for e in tables:
        if id(e) in reached:
            continue
        first = GC.lookup(tables, GC.entry_key(e))
        if first is not e and id(first) in reached:
            continue                           # shadowed by an earlier entry with the same key that a recorded launch already runs
        out.append((f"{e['table']}:{e['line']}", GC.synth_descriptor(e)))
    return out


# ---------------------------------------------------------------- CPU: every selectable (mode, tile, split, loaders) on the interpreter

def _deepest_ring(ld):
    return 4 if ld == 3 else ld


def table_combos():
    """distinct (mode, tile id, split, loaders as production sets them, has concat source) of the entries lookup_tuned can return."""
    tables = GC.load_tables()
    out = set()
    for e in tables:
        if GC.lookup(tables, GC.entry_key(e)) is not e or e["cfg"] < 0:
            continue                           # shadowed; or the fused-LoRA two-launch form (plain GEMMs of their own table keys)
        split = 1 if e["mode"] == 3 else e["split"]
        concat = 1 if e["mode"] == 1 and GC._CONV_COMMENT.search(e["comment"]) and not e["comment"].split("+")[1].startswith("0 ") else 0
        out.add((e["mode"], e["cfg"], split, _deepest_ring(e["loaders"]), e["stride"], e["up"], e["has_k2"], concat))
    return sorted(out)


COMBOS = table_combos()


def _reduced_descriptor(mode, cfg, split, s, up, k2, concat):
    kdeep = max(192, 128 * split)                                  # >= two 64-deep K tiles per split: the split is real
    if mode == 0:
        return dict(kind="gemm", M=70, N=168, K=kdeep, K2=32 if k2 else 0, lda=kdeep + 8, ldb=kdeep, ldd=176, lda2=32 if k2 else 0,
                    ldb2=32 if k2 else 0, ldr=168, bias=True, rowbias=True, rows_per_group=32, residual=True, residual_lo=False,
                    want_lo=False, gact=False, alpha=1.0, out_f32=False)
    if mode == 3:
        return dict(kind="gemm_lora", M=70, N=168, K=192, lda=192, ldb=192, ldd=168, ldt=32, want_t=True, ldr=168, bias=True,
                    residual=True, residual_lo=False, want_lo=False, gact=False)
    C1, C2 = 64, 64 if concat else 0
    if mode == 1:
        Hs = 5 if up else 9
        Ho = (Hs * (2 if up else 1) - 1) // s + 1
        return dict(kind="conv3x3", M=2 * Ho * Ho, N=40, K=9 * (C1 + C2), K2=32 if k2 else 0, mode=0, B=2, Hs=Hs, Ws=Hs, C1=C1, C2=C2,
                    Cout=40, stride=s, upsample=up, pad=1, Ho=Ho, Wo=Ho, ldd=40, ldr=40, bias=True, rowbias=True, rows_per_group=Ho * Ho,
                    residual=True, out_f32=False)
    Ho = 9
    Hs = (Ho - 1) // s + 1
    return dict(kind="conv3x3", M=2 * Ho * Ho, N=40, K=9 * 64, K2=0, mode=1, B=2, Hs=Hs, Ws=Hs, C1=64, C2=0, Cout=40, stride=s, upsample=0,
                pad=1, Ho=Ho, Wo=Ho, ldd=40, ldr=40, bias=False, rowbias=False, rows_per_group=0, residual=True, out_f32=False)


@pytest.fixture
def emu_tools():
    from conftest import emu_cdll
    K._set_backend_for_tests(emu_cdll())
    yield K.lib()
    L = K.lib()
    L.hcp_debug_set_gemm_config(-1); L.hcp_debug_set_gemm_loaders(-1)
    K._set_backend_for_tests(None)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "m{}_id{}_s{}_ld{}_st{}_up{}_k2{}_cat{}".format(*c))
def test_table_combo_on_the_interpreter(emu_tools, combo):
    mode, cfg, split, ld, s, up, k2, concat = combo
    d = _reduced_descriptor(mode, cfg, split, s, up, k2, concat)
    ops = GC.make_operands(d, "cpu")
    L = emu_tools
    L.hcp_debug_set_gemm_config(1024 + cfg + 64 * split)
    L.hcp_debug_set_gemm_loaders(ld)
    outs = GC.run(d, ops)
    GC.check(d, ops, outs)


# ---------------------------------------------------------------- GPU: real shapes, the product library's dispatch

WORST = {}


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
    """check at the real shape; a second run into differently poisoned buffers gives identical bits (every kind sums its split-K /
    token-split partials as ordered slabs: no fp32 atomics on these paths)."""
    ops = GC.make_operands(d, dev)
    outs = GC.run(d, ops)
    ratio = GC.check(d, ops, outs)
    again = GC.run(d, ops, fill=float("inf"))
    for name, t in outs.items():
        if name != "base" and t is not None:
            assert torch.equal(_bits(t), _bits(again[name])), f"{name} of {GC.describe(d)} differs between two runs"
    WORST[d["kind"]] = max(WORST.get(d["kind"], 0.0), ratio)
    del ops, outs, again


def _fixture_ids():
    if not FIXTURE.exists():
        return []
    return [(f"{i:03d}_{it['desc']['kind']}", it["desc"]) for i, it in enumerate(load_fixture())]


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [d for _, d in _fixture_ids()], ids=[i for i, _ in _fixture_ids()])
def test_recorded_launch_against_float64(product, desc):
    _check_twice(desc, product)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [d for _, d in unreached_descriptors()], ids=[i for i, _ in unreached_descriptors()])
def test_unreached_table_entry_against_float64(product, desc):
    _check_twice(desc, product)


@pytest.mark.gpu
def test_fresh_trace_equals_fixture(product):
    sys.path.insert(0, str(ROOT / "tools"))
    import trace_gemm_launches as T
    fresh = T.dumps(T.trace_all())
    assert fresh == FIXTURE.read_text(), "the launches of the benchmark workloads changed: re-run `python tools/trace_gemm_launches.py` on the GPU"


@pytest.mark.gpu
def test_report_worst_ratio_per_kind(product):
    print("\nworst err / bound per kind: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
