"""TEST HELPER: element-wise float64 check of one LoRA weight-gradient / pack launch (csrc/lora.hip through kernels.lora_wgrad /
lora_wgrad_pair / lora_wgrad_grouped / lora_pack / split_hi_lo), described by a plain dict:

    kind  lora_wgrad            one layer dict + transpose_out (False: grad_down = U^T x; True: grad_up = dY^T T);
                                wide=True: a rank above 32 through the loop of ops._lora_grads_wide (both gradients, 32 rank
                                columns a launch, grad_up at out_col0 = 0, 32, ...)
    kind  lora_wgrad_pair       one layer dict
    kind  lora_wgrad_grouped    layers = [layer dicts], grid_blocks (kernels.WGRAD_GRID_BLOCKS for the call), ws_bytes (0: what the
                                launch needs and a margin); a layer with same_as = i names layer i's gradients again (a second pass)
    kind  lora_pack             descs = [dict(K, N, r, alpha, slot0, n0, null)] (one K: they share x), Ntot / bu_ld of the shared images
    kind  split_hi_lo           M, C
    layer dict                  M, K, N, r, scale, slot0, u_split, t_split, ldx, ldy, ldu, ldt (layer(...) fills the defaults);
                                a leading dimension above the width is a column-slice view of a wider tensor
    grad_offset                 float offset of the first gradient view inside the one flat fp32 bucket (the views follow each other
                                without a gap, as the blocks of a real bucket do)

    ops = make_operands(desc, device)          # seeded from a hash of the descriptor
    outs = run(desc, ops)                      # the wrappers; kernels._workspace patched to a NaN-filled buffer
    ratio = check(desc, ops, outs)             # |out - ref| <= bound at every element, else AssertionError; returns max err / bound

Operands.  x and dy: N(0,1) with one scale 2^U(-4,4) per row.  T and U: the same times one scale 2^U(-3,3) per rank column, so neither
a quiet gradient row nor a quiet column can hide behind a loud one.  A split T / U is the two bf16 images of ONE fp32 tensor.  Every
operand is a view into a larger NaN-filled buffer: the rows at and beyond M, the gap columns beyond the width, and the columns of T / U
outside the layer's rank slots [slot0, slot0 + r) are NaN (a NaN there reaches only accumulator rows the kernel discards; any leak into
a live element shows).  The gradients are views at grad_offset into one bucket and start from N(0,1) (the kernels add); every other
bucket word holds a sentinel bit pattern.

Running.  The workspace the wrappers take is NaN-filled.  run() compares every input buffer, padding included, bit for bit with a copy
taken before the call.  check() then asserts that every bucket word outside the gradient views still holds the sentinel, and that the
workspace floats that are no longer NaN are exactly the ones the mirrored launch rules (wgrad_launch, group_geometry, group_plan
below) say a slab element (p < P, q < Q) lives at — qt * splits * nprob * P * 128 minus the q >= Q tails, none when splits == 1.  This
is how the split count of the non-grouped forms, which no API returns, is observed; a reduce thread that reads a word no workgroup
wrote adds a NaN into its gradient element.

Reference and bound per gradient element (U = 2^-24):
    ref = start + scale * sum_m (L_hi + L_lo)[m, p] R[m, q]                                              float64
    accumulation   NL * gemm_check.gamma(M) * |scale| * sum_m (|L_hi| + |L_lo|)[m, p] |R[m, q]|          (the slab sums belong to it)
    scale          U |scale * acc|
    add            U (|start| + |ref|)
    output         nothing: the gradient is fp32
A gradient named twice in one grouped call carries the three terms of both passes.

NL is the one free constant (gemm_check.GAMMA = 2 times NL in front of sqrt(M) U): sqrt(M) is the typical size of an accumulated
rounding error, not its maximum.  It scales the accumulation term only.

lora_pack: every element of every image is compared bit for bit.  The images start as a sentinel, the expected image is the sentinel
with (w * float32(alpha)).to(bfloat16) — one fp32 multiply, round to nearest even — or w.to(bfloat16) written at the descriptor's
placement.  split_hi_lo: hi bit-equal to v.to(bf16), lo to (v - hi.float()).to(bf16).

Measured on MI355X, product library, against this float64 reference over every descriptor of tests/test_lora_launches.py and the
fixture tests/golden/lora_launches.json (its GPU report test prints these figures at every run), worst err / bound:
                          NL = 1    1/2     1/4     1/8     1/16
  lora_wgrad              0.402    0.402   0.696   1.141   1.679
  lora_wgrad_pair         0.470    0.542   0.647   0.743   1.359
  lora_wgrad_grouped      0.489    0.622   0.747   0.942   1.444
  recorded geometries     0.133    0.257   0.483   0.861   1.423      (44 distinct layer geometries of sd15 / sdxl, one-layer calls)
  recorded calls          0.230    0.437   0.794   1.343   2.054      (the whole grouped call of sd15, 160 layers, and of sdxl)
NL = 1 is the smallest power of two that leaves the worst ratio at or below 0.5 (0.489; NL = 1/2 gives 0.622): the bound is
gemm_check's own for wgrad_linear, which measured 0.458 there.  The small cases set it — a few rows, where sqrt(M) allows little and
the two roundings of a (hi + lo) product pair weigh most; the real shapes stay below 0.25.  The interpreter passes under the same NL.
Nothing failed: every element within its bound, no NaN, no sentinel touched, the workspace written exactly where the mirrored rules
say, lora_pack and split_hi_lo bit-equal to torch (subnormal residuals included) — csrc/lora.hip is unchanged.

Mutation test (tests/test_lora_launches.py::test_mutations_are_caught): a torch model of the blocked algorithm with fourteen faults —
last_slab_dropped, slab_added_twice, slab_stride_of_the_other_problem, ragged_row_block_dropped, lo_half_dropped, pcol0_off_by_one,
store_instead_of_add, scale_twice_on_the_direct_path, transposed_index_swapped, q_tail_tile_unwritten, write_to_rank_row_P,
neighbouring_bucket_word_touched, one_slab_too_many, slab_q_tail_written — every one is caught; the last two change no gradient element
and are seen by the workspace check alone.  The old gate (tensor-maximum relerr < 2e-2, 2e-4 with split operands) run on the faulty
model with operands as tests/test_kernels.py drew them (one scale per tensor, gradients from zero, nothing around them) passes
store_instead_of_add, neighbouring_bucket_word_touched, one_slab_too_many and slab_q_tail_written."""
import json
import math

import torch

import gemm_check as GC
from gemm_check import BF, SENTINEL16, SENTINEL32, U, Item

NL = 1.0

WGRAD_KINDS = ("lora_wgrad", "lora_wgrad_pair", "lora_wgrad_grouped")
NAN = float("nan")
BQ, BM, SLAB_ROWS = 128, 64, 64          # WG_BQ, WG_BM, WGRAD_SLAB_ROWS of csrc/lora.hip
HEAD, TAIL = 4, 40                       # sentinel words in front of (HEAD + grad_offset) and behind the gradient views


def cdiv(a, b):
    return (a + b - 1) // b


def layer(M, K, N, r, **kw):
    d = dict(M=M, K=K, N=N, r=r, scale=0.5, slot0=0, u_split=False, t_split=False)
    d.update(kw)
    d.setdefault("ldx", K)
    d.setdefault("ldy", N)
    d.setdefault("ldu", 64 if d["u_split"] else 32)
    d.setdefault("ldt", 64 if d["t_split"] else 32)
    return d


def desc(kind, *a, **kw):
    if kind in ("lora_wgrad", "lora_wgrad_pair"):
        extra = {k: kw.pop(k) for k in ("transpose_out", "wide", "grad_offset") if k in kw}
        d = dict(layer(*a, **kw), kind=kind, grad_offset=0)
        if kind == "lora_wgrad":
            d.update(transpose_out=False, wide=False)
        d.update(extra)
        return d
    assert not a
    d = dict(kind=kind)
    if kind == "lora_wgrad_grouped":
        d.update(grid_blocks=16384, ws_bytes=0, grad_offset=0)
    d.update(kw)
    return d


def layers_of(d):
    return d["layers"] if d["kind"] == "lora_wgrad_grouped" else [d]


def describe(d):
    return json.dumps(d, sort_keys=True)


# ---------------------------------------------------------------- the launch rules of csrc/lora.hip as data

def wgrad_launch(Qa, Qb, nprob, M, P):
    """wgrad_launch: (column tiles of the shared grid, token ranges, rows per range)."""
    qt = cdiv(max(Qa, Qb) if nprob == 2 else Qa, BQ)
    s = cdiv(1024, qt * nprob)
    s = min(s, cdiv(M, 2 * BM), M // (SLAB_ROWS * P))
    s = max(s, 1)
    rows = cdiv(cdiv(M, s), BM) * BM
    return qt, cdiv(M, rows), rows


def group_geometry(M, K, N, P, target):
    """hcp_lora_wgrad_group_geometry: (workgroups, qt_down, qt_up, splits, rows_per_split)."""
    t0, t1 = cdiv(K, BQ), cdiv(N, BQ)
    P = max(P, 1)
    s = cdiv(target if target > 0 else 256, t0 + t1)
    s = min(s, cdiv(M, 4 * BM), M // (SLAB_ROWS * P))
    s = max(s, 1)
    rows = cdiv(cdiv(M, s), BM) * BM
    s = cdiv(M, rows)
    return (t0 + t1) * s, t0, t1, s, rows


def group_plan(layers, grid_blocks, ws_bytes):
    """kernels.lora_wgrad_grouped for one pass: the target it settles on and, per layer, dict(qt0, qt1, splits, rows, block_begin,
    slab_begin (units of 128 floats), tile_begin); total blocks, tiles, slab units."""
    target = max(8, min(256, grid_blocks // len(layers)))
    while True:
        plan, begin, tiles, units = [], 0, 0, 0
        for l in layers:
            nb, t0, t1, s, rows = group_geometry(l["M"], l["K"], l["N"], l["r"], target)
            plan.append(dict(qt0=t0, qt1=t1, splits=s, rows=rows, block_begin=begin, slab_begin=units, tile_begin=tiles))
            begin += nb
            tiles += t0 + t1
            if s > 1:
                units += nb * l["r"]
        if units * 512 <= ws_bytes or target <= 1:
            return target, plan, begin, tiles, units
        target //= 2


def passes_of(d):
    """a grouped call's passes as lists of layer indices: a layer that names an earlier layer's gradients goes to the second."""
    L = d["layers"]
    first = [i for i, l in enumerate(L) if l.get("same_as") is None]
    rest = [i for i, l in enumerate(L) if l.get("same_as") is not None]
    return [first] + ([rest] if rest else [])


def problems(d):
    """the single-form launches of a lora_wgrad descriptor: (which, P, column of L, out_col0, transposed)."""
    if not d["wide"]:
        return [("up" if d["transpose_out"] else "down", d["r"], 0, 0, d["transpose_out"])]
    out = []
    for j in range(0, d["r"], 32):
        pj = min(32, d["r"] - j)
        out += [("down", pj, j, 0, False), ("up", pj, j, j, True)]
    return out


def ws_need(d):
    """floats of workspace the descriptor's launches use (the largest of its launches: they reuse the buffer from its start)."""
    k = d["kind"]
    if k == "lora_wgrad":
        need = 0
        for which, P, _, _, _ in problems(d):
            Q = d["N"] if which == "up" else d["K"]
            qt, s, _ = wgrad_launch(Q, Q, 1, d["M"], P)
            need = max(need, qt * s * P * BQ if s > 1 else 0)
        return need
    if k == "lora_wgrad_pair":
        qt, s, _ = wgrad_launch(d["K"], d["N"], 2, d["M"], d["r"])
        return 2 * qt * s * d["r"] * BQ if s > 1 else 0
    need = 0
    for p in passes_of(d):
        need = max(need, group_plan([d["layers"][i] for i in p], d["grid_blocks"], d["ws_bytes"] or (1 << 40))[4] * BQ)
    return need


def _mark(mask, begin, splits, qt_grid, qt, P, Q, transposed):
    """the slab elements (p < P, q < Q) of one problem: slabs [split][column tile of the grid] from float `begin`."""
    reg = mask[begin:begin + splits * qt_grid * P * BQ].view(splits, qt_grid, P * BQ)[:, :qt]
    w = Q - (qt - 1) * BQ
    if transposed:
        reg = reg.view(splits, qt, BQ, P)
        reg[:, :qt - 1] = True
        reg[:, qt - 1, :w] = True
    else:
        reg = reg.view(splits, qt, P, BQ)
        reg[:, :qt - 1] = True
        reg[:, qt - 1, :, :w] = True


def ws_written(d, n, device):
    """bool [n]: the workspace floats the descriptor's launches write, by the mirrored rules."""
    mask = torch.zeros(n, dtype=torch.bool, device=device)
    k = d["kind"]
    if k == "lora_wgrad":
        for which, P, _, _, tr in problems(d):
            Q = d["N"] if which == "up" else d["K"]
            qt, s, _ = wgrad_launch(Q, Q, 1, d["M"], P)
            if s > 1:
                _mark(mask, 0, s, qt, qt, P, Q, tr)
    elif k == "lora_wgrad_pair":
        qt, s, _ = wgrad_launch(d["K"], d["N"], 2, d["M"], d["r"])
        if s > 1:
            P = d["r"]
            _mark(mask, 0, s, qt, cdiv(d["K"], BQ), P, d["K"], False)
            _mark(mask, qt * s * P * BQ, s, qt, cdiv(d["N"], BQ), P, d["N"], True)
    else:
        for p in passes_of(d):
            ls = [d["layers"][i] for i in p]
            _, plan, _, _, _ = group_plan(ls, d["grid_blocks"], d["ws_bytes"] or (1 << 40))
            for l, g in zip(ls, plan):
                if g["splits"] > 1:
                    b, P = g["slab_begin"] * BQ, l["r"]
                    _mark(mask, b, g["splits"], g["qt0"], g["qt0"], P, l["K"], False)
                    _mark(mask, b + g["qt0"] * g["splits"] * P * BQ, g["splits"], g["qt1"], g["qt1"], P, l["N"], True)
    return mask


def reduce_is_vector(P, ldo, transposed, float_offset):
    """wgrad_reduce_tile's choice (float_offset: of the problem's `out` pointer inside a 16-byte aligned bucket)."""
    return (not transposed or P % 4 == 0) and ldo % 4 == 0 and float_offset % 4 == 0


def grad_layout(d):
    """[(offset of grad_down, offset of grad_up, width of grad_up)] per layer in floats from the bucket's start, and the bucket's size."""
    L = layers_of(d)
    off = HEAD + d["grad_offset"]
    out = []
    for l in L:
        if l.get("same_as") is not None:
            out.append(out[l["same_as"]])
            continue
        out.append((off, off + l["r"] * l["K"], l["r"]))
        off += l["r"] * (l["K"] + l["N"])
    return out, off + TAIL


# ---------------------------------------------------------------- operands

def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _act(g, M, width, ld, dev):
    """([M, width] view at a column offset of a NaN [M + 2, ld] buffer, the buffer)."""
    base = torch.full((M + 2, ld), NAN, dtype=BF, device=dev)
    c0 = 8 if ld - width >= 8 else 0
    v = (g.randn(M, width) * g.scales(M, -4, 4)[:, None]).to(BF)
    base[:M, c0:c0 + width] = v
    return base[:M, c0:c0 + width], base


def _rank_operand(g, M, r, slot0, split, ld, dev, width=32):
    """T / U: (the view the wrapper takes, the buffer, the column offset of the residual half)."""
    v = g.randn(M, r) * g.scales(M, -4, 4)[:, None] * g.scales(r, -3, 3)[None, :]
    hi = v.to(BF)
    half = ld // 2 if split else ld
    lo_off = half if split else 0
    c0 = 32 if half >= 64 and width == 32 else 0
    base = torch.full((M + 2, ld), NAN, dtype=BF, device=dev)
    base[:M, c0 + slot0:c0 + slot0 + r] = hi
    if split:
        base[:M, lo_off + c0 + slot0:lo_off + c0 + slot0 + r] = (v - hi.float()).to(BF)
    view = base[:M] if c0 == 0 and ld in (32, 64) else base[:M, c0:c0 + width]
    return view, base, lo_off


def make_operands(d, device):
    g = GC._Gen(d, device)
    dev = g.dev
    k = d["kind"]
    o = {"_bases": {}}
    if k in WGRAD_KINDS:
        wide = k == "lora_wgrad" and d["wide"]
        for i, l in enumerate(layers_of(d)):
            x, o["_bases"][f"x{i}"] = _act(g, l["M"], l["K"], l["ldx"], dev)
            dy, o["_bases"][f"dy{i}"] = _act(g, l["M"], l["N"], l["ldy"], dev)
            w = 64 if wide else 32
            Uv, o["_bases"][f"U{i}"], ulo = _rank_operand(g, l["M"], l["r"], l["slot0"], l["u_split"], l["ldu"], dev, w)
            Tv, o["_bases"][f"T{i}"], tlo = _rank_operand(g, l["M"], l["r"], l["slot0"], l["t_split"], l["ldt"], dev, w)
            o[i] = dict(x=x, dy=dy, U=Uv, T=Tv, ulo=ulo, tlo=tlo)
        layout, n = grad_layout(d)
        b = torch.empty(n, dtype=torch.float32, device=dev)
        b.view(torch.int32).fill_(SENTINEL32)
        for l, (od, ou, _) in zip(layers_of(d), layout):
            if l.get("same_as") is None:
                cnt = l["r"] * (l["K"] + l["N"])
                b[od:od + cnt] = g.randn(cnt)
        o["bucket0"] = b
    elif k == "lora_pack":
        for i, p in enumerate(d["descs"]):
            wd = g.randn(p["r"], p["K"]) * g.scales(p["r"], -4, 4)[:, None]
            wu = g.randn(p["N"], p["r"]) * g.scales(p["N"], -4, 4)[:, None]
            for w in (wd, wu):               # exact ties of the bf16 rounding, towards an even and towards an odd neighbour
                f = w.view(-1)
                f[::7] = (1.0 + (2 * torch.arange(f[::7].numel(), device=dev) + 1) * 2.0 ** -8).float()
            o[i] = dict(w_down=wd.contiguous(), w_up=wu.contiguous())
    elif k == "split_hi_lo":
        M, C = d["M"], d["C"]
        v = g.randn(M, C) * g.scales(M, -4, 4)[:, None]
        v[0] = v[0].to(BF).float()                                   # exact bf16 values: lo == 0
        v[M // 2] = (v[M // 2] * 2.0 ** -121)                        # |v| ~ 2^-121: v - hi is an fp32 subnormal
        v[M - 1, ::2] = 0.0
        o["v"] = v.contiguous()
    else:
        raise ValueError(k)
    return o


def _tensors(ops):
    out = dict(ops["_bases"])
    for k, v in ops.items():
        if torch.is_tensor(v):
            out[k] = v
        elif isinstance(v, dict) and k != "_bases" and not ops["_bases"]:
            out.update({f"{k}.{n}": t for n, t in v.items() if torch.is_tensor(t)})
    return out


# ---------------------------------------------------------------- running the wrappers

class _Block:
    """what ops._lora_grads_wide asks of a LoRA block."""
    def __init__(self, rank, alpha, gd, gu):
        self.rank, self.alpha_f, self._g = rank, alpha, (gd, gu)

    def grad_views(self):
        return self._g


def grad_views(d, bucket):
    layout, _ = grad_layout(d)
    return [(bucket[od:od + l["r"] * l["K"]].view(l["r"], l["K"]), bucket[ou:ou + l["N"] * w].view(l["N"], w))
            for l, (od, ou, w) in zip(layers_of(d), layout)]


def pack_images(d, dev):
    """the four shared images of a lora_pack descriptor, sentinel-filled."""
    mk = lambda *s: torch.full(s, 0, dtype=torch.int16, device=dev).fill_(SENTINEL16).view(BF)
    bu_ld = d["bu_ld"] or 32
    return dict(ad=mk(32, d["descs"][0]["K"]), adt=mk(d["descs"][0]["K"], 32), bu=mk(d["Ntot"], bu_ld), but=mk(32, d["Ntot"]))


def run(d, ops):
    from hcp_diffusion_amd import kernels as K
    from hcp_diffusion_amd import ops as O
    k = d["kind"]
    before = {n: t.clone() for n, t in _tensors(ops).items()}
    outs = {}
    if k in WGRAD_KINDS:
        dev = ops["bucket0"].device
        n = d.get("ws_bytes") // 4 if d.get("ws_bytes") else ws_need(d) + 4096
        ws = torch.full((max(n, 4),), NAN, dtype=torch.float32, device=dev)
        bucket = ops["bucket0"].clone()
        gv = grad_views(d, bucket)
        outs.update(bucket=bucket, ws=ws, grads=gv)
        real_ws, real_gb = K._workspace, K.WGRAD_GRID_BLOCKS
        K._workspace = lambda t: ws.view(torch.uint8)
        try:
            if k == "lora_wgrad":
                o, (gd, gu) = ops[0], gv[0]
                if d["wide"]:
                    O._lora_grads_wide(_Block(d["r"], d["scale"], gd, gu), d["slot0"], o["T"], o["dy"], o["U"], o["x"])
                elif d["transpose_out"]:
                    K.lora_wgrad(o["T"][:, d["slot0"]:], o["dy"], gu, d["r"], d["scale"], True, lo=o["tlo"])
                else:
                    K.lora_wgrad(o["U"][:, d["slot0"]:], o["x"], gd, d["r"], d["scale"], False, lo=o["ulo"])
            elif k == "lora_wgrad_pair":
                o, (gd, gu) = ops[0], gv[0]
                K.lora_wgrad_pair(o["U"], o["x"], gd, o["T"], o["dy"], gu, d["r"], d["scale"])
            else:
                K.WGRAD_GRID_BLOCKS = d["grid_blocks"]
                items = [(ops[i]["U"], ops[i]["x"], gv[i][0], ops[i]["T"], ops[i]["dy"], gv[i][1], l["r"], l["scale"], l["slot0"],
                          ops[i]["ulo"], ops[i]["tlo"]) for i, l in enumerate(d["layers"])]
                outs["keep"] = K.lora_wgrad_grouped(items)
        finally:
            K._workspace, K.WGRAD_GRID_BLOCKS = real_ws, real_gb
    elif k == "lora_pack":
        import struct
        dev = ops[0]["w_down"].device
        img = pack_images(d, dev)
        buf = bytearray()
        for i, p in enumerate(d["descs"]):
            ptr = lambda name: 0 if p.get("null") else img[name].data_ptr()
            buf += struct.pack("<6Q3if4i", ops[i]["w_down"].data_ptr(), ops[i]["w_up"].data_ptr(), ptr("ad"), ptr("adt"), img["bu"].data_ptr(),
                               ptr("but"), p["K"], p["N"], p["r"], p["alpha"], p["slot0"], p["n0"], d["Ntot"], d["bu_ld"])
        table = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
        K.lora_pack(table, len(d["descs"]))
        outs.update(img)
    else:
        outs["dst"] = K.split_hi_lo(ops["v"])
    if ops.get("bucket0") is not None and ops["bucket0"].is_cuda:
        torch.cuda.synchronize()
    for n, t in _tensors(ops).items():
        assert torch.equal(_bits(t), _bits(before[n])), f"{describe(d)}: the launch changed its input {n}"
    return outs


# ---------------------------------------------------------------- float64 references and bounds

def _cols(t, c, r):
    """columns [c, c + r) of the rows of a 2-D view, reaching beyond the view's own width where the residual half lies there."""
    return torch.as_strided(t, (t.shape[0], r), t.stride(), t.storage_offset() + c).double()


def _problem(L, Lmag, R, start, scale, M):
    """(ref, accumulation term at NL = 1, the other terms) [r, Q] of start + scale L^T R."""
    acc, mag = L.T @ R, Lmag.T @ R.abs()
    ref = start + scale * acc
    return ref, GC.gamma(M) * abs(scale) * mag, U * (scale * acc).abs() + U * (start.abs() + ref.abs())


def wgrad_items(calls, starts, grads):
    """Items of the gradients after `calls`, in order: dicts U, x, T, dy, r, slot0, ulo, tlo, own (index into starts / grads),
    scale_down / scale_up (None: that problem does not run), col0 (first rank column of grad_up).  starts / grads: (grad_down, grad_up)
    per gradient pair before and after.  A gradient no call adds to keeps a zero bound: it must hold its starting bits."""
    z = lambda t: torch.zeros_like(t, dtype=torch.float64)
    st = [[a.double(), [z(a), z(a)], b.double().T.contiguous(), [z(b).T.contiguous(), z(b).T.contiguous()]] for a, b in starts]
    for c in calls:
        s, r, M = st[c["own"]], c["r"], c["x"].shape[0]
        for scale, L, lo, R, k in ((c["scale_down"], c["U"], c["ulo"], c["x"], 0), (c["scale_up"], c["T"], c["tlo"], c["dy"], 2)):
            if scale is None:
                continue
            val = _cols(L, c["slot0"], r)
            mag = val.abs()
            if lo:
                l2 = _cols(L, lo + c["slot0"], r)
                val, mag = val + l2, mag + l2.abs()
            c0 = c.get("col0", 0) if k == 2 else 0
            ref, ba, bo = _problem(val, mag, R.double(), s[k][c0:c0 + r], scale, M)
            s[k] = s[k].clone()
            s[k][c0:c0 + r] = ref
            s[k + 1][0][c0:c0 + r] += ba
            s[k + 1][1][c0:c0 + r] += bo
    items = []
    for own, s in enumerate(st):
        if own not in {c["own"] for c in calls}:
            continue                                  # (a second naming of an earlier pair: checked there)
        a = Item(f"layer {own} grad_down", grads[own][0].double(), s[0], NL * s[1][0] + s[1][1])
        b = Item(f"layer {own} grad_up (p, q = rank column, output row)", grads[own][1].double().T, s[2], NL * s[3][0] + s[3][1])
        a.dims = b.dims = ("p", "q")
        (a.acc, a.other), (b.acc, b.other) = s[1], s[3]
        items += [a, b]
    return items


def calls_of(d, ops):
    L = layers_of(d)
    single = d["kind"] == "lora_wgrad" and not d["wide"]
    wide = d["kind"] == "lora_wgrad" and d["wide"]
    order = [i for p in passes_of(d) for i in p] if d["kind"] == "lora_wgrad_grouped" else [0]
    out = []
    for i in order:
        l, o = L[i], ops[i]
        out.append(dict(U=o["U"], x=o["x"], T=o["T"], dy=o["dy"], r=l["r"], slot0=l["slot0"], ulo=o["ulo"], tlo=o["tlo"],
                        own=l["same_as"] if l.get("same_as") is not None else i,
                        scale_down=None if single and d["transpose_out"] else 1.0 if wide else l["scale"],
                        scale_up=None if single and not d["transpose_out"] else l["scale"]))
    return out


def references(d, ops, outs):
    return wgrad_items(calls_of(d, ops), grad_views(d, ops["bucket0"]), outs["grads"])


def check_call(items, starts, what, down=True, up=True):
    """the element-wise check for a hand-built call (tests/test_kernels.py): items as kernels.lora_wgrad_grouped takes them, after the
    launch; starts: the (grad_down, grad_up) values before it, per item (None: zeros; an item that names an earlier item's gradients
    again shares its start)."""
    calls, st, gr, seen = [], [], [], {}
    for n, it in enumerate(items):
        U_, x, gd, T, dy, gu, r, scale = it[:8]
        slot0 = it[8] if len(it) > 8 else 0
        ulo, tlo = (it[9], it[10]) if len(it) > 10 else (0, 0)
        key = (gd.data_ptr(), gu.data_ptr())
        if key not in seen:
            seen[key] = len(st)
            s = starts[n] if starts is not None and starts[n] is not None else (torch.zeros_like(gd), torch.zeros_like(gu))
            st.append(s)
            gr.append((gd, gu))
        calls.append(dict(U=U_, x=x, T=T, dy=dy, r=r, slot0=slot0, ulo=ulo, tlo=tlo, own=seen[key],
                          scale_down=scale if down else None, scale_up=scale if up else None))
    return GC.compare(what, wgrad_items(calls, st, gr), describe=str)


def pack_expected(d, ops):
    dev = ops[0]["w_down"].device
    img = pack_images(d, dev)
    for i, p in enumerate(d["descs"]):
        wd, wu = ops[i]["w_down"], ops[i]["w_up"]
        al = torch.tensor(p["alpha"], dtype=torch.float32, device=dev)
        s, r, n0 = p["slot0"], p["r"], p["n0"]
        if not p.get("null"):
            img["ad"][s:s + r] = wd.to(BF)
            img["adt"][:, s:s + r] = (wd * al).to(BF).T
            img["but"][s:s + r, n0:n0 + p["N"]] = wu.to(BF).T
        img["bu"][n0:n0 + p["N"], s:s + r] = (wu * al).to(BF)
    return img


def _same_bits(d, name, got, want):
    bad = _bits(got) != _bits(want)
    if bool(bad.any()):
        i = int(torch.argmax(bad.reshape(-1).int()))
        row, col = divmod(i, got.shape[1])
        raise AssertionError(f"{name} of {describe(d)}: {int(bad.sum())} elements differ in bits from torch's round-to-nearest-even; first at "
                             f"row {row} col {col}: got {float(got[row, col])!r} (0x{int(_bits(got)[row, col]) & 0xFFFF:04x}) "
                             f"want {float(want[row, col])!r} (0x{int(_bits(want)[row, col]) & 0xFFFF:04x})")


def measure(items, nl=1.0):
    """worst err / bound of references()' items with NL = nl, without asserting (NaN counts as infinite): only the accumulation term
    is rescaled, nothing is recomputed."""
    worst = 0.0
    for it in items:
        err, bound = (it.got - it.ref).abs(), nl * it.acc + it.other
        r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        worst = max(worst, float(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r).max()))
    return worst


def check(d, ops, outs, items=None):
    k = d["kind"]
    if k == "lora_pack":
        want = pack_expected(d, ops)
        for name in ("ad", "adt", "bu", "but"):
            _same_bits(d, name, outs[name], want[name])
        return 0.0
    if k == "split_hi_lo":
        v = ops["v"]
        hi = v.to(BF)
        _same_bits(d, "(hi | lo)", outs["dst"], torch.cat([hi, (v - hi.float()).to(BF)], 1))
        return 0.0
    layout, n = grad_layout(d)
    live = torch.zeros(n, dtype=torch.bool, device=outs["bucket"].device)
    for l, (od, ou, w) in zip(layers_of(d), layout):
        live[od:od + l["r"] * l["K"]] = True
        live[ou:ou + l["N"] * w] = True
    bad = (outs["bucket"].view(torch.int32) != SENTINEL32) & ~live
    if bool(bad.any()):
        i = int(torch.argmax(bad.int()))
        raise AssertionError(f"{describe(d)}: bucket word {i} outside the gradient views was written ({int(bad.sum())} words; the views "
                             f"are {[(a, b) for a, b, _ in layout]})")
    ws = outs["ws"]
    got, want = ~torch.isnan(ws), ws_written(d, ws.numel(), ws.device)
    if not torch.equal(got, want):
        i = int(torch.argmax((got != want).int()))
        raise AssertionError(f"{describe(d)}: {int(got.sum())} workspace floats were written, the launch rule predicts {int(want.sum())}; "
                             f"first difference at float {i} ({'written' if bool(got[i]) else 'not written'})")
    return GC.compare(d, items if items is not None else references(d, ops, outs), describe=describe)
