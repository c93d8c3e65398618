"""Fused Lion and Adafactor steps on the flat buckets (csrc/optim_factored.hip): kernels against the float64 restatements of
tests/optim_ref.py, the optimizer classes, NativeTrainer's ``optimizer=`` argument and the two native config overlays.

Tolerance of the kernel tests (not fixed in advance): for every case the fp32 torch restatement runs on the CPU next to the float64
one, and its max abs error e32 — per tensor, on p and on each state tensor — is the yardstick: |kernel - f64| <= 4 e32 + ulp32(max|x|)
(x = the compared tensor; for p this is the issue's ulp32(max|p|), for a state tensor it is never larger).  4 covers another summation
order and the hardware rsqrt; the fp32 restatement includes the clip prologue computed in fp32 (optim_ref.clip_factor32), as the
kernels compute it; the ulp floor covers updates smaller than the rounding of what they are added to.

lion_pytorch is not installed; its rule (lion_pytorch/lion_pytorch.py update_fn, the package the reference's
cfgs/train/examples/Lion_optimizer.yaml names) is: p.data.mul_(1 - lr * wd); update = exp_avg.clone().mul_(beta1).add(grad, alpha = 1 -
beta1).sign_(); p.add_(update, alpha = -lr); exp_avg.mul_(beta2).add_(grad, alpha = 1 - beta2) — optim_ref.lion_step line by line."""
import math

import pytest
import torch

import optim_ref
from hcp_diffusion_amd import kernels as K

# (name, logical shape, channels_last storage): the smallest shapes at which each path can go wrong
SHAPES = [
    ("vec3", (3,), False), ("vec4099", (4099,), False),
    ("mat129x200", (129, 200), False), ("mat5x77", (5, 77), False), ("mat320x4", (320, 4), False),
    ("tile8x4_cl", (8, 4, 3, 3), True), ("tile4x8_cl", (4, 8, 3, 3), True), ("tile4x8", (4, 8, 3, 3), False), ("tile16x24_1x1", (16, 24, 1, 1), False),
]
SETTINGS = {
    "ft_sdxl": dict(lr=1e-3, relative_step=False, weight_decay=1e-3),
    "beta1_clip": dict(scale_parameter=False, beta1=0.9, clip_threshold=0.5),
    "warmup": dict(lr=None, relative_step=True, warmup_init=True),
}
CASES = [[s] for s in SHAPES] + [SHAPES]
STATE_KEYS = ("RMS", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "exp_avg")


def ulp32(x):
    x = float(x)
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


class Bucket:
    """The shapes laid out as HostBucket does: 4-element segment padding, 3x3 weights optionally stored channels_last."""

    def __init__(self, shapes, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.shapes, self.offs, n = shapes, [], 0
        for _, shape, _ in shapes:
            self.offs.append(n)
            n += (math.prod(shape) + 3) // 4 * 4
        self.n = n
        self.p0 = [torch.randn(shape, generator=g) * 0.3 for _, shape, _ in shapes]
        self.gs = [[torch.randn(shape, generator=g) * sc for _, shape, _ in shapes] for sc in (0.1, 1.0, 10.0)]

    def view(self, flat, i):
        _, shape, cl = self.shapes[i]
        seg = flat[self.offs[i]:self.offs[i] + math.prod(shape)]
        return seg.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2) if cl else seg.view(shape)

    def flat(self, tensors, dev):
        out = torch.zeros(self.n, dtype=torch.float32)
        for i, t in enumerate(tensors):
            self.view(out, i).copy_(t)
        return out.to(dev)

    def table_rows(self, flat):
        return [(name, self.offs[i], shape, self.view(flat, i).stride()) for i, (name, shape, _) in enumerate(self.shapes)]


_REF = {}


def reference(ci, sname):
    """Per step: the float64 results and the fp32 restatement's error against them, per tensor (computed once per case, shared)."""
    key = (ci, sname)
    if key not in _REF:
        b, kw = Bucket(CASES[ci]), SETTINGS[sname]
        p64, p32 = [p.double() for p in b.p0], [p.clone() for p in b.p0]
        s64, s32 = [{} for _ in p64], [{} for _ in p64]
        steps = []
        for gs in b.gs:
            clip, clip32 = optim_ref.clip_factor(gs, 0.5, 1.0), optim_ref.clip_factor32(gs, 0.5, 1.0)
            want, e32 = [], []
            for i, g in enumerate(gs):
                optim_ref.adafactor_step(p64[i], g.double() * clip, s64[i], **kw)
                optim_ref.adafactor_step(p32[i], g * clip32, s32[i], **kw)
                w = {"p": p64[i].clone()}
                w.update({k: torch.as_tensor(s64[i][k], dtype=torch.float64).clone() for k in STATE_KEYS if k in s64[i]})
                got = {"p": p32[i], **s32[i]}
                want.append(w)
                e32.append({k: float((torch.as_tensor(got[k]).double() - v).abs().max()) for k, v in w.items()})
            steps.append((want, e32))
        _REF[key] = (b, steps)
    return _REF[key]


def run_adafactor(b, kw, dev, nsteps=3, ordered=False):
    """The kernel over bucket b: yields after every step (p views, state views, table).  ordered: the norm through K.sumsq_ordered."""
    p = b.flat(b.p0, dev)
    table = K.AdafactorTable(b.table_rows(p), dev)
    m = torch.zeros_like(p) if kw.get("beta1") is not None else None
    lr = torch.full((1,), kw["lr"], dtype=torch.float32, device=dev) if kw.get("lr") is not None else None
    step, ss = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    part = torch.zeros(K.SUMSQ_PARTIALS, dtype=torch.float32, device=dev)
    kargs = {k: v for k, v in kw.items() if k != "lr"}
    if "relative_step" not in kargs:
        kargs["relative_step"] = lr is None
    for it in range(nsteps):
        g = b.flat(b.gs[it], dev)
        if ordered:
            K.sumsq_ordered(g, ss, part)
        else:
            K.sumsq(g, ss)
        K.adafactor_step(p, g, table, lr, step, m=m, sumsq_t=ss, grad_scale=0.5, max_norm=1.0, **kargs)
        yield it, p, g, m, step, table


@pytest.mark.parametrize("sname", list(SETTINGS))
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[s[0][0] if len(s) == 1 else "bucket" for s in CASES])
def test_adafactor_kernel_vs_float64(backend, ci, sname):
    """Three steps (gradients x 0.1, 1, 10; grad_scale 0.5, clip to norm 1 through K.sumsq) of each shape alone and of all of them in one
    bucket, for FT_sdxl's settings, the beta1 / clip_threshold path and the relative step with warm-up.
    Worst pair measured on the GPU (LAB_NOTEBOOK.md): beta1_clip, mat320x4, step 2, RMS: kernel 2.89e-8, e32 8.7e-10, bound 3.33e-8."""
    b, steps = reference(ci, sname)
    for it, p, g, m, step, table in run_adafactor(b, SETTINGS[sname], backend.device):
        assert step.item() == it + 1
        assert not g.any().item(), "the step leaves the gradients zero"
        want, e32 = steps[it]
        pc, mc = p.cpu(), (m.cpu() if m is not None else None)
        for i, (name, _, _) in enumerate(b.shapes):
            got = {"p": b.view(pc, i), **{k: v.cpu() for k, v in table.views(i).items()}}
            if mc is not None:
                got["exp_avg"] = b.view(mc, i)
            assert set(got) == set(want[i]), (set(got), set(want[i]))
            for k, w in want[i].items():
                err = float((got[k].double() - w).abs().max())
                bound = 4 * e32[i][k] + ulp32(w.abs().max())
                print(f"adafactor {sname} {name} step {it + 1} {k}: kernel {err:.3e} e32 {e32[i][k]:.3e} bound {bound:.3e}")
                assert err <= bound, (sname, name, it, k, err, e32[i][k], bound)


def test_adafactor_restatement_is_the_installed_class():
    """optim_ref.adafactor_step in fp32 is transformers.optimization.Adafactor.step bit for bit (every shape, every setting)."""
    transformers = pytest.importorskip("transformers")
    from transformers.optimization import Adafactor
    for sname, kw in SETTINGS.items():
        b = Bucket(SHAPES)
        params = [torch.nn.Parameter(p.clone()) for p in b.p0]
        opt = Adafactor(params, **kw)
        mine, st = [p.clone() for p in b.p0], [{} for _ in b.p0]
        for gs in b.gs:
            for i, g in enumerate(gs):
                params[i].grad = g.clone()
                optim_ref.adafactor_step(mine[i], g.clone(), st[i], **kw)
            opt.step()
            for i, p in enumerate(params):
                assert torch.equal(p.data, mine[i]), (sname, b.shapes[i][0])
                for k, v in opt.state[p].items():
                    assert torch.equal(torch.as_tensor(v), torch.as_tensor(st[i][k])), (sname, b.shapes[i][0], k)


def test_adafactor_bucket_step_is_bit_reproducible(backend):
    """No floating-point atomic on the path: the mixed bucket stepped twice from identical inputs gives identical bits.  The gradient
    norm comes from K.sumsq_ordered: K.sumsq adds its block sums (9 workgroups for this bucket) with fp32 atomics, so ITS last bit, and
    through the clip factor everything after it, differs from run to run — seen on the GPU with this very test."""
    outs = []
    for _ in range(2):
        b = Bucket(SHAPES)
        *_, (it, p, g, m, step, table) = run_adafactor(b, SETTINGS["beta1_clip"], backend.device, ordered=True)
        outs.append([p.cpu(), m.cpu()] + [t.cpu().clone() for t in table.tensors()])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_adafactor_table_refuses_other_shapes_by_name(backend):
    for shape in [(2, 3, 4), (4, 4, 5, 5), (2, 2, 3, 3, 3)]:
        t = torch.zeros(shape)
        with pytest.raises(ValueError, match="blk.weight"):
            K.AdafactorTable([("blk.weight", 0, t.shape, t.stride())], backend.device)
    assert K.AdafactorTable([("w", 0, (4, 4), (4, 1))], backend.device).descs.numel() == K.lib().hcp_adafactor_desc_bytes()


@pytest.mark.parametrize("n", [3, 4099])
def test_lion_kernel_vs_float64(backend, n):
    """lion_pytorch's rule, three steps with grad_scale 0.5 and the clip to norm 1.  sign() is discontinuous: elements whose float64 sign
    argument is below 1e-5 max|g| at any step are excluded from then on (at most 0.1 % of them; none with these inputs); the momentum is
    compared everywhere."""
    dev = backend.device
    torch.manual_seed(0)
    g0 = torch.randn(n) * 3
    p0 = torch.randn(n)
    lr_v, wd = 1e-2, 1e-2
    p, m = p0.clone().to(dev), torch.zeros(n, device=dev)
    lr = torch.full((1,), lr_v, dtype=torch.float32, device=dev)
    step, ss = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    p64, m64, p32, m32 = p0.double(), torch.zeros(n, dtype=torch.float64), p0.clone(), torch.zeros(n)
    keep = torch.ones(n, dtype=torch.bool)
    for it in range(3):
        gi = g0 * ((it + 1) * 0.5)
        g = gi.clone().to(dev)                   # (the kernel clears it)
        K.sumsq(g, ss)
        K.lion_clip_fused(p, g, m, lr, step, weight_decay=wd, sumsq_t=ss, grad_scale=0.5, max_norm=1.0)
        clip = optim_ref.clip_factor([gi], 0.5, 1.0)
        arg = optim_ref.lion_step(p64, gi.double() * clip, m64, lr_v, weight_decay=wd)
        optim_ref.lion_step(p32, gi * optim_ref.clip_factor32([gi], 0.5, 1.0), m32, lr_v, weight_decay=wd)
        keep &= arg.abs() >= 1e-5 * float((gi.double() * clip).abs().max())
        assert step.item() == it + 1 and not g.any().item()
        assert (~keep).sum().item() <= n // 1000
        for name, got, want, ref32, mask in (("p", p, p64, p32, keep), ("exp_avg", m, m64, m32, torch.ones_like(keep))):
            err = float((got.cpu().double() - want)[mask].abs().max())
            e32 = float((ref32.double() - want)[mask].abs().max())
            bound = 4 * e32 + ulp32(want.abs().max())
            print(f"lion n={n} step {it + 1} {name}: kernel {err:.3e} e32 {e32:.3e} bound {bound:.3e} excluded {(~keep).sum().item()}")
            assert err <= bound, (name, it, err, e32)


# ---------------------------------------------------------------- optimizer classes (seam 4)
class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv2d(4, 8, 3)
        self.proj = torch.nn.Conv2d(8, 6, 1)
        self.fc = torch.nn.Linear(77, 5)
        self.norm = torch.nn.LayerNorm(5)


def _grads(model, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for p in model.parameters():                           # (written INTO the gradient once it exists: the flat runs follow its storage)
        v = (torch.randn(p.shape, generator=g) * scale).to(p.device)
        if p.grad is None:
            p.grad = v
        else:
            p.grad.copy_(v)


def _close(got, want, ref32, what):
    err = float((got.detach().cpu().double() - want).abs().max())
    e32 = float((ref32.double() - want).abs().max())
    bound = 4 * e32 + ulp32(want.abs().max())
    print(f"{what}: kernel {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, e32, bound)


@pytest.mark.parametrize("which", ["lion", "adafactor", "adafactor_beta1"])
def test_fused_optimizer_classes_vs_float64_and_state_dict_round_trip(backend, which):
    """FusedLion / FusedAdafactor over a small module: two steps against the float64 restatement per parameter; state_dict() ->
    load_state_dict() into a fresh instance continues bit-identically; an Adafactor state_dict loads into the installed class."""
    from hcp_diffusion_amd.optim import FusedAdafactor, FusedLion
    dev = backend.device
    kw = {"lion": dict(lr=1e-2, weight_decay=1e-2), "adafactor": dict(lr=1e-3, relative_step=False, weight_decay=1e-3),
          "adafactor_beta1": dict(beta1=0.9, clip_threshold=0.5)}[which]
    cls = FusedLion if which == "lion" else FusedAdafactor
    model = _Small().to(dev)
    p64 = [p.detach().cpu().double() for p in model.parameters()]
    p32 = [p.detach().cpu().clone() for p in model.parameters()]
    s64, s32 = [{} for _ in p64], [{} for _ in p64]
    opt = cls(model.parameters(), **kw)
    for it in range(2):
        _grads(model, 10 + it)
        gs = [p.grad.detach().cpu().clone() for p in model.parameters()]
        opt.step()
        assert all(not p.grad.any().item() for p in model.parameters())
        for i, (p, g) in enumerate(zip(model.parameters(), gs)):
            if which == "lion":
                for pp, st, gg in ((p64[i], s64[i], g.double()), (p32[i], s32[i], g)):
                    st.setdefault("exp_avg", torch.zeros_like(gg))
                    arg = optim_ref.lion_step(pp, gg, st["exp_avg"], kw["lr"], weight_decay=kw["weight_decay"])
                assert float(arg.abs().min()) > 1e-5 * float(g.abs().max()), "no element sits on the discontinuity of sign()"
            else:
                optim_ref.adafactor_step(p64[i], g.double(), s64[i], **kw)
                optim_ref.adafactor_step(p32[i], g.clone(), s32[i], **kw)
            _close(p, p64[i], p32[i], f"{which} step {it + 1} param {i}")
    sd = opt.state_dict()
    for i, st in sd["state"].items():
        for k, v in st.items():
            if k != "step":
                _close(torch.as_tensor(v), torch.as_tensor(s64[i][k], dtype=torch.float64), torch.as_tensor(s32[i][k]), f"{which} state {i} {k}")
    if which != "lion":
        assert all(st["step"] == 2 for st in sd["state"].values())
    # a fresh instance resumed from the dict takes the same third step, bit for bit
    twin = _Small().to(dev)
    twin.load_state_dict(model.state_dict())
    opt2 = cls(twin.parameters(), **kw)
    opt2.load_state_dict(sd)
    _grads(model, 99); _grads(twin, 99)
    opt.step(); opt2.step()
    for a, b_ in zip(model.parameters(), twin.parameters()):
        assert torch.equal(a.detach().cpu(), b_.detach().cpu())
    sa, sb = opt.state_dict()["state"], opt2.state_dict()["state"]
    for i in sa:
        for k in sa[i]:
            assert torch.equal(torch.as_tensor(sa[i][k]).cpu(), torch.as_tensor(sb[i][k]).cpu()), (i, k)
    if which != "lion":
        try:
            from transformers.optimization import Adafactor
        except ImportError:
            return
        third = [torch.nn.Parameter(p.detach().cpu().clone()) for p in twin.parameters()]
        ref = Adafactor(third, **kw)
        ref.load_state_dict(opt2.state_dict())
        for p in third:
            p.grad = torch.zeros_like(p)
        ref.step()                                         # the installed class accepts every field (step, RMS, factored moments, exp_avg)
        assert all(ref.state[p]["step"] == 4 for p in third)


def test_fused_adafactor_constructor_is_the_installed_one():
    from hcp_diffusion_amd.optim import FusedAdafactor, FusedLion
    w = [torch.nn.Parameter(torch.zeros(4, 4))]
    with pytest.raises(ValueError, match="relative_step"):
        FusedAdafactor(w, lr=1e-3)
    with pytest.raises(ValueError, match="warmup_init"):
        FusedAdafactor(w, lr=1e-3, relative_step=False, warmup_init=True)
    assert FusedLion(w).defaults == dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0) or FusedLion(w).defaults["betas"] == (0.9, 0.99)
    d = FusedAdafactor(w).defaults
    assert (d["lr"], d["eps"], d["clip_threshold"], d["decay_rate"], d["beta1"], d["weight_decay"], d["scale_parameter"], d["relative_step"],
            d["warmup_init"]) == (None, (1e-30, 1e-3), 1.0, -0.8, None, 0.0, True, True, False)


# ---------------------------------------------------------------- NativeTrainer optimizer=
def _native_unet(dev):
    from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
    from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, seeded_init_
    torch.manual_seed(0)
    ora = seeded_init_(OracleUNet2DConditionModel(**MICRO_CONFIG), 1)
    nat = NativeUNet2DConditionModel(**MICRO_CONFIG)
    nat.load_state_dict(ora.state_dict())
    return nat.to(dev)


def _opt_trainer(dev, optimizer, rank=4, **kw):
    """The tiny UNet of the trainer tests: LoRA on the attention blocks plus a host bucket (conv_in, conv_out: 3x3 weights + biases)."""
    from hcp_diffusion_amd.trainer import NativeTrainer
    tr = NativeTrainer(_native_unet(dev), [dict(layers=[r"re:.*\.attn.?$"], rank=rank)], lr=1e-3, optimizer=optimizer,
                       train_cfg=[dict(layers=["conv_in", "conv_out"], lr=1e-3)], **kw)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for blk in tr.bucket.blocks:
            blk.layer.W_up.copy_((torch.randn(blk.layer.W_up.shape, generator=g) * 0.05).to(dev))
    tr.bucket.pack()
    cache = {}

    def mk(lat):                                           # deterministic make_noise (capture-safe: tensors made once per shape)
        key = tuple(lat.shape)
        if key not in cache:
            gg = torch.Generator().manual_seed(11)
            cache[key] = (torch.randn(lat.shape, generator=gg).to(dev), torch.randint(0, 1000, (lat.shape[0],), generator=gg).to(dev))
        n, t = cache[key]
        return K.add_noise(lat, n, t, tr.acp), n, t
    tr.make_noise = mk
    return tr


def _tr_batch(dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 4, 8, 8, generator=g).to(dev), torch.randn(1, 24, 32, generator=g).to(dev)


TRAINER_OPTS = {"adafactor": {"type": "adafactor", "lr": None, "relative_step": False}, "lion": {"type": "lion", "betas": (0.9, 0.99)}}


def _bucket_named(tr, st):
    return st.bucket.named_tensors()


@pytest.mark.parametrize("which", list(TRAINER_OPTS))
def test_trainer_one_step_vs_float64_on_the_bucket_gradients(backend, which):
    """One eager step: every parameter of the LoRA and host buckets equals the float64 restatement applied to the bucket's pre-step
    gradients (shared global-norm clip over both buckets, max_grad_norm 1), under the kernel tests' gate."""
    dev = backend.device
    tr = _opt_trainer(dev, TRAINER_OPTS[which])
    lat, ehs = _tr_batch(dev)
    tr.optimizer_step, real_step = (lambda *a, **k: None), tr.optimizer_step
    tr.train_one_step(lat, ehs)
    tr.optimizer_step = real_step
    before = [(st, [(n, p.detach().cpu().clone(), p.grad.detach().cpu().clone()) for n, p in _bucket_named(tr, st)]) for st in tr._states()]
    gs = [g for _, rows in before for _, _, g in rows]
    clip, clip32 = optim_ref.clip_factor(gs, 1.0, tr.max_grad_norm), optim_ref.clip_factor32(gs, 1.0, tr.max_grad_norm)
    tr.optimizer_step()
    for st, rows in before:
        assert not st.bucket.grads.any().item() and st.step_count.item() == 1
        for (n, p0, g), (_, p) in zip(rows, _bucket_named(tr, st)):
            p64, p32 = p0.double(), p0.clone()
            if which == "lion":
                optim_ref.lion_step(p64, g.double() * clip, torch.zeros_like(p64), 1e-3, weight_decay=1e-3)
                optim_ref.lion_step(p32, g * clip32, torch.zeros_like(p32), 1e-3, weight_decay=1e-3)
            else:
                kw = dict(lr=1e-3, relative_step=False, weight_decay=1e-3)
                optim_ref.adafactor_step(p64, g.double() * clip, {}, **kw)
                optim_ref.adafactor_step(p32, g * clip32, {}, **kw)
            _close(p, p64, p32, f"trainer {which} {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(TRAINER_OPTS))
def test_trainer_captured_graph_equals_eager(which):
    """Three steps with the optimizer step captured (the warm-up's snapshot / restore covers the optimizer's own state): parameters and
    optimizer state equal the eager run bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    K._set_backend_for_tests(None)
    dev = torch.device("cuda:0")
    lat, ehs = _tr_batch(dev)
    outs = []
    for use_graph in (False, True):
        tr = _opt_trainer(dev, TRAINER_OPTS[which], use_graph=use_graph)
        for _ in range(3):
            tr.train_one_step(lat, ehs)
        torch.cuda.synchronize()
        assert all(st.step_count.item() == 3 for st in tr._states())
        outs.append([t.clone() for st in tr._states() for t in [st.bucket.params] + [x for x in st.tensors() if x is not st.sumsq]])
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


def test_trainer_optimizer_argument_checks_and_default(backend):
    """Unknown types and Adafactor with a forced shard raise; optimizer=None is {'type': 'adamw'} bit for bit."""
    from hcp_diffusion_amd.trainer import NativeTrainer
    dev = backend.device
    with pytest.raises(ValueError, match="sgd"):
        NativeTrainer(_native_unet(dev), [dict(layers=[r"re:.*\.attn.?$"], rank=4)], optimizer={"type": "sgd"})
    with pytest.raises(ValueError, match="whole tensors|WHOLE tensors"):
        NativeTrainer(_native_unet(dev), None, train_cfg=[dict(layers=["conv_in"])], optimizer={"type": "adafactor"}, shard_optimizer="force")
    lat, ehs = _tr_batch(dev)
    outs = []
    for optimizer in (None, {"type": "adamw"}):
        # rank 2: 6112 LoRA elements = two workgroups of AdamW's K.sumsq, whose atomic adds then commute exactly (three or more do not:
        # the norm's last bit would differ between ANY two AdamW runs on the GPU, whatever `optimizer` says)
        tr = _opt_trainer(dev, optimizer, rank=2)
        assert all(st.bucket.params.numel() <= 8192 for st in tr._states())
        for _ in range(2):
            tr.train_one_step(lat, ehs)
        outs.append([st.bucket.params.cpu().clone() for st in tr._states()] + [st.exp_avg.cpu().clone() for st in tr._states()])
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


def test_new_overlays_load_and_resolve_to_the_new_classes():
    import importlib
    import pathlib
    import yaml
    root = pathlib.Path(__file__).resolve().parent.parent / "cfgs" / "train" / "mi355x"
    want = {"ft_sdxl_adafactor_hip.yaml": ("cfgs/train/examples/FT_sdxl.yaml", {"optimizer": "FusedAdafactor"}),
            "lion_sd15_hip.yaml": ("cfgs/train/examples/Lion_optimizer.yaml", {"optimizer": "FusedLion", "optimizer_pt": "FusedLion"})}
    for name, (base, opts) in want.items():
        cfg = yaml.safe_load((root / name).read_text())
        assert cfg["_base_"] == [base] and cfg["mixed_precision"] == "bf16"
        for key, cls in opts.items():
            mod, _, attr = cfg["train"][key]["_target_"].rpartition(".")
            assert mod == "hcp_diffusion_amd.optim" and attr == cls
            obj = getattr(importlib.import_module(mod), attr)
            kw = {k: v for k, v in cfg["train"][key].items() if k not in ("_target_", "_partial_", "type")}
            kw = {k: float(v) if isinstance(v, str) else v for k, v in kw.items()}       # (YAML 1.1 reads 1e-3 as a string)
            assert isinstance(obj([torch.nn.Parameter(torch.zeros(4, 4))], **kw), torch.optim.Optimizer)
    ada = yaml.safe_load((root / "ft_sdxl_adafactor_hip.yaml").read_text())["train"]["optimizer"]
    assert ada["relative_step"] is False and float(ada["weight_decay"]) == 1e-3


@pytest.mark.parametrize("n", [3, 4099, 40000])
def test_sumsq_ordered_vs_float64_and_itself(backend, n):
    """One workgroup, two, ten (ragged 16-byte body + scalar tail): the fixed-order sum against float64 within the roundings of its adds, and
    twice the same bits."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    gd = g.clone().to(backend.device)
    part = torch.zeros(K.SUMSQ_PARTIALS, dtype=torch.float32, device=backend.device)
    outs = [K.sumsq_ordered(gd, torch.zeros(1, device=backend.device), part).cpu().clone() for _ in range(2)]
    assert torch.equal(*outs)
    want = float((g.double() ** 2).sum())
    # an element passes through <= 16 serial adds in its thread, 6 butterfly levels, 3 wave adds, then <= 1 + 6 + 3 in the finish: 35 roundings
    # of at most half an ulp of the final sum each (all terms are positive)
    assert abs(float(outs[0]) - want) <= 18 * ulp32(want), (float(outs[0]), want)
