"""Native Euler / Euler-ancestral sampler (csrc/sampler.hip, sampler.NativeEulerSampler, scheduler.NativeEulerAncestralScheduler)
against the float64 restatement in tests/euler_ref.py.  Measured errors go to profiles/sampler_euler_accuracy.txt."""
import math
import pathlib
import warnings

import numpy as np
import pytest
import torch

import euler_ref as R
from hcp_diffusion_amd import _lib, kernels as K
from hcp_diffusion_amd.sampler import NativeDDIMSampler, NativeEulerSampler
from hcp_diffusion_amd.scheduler import NativeEulerAncestralScheduler
from hcp_diffusion_amd.unet import NativeUNet2DConditionModel
from oracle.sampler_ref import sample as ddim_ref_sample
from oracle.unet_sd15 import MICRO_CONFIG, OracleUNet2DConditionModel, ddpm_alphas_cumprod, seeded_init_

ACCURACY = pathlib.Path(__file__).resolve().parent.parent / "profiles" / "sampler_euler_accuracy.txt"
ACP = ddpm_alphas_cumprod().numpy()
F32 = 2.0 ** -24          # half an ulp of 1.0: the relative error of one fp32 rounding


def record(key, text):
    """One line per key in the accuracy file (rewritten in place: a rerun updates its own lines)."""
    lines = {}
    if ACCURACY.exists():
        for line in ACCURACY.read_text().splitlines():
            if ": " in line:
                k, v = line.split(": ", 1)
                lines[k] = v
    lines[key] = text
    try:
        ACCURACY.write_text("".join(f"{k}: {v}\n" for k, v in sorted(lines.items())))
    except OSError:                                  # a read-only checkout: the figures are still printed
        pass


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------------- 1. table
@pytest.mark.parametrize("ancestral", [True, False])
@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("n", [1, 4, 20])
def test_table_against_float64(n, spacing, ancestral):
    s = NativeEulerSampler(ancestral=ancestral, timestep_spacing=spacing)
    ref = R.table(ACP, n, spacing, ancestral)
    assert s.timesteps(n).tolist() == ref["timesteps"].tolist()
    if spacing == "leading" and n == 4:
        assert s.timesteps(n).tolist() == [751, 501, 251, 1]
    tab = s.table(n).double().numpy()
    assert tab.shape == (n, 8) and s.table(n).dtype == torch.float32
    sig = s.sigmas(n).double().numpy()
    assert sig.shape == (n + 1,) and sig[-1] == 0
    # the table is float64 arithmetic rounded once: one fp32 rounding of each entry (2x: the float64 evaluation orders may differ by an ulp of float64, far below)
    for col, name in enumerate(["sigma", "sigma_down", "sigma_up", "c_in_next"]):
        assert np.all(np.abs(tab[:, col] - ref[name]) <= 2 * F32 * np.abs(ref[name])), name
    assert np.all(np.abs(sig[:-1] - ref["sigma"]) <= 2 * F32 * ref["sigma"])
    assert np.all(np.abs(tab[:, 6] - ref["sigma_init"]) <= 2 * F32 * ref["sigma_init"]) and np.all(np.abs(tab[:, 7] - ref["c_in"]) <= 2 * F32)
    assert tab[:, 4].tolist() == ref["timesteps"].tolist() and tab[:-1, 5].tolist() == ref["timesteps"][1:].tolist()
    # closed forms: the last sigma_next is 0, so the last sigma_up and sigma_down are 0 and the last c_in_next is 1
    assert tab[-1, 1] == 0 and tab[-1, 2] == 0 and tab[-1, 3] == 1
    assert np.all(tab[:-1, 1] > 0)                      # sigma_down == 0 marks the final row only
    # sigma_up^2 + sigma_down^2 == sigma_next^2: each entry carries one fp32 rounding (relative F32), a square doubles it, and the
    # reference sigma_next is the next row's own rounded sigma (another 2 F32 on its square): 6 F32 in all, 8 allowed
    nxt = np.append(tab[1:, 0], 0.0)
    assert np.all(np.abs(tab[:, 2] ** 2 + tab[:, 1] ** 2 - nxt ** 2) <= 8 * F32 * nxt ** 2)
    if not ancestral:
        assert np.all(tab[:, 2] == 0) and np.all(tab[:, 1] == nxt)


def test_linspace_is_refused():
    with pytest.raises(NotImplementedError, match="int64 timesteps"):
        NativeEulerSampler(timestep_spacing="linspace")
    with pytest.raises(NotImplementedError, match="int64 timesteps"):
        NativeEulerAncestralScheduler(timestep_spacing="linspace")


# ------------------------------------------------------------------------------------------------------------ 2. step kernel, given noise
def _state(backend, seed, step):
    return backend.to(torch.tensor([seed, step], dtype=torch.int64))


def _step_case(backend, shape, guided, row, **kw):
    """(reference x', reference model input, kernel x', kernel model input) of one step of the 4-step ancestral table."""
    s = NativeEulerSampler()
    tab, ref = s.table(4), R.table(ACP, 4)
    x, eu, ec, z = (rnd(10 + i, *shape) for i in range(4))
    g = 6.0
    rx, rm = R.euler_step(x, eu, ec if guided else None, g, R.row_of(ref, row), z, **{k: v for k, v in kw.items()})
    eps2 = torch.cat([eu, ec]) if guided else eu
    mi = backend.to(torch.zeros(((2 if guided else 1) * shape[0],) + tuple(shape[1:])))
    dk = {k: backend.to(v.float().contiguous()) for k, v in kw.items()}
    out = K.euler_step(backend.to(x), backend.to(eps2), backend.to(tab), _state(backend, 3, row), g, noise=backend.to(z), model_in_next=mi, **dk)
    return rx, rm, out.cpu(), mi.cpu(), (x, eps2, tab, z, g, dk)


@pytest.mark.parametrize("row", [0, 2, 3])
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("shape", [(1, 4, 8, 8), (3, 4, 8, 8), (2, 4, 12, 20)])
def test_step_kernel_given_noise(backend, shape, guided, row):
    rx, rm, out, mi, (x, eps2, tab, z, g, _) = _step_case(backend, shape, guided, row)
    tol = 2e-5 * np.abs(rx).max()
    assert np.abs(out.double().numpy() - rx).max() < tol
    B = shape[0]
    c = tab[row, 3]
    assert torch.equal(mi[:B], c * out)                                   # one fp32 product of the stored x'
    if guided:
        assert torch.equal(mi[:B], mi[B:])
    assert np.abs(mi[:B].double().numpy() - rm).max() < 2e-5 * max(np.abs(rm).max(), 1e-30)
    xin = backend.to(x.clone())                                           # in place: the same bits
    K.euler_step(xin, backend.to(eps2), backend.to(tab), _state(backend, 3, row), g, noise=backend.to(z), out=xin)
    assert torch.equal(xin.cpu(), out)
    if row == 3:                                                          # final row: no noise enters, x' = x - sigma eps
        out2 = K.euler_step(backend.to(x), backend.to(eps2), backend.to(tab), _state(backend, 3, row), g, noise=backend.to(z * 0 + 7)).cpu()
        assert torch.equal(out2, out)


# --------------------------------------------------------------------------------------------------------------------- 3. mask blend
def _mask():
    m = torch.zeros(2, 1, 8, 8)
    m[0, 0, :4] = 1.0                                                     # row 0: the top half; row 1: a checkerboard and a soft corner
    m[1, 0, ::2, 1::2] = 1.0
    m[1, 0, 7, 7] = 0.25
    return m


@pytest.mark.parametrize("row", [1, 3])
def test_mask_blend(backend, row):
    shape = (2, 4, 8, 8)
    init, n0 = rnd(21, *shape), rnd(22, *shape)
    rx0, _, plain, plain_mi, _ = _step_case(backend, shape, True, row)
    rx, _, out, mi, (x, eps2, tab, z, g, _) = _step_case(backend, shape, True, row, init=init, noise0=n0, mask=_mask())
    assert np.abs(out.double().numpy() - rx).max() < 2e-5 * np.abs(rx).max()
    sigma = float(tab[row, 0])
    kept = init if row == 3 else init + sigma * n0                        # the sigma of the step just taken; the final step keeps init itself
    m = _mask().expand(shape).bool() & (_mask().expand(shape) == 1)
    assert torch.equal(out[m], kept[m])                                   # every channel of a kept position (1 * a + 0 * b is exact)
    free = _mask().expand(shape) == 0
    assert torch.equal(out[free], plain[free])
    assert torch.equal(mi[:2], tab[row, 3] * out) and torch.equal(mi[2:], mi[:2])
    # m = 0 everywhere is the unmasked step bit for bit, m = 1 everywhere is init + sigma noise0 (init on the final row)
    _, _, zero, zero_mi, _ = _step_case(backend, shape, True, row, init=init, noise0=n0, mask=torch.zeros(2, 1, 8, 8))
    assert torch.equal(zero, plain) and torch.equal(zero_mi, plain_mi)
    _, _, one, _, _ = _step_case(backend, shape, True, row, init=init, noise0=n0, mask=torch.ones(2, 1, 8, 8))
    assert torch.equal(one, kept)


# ---------------------------------------------------------------------------------------------------------------- 4. in-kernel noise
def _draw(dev, shape, seed, step, guided=False):
    """z of the step kernel: x = 0, eps = 0, a row with sigma_down = sigma and sigma_up = 1."""
    row = torch.tensor([1.0, 1.0, 1.0, 1.0, 0, 0, 1.0, 1.0])
    tab = row.repeat(step + 1, 1).contiguous().to(dev)
    x = torch.zeros(shape, device=dev)
    eps2 = torch.zeros(((2 if guided else 1) * shape[0],) + tuple(shape[1:]), device=dev)
    return K.euler_step(x, eps2, tab, torch.tensor([seed, step], dtype=torch.int64).to(dev), 3.0 if guided else 1.0).cpu()


@pytest.mark.parametrize("step", [0, 5])
@pytest.mark.parametrize("seed", [0, (0x1234 << 32) + 77])
def test_in_kernel_noise_against_numpy(backend, seed, step):
    shape = (3, 4, 8, 8)
    n = math.prod(shape)
    w = R.words(n, seed, step)
    z64, u = R.box_muller(w)
    z32, u32 = R.box_muller(w, np.float32)
    assert u.min() > 0 and u32.min() > 0 and np.isfinite(z64).all()
    err32 = np.abs(z32.astype(np.float64) - z64).max()                    # what fp32 arithmetic on these words costs (numpy / libm)
    z = _draw(backend.device, shape, seed, step)
    err = np.abs(z.double().numpy().reshape(-1) - z64).max()
    print(f"in-kernel noise seed={seed} step={step} {backend.name}: kernel {err:.3e}, numpy float32 {err32:.3e}")
    record(f"noise {backend.name} seed={seed} step={step}", f"kernel max|z - z64| = {err:.3e}; numpy float32 max|z32 - z64| = {err32:.3e}; allowed 4x")
    assert err <= 4 * err32


def test_in_kernel_noise_is_a_function_of_seed_step_group(backend):
    shape, dev = (3, 4, 8, 8), backend.device
    a = _draw(dev, shape, 5, 1)
    assert torch.equal(a, _draw(dev, shape, 5, 1))                        # same triple: same bits
    assert torch.equal(a, _draw(dev, shape, 5, 1, guided=True))           # the guided form draws the same z
    assert not torch.equal(a, _draw(dev, shape, 6, 1)) and not torch.equal(a, _draw(dev, shape, 5, 2))
    groups = a.reshape(-1, 4)
    assert len({tuple(g.tolist()) for g in groups}) == groups.shape[0]    # another group: another draw
    assert torch.equal(_draw(dev, (1, 4, 8, 8), 5, 1).reshape(-1), a.reshape(-1)[:256])      # a group's draw does not depend on the launch


@pytest.mark.gpu
def test_in_kernel_noise_moments_past_the_grid_cap():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    K._set_backend_for_tests(None)
    shape = (16, 4, 128, 128)
    n = math.prod(shape)
    assert n == 1 << 20 and n > 4 * K.SAMPLER_MAX_THREADS                 # the grid-stride loop turns over
    z = _draw(torch.device("cuda:0"), shape, 9, 2).double()
    assert torch.isfinite(z).all()                                        # u = 0 would give an infinity
    assert abs(z.mean().item()) < 5 / math.sqrt(n)
    assert abs(z.var(unbiased=False).item() - 1) < 5 * math.sqrt(2 / n)
    w = R.words(n, 9, 2)                                                  # the turned-over loop still indexes groups right: head and tail
    for sl, zs in ((w[:1024], z.reshape(-1)[:4096]), (w[-1024:], z.reshape(-1)[-4096:])):      # against the restatement, 4 x the fp32 yardstick
        z64, z32 = R.box_muller(sl)[0], R.box_muller(sl, np.float32)[0]
        assert np.abs(zs.numpy() - z64).max() <= 4 * np.abs(z32.astype(np.float64) - z64).max()


# -------------------------------------------------------------------------------------------------------- 5. loop against the oracle
_ORACLE = {}


def oracle_setup():
    """Built once per process and left unchanged: the oracle UNet, the inputs and the float64-scheduler references."""
    if not _ORACLE:
        torch.manual_seed(0)
        ora = seeded_init_(OracleUNet2DConditionModel(**MICRO_CONFIG), 1)
        g = torch.Generator().manual_seed(2)
        lat = torch.randn(2, 4, 8, 8, generator=g); cond = torch.randn(2, 24, 32, generator=g); unc = torch.randn(2, 24, 32, generator=g)
        noise, init = rnd(31, 4, 2, 4, 8, 8), rnd(32, 2, 4, 8, 8)
        acp = ddpm_alphas_cumprod()
        _ORACLE.update(ora=ora, lat=lat, cond=cond, unc=unc, noise=noise, init=init, mask=_mask(),
                       ddim=ddim_ref_sample(ora, lat, cond, unc, acp, guidance_scale=5.0, num_inference_steps=4),
                       t2i=R.sample(ora, lat, cond, unc, ACP, 5.0, 4, noise),
                       i2i=R.sample(ora, lat, cond, unc, ACP, 5.0, 4, noise, init=init, strength=0.5),
                       inpaint=R.sample(ora, lat, cond, unc, ACP, 5.0, 4, noise, init=init, strength=0.5, mask=_mask()))
    return _ORACLE


def native_unet(dev):
    o = oracle_setup()
    nat = NativeUNet2DConditionModel(**MICRO_CONFIG)
    nat.load_state_dict(o["ora"].state_dict())
    return nat.to(dev)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_loop_against_the_oracle(backend):
    o, to = oracle_setup(), backend.to
    nat = native_unet(backend.device)
    ddim = NativeDDIMSampler().sample(nat, to(o["lat"]), to(o["cond"]), to(o["unc"]), guidance_scale=5.0, num_inference_steps=4).cpu()
    e_ddim = rel(ddim, o["ddim"])
    bound = min(2 * e_ddim, 2 * 3e-2)                  # sigma space amplifies the early steps by up to sigma_max ~ 14.6: twice the DDIM loop's own error
    s = NativeEulerSampler()
    args = (nat, to(o["lat"]), to(o["cond"]), to(o["unc"]))
    kw = dict(guidance_scale=5.0, num_inference_steps=4, noise=to(o["noise"]))
    e_t2i = rel(s.sample(*args, **kw).cpu(), o["t2i"])
    e_i2i = rel(s.sample(*args, init_latents=to(o["init"]), strength=0.5, **kw).cpu(), o["i2i"])
    e_inp = rel(s.sample(*args, init_latents=to(o["init"]), strength=0.5, mask=to(o["mask"]), **kw).cpu(), o["inpaint"])
    print(f"loop {backend.name}: DDIM {e_ddim:.3e} (bound {bound:.3e}), Euler-a {e_t2i:.3e}, img2img {e_i2i:.3e}, inpaint {e_inp:.3e}")
    record(f"loop {backend.name}", f"relative L2 vs oracle, 4 guided steps [2,4,8,8]: NativeDDIMSampler {e_ddim:.3e}, NativeEulerSampler {e_t2i:.3e} "
                                   f"(bound {bound:.3e}), strength 0.5 {e_i2i:.3e}, masked {e_inp:.3e}")
    assert e_t2i < bound and e_i2i < bound and e_inp < bound
    with pytest.raises(ValueError, match="mask needs init_latents"):
        s.sample(*args, mask=to(o["mask"]), **kw)
    assert s.start_step(4, 0.5) == 2 and s.start_step(20, 0.75) == 5 and s.start_step(4, None) == 0


# --------------------------------------------------------------------------------------------------------------- 6. graph equals eager
@pytest.mark.gpu
def test_graph_equals_eager_and_is_captured_once():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    K._set_backend_for_tests(None)
    dev = torch.device("cuda:0")
    o = oracle_setup()
    nat = native_unet(dev)
    args = (nat, o["lat"].to(dev), o["cond"].to(dev), o["unc"].to(dev))
    kw = dict(guidance_scale=5.0, num_inference_steps=4, init_latents=o["init"].to(dev))
    s = NativeEulerSampler(seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                     # a fall-back to eager would warn
        eager = s.sample(*args, strength=1.0, **kw)
        graph = s.sample(*args, strength=1.0, use_graph=True, **kw)
        assert s.captures == 1 and torch.equal(eager, graph)
        assert not torch.equal(eager, NativeEulerSampler(seed=4).sample(*args, strength=1.0, **kw))      # the seed acts
        s.seed = 8                                                         # another seed, another strength: the same graph
        graph2 = s.sample(*args, strength=0.5, use_graph=True, **kw)
        assert s.captures == 1
        assert torch.equal(graph2, s.sample(*args, strength=0.5, **kw)) and not torch.equal(graph2, graph)
        kw3 = dict(kw, num_inference_steps=3)                              # fewer steps than the captured table holds: still that graph
        assert torch.equal(s.sample(*args, strength=1.0, use_graph=True, **kw3), s.sample(*args, strength=1.0, **kw3)) and s.captures == 1


def test_graph_request_falls_back_with_one_warning(backend):
    o, to = oracle_setup(), backend.to
    nat = native_unet(backend.device)
    nat.register_forward_hook(lambda m, i, out: None)                      # what graphed.capturable() refuses
    s = NativeEulerSampler(seed=3)
    args = (nat, to(o["lat"]), to(o["cond"]), to(o["unc"]))
    with pytest.warns(UserWarning, match="runs eagerly"):
        a = s.sample(*args, guidance_scale=5.0, num_inference_steps=2, use_graph=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                     # one warning per sampler
        b = s.sample(*args, guidance_scale=5.0, num_inference_steps=2, use_graph=True)
    assert torch.equal(a, b) and s.captures == 0


# ------------------------------------------------------------------------------------------------------------------------- 7. seam
def test_scheduler_seam_equals_the_sampler(backend):
    """The reference's denoising loop (utils/pipe_hook.py:116-146, restated here) over NativeEulerAncestralScheduler."""
    o, to = oracle_setup(), backend.to
    nat = native_unet(backend.device)
    lat, cond, unc = to(rnd(41, 2, 4, 8, 8)), to(o["cond"]), to(o["unc"])
    guidance_scale, steps = 5.0, 3
    want = NativeEulerSampler(seed=6).sample(nat, lat, cond, unc, guidance_scale=guidance_scale, num_inference_steps=steps)
    sch = NativeEulerAncestralScheduler(seed=6)
    assert sch.order == 1 and torch.equal(sch.alphas_cumprod, ddpm_alphas_cumprod())
    sch.set_timesteps(steps, device=backend.device)
    assert sch.timesteps.tolist() == R.timesteps(steps).tolist() and abs(sch.init_noise_sigma - R.table(ACP, steps)["sigma_init"][0]) < 1e-5
    prompt_embeds = torch.cat([unc, cond])
    with torch.no_grad():
        latents = lat * sch.init_noise_sigma
        for i, t in enumerate(sch.timesteps):
            latent_model_input = torch.cat([latents] * 2)
            latent_model_input = sch.scale_model_input(latent_model_input, t)
            noise_pred = nat(latent_model_input, to(t).expand(4), prompt_embeds).sample.float()
            noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
            noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
            latents = sch.step(noise_pred, t, latents).prev_sample
    assert torch.equal(latents.cpu(), want.cpu())
    gen = torch.Generator().manual_seed(6)                                 # a generator's seed is the kernel's seed
    sch.set_timesteps(steps)
    x, e = to(rnd(42, 2, 4, 8, 8)), to(rnd(43, 2, 4, 8, 8))
    a = sch.step(e, sch.timesteps[0], x, generator=gen).prev_sample
    sch.set_timesteps(steps)
    assert torch.equal(a, sch.step(e, sch.timesteps[0], x).prev_sample)
    assert not torch.equal(a, sch.step(e, sch.timesteps[0], x, generator=torch.Generator().manual_seed(7)).prev_sample)
    # add_noise in sigma space: orig + noise * sigma_t
    t1 = sch.timesteps[1]
    got = sch.add_noise(x, e, torch.tensor([int(t1)])).cpu().double().numpy()
    ref = x.cpu().double().numpy() + e.cpu().double().numpy() * R.table(ACP, steps)["sigma"][1]
    assert np.abs(got - ref).max() < 2e-5 * np.abs(ref).max()


# --------------------------------------------------------------------------------------------------------------------- 8. boundary
def test_boundary_rejects_bad_arguments_without_launching():
    lib = _lib.load()
    assert {"hcp_euler_step", "hcp_sampler_advance", "hcp_sampler_begin"} <= set(_lib.EXPORTED_SYMBOLS) and _lib.ABI_VERSION >= 9
    from hcp_diffusion_amd.build import SOURCES
    assert "sampler.hip" in SOURCES
    N, one = None, 16                                                      # `one`: a non-null, 16-byte aligned address nothing dereferences
    step = lambda **k: lib.hcp_euler_step(*[{**dict(x=one, eps2=one, out=one, mi=N, n=256, B=1, guided=0, g=1.0, table=one, steps=4, state=one,
                                                    noise=N, init=N, noise0=N, mask=N, chw=256, hw=64, stream=N), **k}[a]
                                            for a in ("x", "eps2", "out", "mi", "n", "B", "guided", "g", "table", "steps", "state", "noise", "init", "noise0",
                                                      "mask", "chw", "hw", "stream")])
    adv = lambda **k: lib.hcp_sampler_advance(*[{**dict(state=one, table=one, steps=4, t=one, rows=2, stream=N), **k}[a]
                                                for a in ("state", "table", "steps", "t", "rows", "stream")])
    beg = lambda **k: lib.hcp_sampler_begin(*[{**dict(state=one, table=one, steps=4, x=one, mi=N, n=256, guided=0, noise=N, init=N, t=one, rows=2,
                                                      start=0, stream=N), **k}[a]
                                              for a in ("state", "table", "steps", "x", "mi", "n", "guided", "noise", "init", "t", "rows", "start", "stream")])
    for fn, name in ((step, b"hcp_euler_step"), (adv, b"hcp_sampler_advance"), (beg, b"hcp_sampler_begin")):
        for bad, word in ((dict(table=N), b"null table or state"), (dict(state=N), b"null table or state"), (dict(steps=0), b"steps must be positive"),
                          (dict(steps=-3), b"steps must be positive")):
            assert fn(**bad) < 0
            msg = lib.hcp_last_error()
            assert name in msg and word in msg, (name, bad, msg)
    for fn in (step, beg):
        for n in (0, 7, 254):
            assert fn(n=n) < 0 and b"multiple of 4" in lib.hcp_last_error()
    assert step(mask=one) < 0 and b"mask needs init and noise0" in lib.hcp_last_error()
    assert step(mask=one, init=one) < 0 and b"mask needs init and noise0" in lib.hcp_last_error()
    assert step(mask=one, init=one, noise0=one, chw=192) < 0 and b"B_rows * chw" in lib.hcp_last_error()
    assert step(x=20) < 0 and b"16-byte aligned" in lib.hcp_last_error()
    assert beg(start=4) < 0 and beg(start=-1) < 0 and b"start_step" in lib.hcp_last_error()
    assert adv(t=N) < 0 and beg(t=N) < 0
