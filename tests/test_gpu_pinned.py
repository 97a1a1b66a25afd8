"""Pinned-frame (mask / x0) and partial (timesteps=, stochastic_encode, decode) DDIM sampling on the MI355X.

Two kinds of statement:
  * bit equality, where it is derivable: tc_ddim_blend is IEEE fp32 multiplies, one subtraction and adds, each rounded on
    its own, so it must reproduce the same expression evaluated by separate torch ops on the CPU (a contracted FMA breaks
    this); the latent the UNet is handed at each step is such a blend; eager and graphed runs launch the same kernels;
  * trajectories against the real reference's goldens (tests/golden/ddim_pinned_tiny.npz, made by make_pinned_golden.py):
    the project's stated tolerance for a CFG-7.5 trajectory, rel-L2 <= 0.15 over all elements (tests/test_gpu_models.py).
    Measured on the MI355X (worst pred_x0 step / final sample): see DESIGN.md section 6.
"""
import contextlib
import sys

import pytest
import torch

from conftest import GOLDEN, load_golden, rel_l2
from tooncrafter_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TRAJECTORY_BOUND = 0.15
SETTINGS = dict(unconditional_guidance_scale=7.5, eta=1.0, timestep_spacing="uniform_trailing", guidance_rescale=0.7)


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.ndim else v) for k, v in load_golden("ddim_pinned_tiny.npz").items()}


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def model(tiny_sd):
    from test_host_logic_cpu import _tiny_model_cfg
    from tooncrafter_amd.utils import instantiate_from_config
    m = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    m.load_state_dict(tiny_sd, strict=False)
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernel, bit for bit

def blend_cpu(x, x0, noise, mask, sqrt_ac, sqrt_1m_ac):
    """The reference's expression as separate fp32 torch ops on the CPU (ddpm3d.py:308-309, ddim.py:180)."""
    orig = x0
    if noise is not None:
        orig = torch.tensor(sqrt_ac, dtype=torch.float32) * x0 + torch.tensor(sqrt_1m_ac, dtype=torch.float32) * noise
    return orig if mask is None else orig * mask + (1. - mask) * x


def on_device(t, offset):
    """A contiguous device copy of `t` whose first element sits `offset` floats past an aligned allocation."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + offset, dtype=torch.float32, device=DEV)
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
    return view


@pytest.mark.parametrize("binding", ["ctypes", "torch"])
@pytest.mark.parametrize("b,n", [(1, 1), (2, 420), (2, 1024), (3, 4099)])
def test_blend_is_bit_exact(hip, binding, b, n):
    """(1,1): one scalar; (2,420): a multiple of 4 below one block; (2,1024): exactly one block of vectors per sample;
    (3,4099): several blocks and a ragged tail of 12297 % 4 = 1.  Each with and without mask / noise, in place, into a
    guarded buffer, and with every or one operand one float off the 16-byte grid (the scalar path)."""
    be = hip if binding == "ctypes" else ops.backend()
    if binding == "torch":
        assert getattr(be, "binding", None) == "torch", "the custom-op layer is not loaded"
    gen = torch.Generator().manual_seed(1000 * b + n)
    x, x0, noise = (torch.randn(b, n, generator=gen) for _ in range(3))
    mask = torch.rand(b, n, generator=gen)
    mask[0, 0] = 1.0
    sa, s1 = float(torch.tensor(0.6234567, dtype=torch.float32)), float(torch.tensor(0.7819113, dtype=torch.float32))
    for use_mask, use_noise in ((True, True), (True, False), (False, True)):
        want = blend_cpu(x, x0, noise if use_noise else None, mask if use_mask else None, sa, s1)
        for off in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 1), (0, 1, 0, 0)):            # offsets of x, x0, noise, mask
            dx, d0 = on_device(x if use_mask else None, off[0]), on_device(x0, off[1])
            dn, dm = on_device(noise if use_noise else None, off[2]), on_device(mask if use_mask else None, off[3])
            tag = (b, n, use_mask, use_noise, off)
            got = be.ddim_blend(dx, d0, dn, dm, sqrt_ac=sa, sqrt_1m_ac=s1)                # a fresh result
            assert got.dtype == torch.float32 and got.shape == (b, n) and torch.equal(got.cpu(), want), tag
            for out_off in (0, 1):                                                        # a guarded result buffer
                guard = torch.full((b * n + 8,), 12345.0, device=DEV)
                out = guard[4 + out_off:4 + out_off + b * n].view(b, n)
                res = be.ddim_blend(dx, d0, dn, dm, sqrt_ac=sa, sqrt_1m_ac=s1, out=out)
                assert res is out and torch.equal(out.cpu(), want), tag
                assert bool((guard[:4 + out_off] == 12345.0).all()) and bool((guard[4 + out_off + b * n:] == 12345.0).all()), tag
            if use_mask:                                                                  # in place: out is x
                res = be.ddim_blend(dx, d0, dn, dm, sqrt_ac=sa, sqrt_1m_ac=s1, out=dx)
                assert res is dx and torch.equal(dx.cpu(), want), tag
                assert torch.equal(d0.cpu(), x0) and torch.equal(dm.cpu(), mask), tag


# ------------------------------------------------------------------------------------------------ 2. validation

def test_blend_refuses_bad_arguments_without_launching(hip):
    flat = torch.full((64,), 7.0, device=DEV)
    x0, x = flat[:16].view(2, 8), flat[32:48].view(2, 8)
    mask = torch.ones(2, 8, device=DEV)
    with pytest.raises(_lib.TooncrafterHipError, match="TC_EINVAL"):
        hip.ddim_blend(None, x0, None, None, out=flat[4:20].view(2, 8))                   # out partially over x0
    with pytest.raises(_lib.TooncrafterHipError, match="TC_EINVAL"):
        hip.ddim_blend(x, x0, None, mask, out=flat[36:52].view(2, 8))                     # out over x, but not exactly
    with pytest.raises(_lib.TooncrafterHipError, match="TC_EINVAL"):
        hip.ddim_blend(None, x0, None, mask)                                              # mask without x
    with pytest.raises(_lib.TooncrafterHipError, match="TC_EINVAL"):
        hip.ddim_blend(None, torch.empty(2, 0, device=DEV), None, None)                   # n = 0
    p = _lib.TcDdimBlendParams()
    p.x0, p.out, p.b, p.n = x0.data_ptr(), x.data_ptr(), 2, 0
    assert hip.lib.tc_ddim_blend(p, None) == -1
    with pytest.raises(RuntimeError, match="tc_ddim_blend failed with code -1"):          # the custom-op binding says the same
        ops.backend().ddim_blend(None, x0, None, mask)
    torch.cuda.synchronize()
    assert bool((flat == 7.0).all()), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ sampler runs

@contextlib.contextmanager
def injected(model, noises, qnoises, calls=None):
    """Both random sources of a sampling run replaced by recorded draws (the hooks the reference's goldens were made
    with: the samplers' module-level `noise_like` and `model.q_sample`); `calls` collects (t, x) of every UNet call."""
    from tooncrafter_amd.lvdm import ddim as my_ddim
    it, qit = iter(noises.to(DEV)), iter(qnoises.to(DEV))
    old_noise, q_sample, multi = my_ddim.noise_like, model.q_sample, model.apply_model_multi

    def apply_model_multi(x, t, conds, **kw):
        if calls is not None:
            calls.append((int(t[0]), x.clone()))
        return multi(x, t, conds, **kw)

    my_ddim.noise_like = lambda shape, device, repeat=False: next(it)
    model.q_sample = lambda x_start, t, noise=None: q_sample(x_start, t, noise=next(qit))
    model.apply_model_multi = apply_model_multi
    try:
        yield
    finally:
        my_ddim.noise_like = old_noise
        del model.q_sample, model.apply_model_multi


def conditioning(g):
    dev = lambda k: g[k].to(DEV)
    cc = dev("c_concat")
    cond = {"c_crossattn": [dev("cond")], "c_concat": [cc]}
    uc = {"c_crossattn": [dev("uncond")], "c_concat": [cc]}
    uc_img = {"c_crossattn": [dev("uncond_img")], "c_concat": [cc]}
    return cond, uc, uc_img


def run(model, g, tag, *, three_way=False, x_T="x_T", calls=None, **kw):
    """One reference run of the fixture on the mirror: (samples, pred_x0 per step, intermediates)."""
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWaySampler
    cond, uc, uc_img = conditioning(g)
    if three_way:
        kw.update(cfg_img=float(g["cfg_img"]), unconditional_conditioning_img_nonetext=uc_img)
    x0s = []
    with torch.no_grad(), injected(model, g[tag + "noises"], g[tag + "qnoises"], calls):
        out, inter = (ThreeWaySampler if three_way else DDIMSampler)(model).sample(
            S=5, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False, unconditional_conditioning=uc,
            fs=g["fs"].to(DEV), x_T=g[x_T].to(DEV), img_callback=lambda p, i: x0s.append(p.clone()), **SETTINGS, **kw)
    return out, x0s, inter


def check_trajectory(name, out, x0s, g, tag):
    errs = [rel_l2(p.cpu(), g[tag + "pred_x0"][i]) for i, p in enumerate(x0s)]
    final = rel_l2(out.cpu(), g[tag + "samples"])
    print(f"{name}: pred_x0 rel-L2 per step", [f"{e:.3e}" for e in errs], f"final {final:.3e}")
    assert len(x0s) == g[tag + "pred_x0"].shape[0] and torch.isfinite(out).all()
    assert max(errs) <= TRAJECTORY_BOUND and final <= TRAJECTORY_BOUND, (name, errs, final)


# ------------------------------------------------------------------------------------------------ 3. when the blend happens

def test_blend_happens_before_each_step_with_that_steps_noise_level(model, g):
    calls = []
    out, x0s, inter = run(model, g, "a_", mask=g["mask_frame"], x0=g["x0"], calls=calls, log_every_t=1)
    assert [t for t, _ in calls] == g["a_t"].tolist() == [999, 799, 599, 399, 199]
    sa, s1 = model.sqrt_alphas_cumprod.float().cpu(), model.sqrt_one_minus_alphas_cumprod.float().cpu()
    x_prev = [v.cpu() for v in inter["x_inter"]]                      # x_T, then every step's x_prev
    assert len(x_prev) == 6
    free = [0, 1, 3]
    for i, (t, x) in enumerate(calls):
        x = x.cpu()
        pinned = sa[t] * g["x0"] + s1[t] * g["a_qnoises"][i]           # CPU fp32, separate ops
        assert torch.equal(x[:, :, 2], pinned[:, :, 2]), f"step {i}: the pinned frame is not q_sample(x0, {t})"
        assert torch.equal(x[:, :, free], x_prev[i][:, :, free]), f"step {i}: a free frame was touched"
    # the result is the last x_prev as it is: no final blend, so the pinned frame is close to x0 and not equal to it
    assert torch.equal(out.cpu(), x_prev[-1])
    assert not torch.equal(out.cpu()[:, :, 2], g["x0"][:, :, 2])


# ------------------------------------------------------------------------------------------------ 4. trajectories

@pytest.mark.parametrize("tag", ["a_", "b_", "c_", "d_"])
def test_pinned_trajectory_vs_reference_golden(model, g, tag):
    kw = dict(a_=dict(mask=g["mask_frame"]), b_=dict(mask=g["mask_frame"], clean_cond=True), c_=dict(mask=g["mask_dense"]),
              d_=dict(mask=g["mask_frame"], three_way=True))[tag]
    out, x0s, _ = run(model, g, tag, x0=g["x0"], **kw)
    check_trajectory(f"pinned run ({tag[0]})", out, x0s, g, tag)


def test_decode_trajectory_vs_reference_golden(model, g):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    cond, uc, _ = conditioning(g)
    sampler = DDIMSampler(model)
    sampler.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    step, x0s, calls = sampler.p_sample_ddim, [], []

    def p_sample_ddim(*a, **kw):                                      # decode() drops pred_x0
        res = step(*a, **kw)
        x0s.append(res[1].clone())
        return res
    sampler.p_sample_ddim = p_sample_ddim
    with torch.no_grad(), injected(model, g["f_noises"], g["f_qnoises"], calls):
        out = sampler.decode(g["e_x_T"].to(DEV), cond, 2, unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    assert [t for t, _ in calls] == g["f_t"].tolist()
    check_trajectory("decode (f)", out, x0s, g, "f_")


# ------------------------------------------------------------------------------------------------ 5. partial runs

def test_stochastic_encode_is_bit_exact(model, g):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    sampler = DDIMSampler(model)
    sampler.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    with torch.no_grad():
        enc = sampler.stochastic_encode(g["x0"].to(DEV), torch.tensor([1], device=DEV), noise=g["e_enc_noise"].to(DEV))
        enc_host_index = sampler.stochastic_encode(g["x0"].to(DEV), [1], noise=g["e_enc_noise"].to(DEV))
    assert torch.equal(enc.cpu(), g["e_x_T"]) and torch.equal(enc_host_index, enc)
    with pytest.raises(NotImplementedError):
        sampler.stochastic_encode(g["x0"].to(DEV), [1], use_original_steps=True)


def test_partial_run_steps_and_trajectory(model, g):
    calls = []
    out, x0s, _ = run(model, g, "e_", x_T="e_x_T", timesteps=3, calls=calls)
    assert [t for t, _ in calls] == g["e_t"].tolist() == [399, 199]          # two steps, not three
    check_trajectory("timesteps=3 (e)", out, x0s, g, "e_")
    calls = []
    run(model, g, "a_", timesteps=5, calls=calls)                           # any five draws will do here
    assert [t for t, _ in calls] == g["subset_t_5"].tolist() == [799, 599, 399, 199]


# ------------------------------------------------------------------------------------------------ 6. clip level

def test_clip_level_pinning(model, g):
    sys.path.insert(0, GOLDEN)
    try:
        import pipeline_stubs as stubs
    finally:
        sys.path.remove(GOLDEN)
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd.lvdm import autoencoder as my_ae
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    saved = model.embedder, model.image_proj_model, my_ae.DiagonalGaussianDistribution.sample
    model.embedder, model.image_proj_model = stubs.StubEmbedder(), stubs.StubImageProj(4)
    model.get_learned_conditioning = lambda prompts: stubs.stub_text(prompts, DEV)
    my_ae.DiagonalGaussianDistribution.sample = lambda self, noise=None: self.mean
    gen = torch.Generator().manual_seed(77)
    videos = torch.randn(1, 3, 4, 64, 64, generator=gen).clamp(-1, 1).to(DEV)
    frame = torch.randn(1, 3, 64, 64, generator=gen).clamp(-1, 1).to(DEV)
    shape = [1, 4, 4, 8, 8]
    plan = pipeline.SamplingPlan(steps=3, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7)
    x_T = g["x_T"].to(DEV)
    try:
        with torch.no_grad():
            x0, mask = pipeline.pin_frames(model, {2: frame}, 4)
            assert x0.shape == (1, 4, 4, 8, 8) and mask.shape == (1, 1, 4, 1, 1) and mask.flatten().tolist() == [0, 0, 1, 0]
            assert torch.equal(x0[:, :, 2], model.encode_first_stage(frame)) and not x0[:, :, [0, 1, 3]].any()
            cond = pipeline.Conditions.build(model, videos, fs=10)

            def direct(m):
                with injected(model, g["a_noises"], g["a_qnoises"]):
                    return DDIMSampler(model).sample(
                        S=3, conditioning=cond.positive, batch_size=1, shape=(4, 4, 8, 8), verbose=False,
                        unconditional_conditioning=cond.negative, mask=m, x0=x0, fs=cond.fs, x_T=x_T, **SETTINGS)[0]
            with injected(model, g["a_noises"], g["a_qnoises"]):
                via_clip = pipeline.sample(model, cond, plan, shape, x_T=x_T, pinned=(x0, mask))
            with injected(model, g["a_noises"], g["a_qnoises"]):                       # the reference callers' route: **kwargs
                plan_kw = pipeline.SamplingPlan(**{**plan.__dict__, "extra": dict(mask=mask, x0=x0, x_T=x_T)})
                via_kwargs = pipeline.sample(model, cond, plan_kw, shape)
            dense = direct(mask)
            assert torch.equal(via_clip, dense) and torch.equal(via_kwargs, dense)
            # a (1,1,T,1,1) bool selector on the CPU == its dense fp32 expansion on the device
            as_bool = direct(torch.tensor([False, False, True, False]).view(1, 1, 4, 1, 1))
            as_dense = direct(mask.expand(1, 4, 4, 8, 8).contiguous())
            assert torch.equal(as_bool, dense) and torch.equal(as_dense, dense)
            with injected(model, g["a_noises"], g["a_qnoises"]):                       # and an unpinned run differs
                assert not torch.equal(pipeline.sample(model, cond, plan, shape, x_T=x_T), dense)
            video = pipeline.synthesize(model, videos, shape, plan=plan, fs=10, keyframes={2: frame})
        assert tuple(video.shape) == (1, 1, 3, 4, 64, 64) and torch.isfinite(video).all()
    finally:
        model.embedder, model.image_proj_model, my_ae.DiagonalGaussianDistribution.sample = saved
        del model.get_learned_conditioning


# ------------------------------------------------------------------------------------------------ 7. graphed forward

def test_pinned_run_graphed_equals_eager(model, g):
    """The blend sits outside the captured UNet forward: with the hipGraph route of apply_model_multi replaying (from the
    second guided step of a run on), a pinned run equals the eager one bit for bit."""
    kw = dict(mask=g["mask_frame"], x0=g["x0"])
    saved = model.use_hipgraph
    try:
        model.use_hipgraph, model._cfg_state = True, None
        out_g, x0s_g, _ = run(model, g, "a_", **kw)
        assert model._cfg_state["graph"] is not None, "the graphed route did not engage"
        model.use_hipgraph, model._cfg_state = False, None
        out_e, x0s_e, _ = run(model, g, "a_", **kw)
        assert model._cfg_state["graph"] is None
    finally:
        model.use_hipgraph, model._cfg_state = saved, None
    assert torch.equal(out_g, out_e)
    assert len(x0s_g) == len(x0s_e) == 5 and all(torch.equal(a, b) for a, b in zip(x0s_g, x0s_e))
