"""DynamiCrafter-family support on the MI355X: tc_ddim_step_eps (the eps instance of the fused DDIM step), the plain
AutoencoderKL first stage, the image cross-attention scale / learnable alpha, and a tiny pipeline of the
training_1024_v1.0 configuration end to end.  Goldens: tests/golden/make_plain_family_golden.py (the real reference, fp32).
Bounds: the fp32 criterion of tests/test_gpu_ops.py for the step; 1.5 x the emulated-contract figure for the plain decoder
(plain_family_cases.DECODER_CONTRACT: the 2.0e-2 of the dual-reference decoder test is under the contract's own error
here); 3.5e-2 for a tiny UNet forward; 0.15 for a CFG-7.5 trajectory."""
import pytest
import torch

import plain_family_cases as pf
from conftest import load_golden, rel_l2
from test_gpu_guard import rnd as guarded
from test_gpu_ops import check
from tooncrafter_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _with_backend(backend, fn):
    prev = ops.set_backend(backend)
    try:
        return fn()
    finally:
        ops.set_backend(prev)


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def tlib():
    from tooncrafter_amd.torch_ops import TorchLibOps
    return TorchLibOps()


# ------------------------------------------------------------------------------------------------ tc_ddim_step_eps
SC = dict(sqrt_ac=0.6, sqrt_1m_ac=0.8, sqrt_a_prev=0.7, dir_coef=0.5, x0_rescale=0.98)
ROWS = {"cfg_rescale_noise": dict(cfg=7.5, resc=0.7, noise=True, three=False),
        "cfg_plain_sigma0": dict(cfg=7.5, resc=0.0, noise=False, three=False),
        "no_cfg": dict(cfg=1.0, resc=0.0, noise=True, three=False),
        "three_way": dict(cfg=7.5, resc=0.7, noise=True, three=True)}


def _step_args(shape, row, make=None):
    gen = torch.Generator().manual_seed(sum(shape))
    make = make or (lambda seed: torch.randn(shape, generator=gen).to(DEV))
    x, ec, eu, ei, nz = (make(s) for s in (42, 43, 44, 45, 46))
    kw = dict(cfg_scale=row["cfg"], guidance_rescale=row["resc"], sigma=0.3 if row["noise"] else 0.0, **SC)
    if row["three"]:
        kw.update(e_uncond_img=ei, cfg_img=2.0)
    return (x, ec, eu if row["cfg"] != 1.0 else None, nz if row["noise"] else None), kw


@pytest.mark.parametrize("shape", [(2, 4, 3, 6, 10), (2, 4, 16, 8, 8)])
@pytest.mark.parametrize("row", list(ROWS))
def test_ddim_step_eps(hip, tlib, shape, row):
    args, kw = _step_args(shape, ROWS[row])
    xp, x0 = hip.ddim_step(*args, parameterization="eps", **kw)
    rp, r0 = pf.eps_step_f64(*args, **kw)
    check(xp, rp.float(), f"eps x_prev {row} {shape}", f32=True)
    check(x0, r0.float(), f"eps pred_x0 {row} {shape}", f32=True)
    tp, t0 = tlib.ddim_step(*args, parameterization="eps", **kw)         # the two bindings: the same bits
    assert torch.equal(tp, xp) and torch.equal(t0, x0)
    # the v step through the new keyword is the call without it, bit for bit, in both bindings -- and not the eps step
    for be in (hip, tlib):
        vp, v0 = be.ddim_step(*args, **kw)
        kp, k0 = be.ddim_step(*args, parameterization="v", **kw)
        assert torch.equal(vp, kp) and torch.equal(v0, k0)
        assert not torch.equal(v0, x0)
    assert hip.ddim_step(*args, parameterization="eps", want_x0=False, **kw)[1] is None
    with pytest.raises(NotImplementedError):
        hip.ddim_step(*args, parameterization="x0", **kw)


@pytest.mark.parametrize("three", [False, True])
def test_guard_ddim_step_eps(hip, three):
    """Every input ends flush with its own device region (tests/test_gpu_guard.py): a read past n elements would fault."""
    shape = (2, 4, 3, 2, 2)
    row = dict(cfg=7.5, resc=0.7, noise=True, three=three)
    args, kw = _step_args(shape, row, make=lambda seed: guarded(*shape, seed=seed, dtype=torch.float32))
    xp, x0 = hip.ddim_step(*args, parameterization="eps", **kw)
    rp, r0 = pf.eps_step_f64(*args, **kw)
    torch.cuda.synchronize()
    assert rel_l2(xp.cpu(), rp.cpu()) < 1e-4 and rel_l2(x0.cpu(), r0.cpu()) < 1e-4


def test_ddim_step_eps_refuses_a_zero_sqrt_ac(hip):
    from tooncrafter_amd._lib import TooncrafterHipError
    args, kw = _step_args((1, 4, 2, 2, 2), ROWS["no_cfg"])
    with pytest.raises(TooncrafterHipError):
        hip.ddim_step(*args, parameterization="eps", **dict(kw, sqrt_ac=0.0))


# ------------------------------------------------------------------------------------------------ plain decoder (a)
@pytest.fixture(scope="module")
def plain_pipeline():
    return pf.tiny_pipeline().to(DEV)


def test_plain_decoder_vs_reference_golden(hip, plain_pipeline):
    g = load_golden("plain_decoder_tiny.npz")
    model = plain_pipeline
    z4, z5 = torch.from_numpy(g["z4"]).to(DEV), torch.from_numpy(g["z5"]).to(DEV)

    def run():
        raw = model.first_stage_model.decode(z4)
        outs = {}
        for flag in (True, False):
            model.perframe_ae = flag
            outs[flag] = (model.decode_first_stage(z4), model.decode_first_stage(z5, ref_context=None))
        model.perframe_ae = True
        as_clip = model.decode_first_stage(z4.permute(1, 0, 2, 3).unsqueeze(0).contiguous())
        again = model.decode_first_stage(z5)
        return raw, outs, as_clip, again
    with torch.no_grad():
        raw, outs, as_clip, again = _with_backend(hip, run)
        emu5 = _with_backend(pf.EpsEmuOps(), lambda: model.decode_first_stage(z5))
    errs = {"dec4": rel_l2(raw.cpu(), torch.from_numpy(g["dec4"])),
            "dec4_core": rel_l2(outs[True][0].cpu(), torch.from_numpy(g["dec4_core_pf1"])),
            "dec5_core": rel_l2(outs[True][1].cpu(), torch.from_numpy(g["dec5_core_pf1"]))}
    e_emu = rel_l2(outs[True][1].cpu(), emu5.cpu())
    print("plain decoder vs reference golden:", {k: f"{v:.3e}" for k, v in errs.items()}, f"; 5-D vs emulated contract {e_emu:.3e}")
    assert tuple(outs[True][1].shape) == (1, 3, 3, 64, 96) and torch.isfinite(outs[True][1]).all()
    for k, v in errs.items():
        assert v < 1.5 * pf.DECODER_CONTRACT[k], (k, v)
    assert e_emu < 1.5 * pf.DECODER_CONTRACT["dec5_core"]
    # perframe_ae True == False, a 4-D latent == the same frames as a 5-D clip, and a second decode, bit for bit (the
    # plain decode is eager: there is no graph replay to compare)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    assert torch.equal(as_clip[0].permute(1, 0, 2, 3), outs[True][0])
    assert torch.equal(again, outs[True][1])


# ------------------------------------------------------------------------------------------------ alpha / scale (c)
def test_alpha_and_scale_unet_vs_reference_golden(hip):
    g = load_golden("unet_alpha_tiny.npz")
    args = (torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["timesteps"]).to(DEV))
    kw = dict(context=torch.from_numpy(g["context"]).to(DEV), fs=torch.from_numpy(g["fs"]).to(DEV))
    un = pf.tiny_unet(image_cross_attention_scale_learnable=True).to(DEV)
    plain = pf.tiny_unet().to(DEV)

    def run():
        y_zero = un(*args, **kw).clone()                                 # every alpha zeroed below, before the run
        pf.set_alphas(un, g)
        y_alpha = un(*args, **kw).clone()
        y_plain = plain(*args, **kw).clone()
        pf.set_image_scale(plain, float(g["scale"]))
        y_scale = plain(*args, **kw).clone()
        return y_zero, y_alpha, y_plain, y_scale
    with torch.no_grad():
        for n, p in un.named_parameters():
            if n.endswith(".alpha"):
                p.zero_()
        y_zero, y_alpha, y_plain, y_scale = _with_backend(hip, run)
    e_a, e_s = rel_l2(y_alpha.cpu(), torch.from_numpy(g["y_alpha"])), rel_l2(y_scale.cpu(), torch.from_numpy(g["y_scale"]))
    print(f"tiny UNet vs reference golden: learnable alpha {e_a:.3e}; image scale 0.5 {e_s:.3e}")
    assert torch.isfinite(y_alpha).all() and e_a < 3.5e-2 and e_s < 3.5e-2
    assert torch.equal(y_zero, y_plain)                                  # alpha 0, scale 1: the model without the flag
    assert rel_l2(y_alpha.cpu(), y_plain.cpu()) > 3.5e-2 and rel_l2(y_scale.cpu(), y_plain.cpu()) > 3.5e-2


# ------------------------------------------------------------------------------------------------ eps trajectories (b)
@pytest.fixture(scope="module")
def eps_pipeline():
    return pf.tiny_pipeline(parameterization="eps", rescale_betas_zero_snr=False).to(DEV)


@pytest.mark.parametrize("tag", ["a_", "m_"])
def test_eps_trajectory_vs_reference_golden(hip, eps_pipeline, tag):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWay
    g = load_golden("ddim_eps_tiny.npz")
    with torch.no_grad():
        out, x0s = _with_backend(hip, lambda: pf.run_sampler(eps_pipeline, DDIMSampler if tag == "a_" else ThreeWay, g, tag, DEV))
    errs = [rel_l2(p.cpu(), torch.from_numpy(g[tag + "pred_x0"][i])) for i, p in enumerate(x0s)]
    final = rel_l2(out.cpu(), torch.from_numpy(g[tag + "samples"]))
    print(f"eps trajectory {tag} vs reference: pred_x0 rel-L2 per step", [f"{e:.3e}" for e in errs], f"final {final:.3e}")
    assert torch.isfinite(out).all() and len(x0s) == 5
    assert max(errs) < 0.15 and final < 0.15


# ------------------------------------------------------------------------------------------------ end to end
def test_tiny_1024_pipeline_end_to_end(hip, plain_pipeline):
    """Conditions.build(hold_endpoints=False) -> sample (2 steps) -> decode_spliced on the tiny training_1024_v1.0 model:
    finite, the right shape, and frame for frame decode_first_stage of the same latents outside the two spliced centre
    frames (the plain decoder's frames are independent, so the splice changes nothing but those two)."""
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import pipeline_stubs as stubs
    from tooncrafter_amd import clip as pipeline
    model = plain_pipeline
    T = 4
    keep = (model.embedder, model.image_proj_model, model.__dict__.get("get_learned_conditioning"))
    model.embedder, model.image_proj_model = stubs.StubEmbedder(), stubs.StubImageProj(T)
    model.get_learned_conditioning = lambda prompts: stubs.stub_text(prompts, DEV)
    gen = torch.Generator().manual_seed(61)
    videos = torch.randn(1, 3, T, 64, 64, generator=gen).clamp(-1, 1).to(DEV)
    x_T = torch.randn(1, 4, T, 8, 8, generator=gen).to(DEV)

    def run():
        cond = pipeline.Conditions.build(model, videos, fs=10, hold_endpoints=False)
        plan = pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7)
        lat = pipeline.sample(model, cond, plan, (1, 4, T, 8, 8), x_T=x_T)
        return cond, lat, pipeline.decode_spliced(model, lat, cond.refs), model.decode_first_stage(lat)
    try:
        with torch.no_grad():
            cond, lat, video, plain = _with_backend(hip, run)
    finally:
        model.embedder, model.image_proj_model = keep[0], keep[1]
        if keep[2] is None:
            del model.get_learned_conditioning
    c = T // 2
    assert tuple(video.shape) == (1, 3, T, 64, 64) and torch.isfinite(video).all() and torch.isfinite(lat).all()
    assert torch.equal(cond.positive["c_concat"][0][:, :, 0], cond.positive["c_concat"][0][:, :, T - 1])   # frame 0 repeated
    outside = [i for i in range(T) if i not in (c - 1, c)]
    assert torch.equal(video[:, :, outside], plain[:, :, outside])
    assert float(video.std()) > 1e-3
