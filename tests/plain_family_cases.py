"""Shared pieces of tests/test_plain_family_cpu.py and tests/test_gpu_plain_family.py (the DynamiCrafter-family support:
plain AutoencoderKL first stage, eps parameterisation, image cross-attention scale / learnable alpha): the tiny
configurations built from the YAML fixtures, the eps statement of the fused step, and the models on synthetic weights.
Fixtures: tests/golden/make_plain_family_golden.py."""
import copy
import json
import os

import torch
import yaml

from conftest import GOLDEN, TINY_UNET_CFG
from emu_ops import EmuOps

YAMLS = ("training_1024_v1.0", "training_512_v1.0")
# Plain decoder, golden (a): rel-L2 of the EMULATED operator contract (tests/emu_ops.py, bf16 between operators, on the CPU)
# against the reference's fp32 output.  All three exceed 2/3 of the 2.0e-2 borrowed from the tiny dual-reference decoder
# test, so that bound is not usable here; the GPU test holds the kernels to 1.5 x these figures instead -- figures of the
# contract, not of the code under test (tests/test_plain_family_cpu.py re-measures them).  In exact arithmetic on the same
# bf16 weights the three are 1.31e-2 / 9.0e-3 / 9.0e-3: the plain decoder's floor is higher than the video decoder's.
DECODER_CONTRACT = {"dec4": 2.548e-2, "dec4_core": 1.766e-2, "dec5_core": 1.750e-2}
DECODER_BORROWED = 2.0e-2
TINY_UNET = dict(model_channels=64, context_dim=96, temporal_length=4, use_checkpoint=False)


def yaml_model(name):
    with open(os.path.join(GOLDEN, name + ".model.yaml")) as f:
        return yaml.safe_load(f)["model"]


def tiny_model_cfg(name="training_1024_v1.0", **overrides):
    """The `model:` node of a YAML fixture with its sizes overridden to tiny and the conditioners replaced by Identity
    (what make_plain_family_golden.tiny_config does to the reference's file); structure and class paths untouched."""
    m = copy.deepcopy(yaml_model(name))
    p = m["params"]
    p["image_size"] = [8, 8]
    p["unet_config"]["params"].update(TINY_UNET)
    p["first_stage_config"]["params"]["ddconfig"]["ch"] = 64
    for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
        p[k] = {"target": "torch.nn.Identity"}
    p.update(overrides)
    return m


def manifest():
    with open(os.path.join(GOLDEN, "plain_family_manifest.json")) as f:
        return json.load(f)


def tiny_pipeline(name="training_1024_v1.0", **overrides):
    """LatentVisualDiffusion of a YAML fixture at tiny sizes, on the synthetic weights the fixtures were made with."""
    from tooncrafter_amd import synth
    from tooncrafter_amd.utils import instantiate_from_config
    model = instantiate_from_config(tiny_model_cfg(name, **overrides)).eval()
    synth.fill_module_(model, seed=1234)
    return model


def tiny_unet(**extra):
    from tooncrafter_amd import synth
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    un = UNetModel(**dict(TINY_UNET_CFG, **extra)).eval()
    synth.fill_module_(un, prefix="model.diffusion_model.", seed=1234)
    return un


def set_alphas(unet, golden):
    """Every block's alpha at the value the fixture recorded for it (distinct, non-zero)."""
    params = dict(unet.named_parameters())
    names = [str(n) for n in golden["alpha_names"]]
    assert names and sorted(names) == sorted(k for k in params if k.endswith(".alpha"))
    with torch.no_grad():
        for n, v in zip(names, golden["alpha_values"]):
            params[n].fill_(float(v))
    unet.invalidate()


def set_image_scale(unet, scale):
    """image_cross_attention_scale where the reference reads it: an attribute of every image cross-attention (UNetModel
    does not thread it, openaimodel3d.py:339-516)."""
    from tooncrafter_amd.lvdm.attention import CrossAttention
    n = 0
    for m in unet.modules():
        if isinstance(m, CrossAttention) and m.image_cross_attention:
            m.image_cross_attention_scale = scale
            n += 1
    return n


def eps_step_f64(x, e_cond, e_uncond, noise, *, cfg_scale, guidance_rescale, sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef,
                 sigma, x0_rescale, e_uncond_img=None, cfg_img=None):
    """One DDIM update of an eps-parameterised model in fp64, as the reference's samplers state it (samplers/ddim.py:226-234,
    257-277; ddim_multiplecond.py:236; utils_diffusion.py:147-158): the guided, rescaled model output IS e_t."""
    d = lambda t: None if t is None else t.double()
    x, ec, eu, ei, nz = d(x), d(e_cond), d(e_uncond), d(e_uncond_img), d(noise)
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))            # the scalars travel as fp32
    e = ec
    if eu is not None:
        if ei is not None:
            ci = cfg_scale if cfg_img is None else cfg_img
            e = eu + f(ci) * (ei - eu) + f(cfg_scale) * (ec - ei)
        else:
            e = eu + f(cfg_scale) * (ec - eu)
        if guidance_rescale > 0:
            dims = list(range(1, e.dim()))
            fac = ec.std(dim=dims, keepdim=True) / e.std(dim=dims, keepdim=True)
            e = f(guidance_rescale) * (e * fac) + (1 - f(guidance_rescale)) * e
    x0 = (x - f(sqrt_1m_ac) * e) / f(sqrt_ac)
    x0 = x0 * f(x0_rescale)
    xp = f(sqrt_a_prev) * x0 + f(dir_coef) * e
    if nz is not None:
        xp = xp + f(sigma) * nz
    return xp, x0


class EpsEmuOps(EmuOps):
    """tests/emu_ops.py plus the `parameterization` keyword of ops.ddim_step: "eps" is the fp64 statement above rounded to
    fp32, "v" the inherited emulation, untouched."""

    def ddim_step(self, x, e_cond, e_uncond, noise, *, parameterization="v", want_x0=True, **kw):
        if parameterization == "v":
            return super().ddim_step(x, e_cond, e_uncond, noise, want_x0=want_x0, **kw)
        assert parameterization == "eps"
        xp, x0 = eps_step_f64(x, e_cond, e_uncond, noise, **kw)
        return xp.float(), (x0.float() if want_x0 else None)


def run_sampler(model, sampler_cls, g, tag, dev="cpu"):
    """The recorded eps trajectory `tag` ("a_": samplers/ddim.py, "m_": ddim_multiplecond.py) on `model`: S = 5, uniform
    spacing, CFG 7.5, rescale 0.7, eta 1, the fixture's noise.  -> (samples, [pred_x0 per step])"""
    from tooncrafter_amd.lvdm import ddim as my_ddim
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    cond = {"c_crossattn": [t("cond")], "c_concat": [t("c_concat")]}
    uc = {"c_crossattn": [t("uncond")], "c_concat": [t("c_concat")]}
    extra = dict(cfg_img=None, unconditional_conditioning_img_nonetext=None)
    if tag == "m_":
        extra = dict(cfg_img=float(g["cfg_img"]),
                     unconditional_conditioning_img_nonetext={"c_crossattn": [t("uncond_img")], "c_concat": [t("c_concat")]})
    it = iter(t(tag + "noises"))
    old = my_ddim.noise_like
    my_ddim.noise_like = lambda shape, device, repeat=False: next(it)
    try:
        x0s = []
        out, _ = sampler_cls(model).sample(S=5, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False,
                                           unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0,
                                           mask=None, x0=None, fs=t("fs"), timestep_spacing="uniform", guidance_rescale=0.7,
                                           x_T=t("x_T"), img_callback=lambda p, i: x0s.append(p.clone()), **extra)
    finally:
        my_ddim.noise_like = old
    return out, x0s
