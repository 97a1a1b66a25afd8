"""DynamiCrafter-family support without a GPU: the plain AutoencoderKL first stage, the eps parameterisation of the fused
DDIM step and the image cross-attention scale / learnable alpha.  The configurations of the reference's
configs/training_{512,1024}_v1.0 build through the drop-in and load strictly; the host logic runs on the emulated
operator contract (tests/emu_ops.py) against the reference's goldens (tests/golden/make_plain_family_golden.py)."""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import plain_family_cases as pf
from conftest import ROOT, TINY_DD_CFG, load_golden, rel_l2
from emu_ops import EmuOps
from tooncrafter_amd import _lib, ops, synth


@pytest.fixture()
def emu():
    prev = ops.set_backend(pf.EpsEmuOps(round_bf16=True))
    yield
    ops.set_backend(prev)


@pytest.fixture()
def dropin_installed():
    from tooncrafter_amd import dropin
    mine = lambda k: k == "lvdm" or k.startswith("lvdm.") or k in ("utils", "utils.utils")
    saved = {k: v for k, v in sys.modules.items() if mine(k)}
    dropin.install(shims=False)
    yield
    for k in [k for k in sys.modules if mine(k)]:
        del sys.modules[k]
    sys.modules.update(saved)


# ------------------------------------------------------------------------------------------------ configurations
@pytest.mark.parametrize("name", pf.YAMLS)
def test_yaml_fixture_names_the_plain_first_stage(name):
    p = pf.yaml_model(name)["params"]
    assert p["first_stage_config"]["target"] == "lvdm.models.autoencoder.AutoencoderKL"
    assert p["perframe_ae"] is True and p["fps_condition_type"] == "fps" and p["parameterization"] == "v"
    assert p["image_size"] == ([72, 128] if "1024" in name else [40, 64])


@pytest.mark.parametrize("name", pf.YAMLS)
def test_yaml_instantiates_through_dropin_at_tiny_sizes(name, dropin_installed):
    from utils.utils import instantiate_from_config              # what scripts/evaluation/inference.py:16 imports
    cls = getattr(importlib.import_module("lvdm.models.autoencoder"), "AutoencoderKL")
    assert cls.__module__ == "tooncrafter_amd.lvdm.autoencoder"
    model = instantiate_from_config(pf.tiny_model_cfg(name))
    from tooncrafter_amd.lvdm import ae_modules, autoencoder
    assert type(model.first_stage_model) is autoencoder.AutoencoderKL
    assert type(model.first_stage_model.decoder) is ae_modules.Decoder
    assert model.perframe_ae is True and model.fps_condition_type == "fps" and model.rand_cond_frame is True
    base = pf.yaml_model(name)["params"]["base_scale"]                   # 0.3 at 1024, 0.7 at 512
    assert model.use_dynamic_rescale and abs(float(model.scale_arr[-1]) - base) < 1e-7


def test_full_1024_yaml_instantiates_on_meta(dropin_installed):
    """The complete training_1024_v1.0 model section (320-channel UNet, ViT-H/14 towers, Resampler, 128-channel plain
    autoencoder) builds through the drop-in; its first stage has the parameters of the reference's AutoencoderKL."""
    from utils.utils import instantiate_from_config
    cfg = pf.yaml_model("training_1024_v1.0")
    with torch.device("meta"):
        model = instantiate_from_config(cfg)
    assert model.image_size == [72, 128] and model.temporal_length == 16
    tiny = pf.manifest()["autoencoder"]
    mine = {k: list(v.shape) for k, v in model.first_stage_model.state_dict().items()}
    assert set(mine) == set(tiny)                                        # same names; the widths are twice the tiny ones
    assert mine["decoder.conv_in.weight"] == [512, 4, 3, 3] and mine["post_quant_conv.weight"] == [4, 4, 1, 1]


def test_state_dicts_load_strictly_from_the_reference_manifests():
    from tooncrafter_amd.lvdm.autoencoder import AutoencoderKL, AutoencoderKL_Dualref
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    man = pf.manifest()
    assert man["ddconfig"] == dict(TINY_DD_CFG)
    ae = AutoencoderKL(ddconfig=dict(TINY_DD_CFG), lossconfig=dict(target="torch.nn.Identity"), embed_dim=4)
    sd = synth.synth_state_dict({k: tuple(v) for k, v in man["autoencoder"].items()}, seed=5)
    assert ae.load_state_dict(sd, strict=True) is not None
    assert {k: list(v.shape) for k, v in ae.state_dict().items()} == man["autoencoder"]
    assert issubclass(AutoencoderKL_Dualref, AutoencoderKL)              # encode is shared, as in the reference
    un = pf.tiny_unet(image_cross_attention_scale_learnable=True)
    sd = synth.synth_state_dict({k: tuple(v) for k, v in man["unet_alpha"].items()}, seed=5)
    un.load_state_dict(sd, strict=True)
    alphas = [k for k in man["unet_alpha"] if k.endswith(".alpha")]
    assert len(alphas) == 16 and all(man["unet_alpha"][k] == [] for k in alphas)
    plain = UNetModel(**pf.TINY_UNET_CFG)
    with pytest.raises(RuntimeError):                                    # without the flag the keys have no home
        plain.load_state_dict(sd, strict=True)


def test_decoder_variants_raise():
    from tooncrafter_amd.lvdm.ae_modules import Decoder
    for bad in (dict(attn_resolutions=[16]), dict(give_pre_end=True), dict(tanh_out=True), dict(use_linear_attn=True)):
        with pytest.raises(NotImplementedError):
            Decoder(**dict(TINY_DD_CFG, **bad))


# ------------------------------------------------------------------------------------------------ (a) plain decoder
def test_plain_decoder_host_logic_vs_reference_golden(emu):
    """Golden (a) on the emulated contract.  These figures decide the bound of the GPU test: the 2.0e-2 borrowed from the
    tiny dual-reference decoder would stand only while the contract itself stayed under 2/3 of it.  It does not (2.55e-2 /
    1.77e-2 / 1.75e-2), so the GPU test uses 1.5 x the figures recorded in plain_family_cases.DECODER_CONTRACT, and this
    test pins that those figures are what the contract gives."""
    g = load_golden("plain_decoder_tiny.npz")
    model = pf.tiny_pipeline()
    z4, z5 = torch.from_numpy(g["z4"]), torch.from_numpy(g["z5"])
    with torch.no_grad():
        raw = model.first_stage_model.decode(z4)
        outs = {}
        for flag in (True, False):
            model.perframe_ae = flag
            outs[flag] = (model.decode_first_stage(z4), model.decode_first_stage(z5, ref_context=None, anything="ignored"))
        as_clip = model.decode_first_stage(z4.permute(1, 0, 2, 3).unsqueeze(0))          # the same two frames as one clip
    e_raw = rel_l2(raw, torch.from_numpy(g["dec4"]))
    e4 = rel_l2(outs[True][0], torch.from_numpy(g["dec4_core_pf1"]))
    e5 = rel_l2(outs[True][1], torch.from_numpy(g["dec5_core_pf1"]))
    print(f"plain decoder, emulated contract vs reference: decode {e_raw:.3e}; decode_core 4-D {e4:.3e}, 5-D {e5:.3e}")
    assert tuple(outs[True][1].shape) == (1, 3, 3, 64, 96) and tuple(raw.shape) == (2, 3, 64, 64)
    got = {"dec4": e_raw, "dec4_core": e4, "dec5_core": e5}
    for k, v in pf.DECODER_CONTRACT.items():
        assert abs(got[k] - v) <= 0.02 * v, (k, got[k], v)               # fp32 summation order of the host BLAS: 2 %
        assert v > pf.DECODER_BORROWED * (2 / 3)                         # why the borrowed bound is not the one in use
    assert np.array_equal(g["dec4_core_pf1"], g["dec4_core_pf0"])        # the reference: perframe_ae does not change the tensor
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    assert torch.equal(as_clip[0].permute(1, 0, 2, 3), outs[True][0])
    with pytest.raises(TypeError):                                       # the plain decoder takes no decode kwargs
        model.first_stage_model.decode(z4, timesteps=2)


def test_post_quant_conv_is_not_composed_into_conv_in():
    """conv_in zero-pads AFTER the 1x1: with a large post_quant bias the border of the image differs from what a composed
    3x3 would give, so the exact-arithmetic decode must match torch's two separate convolutions there."""
    import torch.nn.functional as F
    from tooncrafter_amd.lvdm.autoencoder import AutoencoderKL
    prev = ops.set_backend(EmuOps(round_bf16=False))
    try:
        ae = AutoencoderKL(ddconfig=dict(TINY_DD_CFG), embed_dim=4).eval()
        synth.fill_module_(ae, prefix="first_stage_model.", seed=1234)
        with torch.no_grad():
            ae.post_quant_conv.bias.fill_(3.0)
            z = torch.randn(1, 4, 4, 6, generator=torch.Generator().manual_seed(3))
            from tooncrafter_amd.lvdm.common import Act
            wp, bp = ae._post_quant()
            rows = ops.nchw_to_rows(z.reshape(1, 4, 1, 4, 6), c_pad=64)
            h = ops.gemm(ops.gemm(rows, wp, bp), ae.decoder.pk["wi"], ae.decoder.pk["bi"],
                         conv=dict(kind="3x3", frames=1, cin=64, h_in=4, w_in=6, h_out=4, w_out=6, stride=1, upsample=False))
            got = ops.rows_to_nchw(h, c=h.shape[1], b=1, t=1, h=4, w=6)[:, :, 0]
            bf = lambda t: t.to(torch.bfloat16).float()                  # the packed weights are bf16
            ref = F.conv2d(F.conv2d(bf(z), bf(ae.post_quant_conv.weight), ae.post_quant_conv.bias),
                           bf(ae.decoder.conv_in.weight), ae.decoder.conv_in.bias, padding=1)
        assert rel_l2(got, ref) < 1e-5
        assert rel_l2(got[:, :, 0], ref[:, :, 0]) < 1e-5                 # the top border row
    finally:
        ops.set_backend(prev)


# ------------------------------------------------------------------------------------------------ (c) alpha / scale
def test_alpha_unet_host_logic_vs_reference_golden(emu):
    g = load_golden("unet_alpha_tiny.npz")
    assert float(g["d_alpha"]) > 3.5e-2 and float(g["d_scale"]) > 3.5e-2   # a missing factor cannot pass the bound
    args = (torch.from_numpy(g["x"]), torch.from_numpy(g["timesteps"]))
    kw = dict(context=torch.from_numpy(g["context"]), fs=torch.from_numpy(g["fs"]))
    un = pf.tiny_unet(image_cross_attention_scale_learnable=True)
    pf.set_alphas(un, g)
    plain = pf.tiny_unet()
    with torch.no_grad():
        y_alpha = un(*args, **kw)
        y_plain = plain(*args, **kw)
        assert pf.set_image_scale(plain, float(g["scale"])) == 16
        y_scale = plain(*args, **kw)                                     # the attribute alone re-packs (no invalidate())
    e_a, e_s = rel_l2(y_alpha, torch.from_numpy(g["y_alpha"])), rel_l2(y_scale, torch.from_numpy(g["y_scale"]))
    print(f"tiny UNet, emulated contract vs reference: learnable alpha {e_a:.3e}; image scale 0.5 {e_s:.3e}; "
          f"scale 0.5 against scale 1: {rel_l2(y_scale, y_plain):.3e}")
    assert max(e_a, e_s) < 3.5e-2 * (2 / 3)
    assert rel_l2(y_scale, y_plain) > 3.5e-2


def test_alpha_zero_is_the_model_without_the_flag_and_changes_repack(emu):
    g = load_golden("unet_alpha_tiny.npz")
    args = (torch.from_numpy(g["x"]), torch.from_numpy(g["timesteps"]))
    kw = dict(context=torch.from_numpy(g["context"]), fs=torch.from_numpy(g["fs"]))
    un, plain = pf.tiny_unet(image_cross_attention_scale_learnable=True), pf.tiny_unet()
    with torch.no_grad():
        for n, p in un.named_parameters():
            if n.endswith(".alpha"):
                p.zero_()
        y0, yp = un(*args, **kw), plain(*args, **kw)
        assert torch.equal(y0, yp)                                       # tanh(0) + 1 == 1: the same packed weights
        first = [p for n, p in un.named_parameters() if n.endswith(".alpha")][0]
        first.fill_(0.8)                                                 # in place, no load_state_dict: the pack follows
        y1 = un(*args, **kw)
    assert not torch.equal(y1, y0)


def test_ip_factor_is_folded_into_the_v_rows():
    from tooncrafter_amd.lvdm.attention import CrossAttention
    torch.manual_seed(0)
    ca = CrossAttention(query_dim=64, context_dim=96, heads=1, image_cross_attention=True, image_cross_attention_scale=0.5,
                        image_cross_attention_scale_learnable=True)
    with torch.no_grad():
        ca.alpha.fill_(-0.4)
    s = 0.5 * (float(torch.tanh(torch.tensor(-0.4))) + 1)
    assert abs(ca.ip_factor() - s) < 1e-7
    w = ca.pk["wkv_ip"].float()
    assert torch.equal(w[:64], ca.to_k_ip.weight.detach().to(torch.bfloat16).float())
    assert torch.equal(w[64:], (ca.to_v_ip.weight.detach() * ca.ip_factor()).to(torch.bfloat16).float())
    assert "alpha" in ca.state_dict() and ca.state_dict()["alpha"].shape == ()
    assert "alpha" not in CrossAttention(query_dim=64, context_dim=96, heads=1, image_cross_attention=True).state_dict()


# ------------------------------------------------------------------------------------------------ (b) eps
def test_eps_statement_matches_the_reference_formulas():
    """The fp64 statement the GPU test holds the kernel to, against the lines of the reference written out with torch ops
    (ddim.py:226-234, 258, 262-277) in fp32."""
    gen = torch.Generator().manual_seed(1)
    x, ec, eu, nz = (torch.randn(2, 4, 3, 6, 10, generator=gen) for _ in range(4))
    sc = dict(sqrt_ac=0.6, sqrt_1m_ac=0.8, sqrt_a_prev=0.7, dir_coef=0.5, sigma=0.3, x0_rescale=0.98)
    xp, x0 = pf.eps_step_f64(x, ec, eu, nz, cfg_scale=7.5, guidance_rescale=0.7, **sc)
    e = eu + 7.5 * (ec - eu)
    fac = ec.std(dim=[1, 2, 3, 4], keepdim=True) / e.std(dim=[1, 2, 3, 4], keepdim=True)
    e = 0.7 * (e * fac) + (1 - 0.7) * e
    r0 = (x - 0.8 * e) / 0.6 * 0.98
    rp = 0.7 * r0 + 0.5 * e + 0.3 * nz
    assert rel_l2(x0.float(), r0) < 1e-6 and rel_l2(xp.float(), rp) < 1e-6
    v_p, v_0 = EmuOps().ddim_step(x, ec, eu, nz, cfg_scale=7.5, guidance_rescale=0.7, **sc)
    assert rel_l2(v_0, r0) > 0.1                                         # and it is not the v step


@pytest.mark.parametrize("tag", ["a_", "m_"])
def test_eps_trajectory_host_logic_vs_reference_golden(emu, tag):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWay
    g = load_golden("ddim_eps_tiny.npz")
    model = pf.tiny_pipeline(parameterization="eps", rescale_betas_zero_snr=False)
    with torch.no_grad():
        out, x0s = pf.run_sampler(model, DDIMSampler if tag == "a_" else ThreeWay, g, tag)
    errs = [rel_l2(p, torch.from_numpy(g[tag + "pred_x0"][i])) for i, p in enumerate(x0s)]
    final = rel_l2(out, torch.from_numpy(g[tag + "samples"]))
    print(f"eps trajectory {tag} (emulated contract) vs reference: pred_x0 per step", [f"{e:.3e}" for e in errs], f"final {final:.3e}")
    assert len(x0s) == 5 and max(errs) < 0.15 and final < 0.15


def test_eps_scalars_come_from_the_ddim_tables():
    """ddim.py:251-258: the eps branch divides by sqrt(ddim_alphas[index]) and multiplies by ddim_sqrt_one_minus_alphas[index];
    the v call carries no `parameterization` keyword (its call path is the one it was)."""
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    model = pf.tiny_pipeline(parameterization="eps", rescale_betas_zero_snr=False)
    s = DDIMSampler(model)
    s.make_schedule(5, ddim_discretize="uniform", ddim_eta=1.0, verbose=False)
    sc = s.step_scalars(2, int(s.ddim_timesteps[2]))
    a = torch.tensor(float(s.ddim_alphas[2]), dtype=torch.float32)
    assert sc["parameterization"] == "eps" and sc["sqrt_ac"] == float(a.sqrt())
    assert sc["sqrt_1m_ac"] == float(torch.tensor(float(s.ddim_sqrt_one_minus_alphas[2]), dtype=torch.float32))
    model.parameterization = "v"
    assert "parameterization" not in s.step_scalars(2, int(s.ddim_timesteps[2]))
    model.parameterization = "x0"
    with pytest.raises(NotImplementedError):
        s.p_sample_ddim(torch.zeros(1, 4, 4, 8, 8), None, torch.tensor([401]), index=2)


# ------------------------------------------------------------------------------------------------ the ABI
def test_ddim_step_eps_is_declared_exported_and_registered():
    assert _lib.TC_ABI_VERSION == 14
    with open(os.path.join(ROOT, "include", "tooncrafter_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define TC_ABI_VERSION 14\b", header)
    decl = re.search(r"int tc_ddim_step_eps\(const TcDdimParams\* p, void\* workspace, int64_t workspace_bytes, void\* stream\);", header)
    assert decl and "additive within ABI 14" in header[header.index("int tc_ddim_step(const"):decl.start()]
    assert _lib.SYMBOLS["tc_ddim_step_eps"] == _lib.SYMBOLS["tc_ddim_step"]
    lib = _lib.load()
    assert lib.tc_abi_version() == 14 and hasattr(lib, "tc_ddim_step_eps")
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    v, e = str(t.ddim_step.default._schema), str(t.ddim_step_eps.default._schema)
    assert e.startswith("tooncrafter::ddim_step_eps(") and e == v.replace("::ddim_step(", "::ddim_step_eps(")
    lat = torch.empty(2, 4, 3, 6, 10, dtype=torch.float32, device="meta")
    xp, x0 = t.ddim_step_eps(lat, lat, lat, lat, None, 7.5, 7.5, 0.7, 0.6, 0.8, 0.7, 0.5, 0.3, 0.98)
    assert xp.shape == lat.shape and x0.shape == lat.shape and xp.dtype == torch.float32 and xp.device.type == "meta"
    with pytest.raises((RuntimeError, NotImplementedError)):            # no CPU kernel: no fallback
        c = torch.zeros(1, 4, 1, 2, 2)
        t.ddim_step_eps(c, c, None, None, None, 1.0, 1.0, 0.0, 0.6, 0.8, 0.7, 0.5, 0.0, 1.0)


def test_ddim_step_eps_argument_checks_need_no_gpu():
    """The entry point validates before it launches: NULL struct, a zero sqrt_ac (zero terminal SNR: eps has no such step)
    and a short workspace come back as error codes."""
    import ctypes as C
    lib = _lib.load()
    assert lib.tc_ddim_step_eps(None, None, 0, None) == -1
    buf = (C.c_float * 16)()
    p = _lib.TcDdimParams()
    p.x = p.e_cond = p.x_prev = C.addressof(buf)
    p.b, p.n = 1, 16
    p.sqrt_ac = 0.0
    assert lib.tc_ddim_step_eps(C.byref(p), C.addressof(buf), 1 << 20, None) == -1
    p.sqrt_ac = 0.5
    assert lib.tc_ddim_step_eps(C.byref(p), None, 0, None) != 0
    for binding in (ops.HipOps.ddim_step,):
        with pytest.raises(NotImplementedError):
            binding(None, None, None, None, None, cfg_scale=1.0, guidance_rescale=0.0, sqrt_ac=1.0, sqrt_1m_ac=0.0,
                    sqrt_a_prev=1.0, dir_coef=0.0, sigma=0.0, x0_rescale=1.0, parameterization="x0")
