"""Host logic of the module mirror on CPU, with the operator contract emulated in
PyTorch (tests/emu_ops.py).  Checks layouts, weight packing, state-dict mapping and
sampler scalars against the oracle and the reference goldens -- no GPU involved, and
nothing here measures or ships the emulation."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN as GOLDEN_DIR
from conftest import (FULL_DD_CFG, FULL_UNET_CFG, TINY_DD_CFG, TINY_UNET_CFG, load_golden, rel_l2,
                      sub_state_dict)
from emu_ops import EmuOps
from tooncrafter_amd import ops


@pytest.fixture()
def emu_fp32():
    prev = ops.set_backend(EmuOps(round_bf16=True))
    yield
    ops.set_backend(prev)


def _load(module, sd):
    missing, unexpected = module.load_state_dict(sd, strict=True), None
    return module


def test_state_dict_keys_match_reference_full(manifest):
    from tooncrafter_amd.lvdm.autoencoder import AutoencoderKL_Dualref
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    with torch.device("meta"):
        un = UNetModel(**FULL_UNET_CFG)
        ae = AutoencoderKL_Dualref(ddconfig=dict(FULL_DD_CFG), embed_dim=4)
    mine = {"model.diffusion_model." + k: list(v.shape) for k, v in un.named_parameters()}
    mine.update({"first_stage_model." + k: list(v.shape) for k, v in ae.named_parameters()})
    assert mine == manifest["full"]
    assert sum(p.numel() for p in un.parameters()) == 1438854980      # SURVEY 8c structural KATs
    assert sum(p.numel() for p in ae.decoder.parameters()) == 65778223
    assert sum(p.numel() for p in ae.encoder.parameters()) == 34163592


def test_unet_tiny_host_logic(tiny_sd, emu_fp32):
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    g = load_golden("unet_tiny.npz")
    un = UNetModel(**TINY_UNET_CFG).eval()
    un.load_state_dict(sub_state_dict(tiny_sd, "model.diffusion_model."), strict=True)
    with torch.no_grad():
        y = un(torch.from_numpy(g["x"]), torch.from_numpy(g["timesteps"]), context=torch.from_numpy(g["context"]),
               fs=torch.from_numpy(g["fs"]))
    ref = torch.from_numpy(g["y"])
    assert y.shape == ref.shape
    err = rel_l2(y, ref)
    assert err < 3e-2, err       # bf16 storage between operators, fp32 math inside


def test_decoder_tiny_host_logic(tiny_sd, emu_fp32):
    from tooncrafter_amd.lvdm.autoencoder_dualref import VideoDecoder
    g = load_golden("decoder_tiny.npz")
    vd = VideoDecoder(**TINY_DD_CFG).eval()
    vd.load_state_dict(sub_state_dict(tiny_sd, "first_stage_model.decoder."), strict=True)
    refs = [torch.from_numpy(g[f"ref{i}"]) for i in range(5)]
    with torch.no_grad():
        out = vd.decode_clip(torch.from_numpy(g["z"]), refs, scale=1.0 / 0.18215)
    ref = torch.from_numpy(g["dec_first_stage"])
    assert out.shape == ref.shape
    err = rel_l2(out, ref)
    assert err < 2e-2, err


def test_decoder_batch_of_clips_matches_single_clips(tiny_sd):
    """SURVEY.md 8d config 4 (`perframe_ae=False` geometry): a batch of B clips goes through ONE decoder call
    with timesteps=T -- the only geometry in which the dual-reference fusion (`k[:, [0]*(bt//b)]`,
    autoencoder_dualref.py:282-292) sees each clip's own reference frames.  The result must equal decoding
    every clip on its own (all normalisations and attentions are per clip)."""
    from tooncrafter_amd.lvdm.autoencoder_dualref import VideoDecoder
    prev = ops.set_backend(EmuOps(round_bf16=False))       # exact-arithmetic contract: isolates the host logic
    try:
        _check_decoder_batch(tiny_sd, VideoDecoder)
    finally:
        ops.set_backend(prev)


def _check_decoder_batch(tiny_sd, VideoDecoder):
    vd = VideoDecoder(**TINY_DD_CFG).eval()
    vd.load_state_dict(sub_state_dict(tiny_sd, "first_stage_model.decoder."), strict=True)
    g = torch.Generator().manual_seed(77)
    z = torch.randn(2, 4, 3, 4, 6, generator=g)
    from tooncrafter_amd import synth
    refs = [torch.cat([a, b]) for a, b in zip(synth.synth_ref_context(1, 4, 6, ch=64, seed=11),
                                              synth.synth_ref_context(1, 4, 6, ch=64, seed=12))]
    with torch.no_grad():
        both = vd.decode_clip(z, refs, scale=1.0 / 0.18215)
        singles = [vd.decode_clip(z[i:i + 1], [r[i:i + 1] for r in refs], scale=1.0 / 0.18215) for i in range(2)]
    assert both.shape == (2, 3, 3, 32, 48)
    for i in range(2):
        assert rel_l2(both[i:i + 1], singles[i]) < 1e-4, (i, rel_l2(both[i:i + 1], singles[i]))
    assert rel_l2(both[0:1], singles[1]) > 0.1          # and the clips really differ


def _tiny_model_cfg():
    return dict(
        rescale_betas_zero_snr=True, parameterization="v", linear_start=0.00085, linear_end=0.012,
        num_timesteps_cond=1, timesteps=1000, first_stage_key="video", cond_stage_key="caption",
        cond_stage_trainable=False, conditioning_key="hybrid", image_size=[8, 8], channels=4, scale_by_std=False,
        scale_factor=0.18215, use_ema=False, uncond_type="empty_seq", use_dynamic_rescale=True, base_scale=0.7,
        fps_condition_type="fps", perframe_ae=True, loop_video=True,
        unet_config=dict(target="lvdm.modules.networks.openaimodel3d.UNetModel", params=dict(TINY_UNET_CFG)),
        first_stage_config=dict(target="lvdm.models.autoencoder.AutoencoderKL_Dualref",
                                params=dict(embed_dim=4, monitor="val/rec_loss", ddconfig=dict(TINY_DD_CFG),
                                            lossconfig=dict(target="torch.nn.Identity"))),
        cond_stage_config=dict(target="torch.nn.Identity"),
        img_cond_stage_config=dict(target="torch.nn.Identity"),
        image_proj_stage_config=dict(target="torch.nn.Identity"))


def test_ddim_tiny_trajectory_host_logic(tiny_sd, emu_fp32):
    """Full pipeline mirror: LatentVisualDiffusion + DDIMSampler (batched CFG, fused step, host
    scalars) against the reference's 5-step trajectory."""
    from tooncrafter_amd.lvdm import ddim as my_ddim
    from tooncrafter_amd.utils import instantiate_from_config
    g = load_golden("ddim_tiny.npz")
    model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    missing, unexpected = model.load_state_dict(tiny_sd, strict=False)     # every reference parameter has a home
    assert not unexpected
    assert all(m in dict(model.named_buffers()) for m in missing), missing   # only the schedule buffers
    # schedule buffers equal the reference's, bit for bit
    gs = load_golden("schedule.npz")
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
              "sqrt_one_minus_alphas_cumprod", "scale_arr"):
        assert np.array_equal(getattr(model, k).numpy(), gs[k]), k
    noises = torch.from_numpy(g["noises"])
    it = iter(noises)
    my_ddim.noise_like = lambda shape, device, repeat=False: next(it)
    sampler = my_ddim.DDIMSampler(model)
    cond = {"c_crossattn": [torch.from_numpy(g["cond"])], "c_concat": [torch.from_numpy(g["c_concat"])]}
    uc = {"c_crossattn": [torch.from_numpy(g["uncond"])], "c_concat": [torch.from_numpy(g["c_concat"])]}
    x0s = []
    samples, _ = sampler.sample(S=5, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False,
                                unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0,
                                cfg_img=None, mask=None, x0=None, fs=torch.from_numpy(g["fs"]),
                                timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                                x_T=torch.from_numpy(g["x_T"]), unconditional_conditioning_img_nonetext=None,
                                img_callback=lambda p, i: x0s.append(p.clone()))
    errs = [rel_l2(p, torch.from_numpy(g["pred_x0"][i])) for i, p in enumerate(x0s)]
    final = rel_l2(samples, torch.from_numpy(g["samples"]))
    # CFG 7.5 amplifies the bf16 noise of the two UNet passes by sqrt(7.5^2 + 6.5^2) ~ 10x relative to
    # their difference: the trajectory bound is that amplified floor, not a per-forward bound
    assert max(errs) < 0.15 and final < 0.15, (errs, final)
    # sampler tables equal the reference's
    assert np.array_equal(sampler.ddim_sigmas, gs["s5_trailing_sigmas"])
    assert np.array_equal(sampler.ddim_alphas_prev, gs["s5_trailing_alphas_prev"])


def test_ddim_multicond_trajectory_host_logic(tiny_sd, emu_fp32):
    """Row f3: the mirror of samplers/ddim_multiplecond.py (three UNet passes as one batch-3 call,
    three-way guidance inside the fused step) against the reference's 4-step trajectory."""
    from tooncrafter_amd.lvdm import ddim as my_ddim
    from tooncrafter_amd.utils import get_obj_from_str, instantiate_from_config
    g = load_golden("ddim_mc_tiny.npz")
    model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    model.load_state_dict(tiny_sd, strict=False)
    it = iter(torch.from_numpy(g["noises"]))
    old = my_ddim.noise_like
    my_ddim.noise_like = lambda shape, device, repeat=False: next(it)
    try:
        sampler = get_obj_from_str("lvdm.models.samplers.ddim_multiplecond.DDIMSampler")(model)
        t = lambda k: torch.from_numpy(g[k])
        cond = {"c_crossattn": [t("cond")], "c_concat": [t("c_concat")]}
        uc = {"c_crossattn": [t("uncond")], "c_concat": [t("c_concat")]}
        uc_img = {"c_crossattn": [t("uncond_img")], "c_concat": [t("c_concat")]}
        x0s = []
        samples, _ = sampler.sample(S=4, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False,
                                    unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0,
                                    cfg_img=float(g["cfg_img"]), mask=None, x0=None, fs=t("fs"),
                                    timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=t("x_T"),
                                    unconditional_conditioning_img_nonetext=uc_img,
                                    img_callback=lambda p, i: x0s.append(p.clone()))
    finally:
        my_ddim.noise_like = old
    errs = [rel_l2(p, torch.from_numpy(g["pred_x0"][i])) for i, p in enumerate(x0s)]
    final = rel_l2(samples, torch.from_numpy(g["samples"]))
    assert max(errs) < 0.15 and final < 0.15, (errs, final)
    # the third condition is mandatory, like in the reference (KeyError at ddim_multiplecond.py:220)
    import pytest
    with pytest.raises(KeyError):
        sampler.p_sample_ddim(t("x_T"), cond, torch.tensor([999]), index=3, unconditional_guidance_scale=7.5,
                              unconditional_conditioning=uc, fs=t("fs"))


def test_output_path_host_logic(emu_fp32, tmp_path):
    """Row f4: save_results_seperate mirror -- file naming of inference.py:152, `loop` drops the last frame,
    bytes equal to the reference's clamp/scale/uint8/permute."""
    from tooncrafter_amd import output
    g = torch.Generator().manual_seed(3)
    samples = torch.randn(2, 3, 4, 8, 12, generator=g)
    fakedir = str(tmp_path / "samples")
    seen = []
    written = output.save_results_seperate(["a prompt"], samples, "clip_007.png", fakedir, fps=8, loop=True,
                                           writer=lambda path, fr, fps: (seen.append((path, fr.clone(), fps)), path)[1])
    assert [os.path.basename(w) for w in written] == ["clip_007_sample0.mp4", "clip_007_sample1.mp4"]
    assert all(os.path.dirname(w).endswith("samples_separate") for w in written)
    ref = torch.clamp(samples[:, :, :-1].float(), -1., 1.)
    for i, (path, fr, fps) in enumerate(seen):
        want = (((ref[i] + 1.0) / 2.0) * 255).to(torch.uint8).permute(1, 2, 3, 0)
        assert fps == 8 and fr.dtype == torch.uint8 and torch.equal(fr, want)
    # without an encoder library in the image the default writer produces the .mp4 itself (tooncrafter_amd/mp4.py)
    out = output.save_results_seperate("p", samples[:1], "x.mp4", fakedir)
    if out[0].endswith(".mp4") and os.path.exists(out[0]):
        from test_mp4_cpu import _decode
        clip = _decode(out[0])
        assert (clip["w"], clip["h"], len(clip["frames"])) == (12, 8, 4)
    assert output.save_results_seperate("p", None, "x.mp4", fakedir) == []


def test_resampler_host_logic(emu_fp32):
    """Row f2: the Resampler mirror resolves under the reference's dotted path, carries the reference's
    parameter names and shapes (full inference_512_v1.0.yaml configuration) and reproduces the reference's
    tiny forward through the operator contract."""
    from conftest import GOLDEN as GOLDEN_DIR
    from tooncrafter_amd import synth
    from tooncrafter_amd.utils import instantiate_from_config
    man = json.load(open(os.path.join(GOLDEN_DIR, "resampler_manifest.json")))
    with torch.device("meta"):
        full = instantiate_from_config(dict(target="lvdm.modules.encoders.resampler.Resampler", params=man["full_cfg"]))
    assert type(full).__module__ == "tooncrafter_amd.lvdm.resampler"
    assert {k: list(v.shape) for k, v in full.state_dict().items()} == man["full"]
    tiny = instantiate_from_config(dict(target="lvdm.modules.encoders.resampler.Resampler", params=man["tiny_cfg"])).eval()
    assert {k: list(v.shape) for k, v in tiny.state_dict().items()} == man["tiny"]
    synth.fill_module_(tiny, prefix="image_proj_model.", seed=1234)
    g = load_golden("resampler_tiny.npz")
    with torch.no_grad():
        y = tiny(torch.from_numpy(g["x"]))
    assert y.shape == g["y"].shape and y.dtype == torch.float32
    assert rel_l2(y, torch.from_numpy(g["y"])) < 2e-2, rel_l2(y, torch.from_numpy(g["y"]))


def test_image_proj_model_host_logic(emu_fp32):
    """ImageProjModel (resampler.py:9-23) mirror against the reference class (tests/golden/resampler_tiny.npz)."""
    from tooncrafter_amd import synth
    from tooncrafter_amd.lvdm.resampler import ImageProjModel
    g = load_golden("resampler_tiny.npz")
    ip = ImageProjModel(cross_attention_dim=64, clip_embeddings_dim=96, clip_extra_context_tokens=4).eval()
    assert set(ip.state_dict()) == {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
    synth.fill_module_(ip, prefix="image_proj_model.", seed=1234)
    with torch.no_grad():
        y = ip(torch.from_numpy(g["proj_x"]))
    assert y.shape == g["proj_y"].shape == (3, 4, 64)
    assert rel_l2(y, torch.from_numpy(g["proj_y"])) < 1e-2


def _tiny_towers():
    from tooncrafter_amd import synth
    from tooncrafter_amd.lvdm.openclip import CLIPText, VisionTransformer
    vis = VisionTransformer(width=160, layers=2, heads=2, patch=14, image=42, mlp=320, output_dim=64).eval()   # head dim 80
    txt = CLIPText(embed_dim=64, width=128, layers=3, heads=2, context=7, vocab=50, mlp=256).eval()            # head dim 64
    synth.fill_module_(vis, prefix="embedder.model.visual.", seed=1234)
    synth.fill_module_(txt, prefix="cond_stage_model.model.", seed=1234)
    return vis, txt


def test_openclip_towers_host_logic():
    """Row f2 (oracle/openclip.py itself is pinned to transformers, tests/test_openclip_golden_cpu.py): the tower mirrors against it through the
    exact-arithmetic operator contract -- patch GEMM + positional residual, class token, fused q|k projection,
    V^T by operand swap, head-dim-80 attention as GEMM/softmax/GEMM with K padding, V-bias folded into out_proj,
    causal text mask, penultimate layer."""
    from oracle import openclip as oclip
    prev = ops.set_backend(EmuOps(round_bf16=False))
    try:
        vis, txt = _tiny_towers()
        g = torch.Generator().manual_seed(9)
        img = torch.randn(2, 3, 42, 42, generator=g)
        tok = torch.randint(0, 50, (2, 7), generator=g)
        with torch.no_grad():
            yv, yt = vis.tokens(img), txt.tokens(tok, skip_last=1)
        sdv = {k: v.detach() for k, v in vis.state_dict().items()}
        sdt = {k: v.detach() for k, v in txt.state_dict().items()}
        rv, rt = oclip.vision_tokens(sdv, img, heads=2), oclip.text_tokens(sdt, tok, heads=2, skip_last=1)
        assert yv.shape == rv.shape == (2, 10, 160) and yt.shape == rt.shape == (2, 7, 128)
        # bf16-rounded weights are the only difference left (packers round, the contract here does not)
        assert rel_l2(yv, rv) < 1e-2 and rel_l2(yt, rt) < 1e-2, (rel_l2(yv, rv), rel_l2(yt, rt))
        # 'last' differs from 'penultimate', and dropping the causal mask would show
        assert rel_l2(txt.tokens(tok, skip_last=0), rt) > 5e-2
        sd_nomask = oclip.resblock
        x0 = sdt["token_embedding.weight"][tok] + sdt["positional_embedding"]
        assert rel_l2(oclip.resblock(sdt, "transformer.resblocks.0.", x0, 2, None),
                      oclip.resblock(sdt, "transformer.resblocks.0.", x0, 2, torch.full((7, 7), float("-inf")).triu_(1))) > 1e-2
    finally:
        ops.set_backend(prev)


def test_openclip_conditioners_resolve_and_carry_open_clip_names():
    from tooncrafter_amd.utils import instantiate_from_config
    with torch.device("meta"):
        t = instantiate_from_config(dict(target="lvdm.modules.encoders.condition.FrozenOpenCLIPEmbedder",
                                         params=dict(freeze=True, layer="penultimate")))
        v = instantiate_from_config(dict(target="lvdm.modules.encoders.condition.FrozenOpenCLIPImageEmbedderV2",
                                         params=dict(freeze=True)))
    kt, kv = set(t.state_dict()), set(v.state_dict())
    assert {"model.token_embedding.weight", "model.positional_embedding", "model.ln_final.weight",
            "model.transformer.resblocks.23.attn.in_proj_weight", "model.transformer.resblocks.0.mlp.c_fc.weight",
            "model.text_projection", "model.logit_scale"} <= kt
    assert {"model.visual.conv1.weight", "model.visual.class_embedding", "model.visual.positional_embedding",
            "model.visual.ln_pre.weight", "model.visual.transformer.resblocks.31.attn.out_proj.bias",
            "model.visual.transformer.resblocks.0.mlp.c_proj.weight", "model.visual.ln_post.weight",
            "model.visual.proj"} <= kv
    assert sum(p.numel() for p in t.parameters()) == 354_032_641          # ViT-H/14 text tower
    assert sum(p.numel() for p in v.model.visual.parameters()) == 632_076_800   # ViT-H/14 vision tower
    # the reference deletes only `model.transformer`: the rest of CLIP's text half stays in the module, hence in every
    # checkpoint -- dead weights that load_state_dict(strict=True) (inference.py:32,44) must find a home for
    assert {"model.positional_embedding", "model.text_projection", "model.logit_scale", "model.token_embedding.weight",
            "model.ln_final.weight", "model.ln_final.bias"} <= set(v.state_dict())
    assert "model.attn_mask" not in v.state_dict() and not any(k.startswith("model.transformer.") for k in v.state_dict())
    assert tuple(v.state_dict()["model.visual.positional_embedding"].shape) == (257, 1280)
    import pytest
    with pytest.raises(RuntimeError):
        t.tokenize(["a prompt"])                                          # no BPE vocabulary in this image
    tok = t.tokenize(["", ""])                                            # the scripts' default prompt needs none
    assert tok.shape == (2, 77) and tok[0, :3].tolist() == [49406, 49407, 0] and int(tok.sum()) == 2 * (49406 + 49407)


def test_pipeline_matches_reference_image_guided_synthesis(tiny_sd):
    """The caller row: tooncrafter_amd.clip.image_guided_synthesis (the adapter onto Conditions.build -> sample -> decode_spliced) against the reference's own function
    (scripts/evaluation/inference.py:180-277) run on the tiny model with the shared deterministic conditioner
    stand-ins -- conditioning assembly, first/last-frame encode (2 frames instead of T), c_concat, uncond branch,
    sampler call, both decodes and the centre-frame splice."""
    import sys
    sys.path.insert(0, GOLDEN_DIR)
    import pipeline_stubs as stubs
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd.lvdm import autoencoder as my_ae, ddim as my_ddim
    from tooncrafter_amd.utils import instantiate_from_config
    g = load_golden("pipeline_tiny.npz")
    # exact-arithmetic operator contract (bf16 weights only): a 3-step CFG-7.5 trajectory amplifies bf16
    # activation noise to ~0.13 (measured), which would hide an orchestration error; this way the bound is tight
    prev = ops.set_backend(EmuOps(round_bf16=False))
    try:
        _check_pipeline(tiny_sd, g, stubs, pipeline, my_ae, my_ddim, instantiate_from_config)
    finally:
        ops.set_backend(prev)


def _check_pipeline(tiny_sd, g, stubs, pipeline, my_ae, my_ddim, instantiate_from_config):
    model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    model.load_state_dict(tiny_sd, strict=False)
    model.embedder = stubs.StubEmbedder()
    model.image_proj_model = stubs.StubImageProj(4)
    model.get_learned_conditioning = lambda prompts: stubs.stub_text(prompts)
    videos = torch.from_numpy(g["videos"])
    it = iter(torch.from_numpy(g["noises"]))
    old_noise, old_sample = my_ddim.noise_like, my_ae.DiagonalGaussianDistribution.sample
    my_ddim.noise_like = lambda shape, device, repeat=False: next(it)
    my_ae.DiagonalGaussianDistribution.sample = lambda self, noise=None: self.mean        # as patched in the golden run
    try:
        with torch.no_grad():
            z, hs = pipeline.get_latent_z_with_hidden_states(model, videos)
            torch.manual_seed(2024)                                                       # x_T, as in the golden run
            out = pipeline.image_guided_synthesis(model, ["ignored"], videos, [1, 4, 4, 8, 8], n_samples=1,
                                                  ddim_steps=3, ddim_eta=1.0, unconditional_guidance_scale=7.5,
                                                  cfg_img=None, fs=10, text_input=False, multiple_cond_cfg=False,
                                                  loop=False, interp=True, timestep_spacing="uniform_trailing",
                                                  guidance_rescale=0.7)
    finally:
        my_ddim.noise_like, my_ae.DiagonalGaussianDistribution.sample = old_noise, old_sample
    # latents of the two frames the reference keeps, and the first/last hidden states
    zr = torch.from_numpy(g["z"])
    assert z.shape == zr.shape
    assert rel_l2(z[:, :, [0, -1]], zr[:, :, [0, -1]]) < 2e-2 and float(z[:, :, 1:-1].abs().max()) == 0.0
    assert [list(h.shape) for h in hs] == g["hs_shapes"].tolist()
    for i, h in enumerate(hs):
        assert rel_l2(h[:, ::4, :, ::4, ::4], torch.from_numpy(g[f"hs{i}"])) < 2e-2, i
    ref = torch.from_numpy(g["out"])
    assert out.shape == ref.shape == (1, 1, 3, 4, 64, 64)
    err = rel_l2(out, ref)
    assert err < 3e-2, err


def test_step_scalars_first_step_is_finite():
    """Zero-terminal-SNR: at index S-1 the radicand 1 - a_prev - sigma^2 must be the tiny positive
    fp32 value the reference gets (+5.96e-8), not a negative one (NaN)."""
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddpm3d import DDPM
    gs = load_golden("schedule.npz")

    class M(torch.nn.Module):
        pass
    m = M()
    m.rescale_betas_zero_snr, m.parameterization, m.v_posterior = True, "v", 0.0
    DDPM.register_schedule(m, beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.012)
    m.use_dynamic_rescale = True
    m.scale_arr = torch.from_numpy(gs["scale_arr"])
    m.device = torch.device("cpu")
    s = DDIMSampler(m)
    s.make_schedule(50, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    sc = s.step_scalars(49, 999)
    assert abs(sc["dir_coef"] ** 2 - float(gs["s50_trailing_radicand_f32"][49])) < 1e-12
    assert sc["dir_coef"] > 0 and np.isfinite(sc["dir_coef"])
    for i in range(50):
        r = float(gs["s50_trailing_radicand_f32"][i])
        assert abs(s.step_scalars(i, int(s.ddim_timesteps[i]))["dir_coef"] - np.sqrt(np.float32(r))) < 1e-7


def test_encoder_tiny_host_logic(tiny_sd, emu_fp32):
    """Row f1: AutoencoderKL_Dualref.encode (Encoder + fused quant_conv + posterior) vs the reference."""
    from tooncrafter_amd.lvdm.autoencoder import AutoencoderKL_Dualref
    g = load_golden("encoder_tiny.npz")
    ae = AutoencoderKL_Dualref(ddconfig=dict(TINY_DD_CFG), embed_dim=4).eval()
    missing, unexpected = ae.load_state_dict(sub_state_dict(tiny_sd, "first_stage_model."), strict=True), None
    with torch.no_grad():
        post, hidden = ae.encode(torch.from_numpy(g["frames"]), return_hidden_states=True)
        z = 0.18215 * post.sample(noise=torch.from_numpy(g["noise"]))
    assert rel_l2(post.mean, torch.from_numpy(g["mean"])) < 3e-2
    assert rel_l2(z, torch.from_numpy(g["z"])) < 3e-2
    assert len(hidden) == 5
    for i, h in enumerate(hidden):
        ref = torch.from_numpy(g[f"hid{i}"])
        assert h.shape == ref.shape
        assert rel_l2(h, ref) < 3e-2, i


def test_conv_halo_model_design_artifact():
    """scripts/conv_halo_model.py (the data movement planned for the tap-reuse 3x3 convolution, docs/LAB_NOTEBOOK.md section 8):
    exact against a direct convolution on a ragged image, and bank-conflict-free for every tap."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "conv_halo_model.py")
    spec = importlib.util.spec_from_file_location("conv_halo_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    err, worst = mod.check(frames=1, H=9, W=35, C=64, N=8)
    assert err < 1e-12 and worst == 0


# ---------------------------------------------------------------- the clip pipeline's host rules: timeline plan, writer rule

def test_timeline_segments_on_hand_written_labels():
    from tooncrafter_amd.clip import timeline_segments as seg
    tw, cut, hold = "tween", "cut", "hold"
    # all tween: the batches are the segments in order, cut into chunks
    assert seg((tw,) * 5, 5, 1) == ([], [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)])
    assert seg((tw,) * 5, 5, 2) == ([], [(0, 2), (2, 2), (4, 1)])
    assert seg((tw,) * 5, 5, 8) == ([], [(0, 5)])
    # a held segment at the start, in the middle, at the end
    assert seg((hold, tw, tw, tw), 4, 2) == ([0], [(1, 2), (3, 1)])
    assert seg((tw, tw, cut, tw), 4, 4) == ([2], [(0, 2), (3, 1)])
    assert seg((tw, tw, tw, hold), 4, 2) == ([3], [(0, 2), (2, 1)])
    # two runs with a hold between them, batch 2: three batches, none across the hold, although (2, 3) and (4, 5) would pair up
    assert seg((tw, tw, tw, hold, tw, tw), 6, 2) == ([3], [(0, 2), (2, 1), (4, 2)])
    assert seg((tw, hold, tw), 3, 2) == ([1], [(0, 1), (2, 1)])
    # nothing to sample
    assert seg((cut, hold, hold), 3, 2) == ([0, 1, 2], [])
    for bad in (((tw, tw), 3, 1), ((tw, "fade", tw), 3, 1), ((tw,), 1, 0)):
        with pytest.raises(ValueError):
            seg(*bad)


def test_timeline_segments_without_labels_are_timeline_layouts_batches():
    from tooncrafter_amd import clip
    for k in range(2, 7):
        for batch in range(1, 4):
            assert clip.timeline_segments(None, k - 1, batch) == ([], clip.timeline_layout(k, 4, batch, (4, 6), "rgb24")[2]), (k, batch)


def test_write_frames_picks_the_op_by_one_rule():
    """size x fmt x colour x out: the op and the arguments are those `clip_to_uint8` (out None: frames = (0, t), or the clip alone
    to video_to_uint8) and the timeline (a buffer: frames, out, strides) passed; the product's own request check stands in front
    of the recording, so rgb24 with a colour raises what ops.frames_to_yuv raises, through either entry point."""
    from tooncrafter_amd import output
    from tooncrafter_amd._lib import TooncrafterHipError
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.output import Colour

    class Recorder(HipOps):
        calls = []

        @staticmethod
        def checked(check, *request):
            try:
                check(*request)
            except TooncrafterHipError:                   # the CPU tensor, refused last: after the request checks, which raise ValueError
                pass

        def video_to_uint8(self, video):
            self.calls.append(("video_to_uint8", tuple(video.shape)))

        def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
            self.checked(self._frames_out_args, x, size, filter, fmt, frames)
            self.calls.append(("frames_to_u8", tuple(x.shape), size, filter, fmt, frames, out if out is None else out.data_ptr(), strides))

        def frames_to_yuv(self, x, size=None, filter="bicubic", fmt="nv12", colour=None, frames=None, out=None, strides=None):
            self.checked(self._frames_yuv_out_args, x, size, filter, fmt, colour, frames)
            self.calls.append(("frames_to_yuv", tuple(x.shape), size, filter, fmt, colour, frames, out if out is None else out.data_ptr(),
                               strides))
    spy, calls = Recorder(), Recorder.calls
    x, t, c = torch.zeros(2, 3, 4, 20, 32), 4, Colour()
    buf = torch.zeros(2 * 4 * 40 * 64 * 3, dtype=torch.uint8)
    prev = ops.set_backend(spy)
    try:
        for size in (None, (40, 64)):
            for fmt in ("rgb24", "i420", "nv12"):
                for colour in (None, c):
                    for out in (None, buf):
                        oh, ow = size or (20, 32)
                        frame = oh * ow * 3 if fmt == "rgb24" else oh * ow * 3 // 2
                        strides = (3 * ow if fmt == "rgb24" else ow, frame, (t - 1) * frame)
                        how = dict(size=size, filter="box", fmt=fmt, colour=colour)
                        request = dict(frames=(0, t)) if out is None else dict(frames=(1, t - 1), out=out[frame:], strides=strides)
                        plain = size is None and fmt == "rgb24" and colour is None and out is None
                        calls.clear()
                        if colour is not None and fmt == "rgb24":
                            with pytest.raises(ValueError):
                                output.write_frames(x, **how, **request)
                            with pytest.raises(ValueError):
                                output.clip_to_uint8(x, **how)
                            assert not calls
                            continue
                        output.write_frames(x, filter="box") if plain else output.write_frames(x, **how, **request)
                        tail = (None, None) if out is None else (buf.data_ptr() + frame, strides)
                        if colour is not None:
                            want = ("frames_to_yuv", (2, 3, 4, 20, 32), size, "box", fmt, c, request["frames"], *tail)
                        elif plain:
                            want = ("video_to_uint8", (2, 3, 4, 20, 32))
                        else:
                            want = ("frames_to_u8", (2, 3, 4, 20, 32), size, "box", fmt, request["frames"], *tail)
                        assert calls == [want], (size, fmt, colour, out is not None)
                        if out is None:                                           # clip_to_uint8 is this rule plus `loop`
                            output.clip_to_uint8(x, **how)
                            assert calls == [want, want]
        # frames alone take the clip off the whole-clip op; `loop` is a slice there and a frame count elsewhere
        calls.clear()
        output.write_frames(x, frames=(0, 3))
        output.clip_to_uint8(x, True)
        output.clip_to_uint8(x, True, fmt="nv12", colour=c)
        assert calls == [("frames_to_u8", (2, 3, 4, 20, 32), None, "bicubic", "rgb24", (0, 3), None, None), ("video_to_uint8", (2, 3, 3, 20, 32)),
                         ("frames_to_yuv", (2, 3, 4, 20, 32), None, "bicubic", "nv12", c, (0, 3), None, None)]
        for bad in ("bt709", (1, 2)):
            with pytest.raises(ValueError):
                output.write_frames(x, fmt="nv12", colour=bad)
    finally:
        ops.set_backend(prev)
