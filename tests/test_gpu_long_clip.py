"""Clips longer than 16 frames through the model and the pipeline on the MI355X (the reference's --video_length N,
scripts/evaluation/inference.py:362): every temporal self-attention of the UNet then runs csrc/attention_temporal_long.hip.

Bounds are those of the 16-frame tests: tiny UNet vs emulated contract and vs fp32 oracle 3e-2 (test_gpu_models.py),
full-size UNet vs fp32 oracle rel-L2 2e-2 and cosine 0.9995 (test_gpu_fullsize.py), a CFG-7.5 trajectory 0.15.
"""
import os

import numpy as np
import pytest
import torch

from conftest import TINY_UNET_CFG, rel_l2, sub_state_dict
from emu_ops import EmuOps
from tooncrafter_amd import ops, synth

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


def _tiny_unet(tiny_sd, t):
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    un = UNetModel(**dict(TINY_UNET_CFG, temporal_length=t)).eval()
    un.load_state_dict(sub_state_dict(tiny_sd, "model.diffusion_model."), strict=True)
    return un.to(DEV)


def _tiny_inputs(t, seed):
    """Context 77 text + 256 shared image tokens: what inference.py hands the UNet at --video_length != 16."""
    inp = synth.synth_inputs(1, t, 8, 8, context_dim=TINY_UNET_CFG["context_dim"], n_img_tokens_per_frame=0, seed=seed)
    img = torch.randn(1, 256, TINY_UNET_CFG["context_dim"], generator=torch.Generator().manual_seed(seed + 1))
    inp["cond"] = torch.cat([inp["cond"], img], 1)
    return inp


@pytest.mark.parametrize("t", [24, 32])
def test_tiny_unet_long_clip_vs_contract_and_oracle(hip, tiny_sd, t):
    from oracle import unet as ounet
    un = _tiny_unet(tiny_sd, t)
    inp = _tiny_inputs(t, 40 + t)
    ts = torch.tensor([601])
    args = dict(context=inp["cond"].to(DEV), fs=inp["fs"].to(DEV), x_parts=[inp["x_T"].to(DEV), inp["c_concat"].to(DEV)])
    with torch.no_grad():
        y = _with_backend(hip, lambda: un(None, ts.to(DEV), **args)).cpu()
        un.reset_conditioning()
        y_emu = _with_backend(EmuOps(), lambda: un(None, ts.to(DEV), **args)).cpu()
        ref = ounet.unet_forward(sub_state_dict(tiny_sd, "model.diffusion_model."), dict(TINY_UNET_CFG, temporal_length=t),
                                 torch.cat([inp["x_T"], inp["c_concat"]], 1), ts, inp["cond"], inp["fs"])
    e_emu, e_ref = rel_l2(y, y_emu), rel_l2(y, ref)
    print(f"tiny UNet T = {t}: HIP vs emulated contract {e_emu:.3e}, vs fp32 oracle {e_ref:.3e}")
    assert y.shape == (1, 4, t, 8, 8) and torch.isfinite(y).all()
    assert e_emu <= 3e-2 and e_ref <= 3e-2


def test_tiny_unet_32_frames_hipgraph_replay_matches_eager(hip, tiny_sd):
    un = _tiny_unet(tiny_sd, 32)
    inp = _tiny_inputs(32, 77)
    ts = torch.tensor([339], device=DEV)
    args = dict(context=inp["cond"].to(DEV), fs=inp["fs"].to(DEV), x_parts=[inp["x_T"].to(DEV), inp["c_concat"].to(DEV)])

    def run():
        with torch.no_grad():
            eager = un(None, ts, **args).clone()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                un(None, ts, **args)
            torch.cuda.current_stream().wait_stream(s)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                y = un(None, ts, **args)
            gr.replay()
            torch.cuda.synchronize()
            return eager, y.clone()
    eager, replay = _with_backend(hip, run)
    assert torch.equal(eager, replay)


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm()))


@pytest.mark.timeout(1500)
def test_full_size_unet_32_frames_vs_oracle():
    """320-channel UNet, 32 frames at 40 x 64 latents, context 77 + 256: against the fp32 CPU oracle's output at the
    committed sample positions (tests/golden/long_clip_oracle.npz, tests/golden/make_long_clip_golden.py)."""
    import long_clip_cases as lc
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    if not os.path.exists(lc.GOLDEN_FILE):
        pytest.fail(f"{lc.GOLDEN_FILE} missing: run tests/golden/make_long_clip_golden.py")
    g = dict(np.load(lc.GOLDEN_FILE))
    with torch.device("meta"):
        un = UNetModel(**lc.UNET_CFG)
    un = un.to_empty(device=DEV).eval()
    with torch.no_grad():
        for name, p in un.named_parameters():
            # drawn on the CPU generator: the values the golden was made with (a device generator draws others)
            p.copy_(synth.synth_tensor("model.diffusion_model." + name, tuple(p.shape), 1234, "cpu"))
    inp = lc.inputs()
    with torch.no_grad():
        y = _with_backend(ops.backend(), lambda: un(None, torch.tensor([lc.UNET_T], device=DEV), context=inp["cond"].to(DEV),
                                                    fs=inp["fs"].to(DEV), x_parts=[inp["x_T"].to(DEV), inp["c_concat"].to(DEV)]))
    assert tuple(y.shape) == tuple(g["unet_y_shape"]) and torch.isfinite(y).all()
    flat = y.reshape(-1)
    got = flat[lc.sample_idx(flat.numel(), lc.N_OUT, 3).to(DEV)].cpu()
    ref = torch.from_numpy(g["unet_y"])
    e, c = rel_l2(got, ref), cosine(got, ref)
    nr = float(y.double().norm()) / float(g["unet_y_norm"])
    print(f"full-size UNet T = 32 (B = 1, t = {lc.UNET_T}) HIP vs fp32 CPU oracle: rel-L2 {e:.3e}, cosine {c:.6f}, "
          f"|y| / |ref| {nr:.4f}")
    assert e <= 2e-2 and c >= 0.9995 and abs(nr - 1.0) < 1e-2


def test_tiny_clip_24_frames_pipeline_vs_contract(hip, tiny_sd):
    """Conditions.build -> sample (DDIM-3, CFG 7.5, endpoints held) -> decode_spliced at T = 24 on the HIP kernels and on
    the emulated contract (eta = 0, posterior mean: no draw differs between the two runs).  Measured: latents 9.8e-2,
    decoded clip 1.86e-1."""
    import sys
    from conftest import GOLDEN as GOLDEN_DIR
    from test_gpu_models import _tiny_pipeline
    sys.path.insert(0, GOLDEN_DIR)
    import pipeline_stubs as stubs
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd.lvdm import autoencoder as my_ae
    t = 24
    videos = torch.tanh(torch.randn(1, 3, t, 64, 64, generator=torch.Generator().manual_seed(31))).to(DEV)
    x_T = torch.randn(1, 4, t, 8, 8, generator=torch.Generator().manual_seed(32)).to(DEV)
    plan = pipeline.SamplingPlan(steps=3, eta=0.0, scale=7.5)

    def run(emulated):
        model = _tiny_pipeline(tiny_sd)
        model.embedder = stubs.StubEmbedder()
        model.image_proj_model = stubs.StubImageProj(16)                # 256 image tokens, as at any --video_length
        model.get_learned_conditioning = lambda prompts: stubs.stub_text(prompts, DEV)
        if emulated:
            model.use_hipgraph = False
            model.first_stage_model.decoder.use_hipgraph = False
        old = my_ae.DiagonalGaussianDistribution.sample
        my_ae.DiagonalGaussianDistribution.sample = lambda self, noise=None: self.mean
        try:
            cond = pipeline.Conditions.build(model, videos, fs=10, guided=True, hold_endpoints=True)
            assert cond.positive["c_crossattn"][0].shape[1] == 77 + 256
            lat = pipeline.sample(model, cond, plan, (1, 4, t, 8, 8), x_T=x_T.clone())
            return lat, pipeline.decode_spliced(model, lat, cond.refs)
        finally:
            my_ae.DiagonalGaussianDistribution.sample = old

    with torch.no_grad():
        lat, video = _with_backend(hip, lambda: run(False))
        lat_e, video_e = _with_backend(EmuOps(), lambda: run(True))
    e_lat, e_vid = rel_l2(lat.cpu(), lat_e.cpu()), rel_l2(video.cpu(), video_e.cpu())
    print(f"tiny clip T = {t}, DDIM-3 CFG 7.5: latents HIP vs emulated contract {e_lat:.3e}; decoded video {e_vid:.3e}")
    assert tuple(video.shape) == (1, 3, t, 64, 64) and torch.isfinite(video).all()
    # the trajectory bound of test_gpu_models.py on the latents; the decoded clip under the bound of its pipeline test (0.2:
    # the decoder carries the latents' bf16 noise on, 0.13 of it on the 4-frame clip in the emulated contract already)
    assert e_lat < 0.15 and e_vid < 0.2
