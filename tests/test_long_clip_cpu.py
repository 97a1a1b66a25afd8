"""Clips of up to TC_TEMPORAL_MAX_FRAMES = 64 frames (the reference's --video_length N, scripts/evaluation/inference.py:362)
without a GPU: the model accepts the length, refuses a longer one before anything runs, the emulated contract of the
mirror matches the fp32 oracle at T = 24 with the reference's shared-image-token context (openaimodel3d.py:556-562),
and the long-clip kernel source compiles for gfx950 without scratch."""
import os
import re
import subprocess

import pytest
import torch

from conftest import FULL_UNET_CFG, ROOT, TINY_UNET_CFG, rel_l2, sub_state_dict
from emu_ops import EmuOps
from tooncrafter_amd import _lib, ops, synth
from tooncrafter_amd.lvdm.attention import ContextCache, TemporalTransformer, check_frames
from tooncrafter_amd.lvdm.openaimodel3d import UNetModel

CSRC = os.path.join(ROOT, "tooncrafter_amd", "csrc")


@pytest.mark.parametrize("t", [32, 64])
def test_temporal_transformer_and_full_unet_construct(t):
    tt = TemporalTransformer(320, 5, 64, temporal_length=t)
    assert len(tt.transformer_blocks) == 1
    with torch.device("meta"):
        un = UNetModel(**dict(FULL_UNET_CFG, temporal_length=t))
    assert un.temporal_length == t


def test_65_frames_raise():
    with pytest.raises(ValueError, match="TC_TEMPORAL_MAX_FRAMES = 64"):
        TemporalTransformer(320, 5, 64, temporal_length=65)
    with pytest.raises(ValueError, match="64"):
        with torch.device("meta"):
            UNetModel(**dict(FULL_UNET_CFG, temporal_length=65))
    check_frames(64)
    with pytest.raises(ValueError, match="64"):
        check_frames(65)


class _NoLaunch:
    """A backend that fails the test on any operator call: the frame-count check must come first."""
    def __getattr__(self, name):
        raise AssertionError(f"operator {name} reached with a 65-frame clip")


def test_unet_forward_65_frames_raises_before_any_operator(tiny_sd):
    un = UNetModel(**TINY_UNET_CFG).eval()
    un.load_state_dict(sub_state_dict(tiny_sd, "model.diffusion_model."), strict=True)
    inp = synth.synth_inputs(1, 65, 2, 2, context_dim=TINY_UNET_CFG["context_dim"], n_img_tokens_per_frame=0, seed=1)
    prev = ops.set_backend(_NoLaunch())
    try:
        with pytest.raises(ValueError, match="TC_TEMPORAL_MAX_FRAMES"):
            un(None, torch.tensor([5]), context=inp["cond"], fs=inp["fs"], x_parts=[inp["x_T"], inp["c_concat"]])
    finally:
        ops.set_backend(prev)


def test_sampler_entry_65_frames_raises():
    from tooncrafter_amd.clip import Conditions, SamplingPlan, sample
    with pytest.raises(ValueError, match="TC_TEMPORAL_MAX_FRAMES"):
        sample(object(), Conditions.__new__(Conditions), SamplingPlan(), (1, 4, 65, 8, 8))


def test_header_constant_matches_binding():
    with open(os.path.join(ROOT, "include", "tooncrafter_hip.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define TC_TEMPORAL_MAX_FRAMES (\d+)", hdr).group(1)) == _lib.TC_TEMPORAL_MAX_FRAMES == 64
    assert int(re.search(r"#define TC_ABI_VERSION (\d+)", hdr).group(1)) == _lib.TC_ABI_VERSION
    assert _lib.load().tc_abi_version() == _lib.TC_ABI_VERSION


def test_shared_image_token_route_at_24_frames():
    """inference.py's image projection yields 256 tokens whatever N is: at T = 24 the context is 77 + 256, not
    77 + 16 * 24, and every frame reads the same 256 image tokens (openaimodel3d.py:556-562)."""
    ctx = torch.randn(2, 77 + 256, 96)
    c = ContextCache(ctx, 24)
    assert not c.img_per_frame and c.img_len == 256 and c.text_len == 77
    assert c.img_rows.shape == (2 * 256, 96)
    c16 = ContextCache(torch.randn(1, 77 + 16 * 24, 96), 24)            # 77 + 16 T: the per-frame split
    assert c16.img_per_frame and c16.img_len == 16


def test_emulated_tiny_unet_24_frames_matches_oracle(tiny_sd):
    from oracle import unet as ounet
    cfg = dict(TINY_UNET_CFG, temporal_length=24)
    un = UNetModel(**cfg).eval()
    sd = sub_state_dict(tiny_sd, "model.diffusion_model.")
    un.load_state_dict(sd, strict=True)
    inp = synth.synth_inputs(1, 24, 8, 8, context_dim=cfg["context_dim"], n_img_tokens_per_frame=0, seed=21)
    ctx = torch.cat([inp["cond"], torch.randn(1, 256, cfg["context_dim"], generator=torch.Generator().manual_seed(22))], 1)
    assert ctx.shape[1] == 77 + 256
    ts = torch.tensor([601])
    prev = ops.set_backend(EmuOps())
    try:
        with torch.no_grad():
            y = un(None, ts, context=ctx, fs=inp["fs"], x_parts=[inp["x_T"], inp["c_concat"]])
    finally:
        ops.set_backend(prev)
    with torch.no_grad():
        ref = ounet.unet_forward({k: v.float() for k, v in sd.items()}, cfg, torch.cat([inp["x_T"], inp["c_concat"]], 1),
                                 ts, ctx, inp["fs"])
    e = rel_l2(y, ref)
    print(f"tiny UNet T = 24, context 77 + 256: emulated contract vs fp32 oracle rel-L2 {e:.3e}")
    assert y.shape == ref.shape == (1, 4, 24, 8, 8) and torch.isfinite(y).all()
    assert e < 3e-2


def _hipcc():
    from tooncrafter_amd import build
    try:
        return build._hipcc()
    except RuntimeError:
        return None


def test_long_temporal_kernels_do_not_spill(tmp_path):
    """csrc/attention_temporal_long.hip, both padded lengths (TT = 32, 64), and csrc/attention_temporal_rel.hip, its four
    instances, with the per-source flags of build.py: no scratch, and the MFMA / permlane structure the design rests on is
    in the code."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not on this host")
    from tooncrafter_amd import build
    out = tmp_path / "attention_temporal_long.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", f"-I{ROOT}/include", f"-I{CSRC}",
           *build.EXTRA_FLAGS["attention_temporal_long.hip"], "-S", "--cuda-device-only",
           os.path.join(CSRC, "attention_temporal_long.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    kernels = re.findall(r"^(_Z\w*attn_temporal_long_kernel\w*):", asm, re.M)
    assert len(kernels) == 2, kernels
    assert any("ILi32E" in k for k in kernels) and any("ILi64E" in k for k in kernels)
    sizes = re.findall(r"^; ScratchSize: (\d+)", asm, re.M)
    assert len(sizes) == 2 and all(int(s) == 0 for s in sizes), sizes
    assert "v_mfma_f32_32x32x16_bf16" in asm and "v_permlane32_swap" in asm and "global_store_dwordx4" in asm
    assert "attention_temporal_long.hip" in build.SOURCES
    # csrc/attention_temporal_rel.hip is built from the same wave (csrc/attn_temporal_wave.h): its four instances alike
    out = tmp_path / "attention_temporal_rel.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", f"-I{ROOT}/include", f"-I{CSRC}",
           *build.EXTRA_FLAGS["attention_temporal_rel.hip"], "-S", "--cuda-device-only",
           os.path.join(CSRC, "attention_temporal_rel.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    kernels = re.findall(r"^(_Z\w*attn_temporal_rel_kernel\w*):", asm, re.M)
    assert len(kernels) == 4, kernels
    for inst in ("ILi32ELi4ELb0E", "ILi32ELi4ELb1E", "ILi64ELi4ELb0E", "ILi64ELi2ELb1E"):
        assert any(inst in k for k in kernels), (inst, kernels)
    sizes = re.findall(r"^; ScratchSize: (\d+)", asm, re.M)
    assert len(sizes) == 4 and all(int(s) == 0 for s in sizes), sizes
    assert "v_mfma_f32_32x32x16_bf16" in asm and "v_permlane32_swap" in asm and "global_store_dwordx4" in asm
    assert "attention_temporal_rel.hip" in build.SOURCES
