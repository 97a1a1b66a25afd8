"""The 8-bit spatial self-attention route (TC_FP8_ATTN, ABI 14) in the full-size model: the UNet forward against the fp32
oracle golden (as test_gpu_fullsize.test_unet_full_size_fp8), the routed count, the switch off = the default path bit for
bit, the decoder untouched, and DDIM-50 under test_gpu_ddim50's unchanged bounds."""
import pytest
import torch

import fullsize_cases as fc
from conftest import rel_l2
from test_gpu_ddim50 import _hip_run, _report, oracle_runs  # noqa: F401  (oracle_runs: the module fixture)
from test_gpu_fullsize import cosine
from tooncrafter_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
# TC_FP8=1 + TC_FP8_ATTN=1: rel-L2 of the UNet output against the fp32 oracle, measured 1.915e-2 (TC_FP8=1 alone 1.917e-2,
# bf16 1.44e-2; profiles/r07_q8_attn_model_tests.txt): 1.4x that, under the 3.5e-2 ceiling
UNET_Q8_REL, UNET_Q8_COS = 2.7e-2, 0.999


def _unet_args(inp):
    return dict(context=inp["cond"].to(DEV), fs=inp["fs"].to(DEV)), [inp["x_T"].to(DEV), inp["c_concat"].to(DEV)]


def _count_eligible(be, fn):
    """Run fn() with be.attention wrapped: how many of its calls the 8-bit rule would take if the switch were on."""
    n = [0]
    orig = be.attention

    def counting(q, k, v, *, batch, heads, lq, lk, kv_bdiv=1, out=None, accumulate=False, scale=None, k2=None, **kw):
        if k2 is None and not accumulate and kv_bdiv == 1 and lk >= be.fp8_attn_min_lk:
            n[0] += 1
        return orig(q, k, v, batch=batch, heads=heads, lq=lq, lk=lk, kv_bdiv=kv_bdiv, out=out, accumulate=accumulate,
                    scale=scale, k2=k2, **kw)

    be.attention = counting
    try:
        res = fn()
    finally:
        del be.attention
    return res, n[0]


@pytest.mark.timeout(1500)
def test_unet_full_size_fp8_attn(full_model, golden, inp):
    be = ops.backend()
    un = full_model.model.diffusion_model
    ts = torch.tensor([fc.UNET_T], device=DEV)
    args, parts = _unet_args(inp)
    old, old_attn = be.fp8, be.fp8_attn
    with torch.no_grad():
        try:
            be.fp8, be.fp8_attn = "linear", False
            y8, eligible = _count_eligible(be, lambda: un(None, ts, x_parts=parts, **args).cpu())
            c0 = dict(be.fp8_calls)
            be.fp8_attn = True
            yq = un(None, ts, x_parts=parts, **args).cpu()
        finally:
            be.fp8, be.fp8_attn = old, old_attn
    routed = be.fp8_calls["attn_q8"] - c0["attn_q8"]
    ref = torch.from_numpy(golden["unet_y"])
    eq, cq, e8 = rel_l2(yq, ref), cosine(yq, ref), rel_l2(y8, ref)
    print(f"full-size UNet, TC_FP8=1 + TC_FP8_ATTN=1: {routed} spatial self-attentions on the 8-bit kernel (lk >= "
          f"{be.fp8_attn_min_lk}); rel-L2 vs fp32 oracle {eq:.3e} (TC_FP8=1 alone {e8:.3e}), cosine {cq:.6f}; "
          f"vs TC_FP8=1 alone {rel_l2(yq, y8):.3e}")
    assert eligible > 0 and routed == eligible
    assert torch.isfinite(yq).all() and not torch.equal(yq, y8)
    assert eq <= UNET_Q8_REL and cq >= UNET_Q8_COS


@pytest.mark.timeout(1500)
def test_switch_off_is_the_default_path(full_model, inp):
    be = ops.backend()
    un = full_model.model.diffusion_model
    ts = torch.tensor([fc.UNET_T], device=DEV)
    args, parts = _unet_args(inp)
    assert be.fp8_attn is False, "TC_FP8_ATTN is off by default"
    with torch.no_grad():
        y0 = un(None, ts, x_parts=parts, **args)
        c0 = dict(be.fp8_calls)
        be.fp8_attn = True
        be.fp8_attn = False
        y1 = un(None, ts, x_parts=parts, **args)
    assert torch.equal(y0, y1)
    assert be.fp8_calls == c0


@pytest.mark.timeout(1500)
def test_decoder_never_routed(full_model, inp):
    be = ops.backend()
    dec = full_model.first_stage_model.decoder
    refs = [r.to(DEV) for r in inp["refs"]]
    old, old_graph = be.fp8_attn, dec.use_hipgraph
    c0 = be.fp8_calls["attn_q8"]
    be.fp8_attn, dec.use_hipgraph = True, False
    try:
        with torch.no_grad():
            y = dec.decode_clip(inp["z_dec"].to(DEV), refs, scale=1.0 / 0.18215)
    finally:
        be.fp8_attn, dec.use_hipgraph = old, old_graph
    assert torch.isfinite(y).all()
    assert be.fp8_calls["attn_q8"] == c0


@pytest.mark.timeout(1800)
def test_ddim50_fp8_linear_and_attn(full_model, inp, oracle_runs):  # noqa: F811
    """DDIM-50 with TC_FP8=1 and TC_FP8_ATTN=1 under test_gpu_ddim50's bounds; the sampler re-captures its graph because
    the routing is part of the graph signature."""
    be = ops.backend()
    old, old_attn = be.fp8, be.fp8_attn
    be.fp8, be.fp8_attn = "linear", True
    c0 = be.fp8_calls["attn_q8"]
    try:
        hip = _hip_run(full_model, inp, oracle_runs["noises"])
    finally:
        be.fp8, be.fp8_attn = old, old_attn
    assert be.fp8_calls["attn_q8"] > c0, "the 8-bit attention did not run"
    _report("fp8_linear_attn", hip, oracle_runs)
