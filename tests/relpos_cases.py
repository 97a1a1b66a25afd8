"""Shared pieces of tests/test_relpos_cpu.py and tests/test_gpu_relpos.py (temporal attention with relative position and / or
a causal mask: tc_attn_temporal_rel, use_relative_position / use_causal_attention of the UNet): the fp64 statement of the
attention, its emulated operator, and the tiny UNets of the fixture.  Fixture: tests/golden/make_relpos_golden.py."""
import torch

from conftest import TINY_UNET_CFG
from emu_ops import EmuOps

# variant -> (use_relative_position, use_causal_attention, frames); temporal_length is 4 (TINY_UNET_CFG), so "rel6" clamps
VARIANTS = {"rel": (True, False, 4), "causal": (False, True, 4), "both": (True, True, 4), "rel6": (True, False, 6)}
UNET_BORROWED = 3.5e-2           # test_alpha_and_scale_unet_vs_reference_golden's bound for a tiny UNet forward
# rel-L2 of the EMULATED operator contract (RelEmuOps: bf16 between operators, on the CPU) against the reference's fp32 output
# of each variant -- figures of the contract, not of the code under test; tests/test_relpos_cpu.py re-measures them.  The GPU
# test holds the kernels to UNET_BORROWED where the figure is at most 2/3 of it, and to 1.5 x the figure otherwise.
UNET_CONTRACT = {"rel": 2.259e-2, "causal": 2.454e-2, "both": 2.261e-2, "rel6": 2.148e-2}


def unet_bound(variant):
    c = UNET_CONTRACT[variant]
    return UNET_BORROWED if c <= UNET_BORROWED * 2 / 3 else 1.5 * c


def rel_attn_f64(x, rel_k, rel_v, *, max_rel, causal, scale):
    """The attention over the frames of every pixel and head, in the precision of its arguments (fp64 in the tests):
    x [b, t, hw, 3, heads, 64] = q / k / v, rel_k / rel_v [2 max_rel + 1, 64] or both None.

        idx(i, j) = clamp(j - i, -L, L) + L
        s[i, j]   = scale * (q_i . k_j + q_i . Rk[idx(i, j)]),   -inf for j > i when causal
        o_i       = sum_j softmax_j(s[i, :])[j] * (v_j + Rv[idx(i, j)])            -> [b, t, hw, heads, 64]"""
    t = x.shape[1]
    q, k, v = (x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))          # [b, hw, heads, t, 64]
    s = q @ k.transpose(-1, -2)                                                  # [b, hw, heads, i, j]
    if rel_k is not None:
        fr = torch.arange(t, device=x.device)
        idx = (fr[None, :] - fr[:, None]).clamp(-max_rel, max_rel) + max_rel     # [i, j]
        s = s + torch.einsum("...id,ijd->...ij", q, rel_k.to(x.dtype)[idx])
    s = s * scale
    if causal:
        s = s.masked_fill(torch.ones(t, t, dtype=torch.bool, device=x.device).triu(1), float("-inf"))
    p = s.softmax(-1)
    o = p @ v
    if rel_v is not None:
        o = o + torch.einsum("...ij,ijd->...id", p, rel_v.to(x.dtype)[idx])
    return o.permute(0, 3, 1, 2, 4)


class RelEmuOps(EmuOps):
    """tests/emu_ops.py plus ops.attention_temporal_rel: the statement above in fp32 on the bf16 inputs, the result rounded
    to bf16 like every other operator's."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.rel_calls = 0

    def attention_temporal_rel(self, qkv, rel_k, rel_v, *, b, t, hw, heads, max_rel, causal, scale=None):
        assert (rel_k is None) == (rel_v is None)
        self.rel_calls += 1
        scale = 64 ** -0.5 if scale is None else scale
        x = qkv.to(torch.float32).reshape(b, t, hw, 3, heads, 64)
        tabs = [None if r is None else r.to(torch.float32).to(x.device) for r in (rel_k, rel_v)]
        o = rel_attn_f64(x, *tabs, max_rel=max_rel, causal=causal, scale=scale)
        return self._out(o.reshape(b * t * hw, heads * 64)).contiguous()


def tiny_unet(variant=None, **extra):
    """The tiny UNet of the fixture on the synthetic weights (seed 1234); `variant` None = the flagless model.  The tables
    still hold the synthetic recipe's values: set_tables() gives them the fixture's."""
    from tooncrafter_amd import synth
    from tooncrafter_amd.lvdm.openaimodel3d import UNetModel
    rel, causal = VARIANTS[variant][:2] if variant is not None else (False, False)
    un = UNetModel(**dict(TINY_UNET_CFG, use_relative_position=rel, use_causal_attention=causal, **extra)).eval()
    synth.fill_module_(un, prefix="model.diffusion_model.", seed=1234)
    return un


def set_tables(unet, golden):
    """Every relative-position table at the values the fixture recorded for it."""
    params = dict(unet.named_parameters())
    names = [str(n) for n in golden["table_names"]]
    assert names and sorted(names) == sorted(k for k in params if k.endswith(".embeddings_table"))
    with torch.no_grad():
        for n, v in zip(names, golden["table_values"]):
            params[n].copy_(torch.from_numpy(v))
    unet.invalidate()
    return unet


def unet_inputs(golden, variant, dev="cpu"):
    """(args, kwargs) of the fixture's forward for a variant (4 or 6 frames)."""
    t = VARIANTS[variant][2] if variant in VARIANTS else int(variant)
    f = lambda k: torch.from_numpy(golden[k]).to(dev)
    return (f(f"x{t}"), f("timesteps")), dict(context=f(f"ctx{t}"), fs=f("fs"))
