"""The PyTorch statement of tc_ddim_blend, on top of the operator contract of emu_ops.EmuOps: what lets the pinned-frame
and partial-run host logic of the samplers run without a GPU (tests/test_pinned_cpu.py)."""
import torch

from emu_ops import EmuOps


class EmuPinnedOps(EmuOps):
    def ddim_blend(self, x, x0, noise, mask, *, sqrt_ac=1.0, sqrt_1m_ac=0.0, out=None):
        f = lambda v: torch.tensor(v, dtype=torch.float32, device=x0.device)
        orig = x0 if noise is None else f(sqrt_ac) * x0 + f(sqrt_1m_ac) * noise
        res = orig if mask is None else orig * mask + (1. - mask) * x
        if out is None:
            return res.clone() if res is x0 else res
        out.copy_(res)
        return out
