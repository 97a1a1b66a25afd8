"""tc_ddim_step_ms on the emulated operator contract: the emulated ddim_step plus the one history term, in fp32, so that the
samplers' `solver_order=2` host logic runs without a GPU (tests/test_multistep_cpu.py) and the GPU pipeline has a PyTorch
statement to be compared with (tests/test_gpu_multistep.py).  `ddim_step` also takes the `parameterization` keyword of
ops.ddim_step ("eps": the fp64 statement of tests/plain_family_cases.py rounded to fp32), so one backend serves every model."""
import torch

from emu_seeded_ops import EmuSeededOps
from plain_family_cases import eps_step_f64


class EmuMultistepOps(EmuSeededOps):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ms_calls = []                   # (x0_hist is not None, corr) of every ddim_step_ms call, in order

    def ddim_step(self, x, e_cond, e_uncond, noise, *, parameterization="v", want_x0=True, **kw):
        if parameterization == "v":
            return super().ddim_step(x, e_cond, e_uncond, noise, want_x0=want_x0, **kw)
        assert parameterization == "eps"
        xp, x0 = eps_step_f64(x, e_cond, e_uncond, noise, **kw)
        return xp.float(), (x0.float() if want_x0 else None)

    def ddim_step_ms(self, x, e_cond, e_uncond, noise, x0_hist, *, corr, sigma, x0_rescale, want_x0=True, parameterization="v",
                     pred_x0=None, **kw):
        f = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device)
        self.ms_calls.append((x0_hist is not None, float(corr)))
        first = lambda rescale: self.ddim_step(x, e_cond, e_uncond, None, sigma=sigma, x0_rescale=rescale,
                                               parameterization=parameterization, **kw)
        xp, x0 = first(x0_rescale)                                   # the first-order update without its noise term
        if x0_hist is not None and corr != 0.0:
            x0u = first(1.0)[1]                                      # the prediction before x0_rescale
            xp = xp + f(corr) * (x0u - x0_hist)
        if noise is not None:
            xp = xp + f(sigma) * noise
        if pred_x0 is not None:
            pred_x0.copy_(x0)
            x0 = pred_x0
        return xp, (x0 if want_x0 or pred_x0 is not None else None)
