"""DDIM sampler with separate text / image guidance.

Interface of reference lvdm/models/samplers/ddim_multiplecond.py: the same class as
samplers/ddim.py (make_schedule, sample, ddim_sampling are line-for-line the same there) with a
`p_sample_ddim` (210-288) that runs THREE UNet passes per step -- full condition, unconditional,
and "image kept, text dropped" (`kwargs['unconditional_conditioning_img_nonetext']`) -- and combines

    e = e_uncond + cfg_img * (e_uncond_img - e_uncond) + s * (e_cond - e_uncond_img)        (:236)

before the usual guidance rescale against e_cond, v-parameterisation and DDIM update.
scripts/evaluation/funcs.py:61-76 selects it with `multiple_cond_cfg=True`.

`ddim_sampling` -- pinned frames (`mask` / `x0`, :177-184), `clean_cond`, partial runs (`timesteps=`), per-clip `seeds=`,
the opt-in `solver_order=2` with its history and `multistep_corr` -- `decode` and `stochastic_encode` are inherited from the mirror of samplers/ddim.py, as they are the same code in the reference.

Here the three passes are one batch-3B UNet call (`apply_model_multi`) and the combination is part
of the fused tc_ddim_step kernel (TcDdimParams.e_uncond_img / cfg_img).
"""
from __future__ import annotations

import torch

from .ddim import DDIMSampler as _DDIMSampler


class DDIMSampler(_DDIMSampler):
    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False,
                      quantize_denoised=False, temperature=1., noise_dropout=0., score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                      uc_type=None, cfg_img=None, mask=None, x0=None, guidance_rescale=0.0, _step=None, seeds=None,
                      solver_order=1, x0_hist=None, ms_corr=0.0, **kwargs):
        cfg = unconditional_guidance_scale if cfg_img is None else cfg_img             # :217-218

        def evaluate(use_cfg):
            # the lookup comes first, whatever the guidance: a KeyError like the reference's (:220), and the key stays in kwargs
            cfgs = [c, unconditional_conditioning, kwargs['unconditional_conditioning_img_nonetext']]
            if not use_cfg:
                return self.model.apply_model(x, t, c, **kwargs), None, dict(e_uncond_img=None, cfg_img=cfg)
            if hasattr(self.model, "apply_model_multi"):
                e_c, e_u, e_i = self.model.apply_model_multi(x, t, cfgs, **kwargs)
            else:
                e_c, e_u, e_i = (self.model.apply_model(x, t, cond, **kwargs) for cond in cfgs)
            return e_c, e_u, dict(e_uncond_img=e_i.contiguous(), cfg_img=cfg)

        return self.guided_step(evaluate, x, t, index, repeat_noise, use_original_steps, quantize_denoised, temperature,
                                noise_dropout, score_corrector, unconditional_guidance_scale, unconditional_conditioning,
                                guidance_rescale, _step, seeds, solver_order, x0_hist, ms_corr)
