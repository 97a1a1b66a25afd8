"""DDIM sampler driving the HIP UNet.

Interface of reference lvdm/models/samplers/ddim.py: DDIMSampler.__init__ (11-16),
register_buffer (18-22), make_schedule (24-57), sample (60-132), ddim_sampling
(135-203), p_sample_ddim (206-279), decode (282-301), stochastic_encode (304-317) -- same
signatures, kwargs and return values, so scripts/evaluation/inference.py:244-259 and
funcs.py:61-76 call it unchanged.

What is different underneath:
  * the per-step algebra (CFG combine, guidance rescale with its two unbiased
    stds, v -> eps/x0, dynamic rescale, x_prev) is ONE fused kernel (tc_ddim_step; tc_ddim_step_eps
    for a model with parameterization "eps", ddim.py:234, 258);
  * its six scalars per step are computed on the host from the schedule tables in the
    reference's exact order/precision, so the loop has no device->host sync (the
    reference reads six device scalars per step, ddim.py:251-264);
  * conditional and unconditional UNet passes run as one B=2 call when the model
    offers `apply_model_cfg` (every normalisation in the UNet is per-sample, so this is
    exact), reading the 2.9 GB of weights once per step instead of twice.
  * pinned frames (`mask` / `x0`, ddim.py:173-180) are noised by `model.q_sample` and blended
    into the latent by tc_ddim_blend at the top of each step, with the bits of the
    reference's separate torch ops; the mask is made dense fp32 once per call.
  * `seeds=` (one integer per clip of the batch; not in the reference): every Gaussian draw of the run comes from
    tc_randn_clips, a pure function of (the clip's seed, the stream number below, the element index), instead of the
    process-wide device generator.  A clip then gets the same noise in any batch, slot, process or rank, and the torch
    generator is not touched.  This is Philox noise, not torch's: a seeded run does not reproduce a reference run with
    seed_everything; the unseeded path (seeds=None) is the one that does, and is unchanged.
  * `solver_order=2` (not in the reference; the default 1 is the reference's update, untouched): a second-order multistep
    correction from the previous step's pred_x0, with no further UNet call -- DPM-Solver++(2M) at eta = 0 and its SDE
    variant at eta = 1, on the effective schedule of the dynamic rescale.  It is one more term of the fused kernel
    (tc_ddim_step_ms) and one more host scalar per step (`multistep_corr`); the noise draws are those of order 1.  The
    first step of a run, the step after an alpha = 0 step and the final step (DDIM index 0) stay first order.  Verified
    against an analytic Gaussian model only: what it does to real frames at reduced step counts is unmeasured.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from tqdm import tqdm

from .. import ops
from .utils_diffusion import make_ddim_sampling_parameters, make_ddim_timesteps


# Stream numbers of a seeded run: which draw of its clip a tc_randn_clips call is.  The step draws are keyed by the DDIM
# table position `index`, not by the loop counter, so a partial run (`timesteps=`, `decode`) walks the very draws the
# tail of the full run walks.
STREAM_X_T = 0                 # x_T, when the caller gave none
STREAM_STEP = 1                # + index: the step at DDIM table position `index` (drawn only when sigma != 0)
STREAM_Q_SAMPLE = 0x10000      # + index: the q_sample draw of the pinned-frame blend at that step
STREAM_ENCODE = 0x20000        # stochastic_encode


def noise_like(shape, device, repeat=False):
    """Gaussian draw from the device generator (reference lvdm/common.py:31-34).  Module-level
    name so that parity tests can substitute an injected noise source, as they do for the
    reference (`lvdm.models.samplers.ddim.noise_like`)."""
    if repeat:
        return torch.randn((1, *shape[1:]), device=device).repeat(shape[0], *((1,) * (len(shape) - 1)))
    return torch.randn(shape, device=device)


def subset_timesteps(ddim_timesteps, timesteps):
    """The steps a partial run walks (ddim.py:152-156): the lowest `subset_end` entries of the DDIM sequence, where the
    reference's rule ends ONE short of `timesteps` (S = 5: timesteps=3 -> two steps, timesteps >= 5 -> four)."""
    if timesteps is None:
        return ddim_timesteps
    n = ddim_timesteps.shape[0]
    subset_end = int(min(timesteps / n, 1) * n) - 1
    return ddim_timesteps[:subset_end]


def check_solver_order(solver_order, what):
    """1 (the reference's DDIM update) or 2 (the multistep correction); a host check, before anything is launched."""
    if isinstance(solver_order, bool) or solver_order not in (1, 2):
        raise ValueError(f"{what}: solver_order must be 1 or 2, got {solver_order!r}")
    return int(solver_order)


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.counter = 0

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor) and attr.device != self.model.device:
            attr = attr.to(self.model.device)        # follow the model (the reference hard-codes "cuda")
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize,
                                                  num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        m = self.model
        ac = m.alphas_cumprod.detach().to(torch.float32).cpu()
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        if m.use_dynamic_rescale:
            sa = m.scale_arr.detach().to(torch.float32).cpu()[torch.as_tensor(self.ddim_timesteps, dtype=torch.long)]
            self.ddim_scale_arr = sa
            self.ddim_scale_arr_prev = torch.cat([sa[0:1], sa[:-1]])
        self.register_buffer('betas', m.betas.detach().to(torch.float32))
        self.register_buffer('alphas_cumprod', m.alphas_cumprod.detach().to(torch.float32))
        self.register_buffer('alphas_cumprod_prev', m.alphas_cumprod_prev.detach().to(torch.float32))
        sigmas, alphas, alphas_prev = make_ddim_sampling_parameters(ac, self.ddim_timesteps, ddim_eta, verbose)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sigmas, alphas, alphas_prev
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - alphas)
        # host copies of the two per-timestep fp32 buffers the v-parameterisation reads
        self._sqrt_ac = m.sqrt_alphas_cumprod.detach().to(torch.float32).cpu()
        self._sqrt_1m_ac = m.sqrt_one_minus_alphas_cumprod.detach().to(torch.float32).cpu()

    def step_kind(self):
        """What the model predicts, as the fused step takes it: "v" (tc_ddim_step) or "eps" (tc_ddim_step_eps).  The
        reference's samplers treat "x0" as eps (ddim.py:231-234); that is not reproduced."""
        par = self.model.parameterization
        if par not in ("v", "eps"):
            raise NotImplementedError(f"the fused DDIM step implements the v- and eps-parameterisations, not {par!r}")
        return par

    def step_scalars(self, index: int, t: int):
        """The fp32 scalars of one update, each rounded exactly where the reference's
        `torch.full(size, value)` rounds it (ddim.py:251-266, 271, 277)."""
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
        a_prev = f32(self.ddim_alphas_prev[index])
        sigma = f32(self.ddim_sigmas[index])
        # At eta = 1 the alpha_t = 0 start of a zero-terminal-SNR schedule has sigma^2 = 1 - a_prev in exact arithmetic, and
        # the radicand is 0 give or take a rounding: at S = 7, 11, 14, 15, 20, 25, 33-35, 37-39 (uniform_trailing) it
        # comes out below zero and the reference's sqrt is NaN for the whole run.  Clamped at 0: wherever the reference is
        # finite these are its bits, and the step counts a second-order run would pick (20, 25) work.
        dir_coef = (1. - a_prev - sigma ** 2).clamp(min=0.).sqrt()
        x0_rescale = f32(1.0)
        if self.model.use_dynamic_rescale:
            x0_rescale = self.ddim_scale_arr_prev[index] / self.ddim_scale_arr[index]
        sc = dict(sqrt_ac=float(self._sqrt_ac[t]), sqrt_1m_ac=float(self._sqrt_1m_ac[t]),
                  sqrt_a_prev=float(a_prev.sqrt()), dir_coef=float(dir_coef), sigma=float(sigma),
                  x0_rescale=float(x0_rescale))
        if self.model.parameterization != "v":
            # the eps branch reads the DDIM tables, not the model's per-timestep buffers: a_t = ddim_alphas[index] with an
            # fp32 sqrt, and ddim_sqrt_one_minus_alphas[index] (ddim.py:251-258).  The "v" call carries no extra keyword.
            sc.update(sqrt_ac=float(f32(self.ddim_alphas[index]).sqrt()),
                      sqrt_1m_ac=float(f32(self.ddim_sqrt_one_minus_alphas[index])), parameterization=self.step_kind())
        return sc

    def multistep_corr(self, index: int, t: int, h_prev):
        """(corr, h) of the step at DDIM table position `index`, timestep `t`, for tc_ddim_step_ms.  h is the step's
        increment of lambda = log(sqrt(alpha) * scale / sqrt(1 - alpha)), the log-SNR on the effective schedule of the dynamic
        rescale, taken as the log of one ratio (infinite when alpha_t = 0); `h_prev` is the previous step's, None on the
        first step of a run.  With A = sqrt_a_prev * rho - dir_coef * sqrt_ac / sqrt_1m_ac, the coefficient of the
        un-rescaled prediction in the first-order update (rho = x0_rescale),
            corr = A * h / (2 * h_prev),
        in double from the tables `step_scalars` reads, rounded to fp32 once.  corr = 0 -- a first-order step -- without a
        usable h_prev (first step, or the step after alpha_t = 0) and on the final step, index 0: the jump to
        alphas_cumprod[0] is the largest log-SNR increment of the run, and extrapolating over it costs more than it gains."""
        a_prev, sigma = float(self.ddim_alphas_prev[index]), float(self.ddim_sigmas[index])
        if self.step_kind() == "v":
            sqrt_ac, sqrt_1m_ac = float(self._sqrt_ac[t]), float(self._sqrt_1m_ac[t])
        else:
            sqrt_ac, sqrt_1m_ac = math.sqrt(float(self.ddim_alphas[index])), float(self.ddim_sqrt_one_minus_alphas[index])
        rho = 1.0
        if self.model.use_dynamic_rescale:
            rho = float(self.ddim_scale_arr_prev[index]) / float(self.ddim_scale_arr[index])
        h = math.inf
        if sqrt_ac > 0.0 and 0.0 < a_prev < 1.0 and sqrt_1m_ac > 0.0:
            h = math.log((math.sqrt(a_prev) * rho * sqrt_1m_ac) / (sqrt_ac * math.sqrt(1.0 - a_prev)))
        if index == 0 or h_prev is None or not math.isfinite(h_prev) or h_prev == 0.0 or not math.isfinite(h):
            return 0.0, h
        dir_coef = math.sqrt(max(1.0 - a_prev - sigma * sigma, 0.0))
        corr = (math.sqrt(a_prev) * rho - dir_coef * sqrt_ac / sqrt_1m_ac) * h / (2.0 * h_prev)
        return float(np.float32(corr)), h

    def fused_step(self, x, e_c, e_u, noise, sc, solver_order, x0_hist, ms_corr, **guidance):
        """The fused update of the two- and the three-way sampler: tc_ddim_step at order 1 (the reference's path, the call it
        always was), tc_ddim_step_ms at order 2 -- first order there too while there is no history."""
        if solver_order == 1:
            return ops.ddim_step(x, e_c, e_u, noise, **guidance, **sc)
        return ops.ddim_step_ms(x, e_c, e_u, noise, x0_hist, corr=0.0 if x0_hist is None else ms_corr, **guidance, **sc)

    def loop_step(self, order2, x, c, ts, index, step, **kw):
        """One `p_sample_ddim` call of a sampling loop, with the order-2 bookkeeping.  `order2`: None at order 1, where
        p_sample_ddim gets the keywords it always got; at order 2 the loop's [last pred_x0, last log-SNR increment], [None, None]
        at the start of a run, read for this step's keywords and updated after it (a prediction of x0: the pinned-frame blend
        does not touch it)."""
        if order2 is None:
            return self.p_sample_ddim(x, c, ts, index=index, _step=step, **kw)
        corr, h = self.multistep_corr(index, step, order2[1])
        x_prev, pred_x0 = self.p_sample_ddim(x, c, ts, index=index, _step=step, solver_order=2, x0_hist=order2[0], ms_corr=corr, **kw)
        order2[:] = pred_x0, h
        return x_prev, pred_x0

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1.,
               noise_dropout=0., score_corrector=None, corrector_kwargs=None, verbose=True,
               schedule_verbose=False, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, precision=None, fs=None, timestep_spacing='uniform',
               guidance_rescale=0.0, seeds=None, solver_order=1, **kwargs):
        solver_order = check_solver_order(solver_order, "sample")      # host checks only, before anything is launched
        if seeds is not None:
            seeds = ops.clip_seeds(seeds, batch_size, "sample: seeds")
            if kwargs.get("repeat_noise"):
                raise ValueError("sample: repeat_noise=True shares one draw among the clips; seeds= draws one per clip")
        if conditioning is not None:
            if isinstance(conditioning, dict):
                first = conditioning[list(conditioning.keys())[0]]
                cbs = (first[0] if isinstance(first, (list, tuple)) else first).shape[0]
            else:
                cbs = conditioning.shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_discretize=timestep_spacing, ddim_eta=eta,
                           verbose=schedule_verbose)
        if hasattr(self.model, "reset_conditioning"):
            self.model.reset_conditioning()          # a sampling run = one clip: never reuse cached conditioning
        if len(shape) == 3:
            size = (batch_size, *shape)
        else:
            c, t, h, w = shape
            size = (batch_size, c, t, h, w)
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0,
                                  ddim_use_original_steps=False, noise_dropout=noise_dropout,
                                  temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, verbose=verbose,
                                  precision=precision, fs=fs, guidance_rescale=guidance_rescale, seeds=seeds,
                                  solver_order=solver_order, **kwargs)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None,
                      timesteps=None, quantize_denoised=False, mask=None, x0=None, img_callback=None,
                      log_every_t=100, temperature=1., noise_dropout=0., score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                      verbose=True, precision=None, fs=None, guidance_rescale=0.0, seeds=None, solver_order=1, **kwargs):
        solver_order = check_solver_order(solver_order, "ddim_sampling")
        if ddim_use_original_steps or quantize_denoised or score_corrector is not None:
            raise NotImplementedError("only the DDIM-subsequence sampling path the scripts use")
        device = self.model.betas.device
        b = shape[0]
        if seeds is not None:
            seeds = ops.clip_seeds(seeds, b, "ddim_sampling: seeds")
        if x_T is not None:
            img = x_T
        elif seeds is not None:
            img = ops.randn_clips(seeds, tuple(shape), STREAM_X_T)
        else:
            img = torch.randn(shape, device=device)
        img = img.to(torch.float32).contiguous()
        steps = subset_timesteps(self.ddim_timesteps, timesteps)
        total_steps = steps.shape[0]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        time_range = np.flip(steps)
        iterator = tqdm(time_range, desc='DDIM Sampler', total=total_steps) if verbose else time_range
        clean_cond = kwargs.pop("clean_cond", False)
        if mask is not None:
            assert x0 is not None
            # once per call: whatever broadcasts to the latent (a (1,1,T,1,1) bool frame selector, a dense weight map)
            # becomes the dense fp32 operand of the blend kernel
            mask = torch.as_tensor(mask).to(device=device, dtype=torch.float32).expand(tuple(img.shape)).contiguous()
            x0 = x0.to(device=device, dtype=torch.float32).expand(tuple(img.shape)).contiguous()
        order2 = [None, None] if solver_order == 2 else None
        for i, step in enumerate(iterator):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if mask is not None:
                # ddim.py:173-180: known latents, noised to THIS step's level (the q_sample draw comes before the step's
                # noise_like draw), replace the masked part of the latent.  The timestep goes over as a host integer:
                # q_sample then reads its two coefficients from host tables.  Never in place: `img` may be the caller's
                # x_T or an entry of `intermediates`.
                if clean_cond:
                    img_orig = x0
                elif seeds is not None:
                    img_orig = self.model.q_sample(x0, int(step), noise=ops.randn_clips(seeds, tuple(x0.shape), STREAM_Q_SAMPLE + index))
                else:
                    img_orig = self.model.q_sample(x0, int(step))
                img = ops.ddim_blend(img, img_orig, None, mask)
            img, pred_x0 = self.loop_step(order2, img, cond, ts, index, int(step), temperature=temperature,
                                          noise_dropout=noise_dropout,
                                          unconditional_guidance_scale=unconditional_guidance_scale,
                                          unconditional_conditioning=unconditional_conditioning,
                                          fs=fs, guidance_rescale=guidance_rescale, seeds=seeds, **kwargs)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False,
                      quantize_denoised=False, temperature=1., noise_dropout=0., score_corrector=None,
                      corrector_kwargs=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
                      uc_type=None, conditional_guidance_scale_temporal=None, mask=None, x0=None,
                      guidance_rescale=0.0, _step=None, seeds=None, solver_order=1, x0_hist=None, ms_corr=0.0, **kwargs):
        """`solver_order=2` with `x0_hist` (the previous step's pred_x0) and `ms_corr` (`multistep_corr`): the corrected
        step; the caller's loop carries both, nothing is kept on the sampler."""
        def evaluate(use_cfg):
            if not use_cfg:
                return self.model.apply_model(x, t, c, **kwargs), None, {}
            if hasattr(self.model, "apply_model_cfg"):
                return (*self.model.apply_model_cfg(x, t, c, unconditional_conditioning, **kwargs), {})
            return (self.model.apply_model(x, t, c, **kwargs),
                    self.model.apply_model(x, t, unconditional_conditioning, **kwargs), {})
        return self.guided_step(evaluate, x, t, index, repeat_noise, use_original_steps, quantize_denoised, temperature,
                                noise_dropout, score_corrector, unconditional_guidance_scale, unconditional_conditioning,
                                guidance_rescale, _step, seeds, solver_order, x0_hist, ms_corr)

    def guided_step(self, evaluate, x, t, index, repeat_noise, use_original_steps, quantize_denoised, temperature, noise_dropout,
                    score_corrector, unconditional_guidance_scale, unconditional_conditioning, guidance_rescale, _step, seeds,
                    solver_order, x0_hist, ms_corr):
        """`p_sample_ddim` of the two- and the three-way sampler, which differ in `evaluate(use_cfg)` alone: it runs the model
        and returns (e_cond, e_uncond or None, further guidance keywords of the fused step)."""
        solver_order = check_solver_order(solver_order, "p_sample_ddim")
        if use_original_steps or quantize_denoised or score_corrector is not None or noise_dropout > 0.:
            raise NotImplementedError("p_sample_ddim variant unused by the inference scripts")
        self.step_kind()
        if seeds is not None and repeat_noise:
            raise ValueError("p_sample_ddim: repeat_noise=True shares one draw among the clips; seeds= draws one per clip")
        step = int(t[0]) if _step is None else _step
        use_cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
        e_c, e_u, guidance = evaluate(use_cfg)
        sc = self.step_scalars(index, step)
        # unseeded: always drawn, like the reference (ddim.py:266, ddim_multiplecond.py:277)
        noise = self.step_noise(x, index, sc["sigma"], temperature, repeat_noise, seeds)
        return self.fused_step(x.contiguous(), e_c.contiguous(), None if e_u is None else e_u.contiguous(), noise, sc,
                               solver_order, x0_hist, ms_corr, cfg_scale=unconditional_guidance_scale,
                               guidance_rescale=guidance_rescale if use_cfg else 0.0, **guidance)

    def step_noise(self, x, index, sigma, temperature, repeat_noise, seeds):
        """The step's noise operand of tc_ddim_step (None when sigma == 0), shared by the two- and three-way samplers."""
        if seeds is not None:
            # one tc_randn_clips launch, the temperature applied as its `scale`; nothing is drawn for a deterministic step
            # and the device generator is left alone
            if sigma == 0.0:
                return None
            return ops.randn_clips(seeds, tuple(x.shape), STREAM_STEP + index, scale=temperature)
        # the reference draws the noise every step, also when sigma == 0 (ddim.py:266): draw (and drop) it so
        # the device generator stays in step with the reference for later draws (x_T of the next variant)
        noise = noise_like(x.shape, x.device, repeat_noise)
        if sigma == 0.0:
            return None
        if temperature != 1.:
            noise = noise * temperature
        return noise.to(torch.float32).contiguous()

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None, seeds=None, solver_order=1):
        """The last `t_start` steps of the DDIM sequence from `x_latent` (ddim.py:282-301); `make_schedule` first.  Like the
        reference it hands p_sample_ddim neither `fs` nor a guidance rescale (the UNet falls back to its default_fs).
        `seeds`: one per sample; the steps then draw what a seeded `sample` draws at the same table positions.
        `solver_order=2`: the multistep correction, starting first order (no history) and ending first order at index 0."""
        solver_order = check_solver_order(solver_order, "decode")
        if use_original_steps:
            raise NotImplementedError("only the DDIM-subsequence sampling path the scripts use")
        if seeds is not None:
            seeds = ops.clip_seeds(seeds, x_latent.shape[0], "decode: seeds")
        timesteps = self.ddim_timesteps[:t_start]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        print(f"Running DDIM Sampling with {total_steps} timesteps")
        x_dec = x_latent.to(torch.float32).contiguous()
        order2 = [None, None] if solver_order == 2 else None
        for i, step in enumerate(tqdm(time_range, desc='Decoding image', total=total_steps)):
            index = total_steps - i - 1
            ts = torch.full((x_latent.shape[0],), int(step), device=x_latent.device, dtype=torch.long)
            x_dec, _ = self.loop_step(order2, x_dec, cond, ts, index, int(step),
                                      unconditional_guidance_scale=unconditional_guidance_scale,
                                      unconditional_conditioning=unconditional_conditioning, seeds=seeds)
            if callback:
                callback(i)
        return x_dec

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None, seeds=None):
        """x0 noised to the level of DDIM index `t` (ddim.py:304-317): fast, not an exact inversion.  `t` indexes the DDIM
        tables, one entry per sample; the coefficients are rounded where the reference rounds them (fp32 ddim_alphas, then
        an fp32 sqrt; fp32 sqrt(1 - ddim_alphas)).  `seeds` (one per sample, instead of `noise`): the draw is stream
        STREAM_ENCODE of each sample's seed."""
        if use_original_steps:
            raise NotImplementedError("only the DDIM-subsequence sampling path the scripts use")
        if seeds is not None:
            if noise is not None:
                raise ValueError("stochastic_encode: give `noise` or `seeds`, not both")
            noise = ops.randn_clips(ops.clip_seeds(seeds, x0.shape[0], "stochastic_encode: seeds"), tuple(x0.shape), STREAM_ENCODE)
        if noise is None:
            noise = torch.randn_like(x0)
        idx = [int(v) for v in (t.reshape(-1).tolist() if torch.is_tensor(t) else np.atleast_1d(t).tolist())]
        assert len(idx) == x0.shape[0], "one DDIM index per sample"
        sqrt_a = torch.sqrt(torch.as_tensor(self.ddim_alphas, dtype=torch.float32))
        xs, nz = x0.to(torch.float32).contiguous(), noise.to(torch.float32).contiguous()
        coef = lambda i: dict(sqrt_ac=float(sqrt_a[i]), sqrt_1m_ac=float(self.ddim_sqrt_one_minus_alphas[i]))
        if len(set(idx)) == 1:
            return ops.ddim_blend(None, xs, nz, None, **coef(idx[0]))
        out = torch.empty_like(xs)
        for k, i in enumerate(idx):
            ops.ddim_blend(None, xs[k:k + 1], nz[k:k + 1], None, out=out[k:k + 1], **coef(i))
        return out
