"""The second-order multistep step (tc_ddim_step_ms, DDIMSampler.multistep_corr) stated in numpy float64 from its formulas,
and the analytic problem it is verified on.  Nothing here reads the product code.

One step.  With e the guided (and rescaled) model output,
    v model:   x0u = sqrt_ac x - sqrt_1m_ac e,    e_t = sqrt_ac e + sqrt_1m_ac x
    eps model: x0u = (x - sqrt_1m_ac e) / sqrt_ac, e_t = e
    pred_x0 = x0u rho                                             (rho = x0_rescale = scale_prev / scale)
    x_prev  = sqrt_a_prev pred_x0 + dir_coef e_t + corr (x0u - hist) + sigma_eta z
The first-order update is linear in x0u with coefficient A = sqrt_a_prev rho - dir_coef sqrt_ac / sqrt_1m_ac (substitute
e_t = (x - sqrt_ac x0u) / sqrt_1m_ac); the 2M rule replaces x0u there by x0u + h / (2 h_prev) (x0u - hist), hence
    corr = A h / (2 h_prev),      h = lambda_prev - lambda_t,     lambda = log(sqrt(alpha) scale / sqrt(1 - alpha)).
corr = 0 on the first step of a run (no h_prev), after a step whose alpha_t = 0 (h_prev infinite) and at DDIM index 0.

The analytic problem.  Data x0 ~ N(0, D^2) per element, D = 0.7; v-prediction; betas "linear" 0.00085 .. 0.012 with the
zero-terminal-SNR rescale; uniform_trailing steps; a dynamic rescale scale_arr = linspace(1.0, 0.7, 1000).  The model is
trained on x_t = a_t (s_t x0) + b_t eps (a = sqrt(alpha_cumprod), b = sqrt(1 - alpha_cumprod), s = scale_arr), so with
d = s_t D and var = a^2 d^2 + b^2 the optimal prediction is E[v | x_t] = a b (1 - d^2) / var * x_t, and the probability-flow
solution from x_T (alpha_T = 0, unit variance) down to the end of a DDIM table is x_T sqrt(a_0^2 (s_end D)^2 + 1 - a_0^2)
with a_0^2 = alphas_cumprod[0] and s_end the scale of the table's lowest timestep (x0_rescale is 1 at index 0).
"""
import math

import numpy as np

DATA_STD = 0.7
# RMS error to the exact solution, eta = 0, 4096 elements, fp64: (first-order DDIM, 2M with a first-order final step)
TABLE = {10: (1.17e-1, 6.85e-2), 20: (6.40e-2, 2.38e-2), 50: (2.75e-2, 5.99e-3)}


def f32(v):
    """The value a float scalar has once it crossed the ABI."""
    return float(np.float32(v))


def log_snr_increment(sqrt_ac, sqrt_1m_ac, a_prev, rho):
    """h of one step, as the log of ONE ratio; +inf for alpha_t = 0."""
    if sqrt_ac == 0.0:
        return math.inf
    return math.log((math.sqrt(a_prev) * rho * sqrt_1m_ac) / (sqrt_ac * math.sqrt(1.0 - a_prev)))


def corr_h(sqrt_ac, sqrt_1m_ac, a_prev, sigma_eta, rho, h_prev, index):
    """(corr, h) in float64.  sqrt_ac / sqrt_1m_ac: the step's sqrt(alpha_t) and eps-noise sigma; a_prev: alpha of the step
    below; sigma_eta: the DDIM noise strength; h_prev: the previous step's h or None."""
    h = log_snr_increment(sqrt_ac, sqrt_1m_ac, a_prev, rho)
    if h_prev is None or not math.isfinite(h_prev) or index == 0:
        return 0.0, h
    dir_coef = math.sqrt(max(1.0 - a_prev - sigma_eta ** 2, 0.0))
    a_coef = math.sqrt(a_prev) * rho - dir_coef * sqrt_ac / sqrt_1m_ac
    return a_coef * h / (2.0 * h_prev), h


def step(x, e_cond, e_uncond, noise, hist, *, corr, cfg_scale, guidance_rescale, sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef,
         sigma, x0_rescale, e_uncond_img=None, cfg_img=None, parameterization="v"):
    """(x_prev, pred_x0) in float64; arrays of shape (b, ...), the scalars at their fp32 values."""
    d = lambda t: None if t is None else np.asarray(t, dtype=np.float64)
    x, ec, eu, ei, nz, hist = d(x), d(e_cond), d(e_uncond), d(e_uncond_img), d(noise), d(hist)
    sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef, sigma, x0_rescale, corr = (f32(v) for v in (sqrt_ac, sqrt_1m_ac, sqrt_a_prev,
                                                                                           dir_coef, sigma, x0_rescale, corr))
    e = ec
    if eu is not None:
        s = f32(cfg_scale)
        if ei is not None:
            e = eu + f32(s if cfg_img is None else cfg_img) * (ei - eu) + s * (ec - ei)
        else:
            e = eu + s * (ec - eu)
        if guidance_rescale > 0:
            ax = tuple(range(1, e.ndim))
            fac = ec.std(axis=ax, ddof=1, keepdims=True) / e.std(axis=ax, ddof=1, keepdims=True)
            g = f32(guidance_rescale)
            e = g * (e * fac) + (1.0 - g) * e
    if parameterization == "v":
        x0u, e_t = sqrt_ac * x - sqrt_1m_ac * e, sqrt_ac * e + sqrt_1m_ac * x
    else:
        x0u, e_t = (x - sqrt_1m_ac * e) / sqrt_ac, e
    x0 = x0u * x0_rescale
    xp = sqrt_a_prev * x0 + dir_coef * e_t
    if hist is not None and corr != 0.0:
        xp = xp + corr * (x0u - hist)
    if nz is not None:
        xp = xp + sigma * nz
    return xp, x0


# ---------------------------------------------------------------------------------------------------- the analytic problem

def schedule(zero_snr=True, rescale=True, n=1000):
    """(alphas_cumprod, scale_arr) of the problem in float64."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, n, dtype=np.float64) ** 2
    root = np.sqrt(np.cumprod(1.0 - betas))
    if zero_snr:
        r0, rT = root[0], root[-1]
        root = (root - rT) * (r0 / (r0 - rT))
    return root ** 2, (np.linspace(1.0, 0.7, n) if rescale else np.ones(n))


def v_coef(ac, scale_arr, data_std=DATA_STD):
    """E[v | x_t] = v_coef[t] x_t."""
    a, b = np.sqrt(ac), np.sqrt(1.0 - ac)
    d2 = (scale_arr * data_std) ** 2
    return a * b * (1.0 - d2) / (a * a * d2 + b * b)


def exact_end(x_T, ac, scale_arr, t_lowest, data_std=DATA_STD):
    """The probability-flow solution at the end of a DDIM table whose lowest timestep is `t_lowest`, from x_T at alpha = 0."""
    return np.asarray(x_T, dtype=np.float64) * math.sqrt(ac[0] * (scale_arr[t_lowest] * data_std) ** 2 + 1.0 - ac[0])


def trailing_timesteps(S, n=1000):
    return np.flip(np.round(np.arange(n, 0, -n / S))).astype(np.int64) - 1


def trajectory(x_T, steps, order, coef):
    """The sampler's loop in float64.  steps: one (scalars, corr) per step, first step first -- `scalars` the keywords of
    `step` at the values the device kernel gets, `corr` this step's (ignored at order 1); coef: the model's E[v | x] factor of
    each step.  -> the final latent."""
    x, hist = np.asarray(x_T, dtype=np.float64), None
    for (sc, corr), c in zip(steps, coef):
        x, x0 = step(x, c * x, None, None, hist if order == 2 else None, corr=corr if order == 2 else 0.0, cfg_scale=1.0,
                     guidance_rescale=0.0, **sc)
        hist = x0
    return x
