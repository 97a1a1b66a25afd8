"""Shared pieces of tests/test_multistep_cpu.py and tests/test_gpu_multistep.py: the analytic Gaussian problem of
tests/multistep_ref.py as a stub model the real DDIMSampler runs on, and the float64 twin of such a run."""
import numpy as np
import torch

import multistep_ref as ref


class GaussianModel:
    """What DDIMSampler reads of a model, for data N(0, 0.7^2): the schedule buffers in fp32 and `apply_model`, the closed-form
    optimal prediction (E[v | x_t] = coef[t] x_t; for "eps" E[eps | x_t] = b_t / var_t x_t) with an fp32 coefficient."""

    def __init__(self, device="cpu", zero_snr=True, rescale=True, parameterization="v"):
        ac, sa = ref.schedule(zero_snr=zero_snr, rescale=rescale)
        T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=device)
        self.ac64, self.scale64 = ac, sa
        self.device, self.num_timesteps, self.parameterization, self.use_dynamic_rescale = torch.device(device), 1000, parameterization, rescale
        ac_prev = np.append(1.0, ac[:-1])
        self.betas = T(1.0 - ac / ac_prev)
        self.alphas_cumprod, self.alphas_cumprod_prev = T(ac), T(ac_prev)
        self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod = T(np.sqrt(ac)), T(np.sqrt(1.0 - ac))
        self.scale_arr = T(sa)
        if parameterization == "v":
            coef = ref.v_coef(ac, sa)
        else:
            coef = np.sqrt(1.0 - ac) / (ac * (sa * ref.DATA_STD) ** 2 + 1.0 - ac)
        self.coef = np.asarray(coef, dtype=np.float32)               # host table: no device read in the loop
        self.calls = 0

    def apply_model(self, x, t, c, **kw):
        self.calls += 1
        return x * float(self.coef[int(t[0])])


def x_T(shape=(1, 4, 4, 16, 16), seed=0):
    return np.random.default_rng(seed).standard_normal(int(np.prod(shape))).reshape(shape)


def run_sampler(model, S, order, xT, eta=0.0, **kw):
    """The real sampler on the current backend -> (final latent, sampler).  The module-level noise hook is at its own
    definition for the run: other tests substitute it, and not all of them put it back."""
    from tooncrafter_amd.lvdm import ddim
    s = ddim.DDIMSampler(model)
    x = torch.tensor(xT, dtype=torch.float32, device=model.device)
    old = ddim.noise_like
    ddim.noise_like = lambda shape, device, repeat=False: torch.randn(shape, device=device)
    try:
        out, _ = s.sample(S=S, batch_size=x.shape[0], shape=tuple(x.shape[1:]), conditioning=None, verbose=False, eta=eta,
                          timestep_spacing="uniform_trailing", x_T=x, solver_order=order, **kw)
    finally:
        ddim.noise_like = old
    return out, s


def rms_to_exact(out, xT, model, sampler):
    exact = ref.exact_end(xT, model.ac64, model.scale64, int(sampler.ddim_timesteps[0]))
    return float(np.sqrt(np.mean((out.double().cpu().numpy() - exact) ** 2)))


def f64_twin(model, sampler, xT, order):
    """The run `sampler` just made (its schedule is still in place), in float64 on the very scalars the step kernel was given:
    what separates a device run from this is the kernel's fp32 arithmetic alone."""
    steps, coef, h_prev = [], [], None
    for index in range(len(sampler.ddim_timesteps) - 1, -1, -1):
        t = int(sampler.ddim_timesteps[index])
        sc = dict(sampler.step_scalars(index, t))
        corr, h_prev = sampler.multistep_corr(index, t, h_prev)
        steps.append((sc, corr))
        coef.append(float(model.coef[t]))
    return ref.trajectory(xT, steps, order, coef)
