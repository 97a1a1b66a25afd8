"""Second-order multistep sampling (`solver_order=2`, tc_ddim_step_ms) without a GPU: order 1 stays the path it was, bit for
bit; the host scalar `multistep_corr` against the float64 statement (tests/multistep_ref.py); convergence of the real
sampler on the analytic Gaussian problem; the noise draws; keyword validation and the callers.  The kernel itself is
covered by tests/test_gpu_multistep.py.

Analytic problem, eta = 0, RMS error to the exact solution, real DDIMSampler on the emulated contract (fp32), measured here:
    S    DDIM        2M          ratio
    10   1.170e-01   6.846e-02   0.585
    20   6.398e-02   2.382e-02   0.372
    50   2.754e-02   5.987e-03   0.217
"""
import math

import numpy as np
import pytest
import torch

import multistep_cases as mc
import multistep_ref as ref
import plain_family_cases as pf
from conftest import load_golden, rel_l2
from emu_multistep_ops import EmuMultistepOps


@pytest.fixture(autouse=True)
def own_noise_like(monkeypatch):
    """The module-level hook at its own definition: other tests substitute it, and not all of them put it back."""
    from tooncrafter_amd.lvdm import ddim
    monkeypatch.setattr(ddim, "noise_like", lambda shape, device, repeat=False: torch.randn(shape, device=device))


@pytest.fixture(scope="module")
def emu():
    from tooncrafter_amd import ops
    be = EmuMultistepOps(round_bf16=True)
    prev = ops.set_backend(be)
    yield be
    ops.set_backend(prev)


@pytest.fixture(scope="module")
def tiny_model(tiny_sd, emu):
    from test_host_logic_cpu import _tiny_model_cfg
    from tooncrafter_amd.utils import instantiate_from_config
    model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    model.load_state_dict(tiny_sd, strict=False)
    return model


# ------------------------------------------------------------------------------------------------ 1. order 1 did not move

def _with_keyword(cls, **extra):
    """`cls`, with `extra` added to every `sample` call."""
    class WithKeyword(cls):
        def sample(self, *a, **kw):
            return super().sample(*a, **{**kw, **extra})
    return WithKeyword


def _golden_run(name, tiny_model, extra):
    """The recorded trajectory `name` as the existing CPU test of that fixture runs it, with `extra` added to the sampler's
    `sample` call -> (final, [pred_x0], bound check)."""
    from test_pinned_cpu import _run, _sample_kw
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWay
    T = torch.from_numpy
    if name == "ddim_eps_tiny.npz":
        g = load_golden(name)
        model = pf.tiny_pipeline(parameterization="eps", rescale_betas_zero_snr=False)
        out, x0s = pf.run_sampler(model, _with_keyword(DDIMSampler, **extra), g, "a_")
        return out, x0s, (g["a_samples"], g["a_pred_x0"])
    if name == "ddim_pinned_tiny.npz":
        g = load_golden(name)
        kw = _sample_kw(g, mask=T(g["mask_frame"]).bool(), x0=T(g["x0"]), **extra)
        (out, _), _, x0s = _run(tiny_model, g, "a_", DDIMSampler, lambda s: s.sample(**kw))
        return out, x0s, (g["a_samples"], g["a_pred_x0"])
    g = load_golden(name)
    three = name == "ddim_mc_tiny.npz"
    cond = {"c_crossattn": [T(g["cond"])], "c_concat": [T(g["c_concat"])]}
    uc = {"c_crossattn": [T(g["uncond"])], "c_concat": [T(g["c_concat"])]}
    uc_img = {"c_crossattn": [T(g["uncond_img"])], "c_concat": [T(g["c_concat"])]} if three else None
    from tooncrafter_amd.lvdm import ddim as my_ddim
    it, old, x0s = iter(T(g["noises"])), my_ddim.noise_like, []
    my_ddim.noise_like = lambda shape, device, repeat=False: next(it)
    try:
        out, _ = (ThreeWay if three else DDIMSampler)(tiny_model).sample(
            S=4 if three else 5, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False,
            unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0, cfg_img=float(g["cfg_img"]) if three else None,
            mask=None, x0=None, fs=T(g["fs"]), timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=T(g["x_T"]),
            unconditional_conditioning_img_nonetext=uc_img, img_callback=lambda p, i: x0s.append(p.clone()), **extra)
    finally:
        my_ddim.noise_like = old
    return out, x0s, (g["samples"], g["pred_x0"])


@pytest.mark.parametrize("name", ["ddim_tiny.npz", "ddim_eps_tiny.npz", "ddim_mc_tiny.npz", "ddim_pinned_tiny.npz"])
def test_order_one_is_the_path_it_was(tiny_model, emu, name):
    """`solver_order=1` passed explicitly: the reference's recorded trajectory within the bound of that fixture's own CPU test
    (0.15), bit-equal to a run without the keyword, and tc_ddim_step_ms is not called at all."""
    emu.ms_calls.clear()
    with torch.no_grad():
        plain, plain_x0s, _ = _golden_run(name, tiny_model, {})
        out, x0s, (want, want_x0s) = _golden_run(name, tiny_model, dict(solver_order=1))
    assert emu.ms_calls == []
    assert torch.equal(out, plain) and len(x0s) == len(plain_x0s) == len(want_x0s)
    assert all(torch.equal(a, b) for a, b in zip(x0s, plain_x0s))
    errs = [rel_l2(p, torch.from_numpy(want_x0s[i])) for i, p in enumerate(x0s)]
    final = rel_l2(out, torch.from_numpy(want))
    assert max(errs) < 0.15 and final < 0.15, (name, errs, final)


# ------------------------------------------------------------------------------------------------ 2. the host scalar

def _tables(s, index, t):
    """What the float64 statement takes, from the sampler's schedule tables (inputs of the formula, not its results)."""
    if s.model.parameterization == "v":
        sqrt_ac, sqrt_1m_ac = float(s._sqrt_ac[t]), float(s._sqrt_1m_ac[t])
    else:
        sqrt_ac, sqrt_1m_ac = math.sqrt(float(s.ddim_alphas[index])), float(s.ddim_sqrt_one_minus_alphas[index])
    rho = float(s.ddim_scale_arr_prev[index]) / float(s.ddim_scale_arr[index]) if s.model.use_dynamic_rescale else 1.0
    return sqrt_ac, sqrt_1m_ac, float(s.ddim_alphas_prev[index]), float(s.ddim_sigmas[index]), rho


@pytest.mark.parametrize("par", ["v", "eps"])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("rescale,zero_snr", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("S", [5, 20, 50])
def test_multistep_corr_against_the_float64_statement(S, rescale, zero_snr, eta, par):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    s = DDIMSampler(mc.GaussianModel(zero_snr=zero_snr, rescale=rescale, parameterization=par))
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=eta, verbose=False)
    h_prev = h_prev_ref = None
    nonzero = 0
    for i, index in enumerate(range(S - 1, -1, -1)):
        t = int(s.ddim_timesteps[index])
        corr, h = s.multistep_corr(index, t, h_prev)
        want, want_h = ref.corr_h(*_tables(s, index, t), h_prev_ref, index)
        assert type(corr) is float and corr == float(np.float32(corr)), "one fp32 value"
        assert corr == pytest.approx(want, rel=1e-6, abs=0.0), (index, corr, want)
        if math.isfinite(want_h):
            assert h == pytest.approx(want_h, rel=1e-12) and h > 0
        else:
            assert h == want_h and zero_snr and i == 0               # alpha_t = 0: only the zero-terminal-SNR start
        after_zero = i == 1 and zero_snr
        if i == 0 or index == 0 or after_zero:
            assert corr == 0.0, (index, corr)
        else:
            assert corr != 0.0 and abs(corr) < 1.0, (index, corr)
            nonzero += 1
        h_prev, h_prev_ref = h, want_h
    assert nonzero == S - 2 - (1 if zero_snr else 0)


# ------------------------------------------------------------------------------------------------ 3. convergence

@pytest.fixture(scope="module")
def gaussian_errors(emu):
    """RMS error to the exact solution of the real sampler at eta = 0, {(S, order): error}: computed once."""
    model, xT = mc.GaussianModel(), mc.x_T()
    errs = {}
    for S in (10, 20, 50):
        for order in (1, 2):
            emu.ms_calls.clear()
            out, s = mc.run_sampler(model, S, order, xT)
            errs[S, order] = mc.rms_to_exact(out, xT, model, s)
            assert len(emu.ms_calls) == (S if order == 2 else 0)
            if order == 2:                       # first step, the step after alpha_t = 0 and the last step are first order
                corrs = [c for _, c in emu.ms_calls]
                assert corrs[0] == corrs[1] == corrs[-1] == 0.0 and all(c != 0.0 for c in corrs[2:-1])
                assert [h for h, _ in emu.ms_calls] == [False] + [True] * (S - 1)
    return errs


def test_stub_is_the_documented_problem(gaussian_errors):
    for S, (ddim, _) in ref.TABLE.items():
        print(f"S {S}: DDIM {gaussian_errors[S, 1]:.3e} (documented {ddim:.2e}), 2M {gaussian_errors[S, 2]:.3e}, "
              f"ratio {gaussian_errors[S, 2] / gaussian_errors[S, 1]:.3f}")
    for S, (ddim, _) in ref.TABLE.items():
        assert gaussian_errors[S, 1] == pytest.approx(ddim, rel=0.02), S


def test_second_order_converges_faster(gaussian_errors):
    e = gaussian_errors
    assert e[10, 2] <= 0.7 * e[10, 1]
    assert e[20, 2] <= 0.5 * e[20, 1]
    assert e[50, 2] <= 0.3 * e[50, 1]
    assert e[20, 2] < e[50, 1]


# ------------------------------------------------------------------------------------------------ 4. noise draws

def _seeded_kw(**kw):
    g, T = load_golden("ddim_pinned_tiny.npz"), torch.from_numpy
    cond = {"c_crossattn": [T(g["cond"])], "c_concat": [T(g["c_concat"])]}
    uc = {"c_crossattn": [T(g["uncond"])], "c_concat": [T(g["c_concat"])]}
    base = dict(S=5, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False, unconditional_conditioning=uc,
                fs=T(g["fs"]), unconditional_guidance_scale=7.5, eta=1.0, timestep_spacing="uniform_trailing",
                guidance_rescale=0.7, seeds=[0xC0FFEE])
    base.update(kw)
    return base, g


@pytest.mark.parametrize("eta", [1.0, 0.0])
@pytest.mark.parametrize("three_way", [False, True])
def test_seeded_order_two_run_uses_the_draws_of_order_one(tiny_model, emu, eta, three_way):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWay
    kw, g = _seeded_kw(eta=eta)
    T = torch.from_numpy
    kw.update(mask=T(g["mask_frame"]), x0=T(g["x0"]))
    if three_way:
        kw.update(cfg_img=3.0, unconditional_conditioning_img_nonetext={"c_crossattn": [T(g["uncond_img"])],
                                                                        "c_concat": [T(g["c_concat"])]})
    cls = ThreeWay if three_way else DDIMSampler
    logs, outs = [], []
    rng = torch.get_rng_state()
    for order in (1, 2):
        emu.draws.clear()
        emu.ms_calls.clear()
        with torch.no_grad():
            outs.append(cls(tiny_model).sample(**kw, solver_order=order)[0])
        logs.append(list(emu.draws))
        assert len(emu.ms_calls) == (5 if order == 2 else 0)
    assert torch.equal(torch.get_rng_state(), rng)
    assert logs[0] == logs[1] and len(logs[0]) == (11 if eta else 6)        # x_T, then q_sample (+ the step's draw) per step
    assert torch.isfinite(outs[1]).all() and not torch.equal(outs[0], outs[1])


def test_unseeded_order_two_run_draws_like_order_one(emu):
    """The draw-and-drop at sigma = 0 included: the torch generator ends where the order-1 run leaves it."""
    model, xT = mc.GaussianModel(), mc.x_T((1, 4, 2, 4, 4))
    states = []
    for order, eta in ((1, 0.0), (2, 0.0), (1, 1.0), (2, 1.0)):
        torch.manual_seed(5)
        mc.run_sampler(model, 5, order, xT, eta=eta)
        states.append(torch.get_rng_state())
    torch.manual_seed(5)
    for _ in range(5):
        torch.randn(1, 4, 2, 4, 4)
    assert all(torch.equal(s, torch.get_rng_state()) for s in states)


def test_partial_runs_start_and_end_first_order(emu):
    model, xT = mc.GaussianModel(), mc.x_T((1, 4, 2, 4, 4))
    emu.ms_calls.clear()
    mc.run_sampler(model, 10, 2, xT, timesteps=7)                     # table positions 5 .. 0, alpha_t > 0 throughout
    corrs = [c for _, c in emu.ms_calls]
    assert len(corrs) == 6 and corrs[0] == 0.0 and corrs[-1] == 0.0 and all(c != 0.0 for c in corrs[1:-1])
    assert [h for h, _ in emu.ms_calls] == [False] + [True] * 5
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    s = DDIMSampler(model)
    s.make_schedule(10, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    emu.ms_calls.clear()
    x = torch.tensor(xT, dtype=torch.float32)
    two = s.decode(x, None, 4, solver_order=2)
    corrs = [c for _, c in emu.ms_calls]
    assert len(corrs) == 4 and corrs[0] == 0.0 and corrs[-1] == 0.0 and corrs[1] != 0.0 and corrs[2] != 0.0
    emu.ms_calls.clear()
    one = s.decode(x, None, 4)
    assert emu.ms_calls == [] and not torch.equal(one, two)
    assert not hasattr(s, "hist") and not any("hist" in k or "h_prev" in k for k in vars(s))     # nothing kept on the sampler


def test_reduced_step_counts_are_finite_at_eta_one(emu):
    """The alpha_t = 0 start at eta = 1: 1 - a_prev - sigma^2 is 0 up to a rounding and the reference's sqrt of it is NaN at
    S = 20 and 25 among others.  step_scalars clamps the radicand: the reference's bits wherever those are finite, 0 where
    they are not, and both orders run at the step counts a second-order run is for."""
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    model, xT = mc.GaussianModel(), mc.x_T((1, 4, 2, 4, 4))
    s = DDIMSampler(model)
    was_nan = []
    for S in range(2, 61):                       # from 61 steps on the trailing table repeats a timestep and sigma itself is NaN
        s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
        for index in range(S):
            a_prev = torch.tensor(float(s.ddim_alphas_prev[index]), dtype=torch.float32)
            sigma = torch.tensor(float(s.ddim_sigmas[index]), dtype=torch.float32)
            want = float((1. - a_prev - sigma ** 2).sqrt())                       # ddim.py:271
            got = s.step_scalars(index, int(s.ddim_timesteps[index]))["dir_coef"]
            if math.isnan(want):
                was_nan.append(S)
                assert got == 0.0 and float(1. - a_prev - sigma ** 2) > -1e-6, (S, index)
            else:
                assert got == want, (S, index)
    assert 20 in was_nan and 25 in was_nan and 50 not in was_nan
    for order in (1, 2):
        out, _ = mc.run_sampler(model, 20, order, xT, eta=1.0)
        assert torch.isfinite(out).all(), order


# ------------------------------------------------------------------------------------------------ 5. keywords and callers

def test_solver_order_is_validated_before_any_launch(emu):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWay
    model, xT = mc.GaussianModel(), mc.x_T((1, 4, 2, 4, 4))
    model.calls = 0
    emu.ms_calls.clear()
    x = torch.tensor(xT, dtype=torch.float32)
    for cls in (DDIMSampler, ThreeWay):
        s = cls(model)
        s.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
        for bad in (0, 3, -1, 2.5, "2", None, True):
            with pytest.raises(ValueError):
                s.sample(S=5, batch_size=1, shape=(4, 2, 4, 4), verbose=False, x_T=x, solver_order=bad)
            with pytest.raises(ValueError):
                s.ddim_sampling(None, (1, 4, 2, 4, 4), x_T=x, verbose=False, solver_order=bad)
            with pytest.raises(ValueError):
                s.p_sample_ddim(x, None, torch.tensor([999]), index=4, solver_order=bad)
            with pytest.raises(ValueError):
                s.decode(x, None, 2, solver_order=bad)
    assert model.calls == 0 and emu.ms_calls == []


def test_plan_order_reaches_the_sampler(tiny_model, emu):
    from tooncrafter_amd import clip as pipeline
    kw, g = _seeded_kw()
    T = torch.from_numpy
    cond = pipeline.Conditions(kw["conditioning"], kw["unconditional_conditioning"], None, None, T(g["fs"]))
    shape = [1, 4, 4, 8, 8]
    assert pipeline.SamplingPlan().order == 1
    plan = lambda **k: pipeline.SamplingPlan(steps=4, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=[7], **k)
    emu.ms_calls.clear()
    with torch.no_grad():
        one = pipeline.sample(tiny_model, cond, plan(), shape)
        assert emu.ms_calls == []
        two = pipeline.sample(tiny_model, cond, plan(order=2), shape)
        assert [h for h, _ in emu.ms_calls] == [False, True, True, True] and emu.ms_calls[-1][1] == 0.0
        via_kwargs = pipeline.sample(tiny_model, cond, plan(extra=dict(solver_order=2)), shape)
    assert torch.equal(via_kwargs, two) and not torch.equal(one, two)
    with pytest.raises(ValueError):
        pipeline.sample(tiny_model, cond, plan(order=3), shape)


def test_image_guided_synthesis_maps_the_keyword(monkeypatch):
    import inspect
    from tooncrafter_amd import clip as pipeline
    seen = []
    monkeypatch.setattr(pipeline, "synthesize", lambda model, videos, shape, *, plan, **kw: seen.append(plan) or "clips")
    assert inspect.signature(pipeline.image_guided_synthesis).parameters["solver_order"].default == 1
    assert pipeline.image_guided_synthesis(None, ["p"], None, [1, 4, 4, 8, 8], ddim_steps=20, solver_order=2) == "clips"
    assert pipeline.image_guided_synthesis(None, ["p"], None, [1, 4, 4, 8, 8]) == "clips"     # an unmodified reference call
    assert [p.order for p in seen] == [2, 1] and seen[0].steps == 20 and "solver_order" not in seen[0].extra


# ------------------------------------------------------------------------------------------------ the ABI and the bindings

def test_entry_points_are_declared_exported_and_bound():
    import ctypes
    from tooncrafter_amd import _lib, torch_ops
    from tooncrafter_amd.ops import HipOps
    assert _lib.TC_ABI_VERSION == 14
    assert [f[0] for f in _lib.TcDdimMsParams._fields_] == ["base", "x0_hist", "corr"]
    assert _lib.TcDdimMsParams.x0_hist.offset == ctypes.sizeof(_lib.TcDdimParams)
    lib = _lib.load()
    for name in ("tc_ddim_step_ms", "tc_ddim_step_ms_eps"):
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.TcDdimMsParams), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        assert getattr(lib, name)(None, None, 0, None) == -1
    assert callable(HipOps.ddim_step_ms) and torch_ops.TorchLibOps.ddim_step_ms is not HipOps.ddim_step_ms
    t = torch_ops.load()
    lat = torch.empty(2, 4, 16, 40, 64, dtype=torch.float32, device="meta")
    for op in (t.ddim_step_ms, t.ddim_step_ms_eps):
        for hist in (None, lat):
            xp, x0 = op(lat, lat, lat, None, None, hist, 0.25, 7.5, 7.5, 0.7, 0.6, 0.8, 0.7, 0.5, 0.0, 0.98)
            assert xp.shape == x0.shape == lat.shape and xp.dtype == torch.float32 and xp.device.type == "meta"
    with pytest.raises((RuntimeError, NotImplementedError)):              # no CPU kernel is registered: no fallback
        z = torch.zeros(1, 8)
        t.ddim_step_ms(z, z, None, None, None, z, 0.25, 1.0, 1.0, 0.0, 0.6, 0.8, 0.7, 0.5, 0.0, 1.0)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """The documented refusals return before the launch, so they can be exercised on host pointers."""
    import ctypes
    from tooncrafter_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    ws = (ctypes.c_double * 256)()

    def rc(fn="tc_ddim_step_ms", corr=0.5, hist=base + 512, **kw):
        p = _lib.TcDdimMsParams()
        b = p.base
        b.x, b.e_cond, b.x_prev, b.pred_x0, b.b, b.n = base, base + 128, base + 256, base + 384, 1, 32
        b.sqrt_ac, b.sqrt_1m_ac, b.sqrt_a_prev, b.dir_coef, b.x0_rescale = 0.6, 0.8, 0.7, 0.5, 1.0
        for k, v in kw.items():
            setattr(b, k, v)
        p.x0_hist, p.corr = hist, corr
        return getattr(lib, fn)(ctypes.byref(p), ws, ctypes.sizeof(ws), None)
    assert rc(corr=float("nan")) == -1 and rc(corr=float("inf")) == -1 and rc(corr=float("nan"), hist=None) == -1
    assert rc(pred_x0=base + 512 + 4) == -1 and rc(pred_x0=base + 512 - 4) == -1       # pred_x0 over the history, not exactly
    assert rc(x_prev=base + 512) == -1 and rc(x_prev=base + 512 + 124) == -1            # x_prev over the history
    assert rc(x=None) == -1 and rc(n=1) == -1 and rc(b=0) == -1
    assert rc("tc_ddim_step_ms_eps", sqrt_ac=0.0) == -1
    assert lib.tc_ddim_step_ms(ctypes.byref(_lib.TcDdimMsParams()), None, 0, None) == -1
