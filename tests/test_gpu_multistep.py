"""tc_ddim_step_ms / tc_ddim_step_ms_eps on the MI355X: the kernel against the float64 statement (tests/multistep_ref.py), its
first-order case against tc_ddim_step bit for bit and both against bits recorded before the two were one kernel, the history in place, the refusals, the two bindings, and the samplers'
`solver_order=2` on the device -- the analytic Gaussian problem of tests/test_multistep_cpu.py and the tiny pipeline.

Measured on the MI355X (the tests print them): kernel vs float64, worst rel-L2 over all cases 4.17e-07 (bound 1e-4);
analytic run S = 10, RMS deviation from the float64 twin: order 1 8.17e-08, order 2 1.00e-07 (bound: 4 x order 1);
tiny pipeline at order 2 vs the emulated contract in fp32: worst pred_x0 8.34e-02, final 7.48e-02 (bounds 0.133 / 0.108)."""
import hashlib
import itertools

import numpy as np
import pytest
import torch

import multistep_cases as mc
import multistep_ref as ref
from conftest import load_golden, rel_l2
from emu_multistep_ops import EmuMultistepOps
from test_gpu_models import _tiny_pipeline, _with_backend
from test_gpu_ops import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
SC = dict(sqrt_ac=0.6, sqrt_1m_ac=0.8, sqrt_a_prev=0.7, dir_coef=0.5, x0_rescale=0.98)
# (2, 420): n = 4 * 3 * 5 * 7; (2, 4, 16, 40, 64): the clip's latent at B = 2, several grid strides.  n = 421: no 16-byte
# sample base at b = 2 (the scalar kernel), the vector body plus its one-element tail at b = 1.
SHAPES = [(2, 4, 3, 5, 7), (2, 4, 16, 40, 64), (2, 421), (1, 421)]


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


def draw_operands():
    out = {}
    for shape in SHAPES:
        g = torch.Generator().manual_seed(70 + len(shape) + shape[0])
        out[shape] = tuple(torch.randn(*shape, generator=g) for _ in range(6))
    return out


@pytest.fixture(scope="module")
def operands():
    """x, e_cond, e_uncond, e_uncond_img, noise, hist per shape, on the CPU: drawn once, never written."""
    return draw_operands()


def _case(operands, shape, guidance, noise):
    x, ec, eu, ei, nz, hist = operands[shape]
    return x, ec, (eu if guidance else None), (ei if guidance == 3 else None), (nz if noise else None), hist


def _kw(guidance, resc, noise, par):
    kw = dict(SC, cfg_scale=7.5 if guidance else 1.0, guidance_rescale=resc, sigma=0.3 if noise else 0.0, parameterization=par)
    if guidance == 3:
        kw["cfg_img"] = 3.0
    return kw


def _dev(t):
    return None if t is None else t.to(DEV)


# tests/golden/ddim_step_bits.npz (make_ddim_step_bits.py): what HipOps.ddim_step returned for these operands BEFORE the first-order
# kernels were folded into the one apply kernel.  The small shapes are stored in full, the clip-sized one as a SHA-256.
BITS_HASHED = (2, 4, 16, 40, 64)
BITS_COMBOS = list(itertools.product((0, 2, 3), (0.0, 0.7), (False, True)))


def bits_key(shape, par, guidance, resc, noise):
    return f"{par}.{'x'.join(map(str, shape))}.g{guidance}.r{resc}.n{int(noise)}"


def bits_digest(x_prev, pred_x0):
    h = hashlib.sha256(x_prev.cpu().numpy().tobytes())
    h.update(pred_x0.cpu().numpy().tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


@pytest.mark.parametrize("par", ["v", "eps"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_float64_statement(hip, operands, shape, par):
    worst = 0.0
    for guidance, resc, noise, corr in itertools.product((0, 2, 3), (0.0, 0.7), (False, True), (-0.35, 0.8)):
        x, ec, eu, ei, nz, hist = _case(operands, shape, guidance, noise)
        kw = _kw(guidance, resc, noise, par)
        xp, x0 = hip.ddim_step_ms(_dev(x), _dev(ec), _dev(eu), _dev(nz), _dev(hist), corr=corr, e_uncond_img=_dev(ei), **kw)
        rp, r0 = ref.step(x.numpy(), ec.numpy(), None if eu is None else eu.numpy(), None if nz is None else nz.numpy(),
                          hist.numpy(), corr=corr, e_uncond_img=None if ei is None else ei.numpy(), **kw)
        what = f"{par} {shape} guidance {guidance} rescale {resc} noise {noise} corr {corr}"
        check(xp.cpu(), torch.from_numpy(rp), "ms x_prev " + what, f32=True)
        check(x0.cpu(), torch.from_numpy(r0), "ms pred_x0 " + what, f32=True)
        worst = max(worst, rel_l2(xp.cpu(), torch.from_numpy(rp)), rel_l2(x0.cpu(), torch.from_numpy(r0)))
        # the term is really there: without the history the result is another
        assert rel_l2(hip.ddim_step_ms(_dev(x), _dev(ec), _dev(eu), _dev(nz), None, corr=corr, e_uncond_img=_dev(ei), **kw)[0].cpu(),
                      torch.from_numpy(rp)) > 1e-2
    print(f"{par} {shape}: worst rel-L2 to the float64 statement {worst:.3e}")


@pytest.mark.parametrize("par", ["v", "eps"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_first_order_case_is_tc_ddim_step_bit_for_bit(hip, operands, shape, par):
    for guidance, resc, noise in itertools.product((0, 2, 3), (0.0, 0.7), (False, True)):
        x, ec, eu, ei, nz, hist = (_dev(t) for t in _case(operands, shape, guidance, noise))
        kw = _kw(guidance, resc, noise, par)
        xp, x0 = hip.ddim_step(x, ec, eu, nz, e_uncond_img=ei, **kw)
        for h, corr in ((None, 0.8), (hist, 0.0), (None, 0.0), (hist, -0.0)):
            mp, m0 = hip.ddim_step_ms(x, ec, eu, nz, h, corr=corr, e_uncond_img=ei, **kw)
            assert torch.equal(mp, xp) and torch.equal(m0, x0), (shape, par, guidance, resc, noise, h is None, corr)
        assert hip.ddim_step_ms(x, ec, eu, nz, None, corr=0.0, e_uncond_img=ei, want_x0=False, **kw)[1] is None


@pytest.fixture(scope="module")
def step_bits():
    return load_golden("ddim_step_bits.npz")


@pytest.mark.parametrize("par", ["v", "eps"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_first_order_step_keeps_the_recorded_bits(hip, operands, step_bits, shape, par):
    """`ddim_step` on both bindings, and `ddim_step_ms` without a history or with corr 0, against outputs recorded from the
    separate first-order kernels this project had: the merged kernel is anchored outside itself."""
    from tooncrafter_amd.torch_ops import TorchLibOps
    tlib = TorchLibOps()
    for guidance, resc, noise in BITS_COMBOS:
        x, ec, eu, ei, nz, hist = (_dev(t) for t in _case(operands, shape, guidance, noise))
        kw = _kw(guidance, resc, noise, par)
        key = bits_key(shape, par, guidance, resc, noise)
        results = {"ctypes ddim_step": hip.ddim_step(x, ec, eu, nz, e_uncond_img=ei, **kw),
                   "custom-op ddim_step": tlib.ddim_step(x, ec, eu, nz, e_uncond_img=ei, **kw),
                   "ddim_step_ms(None, 0.8)": hip.ddim_step_ms(x, ec, eu, nz, None, corr=0.8, e_uncond_img=ei, **kw),
                   "ddim_step_ms(hist, 0.0)": hip.ddim_step_ms(x, ec, eu, nz, hist, corr=0.0, e_uncond_img=ei, **kw)}
        for what, (xp, x0) in results.items():
            if shape == BITS_HASHED:
                assert np.array_equal(bits_digest(xp, x0), step_bits[key + ".sha256"]), (what, key)
            else:
                assert torch.equal(xp.cpu(), torch.from_numpy(step_bits[key + ".x_prev"])), (what, key)
                assert torch.equal(x0.cpu(), torch.from_numpy(step_bits[key + ".pred_x0"])), (what, key)
        for be in (hip, tlib):
            xp, none = be.ddim_step(x, ec, eu, nz, e_uncond_img=ei, want_x0=False, **kw)
            assert none is None
            if shape != BITS_HASHED:
                assert torch.equal(xp.cpu(), torch.from_numpy(step_bits[key + ".x_prev"])), ("want_x0=False", key)


@pytest.mark.parametrize("shape", [(2, 4, 3, 5, 7), (2, 421)], ids=lambda s: "x".join(map(str, s)))
def test_history_in_place_and_refusals(hip, operands, shape):
    from tooncrafter_amd._lib import TooncrafterHipError
    x, ec, eu, ei, nz, hist = (_dev(t) for t in _case(operands, shape, 2, True))
    kw = _kw(2, 0.7, True, "v")
    xp, x0 = hip.ddim_step_ms(x, ec, eu, nz, hist, corr=0.8, **kw)
    h = hist.clone()
    ip, i0 = hip.ddim_step_ms(x, ec, eu, nz, h, corr=0.8, pred_x0=h, **kw)
    assert i0 is h and torch.equal(ip, xp) and torch.equal(h, x0) and not torch.equal(h, hist)
    # argument checks: nothing is launched, the would-be result keeps its contents
    numel = x.numel()
    buf = torch.full((numel + 4,), 7.0, device=DEV)
    over_hist, over_pred = buf[:numel].view(x.shape), buf[4:].view(x.shape)
    for bad in (dict(x0_hist=over_hist, pred_x0=over_pred, corr=0.8), dict(x0_hist=over_pred, pred_x0=over_hist, corr=0.0),
                dict(x0_hist=hist, pred_x0=None, corr=float("nan")), dict(x0_hist=None, pred_x0=None, corr=float("inf"))):
        with pytest.raises(TooncrafterHipError):
            hip.ddim_step_ms(x, ec, eu, nz, bad["x0_hist"], corr=bad["corr"], pred_x0=bad["pred_x0"], **kw)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    with pytest.raises(ValueError):
        hip.ddim_step_ms(x, ec, eu, nz, hist.reshape(-1), corr=0.8, **kw)


@pytest.mark.parametrize("par", ["v", "eps"])
def test_both_bindings_give_the_same_bits(hip, operands, par):
    from tooncrafter_amd.torch_ops import TorchLibOps
    tlib = TorchLibOps()
    for shape, guidance in (((2, 4, 3, 5, 7), 3), ((2, 4, 16, 40, 64), 2), ((2, 421), 0)):
        x, ec, eu, ei, nz, hist = (_dev(t) for t in _case(operands, shape, guidance, True))
        kw = _kw(guidance, 0.7, True, par)
        for h, corr in ((hist, -0.35), (None, 0.0)):
            a = hip.ddim_step_ms(x, ec, eu, nz, h, corr=corr, e_uncond_img=ei, **kw)
            b = tlib.ddim_step_ms(x, ec, eu, nz, h, corr=corr, e_uncond_img=ei, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (shape, par, corr)
        inplace = hist.clone()
        c = tlib.ddim_step_ms(x, ec, eu, nz, inplace, corr=-0.35, e_uncond_img=ei, pred_x0=inplace, **kw)
        a = hip.ddim_step_ms(x, ec, eu, nz, hist, corr=-0.35, e_uncond_img=ei, **kw)
        assert c[1] is inplace and torch.equal(c[0], a[0]) and torch.equal(inplace, a[1])
        assert tlib.ddim_step_ms(x, ec, eu, nz, hist, corr=0.8, e_uncond_img=ei, want_x0=False, **kw)[1] is None


def test_analytic_run_on_the_device(hip):
    """The Gaussian problem at S = 10 through the real sampler on HipOps, against the same run in float64 on the same
    scalars.  Order 1 is the path the project had and so the yardstick: the corrected run may deviate at most 4 x as far (one
    more multiply-add per element with |corr| < 1)."""
    model, xT = mc.GaussianModel(device=DEV), mc.x_T((2, 4, 3, 5, 7), seed=3)
    dev, err = {}, {}
    for order in (1, 2):
        out, s = _with_backend(hip, lambda: mc.run_sampler(model, 10, order, xT))
        twin = mc.f64_twin(model, s, xT, order)
        assert torch.isfinite(out).all()
        dev[order] = float(np.sqrt(np.mean((out.double().cpu().numpy() - twin) ** 2)))
        err[order] = mc.rms_to_exact(out, xT, model, s)
    print(f"analytic run, S = 10: RMS deviation from the float64 twin: order 1 {dev[1]:.3e}, order 2 {dev[2]:.3e}; "
          f"RMS error to the exact solution: order 1 {err[1]:.3e}, order 2 {err[2]:.3e}")
    assert dev[1] > 0.0 and dev[2] <= 4.0 * dev[1]
    assert err[2] <= 0.7 * err[1]


def test_tiny_pipeline_at_order_two(hip, tiny_sd):
    """S = 5, CFG 7.5, rescale 0.7, eta = 1, the ddim_tiny.npz inputs and injected draws, `solver_order=2`: the device run
    against the same run on the emulated contract, within the bound the first-order trajectory test allows against its golden."""
    from tooncrafter_amd.lvdm import ddim as my_ddim
    g = load_golden("ddim_tiny.npz")
    model = _tiny_pipeline(tiny_sd)
    dev = lambda k: torch.from_numpy(g[k]).to(DEV)
    cond = {"c_crossattn": [dev("cond")], "c_concat": [dev("c_concat")]}
    uc = {"c_crossattn": [dev("uncond")], "c_concat": [dev("c_concat")]}
    noises = dev("noises")

    def run(order):
        it, old, x0s = iter(noises), my_ddim.noise_like, []
        my_ddim.noise_like = lambda shape, device, repeat=False: next(it)
        try:
            out, _ = my_ddim.DDIMSampler(model).sample(
                S=5, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False, unconditional_guidance_scale=7.5,
                unconditional_conditioning=uc, eta=1.0, fs=dev("fs"), timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                x_T=dev("x_T"), img_callback=lambda p, i: x0s.append(p.clone()), solver_order=order)
            return out, x0s
        finally:
            my_ddim.noise_like = old

    # The bound is the one the first-order trajectory test allows against its golden, an fp32 run of the reference; the
    # matching statement of an order-2 run is the contract in fp32 between operators (round_bf16=False).  The contract with
    # bf16 rounding between operators carries rounding noise of its own, as large as the device's and amplified alike by
    # CFG 7.5: against it the same device run measured 1.161e-01 (worst pred_x0; already 1.143e-01 at the first one, which no
    # history has touched) and 1.103e-01 (final) -- the two noises add in quadrature, and that reference is not used.
    emu = EmuMultistepOps(round_bf16=False)
    with torch.no_grad():
        out, x0s = _with_backend(hip, lambda: run(2))
        first, _ = _with_backend(hip, lambda: run(1))
        want, want_x0s = _with_backend(emu, lambda: run(2))
    assert [h for h, _ in emu.ms_calls] == [False, True, True, True, True]
    assert [c != 0.0 for _, c in emu.ms_calls] == [False, False, True, True, False]
    assert torch.isfinite(out).all() and len(x0s) == 5 and all(torch.isfinite(p).all() for p in x0s)
    errs = [rel_l2(p, w) for p, w in zip(x0s, want_x0s)]
    final = rel_l2(out, want)
    print("order-2 tiny trajectory, device vs the fp32 contract: pred_x0 rel-L2 per step", [f"{e:.3e}" for e in errs],
          f"final {final:.3e}; order 2 vs order 1 on the device {rel_l2(out, first):.3e}")
    assert max(errs) < 0.133 and final < 0.108
    assert not torch.equal(out, first)
