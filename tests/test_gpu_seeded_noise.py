"""Per-clip seeds on the MI355X: tc_randn_clips against its numpy restatement (tests/philox_ref.py), and the samplers and
the clip level on top of it.

  * the Philox words (raw mode) bit for bit, for every tail / alignment / chunking case, inside a guarded buffer;
  * the normals against the float64 restatement.  The bound is measured, not assumed: the same formulas in numpy float32
    deviate from float64 by 1.607e-06 relative to max(1, |z|) on the 2^20-element draw used here
    (tests/test_seeded_noise_cpu.py prints it); the device's logf / sincospif may differ from the host libm by a few ulp, so
    the kernel gets 4x that, 6.43e-06.  Measured on the MI355X: 1.982e-07 (test_normals_match_the_float64_restatement
    prints all three);
  * the row of a seed is the same bits at b = 1, as slot 2 of b = 3 and as the last slot of a batch one larger than the
    per-launch chunk; `scale` is one fp32 multiply; refusals launch nothing; both bindings agree bit for bit;
  * a seeded sampler run on the tiny model is a function of the seeds alone: repeatable whatever the torch generator holds,
    permutable with its clips, and a partial run walks the draws of the full run's tail.
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import philox_ref
from conftest import GOLDEN, load_golden
from tooncrafter_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0
GUARD = 8
SEEDS = (0, 1, 1 << 32, (1 << 64) - 1, 0x243F6A8885A308D3)      # low word only, high word only, both
STREAMS = (0, 1, 0x10007, 0xFFFFFFFF)
SIZES = (1, 3, 4, 5, 1023, 4096)      # no full group, tail only, exact, tail of 1, tail of 3, many blocks
BATCHES = (1, 3, _lib.TC_RANDN_CLIPS + 1)
N_BIG = 1 << 20
S0, S1 = 0xC0FFEE, (1 << 64) - 5
SETTINGS = dict(unconditional_guidance_scale=7.5, eta=1.0, timestep_spacing="uniform_trailing", guidance_rescale=0.7)


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def ref_words():
    """words of every (seed, stream) at the largest size: a shorter draw is its prefix.  Computed once, never modified."""
    tab = {(s, st): philox_ref.words(s, max(SIZES), st) for s in SEEDS for st in STREAMS}
    for w in tab.values():
        w.setflags(write=False)
    return tab


@pytest.fixture(scope="module")
def big():
    """The float64 normals of one 2^20-element draw and what float32 evaluation of the same formulas costs on it."""
    z = philox_ref.normals(SEEDS[4], N_BIG, 1)
    z.setflags(write=False)
    return z, philox_ref.f32_deviation(SEEDS[4], N_BIG, 1, reference=z)


def seeds_for(b):
    return [SEEDS[i % len(SEEDS)] for i in range(b)]


def guarded(b, n, offset):
    """A (b, n) fp32 view `offset` floats past GUARD sentinel floats of a sentinel-filled buffer (offset 1: rows that start
    off the 16-byte grid even when n % 4 == 0), and the check that everything around the view still holds the sentinel."""
    buf = torch.full((b * n + 2 * GUARD + offset,), SENTINEL, device=DEV)
    lo = GUARD + offset
    view = buf[lo:lo + b * n].view(b, n)
    assert view.data_ptr() % 16 == (4 * lo) % 16

    def intact():
        return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + b * n:] == SENTINEL).all())
    return buf, view, intact


# ------------------------------------------------------------------------------------------------ 1. the words, bit for bit

@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("n", SIZES)
def test_words_are_bit_exact_and_nothing_else_is_written(hip, ref_words, b, n):
    seeds = seeds_for(b)
    for stream in STREAMS:
        want = np.stack([ref_words[(s, stream)][:n] for s in seeds])
        for offset in (0, 1):
            _, view, intact = guarded(b, n, offset)
            res = hip.randn_clips(seeds, (b, n), stream, out=view, raw=True)
            assert res is view
            got = view.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want), (b, n, stream, offset)
            assert intact(), (b, n, stream, offset)
    fresh = hip.randn_clips(seeds, (b, n), STREAMS[2], raw=True)
    assert fresh.dtype == torch.int32 and tuple(fresh.shape) == (b, n)
    assert np.array_equal(fresh.cpu().numpy().view(np.uint32), np.stack([ref_words[(s, STREAMS[2])][:n] for s in seeds]))


# ------------------------------------------------------------------------------------------------ 2. the normals

def test_normals_match_the_float64_restatement(hip, big):
    want, f32_dev = big
    z = hip.randn_clips([SEEDS[4]], (1, N_BIG), 1)
    assert z.dtype == torch.float32 and tuple(z.shape) == (1, N_BIG) and bool(torch.isfinite(z).all())
    got = z.cpu().numpy()[0].astype(np.float64)
    dev = philox_ref.deviation(got, want)
    print(f"normals, largest deviation relative to max(1, |z|): GPU {dev:.3e}; numpy float32 {f32_dev:.3e}; bound {4 * f32_dev:.3e}")
    assert dev <= 4 * f32_dev
    mean, var = got.mean(), got.var()
    assert abs(mean) <= 5 / np.sqrt(N_BIG) and abs(var - 1) <= 5 * np.sqrt(2 / N_BIG), (mean, var)


@pytest.mark.parametrize("n", SIZES)
def test_normals_of_every_tail_and_alignment_case(hip, big, n):
    """The Box-Muller path through the same store cases as the words: b = 3, rows on and off the 16-byte grid."""
    bound = 4 * big[1]
    seeds = seeds_for(3)
    want = philox_ref.rows(seeds, n, 0x10007)
    for offset in (0, 1):
        _, view, intact = guarded(3, n, offset)
        hip.randn_clips(seeds, (3, n), 0x10007, out=view)
        assert philox_ref.deviation(view.cpu().numpy(), want) <= bound and intact(), (n, offset)


# ------------------------------------------------------------------------------------------------ 3. invariance

@pytest.mark.parametrize("shape", [(1023,), (4, 4, 8, 8)])
@pytest.mark.parametrize("raw", [False, True])
def test_a_seeds_row_does_not_depend_on_batch_slot_or_chunk(hip, shape, raw):
    """n = 1023: rows 1.. of a batch start off the 16-byte grid; (4, 4, 8, 8): the tiny latent."""
    big_b = _lib.TC_RANDN_CLIPS + 1
    for stream in (0, 3):
        alone = hip.randn_clips([S1], (1, *shape), stream, raw=raw)
        three = hip.randn_clips([S0, 7, S1], (3, *shape), stream, raw=raw)
        many = hip.randn_clips(list(range(big_b - 1)) + [S1], (big_b, *shape), stream, raw=raw)
        assert torch.equal(three[2:3], alone) and torch.equal(many[big_b - 1:], alone)
        assert not torch.equal(three[0:1], alone) and not torch.equal(hip.randn_clips([S1], (1, *shape), stream + 1, raw=raw), alone)


# ------------------------------------------------------------------------------------------------ 4. scale

def test_scale_is_one_fp32_multiply(hip):
    z = hip.randn_clips([S0, S1], (2, 4099), 2)
    half = hip.randn_clips([S0, S1], (2, 4099), 2, scale=0.5)
    assert torch.equal(half, z * 0.5)
    scaled = hip.randn_clips([S0, S1], (2, 4099), 2, scale=0.7)
    want = z.cpu() * torch.tensor(0.7, dtype=torch.float32)                 # fp32(z) * fp32(0.7), rounded once, on the host
    assert torch.equal(scaled.cpu(), want)
    assert torch.equal(hip.randn_clips([S0, S1], (2, 4099), 2, scale=1.0), z)


# ------------------------------------------------------------------------------------------------ 5. refusals

def test_refusals_launch_nothing(hip):
    buf = torch.full((64,), SENTINEL, device=DEV)
    seeds = (ctypes.c_uint64 * 2)(1, 2)

    def rc(**kw):
        p = _lib.TcRandnParams(out=buf.data_ptr(), seeds=seeds, b=2, n=8, stream=0, scale=1.0, raw=0)
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib.tc_randn_clips(ctypes.byref(p), torch.cuda.current_stream().cuda_stream)
    assert hip.lib.tc_randn_clips(None, None) == -1
    assert rc(out=None) == -1 and rc(seeds=None) == -1 and rc(b=0) == -1 and rc(n=0) == -1
    assert rc(n=(1 << 34) + 1) == -3                                      # only argument-checked: nothing that large exists
    for bad in (dict(seeds=[1]), dict(seeds=[1, -2]), dict(seeds=[1, 1 << 64]), dict(shape=(2, 0)), dict(stream=1 << 32)):
        with pytest.raises(ValueError):
            hip.randn_clips(**{**dict(seeds=[1, 2], shape=(2, 8), stream=0, out=buf[:16].view(2, 8)), **bad})
    with pytest.raises(_lib.TooncrafterHipError):
        hip.randn_clips([1, 2], (2, 8), 0, out=torch.zeros(2, 8))            # a CPU tensor
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused call wrote something"
    assert rc() == 0                                                        # and the same block, unrefused, does write
    torch.cuda.synchronize()
    assert bool((buf[:16] != SENTINEL).all()) and bool((buf[16:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 6. the two bindings

def test_torch_op_equals_ctypes_bit_for_bit(hip):
    be = ops.backend()
    assert getattr(be, "binding", None) == "torch", "the custom-op layer is not loaded"
    seeds = [0, 1 << 63, (1 << 64) - 1] + list(range(3, _lib.TC_RANDN_CLIPS + 2))       # two's-complement seeds, two launches
    for shape, stream, scale in (((len(seeds), 1023), 0x10007, 1.0), ((len(seeds), 4, 4, 8, 8), 5, 0.7)):
        for raw in (False, True):
            a = hip.randn_clips(seeds, shape, stream, scale, raw=raw)
            b = be.randn_clips(seeds, shape, stream, scale, raw=raw)
            assert a.dtype == b.dtype and tuple(b.shape) == shape and b.is_cuda and torch.equal(a, b), (shape, raw)
    direct = torch.ops.tooncrafter.randn_clips([-1], [1, 1023], 0x10007, 1.0, False)
    assert torch.equal(direct, hip.randn_clips([(1 << 64) - 1], (1, 1023), 0x10007))
    meta = torch._C.DispatchKeySet(torch._C.DispatchKey.Meta)
    y = torch.ops.tooncrafter.randn_clips.default.redispatch(meta, [5, -1], [2, 4, 16, 40, 64], 3, 1.0, False)
    assert tuple(y.shape) == (2, 4, 16, 40, 64) and y.dtype == torch.float32 and y.device.type == "meta"
    with pytest.raises(RuntimeError, match="one seed per clip"):
        torch.ops.tooncrafter.randn_clips([1], [2, 8], 0, 1.0, False)


# ------------------------------------------------------------------------------------------------ 7. the sampler

@pytest.fixture(scope="module")
def model(tiny_sd):
    from test_host_logic_cpu import _tiny_model_cfg
    from tooncrafter_amd.utils import instantiate_from_config
    m = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    m.load_state_dict(tiny_sd, strict=False)
    return m.to(DEV)


@pytest.fixture(scope="module")
def two_clips():
    """Conditioning of two different clips (the pinned fixture's, and a variation of it) and the same with the clips swapped."""
    g = {k: torch.from_numpy(v) for k, v in load_golden("ddim_pinned_tiny.npz").items() if v.ndim}

    def pair(t, other):
        return torch.cat([t, other]).to(DEV)
    parts = dict(cond=pair(g["cond"], g["cond"].flip(1) * 0.5), uncond=pair(g["uncond"], g["uncond"]),
                 cc=pair(g["c_concat"], g["c_concat"].flip(2)), fs=pair(g["fs"], g["fs"] + 5),
                 x0=pair(g["x0"], g["x0"].flip(3)))

    def build(order):
        p = {k: v[order].contiguous() for k, v in parts.items()}
        return dict(conditioning={"c_crossattn": [p["cond"]], "c_concat": [p["cc"]]},
                    unconditional_conditioning={"c_crossattn": [p["uncond"]], "c_concat": [p["cc"]]}, fs=p["fs"]), p["x0"]
    return build([0, 1]), build([1, 0]), g["mask_frame"]


def run(model, cond, seeds, **kw):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    with torch.no_grad():
        return DDIMSampler(model).sample(S=5, batch_size=2, shape=(4, 4, 8, 8), verbose=False, seeds=seeds, **cond, **SETTINGS, **kw)


def test_seeded_run_is_a_function_of_the_seeds(model, two_clips):
    (cond, _), (swapped, _), _ = two_clips
    torch.manual_seed(1)
    state = torch.cuda.get_rng_state()
    a, _ = run(model, cond, [S0, S1])
    assert torch.equal(torch.cuda.get_rng_state(), state), "a seeded run touched the device generator"
    torch.manual_seed(2)
    b, _ = run(model, cond, [S0, S1])
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and not torch.equal(a[0], a[1])
    other, _ = run(model, cond, [S0, S1 - 1])
    assert torch.equal(other[0], a[0]) and not torch.equal(other[1], a[1])   # clip 0 does not see clip 1's seed
    c, _ = run(model, swapped, [S1, S0])                                     # clips and seeds swapped: swapped latents
    assert torch.equal(c[0], a[1]) and torch.equal(c[1], a[0])


@pytest.mark.parametrize("pinned", [False, True])
def test_partial_run_reproduces_the_full_runs_tail(model, two_clips, pinned):
    """timesteps=3 walks DDIM table positions 1 and 0: started from the full run's latent after position 2, it draws the
    full run's last draws (keyed by the position, not by the loop counter) and ends on the same bits."""
    (cond, x0), _, mask = two_clips
    kw = dict(mask=mask, x0=x0) if pinned else {}
    full, inter = run(model, cond, [S0, S1], log_every_t=1, **kw)
    assert len(inter["x_inter"]) == 6 and torch.equal(inter["x_inter"][-1], full)
    tail, _ = run(model, cond, [S0, S1], x_T=inter["x_inter"][3], timesteps=3, **kw)
    assert torch.equal(tail, full)
    if pinned:
        free, _ = run(model, cond, [S0, S1])
        assert not torch.equal(free, full)


def test_decode_and_encode_take_seeds(model, two_clips):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler, STREAM_ENCODE
    (cond, x0), _, _ = two_clips
    s = DDIMSampler(model)
    s.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    state = torch.cuda.get_rng_state()
    with torch.no_grad():
        enc = s.stochastic_encode(x0, [1, 1], seeds=[S0, S1])
        want = s.stochastic_encode(x0, [1, 1], noise=ops.randn_clips([S0, S1], tuple(x0.shape), STREAM_ENCODE))
        dec = s.decode(enc, cond["conditioning"], 2, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=cond["unconditional_conditioning"], seeds=[S0, S1])
        again = s.decode(enc, cond["conditioning"], 2, unconditional_guidance_scale=7.5,
                         unconditional_conditioning=cond["unconditional_conditioning"], seeds=[S0, S1])
    assert torch.equal(enc, want) and torch.equal(dec, again) and bool(torch.isfinite(dec).all())
    assert torch.equal(torch.cuda.get_rng_state(), state)


def test_unseeded_run_consumes_the_device_generator_as_before(model, two_clips, monkeypatch):
    """seeds=None: x_T and one draw per step from the device generator, as the existing trajectory tests pin.  The
    module-level hook is set to its own definition here: other tests substitute it, and not all of them put it back."""
    from tooncrafter_amd.lvdm import ddim
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    monkeypatch.setattr(ddim, "noise_like", lambda shape, device, repeat=False: torch.randn(shape, device=device))
    (cond, _), _, _ = two_clips
    torch.manual_seed(3)
    with torch.no_grad():
        a, inter = DDIMSampler(model).sample(S=5, batch_size=2, shape=(4, 4, 8, 8), verbose=False, log_every_t=1, **cond, **SETTINGS)
    state = torch.cuda.get_rng_state()
    torch.manual_seed(3)
    draws = [torch.randn((2, 4, 4, 8, 8), device=DEV) for _ in range(6)]
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(inter["x_inter"][0], draws[0])


# ------------------------------------------------------------------------------------------------ 8. clip level

def test_variant_of_a_seeded_clip_can_be_regenerated_alone(model):
    sys.path.insert(0, GOLDEN)
    try:
        import pipeline_stubs as stubs
    finally:
        sys.path.remove(GOLDEN)
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd.lvdm import autoencoder as my_ae
    saved = model.embedder, model.image_proj_model, my_ae.DiagonalGaussianDistribution.sample
    model.embedder, model.image_proj_model = stubs.StubEmbedder(), stubs.StubImageProj(4)
    model.get_learned_conditioning = lambda prompts: stubs.stub_text(prompts, DEV)
    my_ae.DiagonalGaussianDistribution.sample = lambda self, noise=None: self.mean     # the encoder's draw is out of scope
    videos = torch.randn(1, 3, 4, 64, 64, generator=torch.Generator().manual_seed(77)).clamp(-1, 1).to(DEV)
    shape = [1, 4, 4, 8, 8]
    mk = lambda seeds: pipeline.SamplingPlan(steps=3, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=seeds)
    try:
        with torch.no_grad():
            torch.manual_seed(4)
            both = pipeline.synthesize(model, videos, shape, plan=mk([S0]), fs=10, variants=2)
            torch.manual_seed(5)
            alone = pipeline.synthesize(model, videos, shape, plan=mk([pipeline.variant_seed(S0, 1)]), fs=10, variants=1)
            via_kwargs = pipeline.image_guided_synthesis(model, None, videos, shape, n_samples=1, ddim_steps=3, ddim_eta=1.0,
                                                         unconditional_guidance_scale=7.5, fs=10, interp=True,
                                                         timestep_spacing="uniform_trailing", guidance_rescale=0.7, seeds=[S0])
        assert tuple(both.shape) == (1, 2, 3, 4, 64, 64) and bool(torch.isfinite(both).all())
        assert torch.equal(both[:, 1], alone[:, 0]) and not torch.equal(both[:, 0], both[:, 1])
        assert torch.equal(via_kwargs[:, 0], both[:, 0])
    finally:
        model.embedder, model.image_proj_model, my_ae.DiagonalGaussianDistribution.sample = saved
        del model.get_learned_conditioning
