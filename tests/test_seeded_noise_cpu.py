"""Per-clip seeds without a GPU: the numpy restatement of tc_randn_clips (tests/philox_ref.py) reproduces the Random123
known-answer vectors and has the moments of N(0, 1); the entry point is declared, exported and bound with the header's struct
layout (ABI still 14: one struct, one symbol); the samplers ask an emulated backend (tests/emu_seeded_ops.py) for exactly
the documented streams and leave the torch generator alone.  The kernel itself is covered by tests/test_gpu_seeded_noise.py.

fp32 error budget (test_f32_evaluation_error_is_recorded): the formulas evaluated in numpy float32 deviate from float64 by at
most 1.607e-06 relative to max(1, |z|) on the 2^20-element sample below; the GPU test allows the kernel 4x that, 6.43e-06,
and measures 1.982e-07 on the MI355X."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import philox_ref
from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "tooncrafter_hip.h")
FIELDS = ("out", "seeds", "b", "n", "stream", "scale", "raw")
N = 1 << 20
SEEDS = (0, 1, 1 << 32, (1 << 64) - 1, 0x243F6A8885A308D3)      # low word only, high word only, both


# ------------------------------------------------------------------------------------------------ the restatement itself

@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """The Random123 known-answer vectors of philox4x32-10 (counter, key -> output)."""
    got = philox_ref.philox4x32_10(counter, key)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_words_follow_the_indexing_rule():
    """Element 4q + m is word m of counter (q, 0, stream, 0) under key (lo32(seed), hi32(seed)); a prefix of a longer
    draw is the shorter draw."""
    seed, stream = 0x0123456789ABCDEF, 0x10007
    w = philox_ref.words(seed, 11, stream)
    assert w.dtype == np.uint32 and w.shape == (11,)
    for q in range(3):
        block = philox_ref.philox4x32_10((q, 0, stream, 0), (0x89ABCDEF, 0x01234567))
        assert [int(v) for v in block][:min(4, 11 - 4 * q)] == w[4 * q:4 * q + 4].tolist()
    assert np.array_equal(philox_ref.words(seed, 5, stream), w[:5])
    assert not np.array_equal(philox_ref.words(seed, 11, stream + 1), w)
    assert not np.array_equal(philox_ref.words(seed + (1 << 32), 11, stream), w)


def test_uniforms_are_exact_and_inside_the_open_interval():
    w = np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0x1FF, 0x200], dtype=np.uint32)
    u, v = philox_ref.uniforms(w)
    assert u.tolist() == [2.0 ** -24, 1.0 - 2.0 ** -24, 2.0 ** -24] and v.tolist() == [0.0, 1.0 - 2.0 ** -23, 2.0 ** -23]
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)      # exact in fp32
    assert np.isfinite(np.log(u)).all()


@pytest.fixture(scope="module")
def draws():
    """2^20 normals per seed on stream 1, and stream 2 of the first seed: computed once."""
    z = {(s, 1): philox_ref.normals(s, N, 1) for s in SEEDS}
    z[(SEEDS[0], 2)] = philox_ref.normals(SEEDS[0], N, 2)
    return z


def test_moments_of_the_restatement(draws):
    """5-sigma bounds of an exact N(0, 1) sample of N elements: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N); the
    sample correlation of two independent draws <= 5 / sqrt(N).  That the chosen seeds pass is a condition on the inputs."""
    for key, z in draws.items():
        assert z.dtype == np.float64 and z.shape == (N,) and np.isfinite(z).all(), key
        mean, var = z.mean(), z.var()
        print(f"seed {key[0]:#x} stream {key[1]}: mean {mean:+.3e} var-1 {var - 1:+.3e} max |z| {np.abs(z).max():.3f}")
        assert abs(mean) <= 5 / np.sqrt(N) and abs(var - 1) <= 5 * np.sqrt(2 / N), key
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])
    pairs = [((SEEDS[i], 1), (SEEDS[j], 1)) for i in range(len(SEEDS)) for j in range(i + 1, len(SEEDS))]
    pairs.append(((SEEDS[0], 1), (SEEDS[0], 2)))
    for a, b in pairs:
        c = corr(draws[a], draws[b])
        assert abs(c) <= 5 / np.sqrt(N), (a, b, c)
    # the two normals of one Box-Muller pair share r: uncorrelated all the same
    z = draws[(SEEDS[4], 1)]
    assert abs(corr(z[0::2], z[1::2])) <= 5 / np.sqrt(N // 2)


def test_f32_evaluation_error_is_recorded(draws):
    """The same formulas in numpy float32 against float64, relative to max(1, |z|): the measure the GPU test's bound is
    4x of (module docstring).  Sanity bound from the formulas: the angle pi_f32 * (2 v) carries the rounding
    of pi and of the product, <= 2 * 2^-24 * 2 pi = 7.5e-7, which moves z by at most r * 7.5e-7 with r <= sqrt(-2 ln 2^-24)
    = 5.77; r itself is good to ~2 ulp: below 8e-6 in all."""
    dev = philox_ref.f32_deviation(SEEDS[4], N, 1, reference=draws[(SEEDS[4], 1)])
    print(f"float32 evaluation, largest deviation relative to max(1, |z|): {dev:.3e}")
    assert 0 < dev < 8e-6


# ------------------------------------------------------------------------------------------------ ABI

def test_header_declares_the_entry_point_and_abi_is_unchanged():
    from tooncrafter_amd import _lib
    with open(HEADER) as f:
        header = f.read()
    assert re.search(r"\bint\s+tc_randn_clips\s*\(\s*const\s+TcRandnParams\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"#define\s+TC_ABI_VERSION\s+14\b", header) and _lib.TC_ABI_VERSION == 14
    doc = header[header.index("Per-clip Gaussian noise"):header.index("int tc_randn_clips")]
    for word in ("additive within ABI 14", "Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "ten rounds",
                 "(q, 0, stream, 0)", "2^34", "TC_ESHAPE", "TC_EINVAL", "HOST array", "sincospif", "logf"):
        assert word in doc, word
    assert int(re.search(r"#define\s+TC_RANDN_CLIPS\s+(\d+)", header).group(1)) == _lib.TC_RANDN_CLIPS


def test_ctypes_struct_matches_the_compiled_header(tmp_path):
    """A probe compiled against the header prints sizeof and every offsetof; the ctypes mirror must agree."""
    from tooncrafter_amd import _lib
    assert tuple(f[0] for f in _lib.TcRandnParams._fields_) == FIELDS
    cc = next((c for c in (os.environ.get("CC"), shutil.which("cc"), shutil.which("gcc"), shutil.which("g++"),
                           shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cc, "no C compiler for the layout probe"
    src = tmp_path / "probe.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "tooncrafter_hip.h"', 'int main(void) {',
             '  printf("%zu %d", sizeof(TcRandnParams), TC_ABI_VERSION);']
    lines += [f'  printf(" %zu", offsetof(TcRandnParams, {f}));' for f in FIELDS]
    lines += ['  return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-x", "c", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.TcRandnParams) and got[1] == 14
    assert got[2:] == [getattr(_lib.TcRandnParams, f).offset for f in FIELDS]


def test_library_exports_and_binds_the_symbol():
    from tooncrafter_amd import _lib, build
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    assert hasattr(lib, "tc_randn_clips")
    res, args = _lib.SYMBOLS["tc_randn_clips"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.TcRandnParams), ctypes.c_void_p]
    assert _lib.load().tc_abi_version() == 14
    from tooncrafter_amd.ops import HipOps
    assert callable(HipOps.randn_clips)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """The documented refusals return before the launch, so they can be exercised on host pointers."""
    from tooncrafter_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 16)(*([7.0] * 16))
    seeds = (ctypes.c_uint64 * 2)(1, 2)

    def rc(**kw):
        p = _lib.TcRandnParams(out=ctypes.addressof(buf), seeds=seeds, b=2, n=8, stream=0, scale=1.0, raw=0)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.tc_randn_clips(ctypes.byref(p), None)
    assert lib.tc_randn_clips(None, None) == -1
    assert rc(out=None) == -1 and rc(seeds=None) == -1
    assert rc(b=0) == -1 and rc(b=-1) == -1 and rc(n=0) == -1 and rc(n=-5) == -1
    assert rc(n=(1 << 34) + 1) == -3 and rc(n=(1 << 34) + 1, raw=1) == -3
    assert list(buf) == [7.0] * 16


def test_meta_kernel_infers_shape_and_dtype():
    """The op takes no tensor, so the Meta kernel is reached by naming its dispatch key."""
    from tooncrafter_amd import torch_ops
    t = torch_ops.load()
    schema = str(t.randn_clips.default._schema)
    assert schema == "tooncrafter::randn_clips(int[] seeds, int[] shape, int stream, float scale, bool raw) -> Tensor", schema
    meta = torch._C.DispatchKeySet(torch._C.DispatchKey.Meta)
    y = t.randn_clips.default.redispatch(meta, [5, -1], [2, 4, 16, 40, 64], 3, 1.0, False)
    assert tuple(y.shape) == (2, 4, 16, 40, 64) and y.dtype == torch.float32 and y.device.type == "meta"
    y = t.randn_clips.default.redispatch(meta, [5], [1, 7], 3, 1.0, True)
    assert tuple(y.shape) == (1, 7) and y.dtype == torch.int32 and y.device.type == "meta"
    with pytest.raises(RuntimeError):
        t.randn_clips.default.redispatch(meta, [5], [2, 7], 3, 1.0, False)         # one seed, two clips


def test_binding_checks_seeds_shape_and_stream_on_the_host():
    from tooncrafter_amd import ops
    for bad in ([-1], [1 << 64], [1.0], ["3"], [None], [True], 7, "7", [1, 2]):
        with pytest.raises(ValueError):
            ops.clip_seeds(bad, 1)
    assert ops.clip_seeds((np.int64(5),), 1) == [5] and ops.clip_seeds([(1 << 64) - 1, 0], 2) == [(1 << 64) - 1, 0]
    args = ops.HipOps._randn_args
    for bad in (dict(shape=()), dict(shape=(1, 0)), dict(stream=-1), dict(stream=1 << 32)):
        with pytest.raises(ValueError):
            args(**{**dict(seeds=[1], shape=(1, 4), stream=0), **bad})


# ------------------------------------------------------------------------------------------------ variant seeds

def test_variant_seed_is_the_documented_function():
    from tooncrafter_amd.clip import variant_seed
    m = (1 << 64) - 1

    def written_out(seed, k):
        z = (seed + k * 0x9E3779B97F4A7C15) % (1 << 64)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
        return z ^ (z >> 31)
    for seed in (0, 1, 42, 1 << 63, m):
        assert variant_seed(seed, 0) == seed
        for k in (1, 2, 3, 1000):
            v = variant_seed(seed, k)
            assert v == written_out(seed, k) and 0 <= v <= m and v != seed
    # splitmix64's published first outputs from state 0 are its finaliser at 1 * gamma and 2 * gamma
    assert variant_seed(0, 1) == 0xE220A8397B1DCDAF and variant_seed(0, 2) == 0x6E789E6AA1B965F4
    for bad in ((-1, 0), (1 << 64, 1), (3, -1)):
        with pytest.raises(ValueError):
            variant_seed(*bad)


# ------------------------------------------------------------------------------------------------ the samplers' host logic

S0, S1 = 0xC0FFEE, (1 << 64) - 5


@pytest.fixture(scope="module")
def emu():
    from emu_seeded_ops import EmuSeededOps
    from tooncrafter_amd import ops
    be = EmuSeededOps(round_bf16=True)
    prev = ops.set_backend(be)
    yield be
    ops.set_backend(prev)


@pytest.fixture(scope="module")
def emu_model(tiny_sd, emu):
    from test_host_logic_cpu import _tiny_model_cfg
    from tooncrafter_amd.utils import instantiate_from_config
    model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    model.load_state_dict(tiny_sd, strict=False)
    return model


@pytest.fixture()
def audit(emu_model, emu):
    """Every keyword that reaches the model's UNet entry points during the test; the draw log starts empty."""
    seen = []
    names = [n for n in ("apply_model", "apply_model_cfg", "apply_model_multi") if hasattr(emu_model, n)]
    saved = {n: getattr(emu_model, n) for n in names}

    def wrap(fn):
        def inner(*a, **kw):
            seen.append(sorted(kw))
            return fn(*a, **kw)
        return inner
    for n in names:
        setattr(emu_model, n, wrap(saved[n]))
    emu.draws.clear()
    yield seen
    for n in names:
        delattr(emu_model, n)
    emu.draws.clear()


def _kw(**kw):
    g, T = load_golden("ddim_pinned_tiny.npz"), torch.from_numpy
    cond = {"c_crossattn": [T(g["cond"])], "c_concat": [T(g["c_concat"])]}
    uc = {"c_crossattn": [T(g["uncond"])], "c_concat": [T(g["c_concat"])]}
    base = dict(S=5, conditioning=cond, batch_size=1, shape=(4, 4, 8, 8), verbose=False, unconditional_conditioning=uc,
                fs=T(g["fs"]), unconditional_guidance_scale=7.5, eta=1.0, timestep_spacing="uniform_trailing",
                guidance_rescale=0.7)
    base.update(kw)
    return base, g


def _streams(emu):
    return [d[2] for d in emu.draws]


def test_full_run_asks_for_the_documented_streams(emu_model, emu, audit):
    from tooncrafter_amd.lvdm import ddim
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    assert (ddim.STREAM_X_T, ddim.STREAM_STEP, ddim.STREAM_Q_SAMPLE, ddim.STREAM_ENCODE) == (0, 1, 0x10000, 0x20000)
    kw, _ = _kw(seeds=[S0], temperature=0.5, log_every_t=1)
    rng = torch.get_rng_state()
    sampler = DDIMSampler(emu_model)
    out, inter = sampler.sample(**kw)
    assert torch.equal(torch.get_rng_state(), rng), "a seeded run touched the torch generator"
    assert (np.asarray(sampler.ddim_sigmas) != 0).all()
    assert _streams(emu) == [0, 5, 4, 3, 2, 1]                       # x_T, then 1 + index for index = 4 .. 0
    assert all(d[0] == (S0,) and d[1] == (1, 4, 4, 8, 8) for d in emu.draws)
    assert [d[3] for d in emu.draws] == [1.0] + [0.5] * 5            # the temperature goes in as the scale
    x_T = torch.from_numpy(philox_ref.normals(S0, 4 * 4 * 8 * 8, 0).astype(np.float32)).view(1, 4, 4, 8, 8)
    assert torch.equal(inter["x_inter"][0], x_T) and torch.isfinite(out).all()
    assert audit and all("seeds" not in k for k in audit), "seeds reached the UNet"
    # the same seeds again: the same latents; another seed: others
    emu.draws.clear()
    again, _ = DDIMSampler(emu_model).sample(**kw)
    other, _ = DDIMSampler(emu_model).sample(**{**kw, "seeds": [S1]})
    assert torch.equal(again, out) and not torch.equal(other, out)


def test_partial_decode_and_encode_streams(emu_model, emu, audit):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    kw, g = _kw(seeds=[S0], x_T=torch.from_numpy(g_x_T()), timesteps=3)
    DDIMSampler(emu_model).sample(**kw)
    assert _streams(emu) == [2, 1]                                   # table positions 1 and 0: the full run's tail
    emu.draws.clear()
    s = DDIMSampler(emu_model)
    s.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    rng = torch.get_rng_state()
    s.decode(kw["x_T"], kw["conditioning"], 2, unconditional_guidance_scale=7.5,
             unconditional_conditioning=kw["unconditional_conditioning"], seeds=[S0])
    assert _streams(emu) == [2, 1]
    emu.draws.clear()
    x0 = torch.from_numpy(g["x0"])
    enc = s.stochastic_encode(x0, [1], seeds=[S0])
    assert _streams(emu) == [0x20000] and torch.equal(torch.get_rng_state(), rng)
    noise = torch.from_numpy(philox_ref.normals(S0, x0.numel(), 0x20000).astype(np.float32)).view(x0.shape)
    assert torch.equal(enc, s.stochastic_encode(x0, [1], noise=noise))
    with pytest.raises(ValueError):
        s.stochastic_encode(x0, [1], noise=noise, seeds=[S0])
    assert all("seeds" not in k for k in audit)


def g_x_T():
    return load_golden("ddim_pinned_tiny.npz")["x_T"]


@pytest.mark.parametrize("three_way", [False, True])
def test_pinned_run_streams(emu_model, emu, audit, three_way):
    """The q_sample draw of a step (0x10000 + index) comes before that step's own draw (1 + index), and the pinned frame
    the UNet sees is q_sample(x0, t) with exactly that draw."""
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWaySampler
    kw, g = _kw(seeds=[S0])
    T = torch.from_numpy
    kw.update(mask=T(g["mask_frame"]), x0=T(g["x0"]), x_T=T(g["x_T"]))
    if three_way:
        kw.update(cfg_img=3.0, unconditional_conditioning_img_nonetext={"c_crossattn": [T(g["uncond_img"])],
                                                                        "c_concat": [T(g["c_concat"])]})
    calls, multi = [], emu_model.apply_model_multi

    def apply_model_multi(x, t, conds, **k):
        calls.append((int(t[0]), x.clone()))
        return multi(x, t, conds, **k)
    emu_model.apply_model_multi = apply_model_multi
    rng = torch.get_rng_state()
    (ThreeWaySampler if three_way else DDIMSampler)(emu_model).sample(**kw)
    assert torch.equal(torch.get_rng_state(), rng)
    assert _streams(emu) == [0x10004, 5, 0x10003, 4, 0x10002, 3, 0x10001, 2, 0x10000, 1]
    sa, s1 = emu_model.sqrt_alphas_cumprod, emu_model.sqrt_one_minus_alphas_cumprod
    assert [t for t, _ in calls] == g["a_t"].tolist()
    for i, (t, x) in enumerate(calls):
        qn = T(philox_ref.normals(S0, T(g["x0"]).numel(), 0x10000 + 4 - i).astype(np.float32)).view(g["x0"].shape)
        assert torch.equal(x[:, :, 2], (sa[t] * T(g["x0"]) + s1[t] * qn)[:, :, 2]), i
    emu.draws.clear()                                                # clean_cond: x0 as it is, no q_sample draw
    DDIMSampler(emu_model).sample(**{k: v for k, v in kw.items() if k not in ("cfg_img", "unconditional_conditioning_img_nonetext")},
                                  clean_cond=True)
    assert _streams(emu) == [5, 4, 3, 2, 1]
    assert all("seeds" not in k for k in audit)


def test_deterministic_run_draws_no_step_noise(emu_model, emu, audit):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    kw, _ = _kw(seeds=[S0], eta=0.0)
    rng = torch.get_rng_state()
    DDIMSampler(emu_model).sample(**kw)
    assert _streams(emu) == [0] and torch.equal(torch.get_rng_state(), rng)


def test_bad_seeds_are_refused_before_the_backend_is_called(emu_model, emu, audit):
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    from tooncrafter_amd.lvdm.ddim_multiplecond import DDIMSampler as ThreeWaySampler
    for cls in (DDIMSampler, ThreeWaySampler):
        for bad in (dict(seeds=[S0, S1]), dict(seeds=[]), dict(seeds=[-1]), dict(seeds=[1 << 64]), dict(seeds=[0.5]),
                    dict(seeds=[S0], repeat_noise=True)):
            with pytest.raises(ValueError):
                cls(emu_model).sample(**_kw(**bad)[0])
    s = DDIMSampler(emu_model)
    s.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    x = torch.zeros(1, 4, 4, 8, 8)
    with pytest.raises(ValueError):
        s.decode(x, None, 2, seeds=[S0, S1])
    with pytest.raises(ValueError):
        s.stochastic_encode(x, [1], seeds=[1 << 64])
    with pytest.raises(ValueError):
        s.ddim_sampling(None, (1, 4, 4, 8, 8), seeds=[S0, S1])
    assert emu.draws == [] and audit == []


def test_unseeded_run_still_draws_from_the_torch_generator(emu_model, emu, audit, monkeypatch):
    """seeds=None: x_T and one draw per step from the device generator, none from the backend.  The module-level hook is
    set to its own definition here: other tests substitute it, and not all of them put it back."""
    from tooncrafter_amd.lvdm import ddim
    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    monkeypatch.setattr(ddim, "noise_like", lambda shape, device, repeat=False: torch.randn(shape, device=device))
    kw, _ = _kw()
    torch.manual_seed(11)
    a, _ = DDIMSampler(emu_model).sample(**kw)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    want = [torch.randn(1, 4, 4, 8, 8) for _ in range(6)]
    assert torch.equal(torch.get_rng_state(), state), "the unseeded run consumes x_T and one draw per step"
    torch.manual_seed(11)
    b, inter = DDIMSampler(emu_model).sample(**{**kw, "log_every_t": 1})
    assert torch.equal(a, b) and torch.equal(inter["x_inter"][0], want[0]) and emu.draws == []


def test_clip_level_hands_the_seeds_on(emu_model, emu, audit):
    """SamplingPlan.seeds, `seeds` among plan.extra (the reference callers' **kwargs route) and the variant rule."""
    from tooncrafter_amd import clip as pipeline
    kw, g = _kw()
    T = torch.from_numpy
    cond = pipeline.Conditions(kw["conditioning"], kw["unconditional_conditioning"], None, None, T(g["fs"]))
    shape = [1, 4, 4, 8, 8]
    plan = pipeline.SamplingPlan(steps=3, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=[S0])
    assert pipeline.SamplingPlan().seeds is None
    a = pipeline.sample(emu_model, cond, plan, shape)
    assert _streams(emu) == [0, 3, 2, 1] and all(d[0] == (S0,) for d in emu.draws)
    emu.draws.clear()
    via_kwargs = pipeline.SamplingPlan(steps=3, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, extra=dict(seeds=[S0]))
    assert torch.equal(pipeline.sample(emu_model, cond, via_kwargs, shape), a)
    emu.draws.clear()
    v1 = pipeline.sample(emu_model, cond, plan, shape, variant=1)
    assert all(d[0] == (pipeline.variant_seed(S0, 1),) for d in emu.draws) and not torch.equal(v1, a)
    alone = pipeline.SamplingPlan(steps=3, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7,
                                  seeds=[pipeline.variant_seed(S0, 1)])
    assert torch.equal(pipeline.sample(emu_model, cond, alone, shape), v1)
    with pytest.raises(ValueError):
        pipeline.sample(emu_model, cond, pipeline.SamplingPlan(steps=3, seeds=[S0, S1]), shape)
    assert all("seeds" not in k for k in audit)
