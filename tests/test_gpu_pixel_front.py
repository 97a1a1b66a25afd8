"""The pixel front end on the MI355X (csrc/pixel_front.hip):

  * tc_frames_from_u8 against tests/golden/pixel_front.npz -- what the script's PIL transform makes of the same bytes -- with
    torch.equal, one case per way to go wrong, plus padded rows, several images, untouched slots and both bindings;
  * tc_clip_patches against an fp64 numpy statement of kornia's antialiased bicubic resize, the CLIP normalisation and the
    unfold: every element within one bf16 ulp of the statement's bf16 rounding, pad columns zero, and no more elements off
    that rounding than twice what the existing torch path (kornia_resize + normalise + unfold + .to(bf16)) leaves, plus 8.
    An element differs from the rounded statement when the evaluation's own rounding error carries it over a bf16 rounding
    boundary, which a different summation order does for different elements, about as often (hence 2x; the 8 keeps a zero
    count from making the bound vacuous).  The existing path is the yardstick, not the code under test.  One ulp is asked of
    EVERY element, the ones near zero included, where the CLIP mean has cancelled the pixel value and a bf16 ulp is smaller
    than the error of an fp32 sum of O(1) terms (the existing fp32 path is up to tens of ulps off there): the kernel
    therefore sums in double;
  * Conditions.from_uint8 / synthesize_u8 on the tiny model with tiny towers.

The counts and the token errors go to profiles/r10_pixel_front_tests.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROFILE = os.path.join(ROOT, "profiles", "r10_pixel_front_tests.txt")
FRAME_CASES = ["down_odd_crop", "up_2tap", "crop_only", "half", "portrait_k19", "bars_even", "half_even_top", "one_wide"]
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
S, PATCH, LD = 28, 14, 592                         # a two-by-two grid of real 14 x 14 patches; 588 columns padded to 592


def record(key, text):
    """one line per key in the profile file, kept sorted; lines of other keys stay"""
    lines = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as f:
            lines = dict(ln.rstrip("\n").split(": ", 1) for ln in f if ": " in ln and not ln.startswith("#"))
    lines[key] = text
    with open(PROFILE, "w") as f:
        f.write("# tests/test_gpu_pixel_front.py on the MI355X.  clip_patches: elements that differ from the bf16 rounding of the fp64\n"
                "# statement, kernel vs the existing torch path; tokens: rel-L2 to the fp32 oracle tower, new path vs existing.\n")
        for k in sorted(lines):
            f.write(f"{k}: {lines[k]}\n")


@pytest.fixture(scope="module")
def g():
    return load_golden("pixel_front.npz")


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------------------------------------ tc_frames_from_u8

@pytest.mark.parametrize("name", FRAME_CASES)
def test_frames_equal_the_pil_transform(hip, g, name):
    h, w = (int(v) for v in g[name + ".size"])
    img = torch.from_numpy(g[name + ".src"])[None].to(DEV)
    out = hip.frames_from_u8(img, (h, w), [1], b=1, t=2)
    assert out.shape == (1, 3, 2, h, w) and out.dtype == torch.float32
    assert torch.equal(out[0, :, 1].cpu(), torch.from_numpy(g[name + ".y"])), name
    assert not out[0, :, 0].any()                                                 # the frame no slot names


def test_padded_rows_three_images_and_untouched_slots(hip, g):
    """Rows 3 * sw + 5 bytes apart, images to (0, 0), (0, t - 1) and (1, 0) of a (2, 3, 4, H, W) tensor of sentinels that ends
    where its allocation ends, behind a guard: every other frame and the guard keep the sentinel."""
    h, w = (int(v) for v in g["multi.size"])
    src = torch.from_numpy(g["multi.src"])
    n, sh, sw, _ = src.shape
    pitch = 3 * sw + 5
    held = torch.randint(0, 256, (n, sh, pitch), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    held[:, :, :3 * sw] = src.reshape(n, sh, 3 * sw)
    held = held.to(DEV)
    imgs = held.as_strided((n, sh, sw, 3), (sh * pitch, pitch, 3, 1))
    b, t, guard, sentinel = 2, 4, 1024, -77.0
    buf = torch.full((guard + b * 3 * t * h * w,), sentinel, dtype=torch.float32, device=DEV)
    out = buf[guard:].view(b, 3, t, h, w)
    assert out.data_ptr() + out.numel() * 4 == buf.data_ptr() + buf.numel() * 4
    from tooncrafter_amd import clip
    res = clip.frames_from_uint8(imgs, (h, w), [(0, 0), (0, t - 1), (1, 0)], t, out=out)
    assert res is out
    got, want = out.cpu(), torch.from_numpy(g["multi.y"])
    for i, (bb, ff) in enumerate([(0, 0), (0, t - 1), (1, 0)]):
        assert torch.equal(got[bb, :, ff], want[i]), (bb, ff)
    named = torch.zeros(b, t, dtype=torch.bool)
    named[0, 0] = named[0, t - 1] = named[1, 0] = True
    assert (got.permute(0, 2, 1, 3, 4)[~named] == sentinel).all() and (buf[:guard] == sentinel).all()
    # without `out`: a new tensor, b from the slots, zero where no slot points
    fresh = clip.frames_from_uint8(imgs, (h, w), [(0, 0), (0, t - 1), (1, 0)], t).cpu()
    assert fresh.shape == (2, 3, t, h, w) and torch.equal(fresh[1, :, 0], want[2]) and not fresh.permute(0, 2, 1, 3, 4)[~named].any()


@pytest.mark.parametrize("name", ["down_odd_crop", "crop_only", "one_wide"])
def test_torch_op_binding_equals_ctypes(hip, g, name):
    from tooncrafter_amd import torch_ops
    tl = torch_ops.TorchLibOps()
    h, w = (int(v) for v in g[name + ".size"])
    img = torch.from_numpy(g[name + ".src"])[None].to(DEV)
    a = hip.frames_from_u8(img, (h, w), [2], b=1, t=3)
    b = tl.frames_from_u8(img, (h, w), [2], b=1, t=3)
    assert torch.equal(a, b) and torch.equal(b[0, :, 2].cpu(), torch.from_numpy(g[name + ".y"]))
    with pytest.raises(RuntimeError, match="outside the clip tensor"):             # the op checks the slots the C entry point would refuse
        tl.t.frames_from_u8(img, [3], 1, 3, h, w, None, None, None, None)


def test_more_images_than_one_call_takes(hip):
    """17 images of 5 x 7 (resized to 4 x 5: both passes run) into slots 0 .. 16 of a (2, 3, 9, 4, 6) clip tensor, which takes
    two calls of the entry point: the same images sent one to a call into a zeroed `out`, and slot 17 stays zero."""
    from tooncrafter_amd import _lib
    n, b, t, size = _lib.TC_FRAMES_U8_MAX + 1, 2, 9, (4, 6)
    assert n == 17 and hip.resized_size(5, 7, *size) == (4, 5)
    imgs = torch.randint(0, 256, (n, 5, 7, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(17)).to(DEV)
    got = hip.frames_from_u8(imgs, size, list(range(n)), b=b, t=t)
    want = torch.zeros(b, 3, t, *size, dtype=torch.float32, device=DEV)
    for i in range(n):
        hip.frames_from_u8(imgs[i:i + 1], size, [i], b=b, t=t, out=want)
    assert got.shape == want.shape and torch.equal(got, want)
    assert want[1, :, 7].any() and not got[1, :, 8].any()                         # slot 16 is written, slot 17 = (1, 8) is not


# ------------------------------------------------------------------------------------------------ tc_clip_patches

def blur_rule(factor):
    sigma = max((factor - 1.0) / 2.0, 0.001)
    ks = int(max(2.0 * 2 * sigma, 3))
    return sigma, ks + 1 if ks % 2 == 0 else ks


def blur_axis(x, factor, axis):
    sigma, ks = blur_rule(factor)
    k = np.exp(-(np.arange(ks, dtype=np.float64) - ks // 2) ** 2 / (2.0 * sigma ** 2))
    k /= k.sum()
    pad = [(0, 0)] * x.ndim
    pad[axis] = (ks // 2, ks // 2)
    xp = np.moveaxis(np.pad(x, pad, mode="reflect"), axis, -1)
    n = x.shape[axis]
    return np.moveaxis(sum(k[i] * xp[..., i:i + n] for i in range(ks)), -1, axis)


def cubic_taps(t, a=-0.75):
    near = lambda v: ((a + 2.0) * v - (a + 3.0)) * v * v + 1.0
    far = lambda v: ((a * v - 5.0 * a) * v + 8.0 * a) * v - 4.0 * a
    return np.stack([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)], -1)


def bicubic_axis(x, out, axis):
    n = x.shape[axis]
    src = np.arange(out, dtype=np.float64) * ((n - 1) / (out - 1) if out > 1 else 0.0)
    i0 = np.floor(src).astype(np.int64)
    wts = cubic_taps(src - i0)
    x = np.moveaxis(x, axis, -1)
    acc = sum(x[..., np.clip(i0 - 1 + k, 0, n - 1)] * wts[:, k] for k in range(4))
    return np.moveaxis(acc, -1, axis)


def statement(x, size=S, patch=PATCH):
    """fp64: kornia's resize (blur if a factor exceeds 1, rows first; bicubic, align_corners), (x + 1) / 2, CLIP mean / std,
    unfold to [(b gy gx), (c py px)]"""
    x = x.astype(np.float64)
    b, _, h, w = x.shape
    fy, fx = h / size, w / size
    if max(fy, fx) > 1:
        x = blur_axis(blur_axis(x, fx, 3), fy, 2)
    y = bicubic_axis(bicubic_axis(x, size, 2), size, 3)
    y = ((y + 1.0) / 2.0 - np.float64(np.float32(MEAN)).reshape(1, 3, 1, 1)) / np.float64(np.float32(STD)).reshape(1, 3, 1, 1)
    g = size // patch
    return y, y.reshape(b, 3, g, patch, g, patch).transpose(0, 2, 4, 1, 3, 5).reshape(b * g * g, 3 * patch * patch)


def to_bf16_once(v):
    """fp64 -> bf16 in one rounding (8 significant bits, half to even); through fp32 it would be two"""
    m, e = np.frexp(v)
    return torch.from_numpy(np.ldexp(np.rint(m * 256.0), e - 8).astype(np.float32)).to(torch.bfloat16)


def ulps_apart(a, b):
    def ordered(t):
        bits = t.view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7fff), bits)
    return (ordered(a) - ordered(b)).abs()


def existing_path(x, size, patch, ld):
    """what FrozenOpenCLIPImageEmbedderV2.preprocess and CLIPVision.tokens build today, on the device"""
    from tooncrafter_amd.lvdm.condition import kornia_resize
    y = kornia_resize(x.float(), (size, size), interpolation="bicubic", align_corners=True, antialias=True)
    y = (y + 1.) / 2.
    y = (y - torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)) / torch.tensor(STD, device=x.device).view(1, 3, 1, 1)
    b, g = x.shape[0], size // patch
    pat = y.reshape(b, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, 3 * patch * patch)
    a = torch.zeros((pat.shape[0], ld), dtype=torch.bfloat16, device=x.device)
    a[:, :pat.shape[1]] = pat.to(torch.bfloat16)
    return a


def clip_input(name):
    if name == "frame_320x512":       # the BASELINE frame of the resize pin: its two stored planes and their mean
        x = load_golden("resize_kornia.npz")["frame_320x512.x"].astype(np.float32)
        return np.concatenate([x, x.mean(0, keepdims=True)])[None], 224
    shape = {"down_40x64": (1, 3, 40, 64), "one_axis_28x64": (1, 3, 28, 64), "up_20x20": (1, 3, 20, 20),
             "taps19_300x290": (1, 3, 300, 290), "two_images_33x50": (2, 3, 33, 50)}[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    yy, xx = np.meshgrid(np.linspace(0, 1, shape[2]), np.linspace(0, 1, shape[3]), indexing="ij")
    base = np.stack([[np.sin(5.0 * (c + 1) * xx + 3.0 * yy + i) * np.cos(4.0 * yy * (c + 1)) for c in range(3)] for i in range(shape[0])])
    return np.clip(0.6 * base + 0.4 * rng.standard_normal(shape), -1.0, 1.0).astype(np.float32), S


def test_the_statement_reproduces_the_resize_pin():
    """The fp64 statement above, before normalisation, against the scipy statement stored in resize_kornia.npz."""
    gk = load_golden("resize_kornia.npz")
    x = gk["frame_320x512.x"].astype(np.float64)[None]
    x = blur_axis(blur_axis(x, 512 / 224, 3), 320 / 224, 2)
    y = bicubic_axis(bicubic_axis(x, 224, 2), 224, 3)[0]
    assert np.abs(y - gk["frame_320x512.y"]).max() < 1e-6                         # the fixture is stored in fp32


@pytest.mark.parametrize("binding", ["ctypes", "torch"])
@pytest.mark.parametrize("name", ["down_40x64", "one_axis_28x64", "up_20x20", "taps19_300x290", "two_images_33x50", "frame_320x512"])
def test_clip_patches_against_the_fp64_statement(hip, name, binding):
    """down_40x64: factors above 1 on both axes (3 taps each); one_axis_28x64: a factor of exactly 1, where sigma is 0.001 and the
    3-tap kernel is the identity; up_20x20: no blur; taps19_300x290: sigma 4.86 / 4.68, 19 taps, reflect over 9 pixels;
    two_images_33x50: B = 2, odd sizes; frame_320x512: the real 224 / 14 geometry."""
    from tooncrafter_amd import torch_ops
    be = hip if binding == "ctypes" else torch_ops.TorchLibOps()
    x_np, size = clip_input(name)
    _, rows = statement(x_np, size, PATCH)
    want = to_bf16_once(rows)
    x = torch.from_numpy(x_np).to(DEV)
    a = be.clip_patches(x, size=size, patch=PATCH, ld=LD, mean=MEAN, std=STD).cpu()
    g = size // PATCH
    assert a.shape == (x.shape[0] * g * g, LD) and a.dtype == torch.bfloat16
    assert not a[:, 588:].any()
    old = existing_path(x, size, PATCH, LD).cpu()
    n_new, n_old = int((a[:, :588] != want).sum()), int((old[:, :588] != want).sum())
    worst = int(ulps_apart(a[:, :588], want).max())
    print(f"clip_patches {name} [{binding}]: {n_new} of {want.numel()} elements off the rounded statement (worst {worst} ulp); "
          f"existing torch path {n_old}")
    if binding == "ctypes":
        record(f"clip_patches {name}", f"kernel {n_new}, existing torch path {n_old}, of {want.numel()} elements; worst {worst} bf16 ulp")
    assert worst <= 1
    assert n_new <= 2 * n_old + 8, (n_new, n_old)


def test_clip_patches_refusals_launch_nothing(hip):
    from tooncrafter_amd import _lib
    out = torch.full((4, LD), 3.0, dtype=torch.bfloat16, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)

    def rc(h, w, size):
        x = torch.zeros(1, 3, h, w, device=DEV)
        p = _lib.TcClipPatchesParams(x=x.data_ptr(), out=out.data_ptr(), b=1, h=h, w=w, size=size, patch=PATCH, ld=LD, antialias=1,
                                     workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        p.mean[:], p.std[:] = MEAN, STD
        return hip.lib.tc_clip_patches(C.byref(p), None)
    assert rc(64, 1, S) == -3 and rc(1, 64, S) == -3                              # the 3-tap kernel's reflect border on one pixel
    assert rc(40, 64, 30) == -3                                                   # S % patch != 0
    torch.cuda.synchronize()
    assert (out == 3.0).all() and not ws.any()
    with pytest.raises(ValueError):
        hip.clip_patches(torch.zeros(1, 3, 40, 64, device=DEV), size=30, patch=PATCH, ld=LD, mean=MEAN, std=STD)


# ------------------------------------------------------------------------------------------------ end to end, tiny model

class TinyImageProj(torch.nn.Module):
    """(B, tokens, 160) -> (B, 16 * t, 96): a fixed linear stand-in for the resampler (not under test here)"""

    def __init__(self, t):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.w = torch.randn(160, 96, generator=gen) * 160 ** -0.5
        self.mix = torch.randn(1, 16 * t, 1, generator=gen)
        self.bias = 0.3 * torch.randn(1, 16 * t, 96, generator=gen)

    def forward(self, x):
        v = x.float().mean(1) @ self.w.to(x.device)
        return v[:, None, :] * self.mix.to(x.device) + self.bias.to(x.device)


@pytest.fixture(scope="module")
def tiny(tiny_sd):
    """The tiny LatentVisualDiffusion of the GPU model tests with a tiny image tower (the geometry of _tiny_towers) as its
    embedder; text from the pipeline stubs; the encoder's posterior taken at its mean so that two builds agree."""
    import sys
    sys.path.insert(0, GOLDEN)
    import pipeline_stubs as stubs
    from test_host_logic_cpu import _tiny_model_cfg
    from tooncrafter_amd import synth
    from tooncrafter_amd.lvdm import autoencoder as my_ae
    from tooncrafter_amd.lvdm import openclip
    from tooncrafter_amd.lvdm.condition import FrozenOpenCLIPImageEmbedderV2
    from tooncrafter_amd.utils import instantiate_from_config
    openclip.ARCH["tiny-test"] = dict(embed_dim=64, vision=dict(width=160, layers=2, heads=2, patch=14, image=42, mlp=320),
                                      text=dict(width=128, layers=3, heads=2, context=7, vocab=50, mlp=256))
    saved = my_ae.DiagonalGaussianDistribution.sample
    try:
        model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
        model.load_state_dict(tiny_sd, strict=False)
        emb = FrozenOpenCLIPImageEmbedderV2(arch="tiny-test").eval()
        synth.fill_module_(emb, prefix="embedder.", seed=1234)
        sd = {k[len("model.visual."):]: v.detach().clone() for k, v in emb.state_dict().items() if k.startswith("model.visual.")}
        model.embedder, model.image_proj_model = emb, TinyImageProj(4)
        model = model.to(DEV)
        model.get_learned_conditioning = lambda prompts: stubs.stub_text(prompts, DEV)
        my_ae.DiagonalGaussianDistribution.sample = lambda self, noise=None: self.mean
        yield model, sd
    finally:
        my_ae.DiagonalGaussianDistribution.sample = saved
        del openclip.ARCH["tiny-test"]


def shim_frames(crop_u8):
    """ToTensor and Normalize(0.5, 0.5) of the transform, on the resized and cropped bytes of the fixture: torch's own ops"""
    x = torch.from_numpy(crop_u8.copy()).permute(0, 3, 1, 2).to(torch.float32).div(255.0)
    return (x - torch.tensor(0.5).view(-1, 1, 1)) / torch.tensor(0.5).view(-1, 1, 1)


def test_conditions_from_uint8_equal_conditions_build(tiny, g):
    from oracle import openclip as oclip
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd.lvdm.condition import kornia_resize
    model, sd = tiny
    h, w = (int(v) for v in g["e2e.size"])
    first, last = (torch.from_numpy(g["e2e.src"][i])[None].to(DEV) for i in range(2))
    frames = shim_frames(g["e2e.crop_u8"])                                        # (2, 3, h, w): first, last
    videos = torch.zeros(1, 3, 4, h, w)
    videos[0, :, 0], videos[0, :, 3] = frames[0], frames[1]
    with torch.no_grad():
        new = pipeline.Conditions.from_uint8(model, first, last, size=(h, w), t=4, fs=10)
        old = pipeline.Conditions.build(model, videos.to(DEV), fs=10)
        assert torch.equal(new.positive["c_concat"][0], old.positive["c_concat"][0]) and new.negative["c_concat"][0] is new.endpoints
        assert len(new.refs) == len(old.refs) and all(torch.equal(a, b) for a, b in zip(new.refs, old.refs))
        assert new.positive["c_crossattn"][0].shape == old.positive["c_crossattn"][0].shape
        assert torch.equal(new.fs, old.fs)
        # the image tokens: both paths against the fp32 oracle tower on the fp32 CPU preprocessing of the same frame
        x = frames[:1]
        y_old = model.embedder(x.to(DEV)).cpu()
        y_new = model.embedder.encode_on_device_front(x.to(DEV)).cpu()
        pre = (kornia_resize(x, (42, 42)) + 1.) / 2.
        pre = (pre - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
        want = oclip.vision_tokens(sd, pre, heads=2)
    e_new, e_old = rel_l2(y_new, want), rel_l2(y_old, want)
    print(f"image tokens vs the fp32 oracle tower: from_uint8 path {e_new:.3e}, existing path {e_old:.3e}")
    record("tokens tiny tower 64x64 -> 42", f"from_uint8 path {e_new:.3e}, existing path {e_old:.3e}")
    assert y_new.shape == y_old.shape == (1, 10, 160)
    assert e_new <= 1.25 * e_old, (e_new, e_old)


def test_synthesize_u8_returns_device_uint8_frames(tiny, g):
    from tooncrafter_amd import clip as pipeline
    model, _ = tiny
    h, w = (int(v) for v in g["e2e.size"])
    first, last = (torch.from_numpy(g["e2e.src"][i])[None].to(DEV) for i in range(2))
    plan = pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7)
    with torch.no_grad():
        video = pipeline.synthesize_u8(model, first, last, [1, 4, 4, h // 8, w // 8], size=(h, w), plan=plan, fs=10)
    assert video.shape == (1, 4, h, w, 3) and video.dtype == torch.uint8 and video.is_cuda
    # a clip's last frame is a keyframe the next clip can start from without leaving the device
    with torch.no_grad():
        nxt = pipeline.Conditions.from_uint8(model, video[:, -1], last, size=(h, w), t=4, fs=10)
    assert nxt.endpoints.shape == (1, 4, 4, h // 8, w // 8) and torch.isfinite(nxt.endpoints).all()
