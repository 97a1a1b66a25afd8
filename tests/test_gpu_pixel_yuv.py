"""The planar-YUV front end and the keyframe timeline on the MI355X (csrc/pixel_front.hip: tc_frames_from_yuv):

  * conversion, bit for bit: frames_from_yuv(planes) equals, under torch.equal, frames_from_u8 of the RGB image the numpy
    statement (tests/pixel_yuv_ref.py) makes of the same planes -- every format x siting at the sizes where an index can go
    wrong (2 x 2, odd both ways, one row, crop only, both resample passes with partial blocks), BT.709 full on two of them, and
    one case against PIL's resize and torch's value arithmetic, so that the composition is the script's transform;
  * layout: three images, pitched rows, a chroma plane away from its luma plane, guards around every plane and the output,
    frames no slot names, the six low bits of P010 words;
  * both bindings; the round trip through the back end on the device; Conditions.from_planes; synthesize_timeline_u8 against
    the synthesize_u8 calls it is made of, on the tiny model."""
import numpy as np
import pytest
import torch

import pixel_back_ref as back
import pixel_yuv_ref as ref
from conftest import load_golden
from test_gpu_pixel_front import tiny  # noqa: F401  (the tiny model with a tiny image tower, a module-scoped fixture)
from test_pixel_front_cpu import pil_resize

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMATS = ("i420", "nv12", "p010")
# (source size, target size): the smallest pictures at which an index can go wrong
SIZES = {
    "2x2_up": ((2, 2), (4, 6)),                    # one chroma sample: every neighbour index is clamped; the resize enlarges
    "5x7_odd": ((5, 7), (4, 6)),                   # odd both ways: the last chroma row and column cover one luma row / column
    "1x9_row": ((1, 9), (2, 6)),                   # a single row: j' is clamped both ways
    "64x96_crop": ((64, 96), (64, 80)),            # the shorter side is the target's already: no resize, crop only
    "300x290_both": ((300, 290), (64, 96)),        # both resample passes, partial blocks, bars left and right
}


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


def device_planes(planes, fmt, **options):
    from tooncrafter_amd import clip
    t = [torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in planes]
    return clip.Planes(t[0], tuple(t[1:]), fmt, **options)


def want_frames(hip, planes, fmt, size, slots, b, t, siting="center", standard="bt601", range_="limited"):
    """frames_from_u8 of the statement's RGB image"""
    m = ref.matrix(standard, range_, 10 if fmt == "p010" else 8)
    rgb = ref.rgb_image(planes, fmt, m, siting)
    return hip.frames_from_u8(torch.from_numpy(rgb).to(DEV), size, slots, b=b, t=t), rgb


# ------------------------------------------------------------------------------------------------ conversion, bit for bit

@pytest.mark.parametrize("siting", ref.SITINGS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", list(SIZES))
def test_frames_equal_frames_from_u8_of_the_statement(hip, case, fmt, siting):
    (sh, sw), size = SIZES[case]
    planes = ref.random_planes(np.random.default_rng(8100 + sh * sw), 1, sh, sw, fmt)
    got = hip.frames_from_yuv(device_planes(planes, fmt, siting=siting), size, [1], b=1, t=2)
    want, _ = want_frames(hip, planes, fmt, size, [1], 1, 2, siting)
    assert got.shape == (1, 3, 2, *size) and got.dtype == torch.float32
    assert torch.equal(got, want), (case, fmt, siting)
    assert not got[0, :, 0].any()                                                 # the frame no slot names


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", ["5x7_odd", "300x290_both"])
def test_bt709_full_range(hip, case, fmt):
    (sh, sw), size = SIZES[case]
    planes = ref.random_planes(np.random.default_rng(8200 + sh), 1, sh, sw, fmt)
    got = hip.frames_from_yuv(device_planes(planes, fmt, standard="bt709", range="full", siting="left"), size, [0], b=1, t=1)
    want, _ = want_frames(hip, planes, fmt, size, [0], 1, 1, "left", "bt709", "full")
    assert torch.equal(got, want)
    # a caller's own matrix is data too: the same integers given explicitly
    m = ref.matrix("bt709", "full", 10 if fmt == "p010" else 8)
    assert torch.equal(hip.frames_from_yuv(device_planes(planes, fmt, matrix=m, siting="left"), size, [0], b=1, t=1), want)


def half_even(d):
    q = d >> 1
    return q + 1 if (d & 1) and (q & 1) else q


def test_the_composition_is_the_scripts_transform(hip):
    """NV12 -> the statement's RGB -> PIL's resize (its numpy statement) -> CenterCrop -> torch's (v / 255 - 0.5) / 0.5"""
    (sh, sw), (h, w) = (40, 70), (16, 24)                                         # -> 16 x 28, cropped to 24 wide
    planes = ref.random_planes(np.random.default_rng(8300), 1, sh, sw, "nv12")
    rgb = ref.rgb_image(planes, "nv12", ref.matrix("bt601", "limited", 8), "center")[0]
    rh, rw = hip.resized_size(sh, sw, h, w)
    assert (rh, rw) == (16, 28)
    resized = pil_resize(rgb, rh, rw)
    top, left = half_even(rh - h), half_even(rw - w)
    crop = torch.from_numpy(resized[top:top + h, left:left + w].copy())
    want = (crop.permute(2, 0, 1).to(torch.float32).div(255.0) - 0.5) / 0.5
    got = hip.frames_from_yuv(device_planes(planes, "nv12"), (h, w), [0], b=1, t=1)
    assert torch.equal(got[0, :, 0].cpu(), want)


# ------------------------------------------------------------------------------------------------ layout

def carve(buf, offset, shape, strides, dtype):
    """a strided view of `dtype` elements into the uint8 device buffer `buf`, `offset` bytes in (strides in elements)"""
    es = torch.empty((), dtype=dtype).element_size()
    assert offset % es == 0
    typed = buf[offset:].view(dtype) if es > 1 else buf[offset:]
    return typed.as_strided(shape, strides)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pitched_planes_guards_and_untouched_slots(hip, fmt):
    """Three 5 x 7 images whose rows are padded, the chroma plane far from the luma plane and images apart by more than a plane,
    in one buffer of random bytes that must come back unchanged; the output between two guards of sentinels, in a clip tensor
    whose other frames keep theirs."""
    from tooncrafter_amd import clip
    n, sh, sw, (h, w) = 3, 5, 7, (4, 6)
    ch, cw = 3, 4
    planes = ref.random_planes(np.random.default_rng(8400), n, sh, sw, fmt, low_bits=True)
    dtype = torch.int16 if fmt == "p010" else torch.uint8                         # int16 words: the bits are what is read
    py, pc = sw + 5, (cw if fmt == "i420" else 2 * cw) + 6                        # pitches in elements
    sy, sc = sh * py + 14, ch * pc + 8                                            # image strides in elements
    held = torch.randint(0, 256, (8192,), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).to(DEV)
    y = carve(held, 64, (n, sh, sw), (sy, py, 1), dtype)
    cshape, cstr = ((n, ch, cw), (sc, pc, 1)) if fmt == "i420" else ((n, ch, cw, 2), (sc, pc, 2, 1))
    chroma = [carve(held, 4096 + 1024 * i, cshape, cstr, dtype) for i in range(len(planes) - 1)]      # not where luma ends
    for dst, p in zip([y] + chroma, planes):
        dst.copy_(torch.from_numpy(p.view(np.int16) if fmt == "p010" else p).to(DEV))
    before = held.clone()
    b, t, guard, sentinel = 2, 4, 1024, -77.0
    buf = torch.full((guard + b * 3 * t * h * w + guard,), sentinel, dtype=torch.float32, device=DEV)
    out = buf[guard:guard + b * 3 * t * h * w].view(b, 3, t, h, w)
    slots = [(0, 0), (0, t - 1), (1, 0)]
    res = clip.frames_from_planes(clip.Planes(y, tuple(chroma), fmt), (h, w), slots, t, out=out)
    assert res is out and torch.equal(held, before)
    want, _ = want_frames(hip, planes, fmt, (h, w), [i * t + f for i, f in slots], b, t)
    named = torch.zeros(b, t, dtype=torch.bool)
    for i, f in slots:
        named[i, f] = True
        assert torch.equal(out[i, :, f], want[i, :, f]), (i, f)
    got = out.cpu()
    assert (got.permute(0, 2, 1, 3, 4)[~named] == sentinel).all()
    assert (buf[:guard] == sentinel).all() and (buf[-guard:] == sentinel).all()
    # without `out`: a new tensor, zero where no slot points; both bindings
    from tooncrafter_amd import torch_ops
    for ops in (hip, torch_ops.TorchLibOps()):
        fresh = ops.frames_from_yuv(clip.Planes(y, tuple(chroma), fmt), (h, w), [i * t + f for i, f in slots], b=b, t=t)
        assert torch.equal(fresh, want)


def test_p010_low_six_bits_are_ignored(hip):
    (sh, sw), size = SIZES["5x7_odd"]
    clean = ref.random_planes(np.random.default_rng(8500), 1, sh, sw, "p010")
    noise = np.random.default_rng(8501)
    dirty = tuple(p | noise.integers(0, 64, p.shape).astype(np.uint16) for p in clean)
    assert any((a != b).any() for a, b in zip(clean, dirty))
    a = hip.frames_from_yuv(device_planes(clean, "p010"), size, [0], b=1, t=1)
    b = hip.frames_from_yuv(device_planes(dirty, "p010"), size, [0], b=1, t=1)
    assert torch.equal(a, b)
    # int16 words are the same bits
    c = hip.frames_from_yuv(device_planes(tuple(p.view(np.int16) for p in dirty), "p010"), size, [0], b=1, t=1)
    assert torch.equal(a, c)


def test_more_images_than_one_call_takes(hip):
    """17 NV12 images of 5 x 7 (resized to 4 x 5: both passes run) into slots 0 .. 16 of a (2, 3, 9, 4, 6) clip tensor, which
    takes two calls of the entry point: the same images sent one to a call into a zeroed `out`, and slot 17 stays zero."""
    from tooncrafter_amd import _lib
    n, b, t, size = _lib.TC_FRAMES_U8_MAX + 1, 2, 9, (4, 6)
    assert n == 17 and hip.resized_size(5, 7, *size) == (4, 5)
    planes = device_planes(ref.random_planes(np.random.default_rng(8450), n, 5, 7, "nv12"), "nv12")
    got = hip.frames_from_yuv(planes, size, list(range(n)), b=b, t=t)
    want = torch.zeros(b, 3, t, *size, dtype=torch.float32, device=DEV)
    for i in range(n):
        hip.frames_from_yuv(planes[i:i + 1], size, [i], b=b, t=t, out=want)
    assert got.shape == want.shape and torch.equal(got, want)
    assert want[1, :, 7].any() and not got[1, :, 8].any()                         # slot 16 is written, slot 17 = (1, 8) is not


# ------------------------------------------------------------------------------------------------ bindings

@pytest.mark.parametrize("case,fmt,siting", [("5x7_odd", "i420", "center"), ("64x96_crop", "nv12", "left"), ("300x290_both", "p010", "nearest")])
def test_torch_op_binding_equals_ctypes(hip, case, fmt, siting):
    from tooncrafter_amd import _lib, torch_ops
    tl = torch_ops.TorchLibOps()
    (sh, sw), size = SIZES[case]
    planes = device_planes(ref.random_planes(np.random.default_rng(8600 + sh), 2, sh, sw, fmt), fmt, siting=siting)
    a = hip.frames_from_yuv(planes, size, [2, 3], b=2, t=3)
    b = tl.frames_from_yuv(planes, size, [2, 3], b=2, t=3)
    assert torch.equal(a, b) and a[0, :, 2].any() and not a[0, :, :2].any()
    m = hip.yuv_matrix("bt601", "limited", 10 if fmt == "p010" else 8)
    with pytest.raises(RuntimeError, match="outside the clip tensor"):             # the op checks the slots the C entry point would refuse
        tl.t.frames_from_yuv(planes.y, planes.chroma[0], planes.chroma[1] if fmt == "i420" else None, _lib.TC_YUV_FORMATS[fmt], m,
                             _lib.TC_CHROMA_SITINGS[siting], [0, 6], 2, 3, size[0], size[1], None, None, None, None)


# ------------------------------------------------------------------------------------------------ round trip on the device

@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_round_trip_through_the_back_end(hip, fmt):
    """The 52^3 colour grid (0, 5, .. 255 per channel) as 2 x 2 blocks of one colour: 52 frames of 52 x 52 blocks, 104 x 104
    pixels each (one frame holds 52^2 blocks, so the grid's third axis is the frame).  tc_frames_to_u8 to planes,
    planes_from_packed, frames_from_yuv(NEAREST): within (1, 1, 2) code values of tc_video_to_u8 of the same clip."""
    from tooncrafter_amd import clip
    v = np.arange(52) * 5
    r, g, b = np.meshgrid(v, v, v, indexing="ij")                                  # frame, block row, block column
    codes = np.stack([r, g, b], axis=0).repeat(2, axis=2).repeat(2, axis=3)        # (3, 52, 104, 104)
    x = torch.from_numpy(((codes + 0.5) / 255.0 * 2.0 - 1.0).astype(np.float32))[None].to(DEV)
    direct = hip.video_to_uint8(x)                                                # (1, 52, 104, 104, 3)
    assert np.array_equal(direct[0].cpu().numpy(), codes.transpose(1, 2, 3, 0))
    packed = hip.frames_to_u8(x, fmt=fmt)                                         # (1, 52, 104 * 104 * 3 / 2)
    planes = clip.planes_from_packed(packed, 104, 104, fmt, siting="nearest")
    assert len(planes) == 52 and planes.y.data_ptr() == packed.data_ptr()
    back_f = clip.frames_from_planes(planes, (104, 104), [(0, f) for f in range(52)], 52)      # four calls of at most 16 images
    # every value is a byte's (v / 255 - 0.5) / 0.5: rounding (not truncating) v' * 127.5 + 127.5 gives the byte back
    back_u8 = (back_f.double() * 127.5 + 127.5).round().to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()
    err = (back_u8.to(torch.int16) - direct.to(torch.int16)).abs().flatten(0, 3).max(dim=0).values.cpu().tolist()
    print(f"round trip through {fmt}: worst error in (R, G, B) {err}")
    assert err[0] <= 1 and err[1] <= 1 and err[2] <= 2, err
    # and bit for bit the statement's RGB of the planes the back end wrote
    flat = packed[0].cpu().numpy()
    n = 104 * 104
    y = flat[:, :n].reshape(52, 104, 104)
    if fmt == "i420":
        cb, cr = flat[:, n:n + n // 4].reshape(52, 52, 52), flat[:, n + n // 4:].reshape(52, 52, 52)
    else:
        cbcr = flat[:, n:].reshape(52, 52, 52, 2)
        cb, cr = cbcr[..., 0], cbcr[..., 1]
    rgb = ref.to_rgb(y, ref.upsample(cb, 104, 104, "nearest"), ref.upsample(cr, 104, 104, "nearest"), ref.matrix("bt601", "limited", 8))
    assert np.array_equal(back_u8[0].cpu().numpy(), rgb)


# ------------------------------------------------------------------------------------------------ conditions and the timeline

@pytest.fixture(scope="module")
def g():
    return load_golden("pixel_front.npz")


def nv12_of(rgb):
    """(n, h, w, 3) uint8, even sizes -> NV12 planes (y, cbcr) by the back end's integer rule"""
    y, cb, cr = back.yuv420(rgb)
    return y, np.stack([cb, cr], axis=-1)


def test_conditions_from_planes_equal_conditions_from_uint8(tiny, g):  # noqa: F811
    from tooncrafter_amd import clip as pipeline
    model, _ = tiny
    h, w = (int(v) for v in g["e2e.size"])
    src = np.ascontiguousarray(g["e2e.src"][:, :36, :52])                          # the fixture's frames, cut to an even size
    planes = nv12_of(src)
    rgb = ref.rgb_image(planes, "nv12", ref.matrix("bt601", "limited", 8), "center")      # what those planes hold, as RGB
    first_u8, last_u8 = (torch.from_numpy(rgb[i:i + 1]).to(DEV) for i in range(2))
    both = device_planes(planes, "nv12")
    with torch.no_grad():
        new = pipeline.Conditions.from_planes(model, both[0:1], both[1:2], size=(h, w), t=4, fs=10)
        old = pipeline.Conditions.from_uint8(model, first_u8, last_u8, size=(h, w), t=4, fs=10)
    assert torch.equal(new.endpoints, old.endpoints) and new.endpoints.shape == (1, 4, 4, h // 8, w // 8)
    assert torch.equal(new.positive["c_concat"][0], old.positive["c_concat"][0]) and new.negative["c_concat"][0] is new.endpoints
    assert len(new.refs) == len(old.refs) and all(torch.equal(a, b) for a, b in zip(new.refs, old.refs))
    assert torch.equal(new.positive["c_crossattn"][0], old.positive["c_crossattn"][0])
    assert torch.equal(new.fs, old.fs)


@pytest.fixture(scope="module")
def keyframes(g):
    """four uint8 keyframes on the device: the fixture's two, and two made of them"""
    a, b = g["e2e.src"][0], g["e2e.src"][1]
    return torch.from_numpy(np.stack([a, b, a[::-1, ::-1].copy(), 255 - b])).to(DEV)


def plan_with(seeds):
    from tooncrafter_amd import clip as pipeline
    return pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=seeds)


def splice(clips):
    """the header's rule in numpy: all of clip 0, frames 1 .. t-1 of every later clip"""
    clips = [c.cpu().numpy() for c in clips]
    return np.concatenate([clips[0]] + [c[1:] for c in clips[1:]], axis=0)


@pytest.mark.parametrize("fmt", ["rgb24", "i420"])
def test_timeline_of_three_keyframes_is_its_two_synthesize_u8_calls(tiny, keyframes, g, fmt, tmp_path):  # noqa: F811
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd import mp4
    model, _ = tiny
    h, w = (int(v) for v in g["e2e.size"])
    shape, s0, s1 = [1, 4, 4, h // 8, w // 8], 11, (1 << 63) + 5
    with torch.no_grad():
        video = pipeline.synthesize_timeline_u8(model, keyframes[:3], shape, size=(h, w), plan=plan_with([s0, s1]), fs=10, out_fmt=fmt)
        parts = [pipeline.synthesize_u8(model, keyframes[i:i + 1], keyframes[i + 1:i + 2], shape, size=(h, w), plan=plan_with([s]), fs=10,
                                        out_fmt=fmt)[0] for i, s in enumerate((s0, s1))]
    assert video.shape == ((7, h, w, 3) if fmt == "rgb24" else (7, h * w * 3 // 2)) and video.dtype == torch.uint8 and video.is_cuda
    assert np.array_equal(video.cpu().numpy(), splice(parts))
    assert not np.array_equal(parts[0].cpu().numpy(), parts[1].cpu().numpy())
    if fmt == "i420":                                                             # the buffer is what the writer takes
        path = mp4.write_mp4_i420(str(tmp_path / "timeline.mp4"), video.cpu(), w, h, 8)
        assert (tmp_path / "timeline.mp4").stat().st_size > 7 * h * w and path.endswith("timeline.mp4")


def test_timeline_in_batches_of_two(tiny, keyframes, g):  # noqa: F811
    from tooncrafter_amd import clip as pipeline
    model, _ = tiny
    h, w = (int(v) for v in g["e2e.size"])
    shape, seeds = [2, 4, 4, h // 8, w // 8], [21, 22, 23]
    with torch.no_grad():
        video = pipeline.synthesize_timeline_u8(model, keyframes[:3], shape, size=(h, w), plan=plan_with(seeds[:2]), fs=10)
        pair = pipeline.synthesize_u8(model, keyframes[:2], keyframes[1:3], shape, size=(h, w), plan=plan_with(seeds[:2]), fs=10)
        assert np.array_equal(video.cpu().numpy(), splice([pair[0], pair[1]]))
        # four keyframes: a full batch and a short one
        longer = pipeline.synthesize_timeline_u8(model, keyframes, shape, size=(h, w), plan=plan_with(seeds), fs=10)
    assert longer.shape == (10, h, w, 3) and longer.dtype == torch.uint8
    assert torch.equal(longer[:7], video)                                         # the first batch is the same request
    assert longer[7:].float().std() > 0


def test_timeline_from_planes(tiny, keyframes, g):  # noqa: F811
    """NV12 keyframes: the timeline of the planes is the timeline of the RGB the statement makes of them"""
    from tooncrafter_amd import clip as pipeline
    model, _ = tiny
    h, w = (int(v) for v in g["e2e.size"])
    planes = nv12_of(np.ascontiguousarray(keyframes[:3, :36, :52].cpu().numpy()))
    rgb = torch.from_numpy(ref.rgb_image(planes, "nv12", ref.matrix("bt601", "limited", 8), "center")).to(DEV)
    shape = [1, 4, 4, h // 8, w // 8]
    with torch.no_grad():
        a = pipeline.synthesize_timeline_u8(model, device_planes(planes, "nv12"), shape, size=(h, w), plan=plan_with([31, 32]), fs=10)
        b = pipeline.synthesize_timeline_u8(model, rgb, shape, size=(h, w), plan=plan_with([31, 32]), fs=10)
    assert a.shape == (7, h, w, 3) and torch.equal(a, b)


def test_timeline_with_every_option_is_its_parts(tiny, keyframes, g):  # noqa: F811
    """shots, still, match, a planar format and a named colour at once: segments 0 and 2 are their synthesize_u8 calls with the
    same options, the held segment 1 is the writer's bytes of its two keyframes (e2e.size is a multiple of 8, as still= needs)"""
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd.output import Colour, ColourMatch, clip_to_uint8
    model, _ = tiny
    h, w = (int(v) for v in g["e2e.size"])
    assert h % 8 == 0 and w % 8 == 0
    shape, seeds = [1, 4, 4, h // 8, w // 8], [41, 42, (1 << 62) + 43]
    options = dict(size=(h, w), fs=10, still=pipeline.StillRegions(), match=ColourMatch("mkl", 0.5), out_fmt="nv12",
                   out_colour=Colour("bt709", "full", "left"))
    with torch.no_grad():
        video = pipeline.synthesize_timeline_u8(model, keyframes, shape, plan=plan_with(seeds),
                                                shots=pipeline.ShotPlan(("tween", "hold", "tween")), **options)
        first, third = (pipeline.synthesize_u8(model, keyframes[i:i + 1], keyframes[i + 1:i + 2], shape, plan=plan_with([seeds[i]]),
                                               **options)[0] for i in (0, 2))
        ends = pipeline.frames_from_uint8(keyframes[1:3], (h, w), [(0, 0), (0, 1)], 2)
        held = clip_to_uint8(ends[:, :, [0, 0, 0, 1]], fmt="nv12", colour=options["out_colour"])[0]
    assert video.shape == (10, h * w * 3 // 2) and video.dtype == torch.uint8 and video.is_cuda
    assert np.array_equal(video.cpu().numpy(), splice([first, held, third]))
    assert not torch.equal(first, third) and not torch.equal(video[1], video[2]) and torch.equal(video[4], video[5])
