"""Planar frames out in a named colour on the MI355X (csrc/pixel_back.hip: tc_frames_to_yuv), bit for bit against the numpy
statement of tests/pixel_colour_ref.py, through both bindings (HipOps, TorchLibOps):

  * with the BT.601 limited 8-bit matrix and centre siting the new entry point writes tc_frames_to_u8's bytes;
  * 8 bit: BT.709 limited, BT.601 full, BT.709 full x centre / left x I420 / NV12, resampled and at the clip's own size;
  * P010: the 16-bit value, the 16-bit resample (upscale with overshoot, downscale with many taps) and the 24-bit colour step;
  * saturated colours and samples outside [-1, 1]; left siting at the picture's left edge;
  * placement into a sentinel buffer of which every byte is compared; refusals leave it untouched;
  * the round trip through the front end, against the statements of both directions; the keyframe timeline in its source's
    colour.

Nothing expected comes from the kernels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pixel_colour_ref as ref
import pixel_yuv_ref as front
from conftest import load_golden
from test_gpu_pixel_front import tiny  # noqa: F401  (the tiny model with a tiny image tower, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
CASES_8 = [("bt709", "limited"), ("bt601", "full"), ("bt709", "full")]
CASES_10 = [("bt709", "limited"), ("bt601", "full")]


@pytest.fixture(scope="module")
def g():
    return load_golden("pixel_back.npz")


@pytest.fixture(scope="module")
def x(g):
    return torch.from_numpy(g["x"]).to(DEV)


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def tl():
    from tooncrafter_amd.torch_ops import TorchLibOps
    return TorchLibOps()


@functools.lru_cache(maxsize=None)
def golden_rgb(size, name, bits):
    """the statement's resized RGB frames of the fixture's clip, computed once per (size, filter, depth) and left unchanged"""
    rgb = ref.rgb_frames(load_golden("pixel_back.npz")["x"], size, name, bits)
    rgb.setflags(write=False)
    return rgb


def colour_of(standard, range_, siting, bits=8):
    from tooncrafter_amd.output import Colour
    return Colour(standard, range_, siting, bits)


def want_packed(size, name, fmt, c):
    return ref.packed(golden_rgb(size, name, c.bits), "p010" if c.bits == 10 else fmt, ref.out_matrix(c.standard, c.range, c.bits), c.siting)


def same(t, want):
    return t.dtype == torch.uint8 and tuple(t.shape) == want.shape and np.array_equal(t.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the old entry point is inside

@pytest.mark.parametrize("size", [(46, 72), None], ids=["46x72", "identity"])
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_bt601_limited_centre_is_frames_to_u8(hip, tl, x, fmt, size):
    c = colour_of("bt601", "limited", "center")
    old = hip.frames_to_u8(x, size=size, fmt=fmt)
    assert same(old, want_packed(size, "bicubic", fmt, c))                        # the general statement contains the 601 one
    for ops in (hip, tl):
        assert torch.equal(ops.frames_to_yuv(x, size=size, fmt=fmt, colour=c), old)


# ------------------------------------------------------------------------------------------------ 8 bit

@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("siting", ["center", "left"])
@pytest.mark.parametrize("case", CASES_8, ids=lambda c: "-".join(c))
def test_8bit_colours_equal_the_statement(hip, tl, x, case, siting, fmt):
    c = colour_of(*case, siting)
    for size in ((46, 72), None):
        want = want_packed(size, "bicubic", fmt, c)
        oh, ow = size or (20, 32)
        assert want.shape == (2, 3, oh * ow * 3 // 2)
        assert same(hip.frames_to_yuv(x, size=size, fmt=fmt, colour=c), want), size
        assert same(tl.frames_to_yuv(x, size=size, fmt=fmt, colour=c), want), size
    assert not np.array_equal(want, want_packed(None, "bicubic", fmt, colour_of("bt601", "limited", siting)))      # the case says something


# ------------------------------------------------------------------------------------------------ P010

@pytest.mark.parametrize("size,name", [(None, "bicubic"), ((46, 72), "lanczos"), ((14, 22), "box")], ids=["identity", "46x72-lanczos", "14x22-box"])
@pytest.mark.parametrize("siting", ["center", "left"])
@pytest.mark.parametrize("case", CASES_10, ids=lambda c: "-".join(c))
def test_p010_equals_the_statement(hip, tl, x, case, siting, size, name):
    c = colour_of(*case, siting, 10)
    want = want_packed(size, name, "nv12", c)
    oh, ow = size or (20, 32)
    assert want.shape == (2, 3, oh * ow * 3)
    for ops in (hip, tl):
        got = ops.frames_to_yuv(x, size=size, filter=name, fmt="nv12", colour=c)
        assert same(got, want)
        words = got.cpu().numpy().view("<u2")
        assert not (words & 63).any() and (words >> 6).max() > 255                # ten bits in the upper end of each word
    if size == (46, 72):                                                          # the upscale overshoots: the 16-bit clip works
        rgb = golden_rgb(size, name, 10)
        assert (rgb == 0).any() and (rgb == 65535).any()


# ------------------------------------------------------------------------------------------------ saturated colours, the left edge

def test_saturated_colours_stay_inside_their_range(hip, tl):
    """4 x 4 frames: black, white, the six other cube corners, and one frame far outside [-1, 1] (the value step clamps)"""
    corners = [(r, g, b) for r in (-1.0, 1.0) for g in (-1.0, 1.0) for b in (-1.0, 1.0)]
    frames = np.empty((1, 3, 9, 4, 4), np.float32)
    for f, rgb in enumerate(corners):
        frames[0, :, f] = np.array(rgb, np.float32)[:, None, None]
    frames[0, :, 8] = np.linspace(-7.0, 9.0, 48, dtype=np.float32).reshape(3, 4, 4)
    xs = torch.from_numpy(frames).to(DEV)
    for bits, (lo, hi, top) in ((8, (16, 235, 255)), (10, (64, 940, 1023))):
        rgb = ref.rgb_frames(frames, None, "bicubic", bits)
        for case in (("bt709", "limited"), ("bt601", "full"), ("bt709", "full")):
            for siting in ("center", "left"):
                c = colour_of(*case, siting, bits)
                m = ref.out_matrix(c.standard, c.range, bits)
                want = ref.packed(rgb, "p010" if bits == 10 else "nv12", m, siting)
                for ops in (hip, tl):
                    assert same(ops.frames_to_yuv(xs, fmt="nv12", colour=c), want), (case, siting, bits)
                y, cb, cr = ref.yuv420(rgb[0], m, siting, bits)
                if case[1] == "limited":
                    assert y.min() == lo and y.max() == hi                        # black and white land exactly
                else:
                    assert y.min() == 0 and y.max() == top
                    assert cb[1].max() == top and cr[4].max() == top              # blue (frame 1) / red (frame 4): 256 q before the clip
                assert (cb[0] == 128 << (bits - 8)).all() and (cr[7] == 128 << (bits - 8)).all()      # black, white: neutral


@pytest.mark.parametrize("bits", [8, 10])
def test_left_siting_clamps_at_the_left_edge(hip, bits):
    """column 0 differs from column 1 in every channel: chroma sample bx = 0 takes P[0] three times (the clamped tap, twice
    itself) and P[1] once, per row"""
    frame = np.empty((1, 3, 1, 4, 6), np.float32)
    frame[0, :, 0] = np.array([-0.9, 0.1, 0.7], np.float32)[:, None, None]
    frame[0, :, 0, :, 0] = np.array([[0.8, -0.6, -0.2]], np.float32).T
    frame[0, :, 0, 2:, 1] = np.array([[0.3, 0.9, -1.0]], np.float32).T
    c = colour_of("bt709", "limited", "left", bits)
    m = ref.out_matrix("bt709", "limited", bits)
    rgb = ref.rgb_frames(frame, None, "bicubic", bits)
    got = hip.frames_to_yuv(torch.from_numpy(frame).to(DEV), fmt="nv12", colour=c)
    assert same(got, ref.packed(rgb, "p010" if bits == 10 else "nv12", m, "left"))
    # the first chroma sample of each chroma row, written out
    p = rgb[0, 0].astype(np.int64)
    F, top = ref.depth(bits)[1:]
    samples = got[0, 0].cpu().numpy().view("<u2") >> 6 if bits == 10 else got[0, 0].cpu().numpy()
    chroma = samples[4 * 6:].reshape(2, 3, 2)
    for by in range(2):
        s = sum(3 * p[2 * by + dy, 0] + p[2 * by + dy, 1] for dy in range(2))
        for k, row in enumerate((m[3:6], m[6:9])):
            want = np.clip((row[0] * s[0] + row[1] * s[1] + row[2] * s[2] + (m[10] << (F + 3)) + (1 << (F + 2))) >> (F + 3), 0, top)
            assert chroma[by, 0, k] == want
    assert not np.array_equal(chroma[:, 0, 0], ref.yuv420(rgb[0, 0], m, "center", bits)[1][:, 0])      # the siting matters here


# ------------------------------------------------------------------------------------------------ placement and refusals

def hip_params(hip, x, out, size, name, code, c, f0, nf, pitch, frame_stride, clip_stride):
    """the C struct filled by hand (tables from HipOps' caches)"""
    from tooncrafter_amd import _lib
    b, _, t, h, w = x.shape
    m = ref.out_matrix(c.standard, c.range, c.bits)
    p = _lib.TcFramesYuvOutParams(x=x.data_ptr(), out=out.data_ptr(), b=b, t=t, h=h, w=w, f0=f0, nf=nf, oh=size[0], ow=size[1], format=code,
                                  pitch=pitch, frame_stride=frame_stride, clip_stride=clip_stride, siting=ref.SITINGS[c.siting],
                                  m=(C.c_int32 * 11)(*m))
    if size[1] != w:
        hb, hc = hip.resize_tables_filter(name, w, size[1], x.device)
        p.h_bounds, p.h_coefs, p.h_kmax = hb.data_ptr(), hc.data_ptr(), hc.shape[1]
    if size[0] != h:
        vb, vc = hip.resize_tables_filter(name, h, size[0], x.device)
        p.v_bounds, p.v_coefs, p.v_kmax = vb.data_ptr(), vc.data_ptr(), vc.shape[1]
    return p


@pytest.mark.parametrize("bits", [8, 10], ids=["nv12", "p010"])
def test_placement_touches_only_the_addressed_bytes(hip, x, bits):
    """b = 2, frames 1 and 2 of each clip, rows 6 bytes longer than their samples, slack between frames and between clips, a
    guard in front, the last frame ending where the allocation ends: the whole buffer is compared."""
    from tooncrafter_amd import _lib
    size, es = (46, 72), 1 if bits == 8 else 2
    oh, ow = size
    c = colour_of("bt709", "limited", "left", bits)
    m = ref.out_matrix(c.standard, c.range, bits)
    fmt = "p010" if bits == 10 else "nv12"
    rgb = golden_rgb(size, "bicubic", bits)
    f0, nf, guard = 1, 2, 512
    pitch = es * ow + 6
    fb = ref.frame_bytes(fmt, oh, pitch)
    frame_stride = fb + 38
    clip_stride = nf * frame_stride + 102
    total = guard + clip_stride + frame_stride + fb
    want = np.full(total, SENTINEL, np.uint8)
    for i in range(2):
        for j in range(nf):
            ref.place(want[guard + i * clip_stride + j * frame_stride:], rgb[i, f0 + j], fmt, pitch, m, c.siting)
    assert (want[guard:] != SENTINEL).any() and (want[:guard] == SENTINEL).all()
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    p = hip_params(hip, x, buf[guard:], size, "bicubic", ref.FORMATS[fmt], c, f0, nf, pitch, frame_stride, clip_stride)
    need = hip.lib.tc_frames_to_yuv_workspace(C.byref(p))
    assert need == es * (4 * 20 * 32 * 3 + 4 * 20 * 72 * 3)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    _lib.check(hip.lib.tc_frames_to_yuv(C.byref(p), torch.cuda.current_stream().cuda_stream), "tc_frames_to_yuv")
    assert np.array_equal(buf.cpu().numpy(), want)
    buf2 = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf2[guard:]
    kw = dict(size=size, fmt="nv12", colour=c, frames=(f0, nf), strides=(pitch, frame_stride, clip_stride))
    assert hip.frames_to_yuv(x, out=view, **kw) is view
    assert np.array_equal(buf2.cpu().numpy(), want)
    with pytest.raises(ValueError):                                               # one byte short: refused on the host
        hip.frames_to_yuv(x, out=view[:-1], **kw)


def test_refused_requests_write_nothing(hip, x):
    from tooncrafter_amd._lib import TooncrafterHipError
    out = torch.full((1 << 17,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    c8, c10 = colour_of("bt709", "limited", "left"), colour_of("bt709", "limited", "left", 10)

    def rc(*args):
        p = hip_params(hip, x, out, *args)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        return hip.lib.tc_frames_to_yuv(C.byref(p), stream)
    for size in ((45, 72), (46, 71), (21, 32)):                                   # odd sizes
        assert rc(size, "bicubic", 2, c8, 0, 1, 80, 80 * 72, 80 * 72) == -3
        assert rc(size, "bicubic", 3, c10, 0, 1, 160, 160 * 72, 160 * 72) == -3
        with pytest.raises(ValueError):
            hip.frames_to_yuv(x, size=size, fmt="nv12", colour=c10)
    assert rc((46, 72), "bicubic", 3, c10, 0, 1, 151, 151 * 69, 151 * 69 + 1) == -2      # P010: an odd pitch
    assert rc((46, 72), "bicubic", 3, c10, 0, 2, 150, 150 * 69 + 1, 2 * 150 * 69 + 2) == -2      # ... an odd frame stride
    with pytest.raises(TooncrafterHipError):
        hip.frames_to_yuv(x, size=(46, 72), fmt="nv12", colour=c10, frames=(0, 1), out=out, strides=(151, 151 * 69, 151 * 69 + 1))
    assert rc((46, 72), "bicubic", 0, c8, 0, 1, 216, 216 * 46, 216 * 46) == -1    # RGB24 is the other entry point's
    p = hip_params(hip, x, out, (46, 72), "bicubic", 2, c8, 0, 1, 80, 80 * 69, 80 * 69)
    p.siting = 0                                                                  # NEAREST
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    assert hip.lib.tc_frames_to_yuv(C.byref(p), stream) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ round trip, timeline

@pytest.mark.parametrize("bits", [8, 10])
def test_round_trip_equals_the_statements_of_both_directions(hip, x, bits):
    """clip_to_uint8(fmt="nv12", colour=) -> planes_from_frames -> frames_from_planes at the clip's own size: the front end's
    statement (tests/pixel_yuv_ref.py) applied to the back end's statement of the planes"""
    from tooncrafter_amd import clip, ops, output
    c = colour_of("bt709", "limited", "left", bits)
    prev = ops.set_backend(hip)
    try:
        packed = output.clip_to_uint8(x, fmt="nv12", colour=c)
        assert same(packed, want_packed(None, "bicubic", "nv12", c))
        planes = clip.planes_from_frames(packed, 20, 32, "nv12", c)
        assert len(planes) == 6 and planes.y.data_ptr() == packed.data_ptr() and planes.fmt == ("p010" if bits == 10 else "nv12")
        assert output.Colour.of(planes) == c
        slots = [(i, f) for i in range(2) for f in range(3)]
        got = clip.frames_from_planes(planes, (20, 32), slots, 3)
    finally:
        ops.set_backend(prev)
    y, cb, cr = ref.yuv420(golden_rgb(None, "bicubic", bits).reshape(6, 20, 32, 3), ref.out_matrix("bt709", "limited", bits), "left", bits)
    stored = (y, np.stack([cb, cr], axis=-1))
    if bits == 10:
        stored = tuple((v.astype(np.uint16) << 6) for v in stored)
    else:
        stored = tuple(v.astype(np.uint8) for v in stored)
    rgb = front.rgb_image(stored, "p010" if bits == 10 else "nv12", front.matrix("bt709", "limited", bits), "left")
    want = hip.frames_from_u8(torch.from_numpy(rgb).to(DEV), (20, 32), [i * 3 + f for i, f in slots], b=2, t=3)
    assert got.shape == (2, 3, 3, 20, 32) and torch.equal(got, want)


def test_timeline_leaves_in_the_colour_it_came_in(tiny):  # noqa: F811
    """three BT.709 NV12 keyframes, out_colour="source": the video is the per-segment synthesize_u8(out_colour=Colour.of(kf))
    pieces, spliced by timeline_layout's rule"""
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd.output import Colour
    model, _ = tiny
    fr = load_golden("pixel_front.npz")
    h, w = (int(v) for v in fr["e2e.size"])
    a, b = fr["e2e.src"][0][:36, :52], fr["e2e.src"][1][:36, :52]
    src = np.ascontiguousarray(np.stack([a, b, a[::-1, ::-1]]))
    y, cb, cr = ref.yuv420(src, ref.out_matrix("bt709", "limited", 8), "left", 8)
    stored = (y.astype(np.uint8), np.stack([cb, cr], axis=-1).astype(np.uint8))
    t = [torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in stored]
    keyframes = pipeline.Planes(t[0], (t[1],), "nv12", standard="bt709", range="limited", siting="left")
    c = Colour.of(keyframes)
    assert c == Colour("bt709", "limited", "left", 8)
    rgb = torch.from_numpy(front.rgb_image(stored, "nv12", front.matrix("bt709", "limited", 8), "left")).to(DEV)
    shape, seeds = [1, 4, 4, h // 8, w // 8], [41, 42]

    def plan(s):
        return pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=s)
    with torch.no_grad():
        video = pipeline.synthesize_timeline_u8(model, keyframes, shape, size=(h, w), plan=plan(seeds), fs=10, out_fmt="nv12",
                                                out_colour="source")
        parts = [pipeline.synthesize_u8(model, rgb[i:i + 1], rgb[i + 1:i + 2], shape, size=(h, w), plan=plan([s]), fs=10, out_fmt="nv12",
                                        out_colour=c)[0] for i, s in enumerate(seeds)]
        plain = pipeline.synthesize_u8(model, rgb[:1], rgb[1:2], shape, size=(h, w), plan=plan(seeds[:1]), fs=10, out_fmt="nv12")[0]
    total, frame, batches = pipeline.timeline_layout(3, 4, 1, (h, w), "nv12", c)
    assert video.shape == (total, frame) == (7, h * w * 3 // 2) and video.dtype == torch.uint8 and video.is_cuda
    want = np.concatenate([parts[0].cpu().numpy()] + [p.cpu().numpy()[1:] for p in parts[1:]], axis=0)
    assert np.array_equal(video.cpu().numpy(), want)
    assert not torch.equal(parts[0], plain)                                       # BT.709 / left is not the default's bytes
    # the same timeline as P010, two segments in one batch: twice the bytes per frame, spliced by the same rule
    c10 = Colour("bt709", "limited", "left", 10)
    with torch.no_grad():
        wide = pipeline.synthesize_timeline_u8(model, keyframes, [2, *shape[1:]], size=(h, w), plan=plan(seeds), fs=10, out_fmt="nv12",
                                               out_colour=c10)
        pair = pipeline.synthesize_u8(model, rgb[:2], rgb[1:3], [2, *shape[1:]], size=(h, w), plan=plan(seeds), fs=10, out_fmt="nv12",
                                      out_colour=c10)
    assert wide.shape == (7, h * w * 3) == pipeline.timeline_layout(3, 4, 2, (h, w), "nv12", c10)[:2]
    assert torch.equal(wide, torch.cat([pair[0], pair[1, 1:]]))
    words = wide.cpu().numpy().view("<u2")
    assert not (words & 63).any() and (words >> 6).max() > 255
