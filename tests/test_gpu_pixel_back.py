"""The pixel back end on the MI355X (csrc/pixel_back.hip), bit for bit:

  * identity: packed RGB at the clip's own size is tc_video_to_u8's bytes;
  * resample: bicubic, Lanczos, bilinear and box against tests/golden/pixel_back.npz -- what PIL.Image.resize makes of the same
    uint8 frames -- for a non-integer upscale, a downscale, a horizontal-only and a vertical-only case;
  * formats: I420 and NV12 equal the integer BT.601 statement (tests/pixel_back_ref.py) applied to the expected RGB;
  * placement: padded rows, slack between frames and clips, a first frame other than 0, into a buffer of sentinels of which
    every byte is compared; two clips spliced into one video; one call under graph capture.

Everything expected comes from the fixture and the numpy statement; PIL is not used here.  The calls go through the C ABI
(ctypes: HipOps, or the struct filled by hand) and, for a subset, through the custom op (TorchLibOps)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pixel_back_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(46, 72), (14, 22), (20, 50), (34, 32)]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def g():
    return load_golden("pixel_back.npz")


@pytest.fixture(scope="module")
def x(g):
    return torch.from_numpy(g["x"]).to(DEV)


@pytest.fixture(scope="module")
def u8(g):
    """the clip's uint8 frames (b, t, h, w, 3) by the statement; test_identity ties them to tc_video_to_u8"""
    return ref.to_u8(g["x"])


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def tl():
    from tooncrafter_amd.torch_ops import TorchLibOps
    return TorchLibOps()


def expected_rgb(g, u8, size, name):
    return u8 if size is None or tuple(size) == u8.shape[2:4] else g[f"{name}.{size[0]}x{size[1]}"]


def same(t, want):
    return t.dtype == torch.uint8 and tuple(t.shape) == want.shape and np.array_equal(t.cpu().numpy(), want)


def test_identity_is_tc_video_to_u8(hip, tl, x, u8):
    want = hip.video_to_uint8(x)
    assert same(want, u8)                                                         # the statement's value rule is the kernel's
    for ops in (hip, tl):
        got = ops.frames_to_u8(x)
        assert got.shape == (2, 3, 20, 32, 3) and torch.equal(got, want)
    assert torch.equal(hip.frames_to_u8(x, size=(20, 32), filter="lanczos"), want)           # same size: no pass runs
    p = hip_params(hip, x, torch.empty(1, dtype=torch.uint8, device=DEV), (20, 32), "bicubic", "rgb24", 0, 3, 96, 20 * 96, 3 * 20 * 96)
    assert hip.lib.tc_frames_to_u8_workspace(C.byref(p)) == 0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["bicubic", "lanczos", "bilinear", "box"])
def test_resample_equals_pil(hip, tl, g, x, name, size):
    want = g[f"{name}.{size[0]}x{size[1]}"]
    assert same(hip.frames_to_u8(x, size=size, filter=name), want)
    if size in ((46, 72), (20, 50)) or name == "lanczos":
        assert same(tl.frames_to_u8(x, size=size, filter=name), want)


@pytest.mark.parametrize("size", [(46, 72), None], ids=["46x72", "identity"])
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_planar_formats_equal_the_integer_statement(hip, tl, g, x, u8, fmt, size):
    rgb = expected_rgb(g, u8, size, "bicubic")
    want = ref.packed(rgb, fmt)
    oh, ow = rgb.shape[2:4]
    assert want.shape == (2, 3, oh * ow * 3 // 2)
    assert same(hip.frames_to_u8(x, size=size, fmt=fmt), want)
    assert same(tl.frames_to_u8(x, size=size, fmt=fmt), want)
    # the planes are where the header says: Y rows, then Cb, Cr (I420) or their pairs (NV12)
    y, cb, cr = ref.yuv420(rgb[1, 2])
    n = oh * ow
    assert np.array_equal(want[1, 2, :n].reshape(oh, ow), y)
    chroma = want[1, 2, n:]
    if fmt == "i420":
        assert np.array_equal(chroma[:n // 4].reshape(oh // 2, ow // 2), cb) and np.array_equal(chroma[n // 4:].reshape(oh // 2, ow // 2), cr)
    else:
        assert np.array_equal(chroma[0::2].reshape(oh // 2, ow // 2), cb) and np.array_equal(chroma[1::2].reshape(oh // 2, ow // 2), cr)


def hip_params(hip, x, out, size, name, fmt, f0, nf, pitch, frame_stride, clip_stride):
    """the C struct filled by hand (tables and workspace from HipOps' caches); the tensors it points to are kept on it"""
    from tooncrafter_amd import _lib
    b, _, t, h, w = x.shape
    p = _lib.TcFramesOutParams(x=x.data_ptr(), out=out.data_ptr(), b=b, t=t, h=h, w=w, f0=f0, nf=nf, oh=size[0], ow=size[1],
                               format=ref.FORMATS.index(fmt), pitch=pitch, frame_stride=frame_stride, clip_stride=clip_stride)
    if size[1] != w:
        hb, hc = hip.resize_tables_filter(name, w, size[1], x.device)
        p.h_bounds, p.h_coefs, p.h_kmax = hb.data_ptr(), hc.data_ptr(), hc.shape[1]
    if size[0] != h:
        vb, vc = hip.resize_tables_filter(name, h, size[0], x.device)
        p.v_bounds, p.v_coefs, p.v_kmax = vb.data_ptr(), vc.data_ptr(), vc.shape[1]
    return p


def test_odd_sizes_are_refused_in_the_planar_formats(hip, x):
    out = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for fmt in ("i420", "nv12"):
        for size in ((45, 72), (46, 71), (21, 32)):
            p = hip_params(hip, x, out, size, "bicubic", fmt, 0, 1, 80, 80 * 48 * 2, 80 * 48 * 2)
            p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
            assert hip.lib.tc_frames_to_u8(C.byref(p), torch.cuda.current_stream().cuda_stream) == -3, (fmt, size)
            with pytest.raises(ValueError):
                hip.frames_to_u8(x, size=size, fmt=fmt)
    p = hip_params(hip, x, out, (46, 72), "bicubic", "i420", 0, 1, 81, 81 * 48 * 2, 81 * 48 * 2)          # I420: Cb rows pitch / 2 apart
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    assert hip.lib.tc_frames_to_u8(C.byref(p), torch.cuda.current_stream().cuda_stream) == -3
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("fmt", ["rgb24", "i420", "nv12"])
@pytest.mark.parametrize("size", [(46, 72), (20, 32)], ids=["46x72", "identity"])
def test_placement_touches_only_the_addressed_bytes(hip, g, x, u8, fmt, size):
    """b = 2, frames 1 and 2 of each clip, rows 5 (RGB) or 6 (YUV) bytes longer than their pixels, slack between frames and
    between clips, a guard in front, the last frame ending where the allocation ends: the whole buffer is compared."""
    from tooncrafter_amd import _lib
    rgb = expected_rgb(g, u8, size, "bicubic")
    oh, ow = size
    f0, nf, guard = 1, 2, 512
    pitch = 3 * ow + 5 if fmt == "rgb24" else ow + 6
    fb = ref.frame_bytes(fmt, oh, pitch)
    frame_stride = fb + 37
    clip_stride = nf * frame_stride + 101
    total = guard + clip_stride + frame_stride + fb
    want = np.full(total, SENTINEL, np.uint8)
    for i in range(2):
        for j in range(nf):
            ref.place(want[guard + i * clip_stride + j * frame_stride:], rgb[i, f0 + j], fmt, pitch)
    assert (want[guard:] != SENTINEL).any() and (want[:guard] == SENTINEL).all()
    # through the struct filled by hand
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    p = hip_params(hip, x, buf[guard:], size, "bicubic", fmt, f0, nf, pitch, frame_stride, clip_stride)
    need = hip.lib.tc_frames_to_u8_workspace(C.byref(p))
    assert need == (0 if fmt == "rgb24" and size == (20, 32) else 4 * 20 * 32 * 3 + (4 * 20 * 72 * 3 if size[1] != 32 else 0))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    _lib.check(hip.lib.tc_frames_to_u8(C.byref(p), torch.cuda.current_stream().cuda_stream), "tc_frames_to_u8")
    assert np.array_equal(buf.cpu().numpy(), want)
    # and through HipOps.frames_to_u8(out=, strides=)
    buf2 = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf2[guard:]
    assert hip.frames_to_u8(x, size=size, fmt=fmt, frames=(f0, nf), out=view, strides=(pitch, frame_stride, clip_stride)) is view
    assert np.array_equal(buf2.cpu().numpy(), want)
    with pytest.raises(ValueError):                                               # one byte short: refused on the host
        hip.frames_to_u8(x, size=size, fmt=fmt, frames=(f0, nf), out=view[:-1], strides=(pitch, frame_stride, clip_stride))


@pytest.mark.parametrize("fmt,size", [("rgb24", (20, 32)), ("rgb24", (14, 22)), ("i420", (46, 72))])
def test_splice_equals_the_host_concatenation(hip, g, x, u8, fmt, size):
    """A keyframe sequence in one video buffer: the first clip whole, every further clip without its first frame (the previous
    clip's last keyframe) at clip_stride = (t - 1) frames; and `loop`, nf = t - 1."""
    rgb = ref.packed(expected_rgb(g, u8, size, "bicubic"), fmt)                   # (2, 3, ...) per-frame bytes
    t = 3
    frames = rgb.reshape(2, t, -1)
    fb = frames.shape[2]
    video = torch.full(((t + 2 * (t - 1)) * fb,), SENTINEL, dtype=torch.uint8, device=DEV)
    pitch = 3 * size[1] if fmt == "rgb24" else size[1]
    hip.frames_to_u8(x[:1], size=size, fmt=fmt, out=video, strides=(pitch, fb, t * fb))
    later = x[[1, 0]].contiguous()                                                # two further clips in one call
    hip.frames_to_u8(later, size=size, fmt=fmt, frames=(1, t - 1), out=video[t * fb:], strides=(pitch, fb, (t - 1) * fb))
    want = np.concatenate([frames[0], frames[1, 1:], frames[0, 1:]]).reshape(-1)
    assert np.array_equal(video.cpu().numpy(), want)
    loop = hip.frames_to_u8(x, size=size, fmt=fmt, frames=(0, t - 1))
    assert np.array_equal(loop.cpu().numpy().reshape(2, t - 1, -1), frames[:, :t - 1])
    from tooncrafter_amd import ops, output
    prev = ops.set_backend(hip)
    try:
        assert torch.equal(output.clip_to_uint8(x, loop=True, size=size, fmt=fmt), loop)
        assert torch.equal(output.clip_to_uint8(x, loop=True), hip.video_to_uint8(x[:, :, :-1]))
    finally:
        ops.set_backend(prev)


from test_gpu_pixel_front import tiny  # noqa: E402,F401  the tiny model with a tiny image tower (a module-scoped fixture)


def test_synthesize_u8_delivers_planes_the_writer_takes(tiny, tmp_path):
    """uint8 keyframes in, I420 planes at a delivery size out, on the device; with per-clip seeds the run repeats, so the planes
    are the statement's resize and conversion of the RGB frames the same call returns by default; the writer stores them."""
    from test_mp4_cpu import _decode
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd import mp4
    model, _ = tiny
    fr = load_golden("pixel_front.npz")
    h, w = (int(v) for v in fr["e2e.size"])
    first, last = (torch.from_numpy(fr["e2e.src"][i])[None].to(DEV) for i in range(2))
    plan = pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=[77])
    oh, ow = 2 * h + 2, 2 * w - 6
    with torch.no_grad():
        rgb = pipeline.synthesize_u8(model, first, last, [1, 4, 4, h // 8, w // 8], size=(h, w), plan=plan, fs=10)
        planes = pipeline.synthesize_u8(model, first, last, [1, 4, 4, h // 8, w // 8], size=(h, w), plan=plan, fs=10,
                                        out_size=(oh, ow), out_filter="lanczos", out_fmt="i420")
    assert planes.shape == (1, 4, oh * ow * 3 // 2) and planes.dtype == torch.uint8 and planes.is_cuda
    want = ref.packed(ref.resize(rgb.cpu().numpy(), oh, ow, "lanczos"), "i420")
    assert np.array_equal(planes.cpu().numpy(), want)
    d = _decode(mp4.write_mp4_i420(str(tmp_path / "clip.mp4"), planes[0].cpu(), ow, oh, fps=8))
    assert (d["w"], d["h"], len(d["frames"])) == (ow, oh, 4)
    n = oh * ow
    for i in range(4):
        assert np.array_equal(np.concatenate([p.ravel() for p in d["frames"][i]]), want[0, i])
        assert d["frames"][i][0].shape == (oh, ow) and n == d["frames"][i][0].size


@pytest.mark.parametrize("binding", ["ctypes", "torch"])
def test_graph_replay_equals_eager(hip, tl, g, x, binding):
    ops = hip if binding == "ctypes" else tl
    kw = dict(size=(46, 72), filter="lanczos", fmt="nv12", frames=(1, 2))
    want = ref.packed(g["lanczos.46x72"][:, 1:3], "nv12")
    eager = ops.frames_to_u8(x, **kw)
    assert same(eager, want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.frames_to_u8(x, **kw)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = ops.frames_to_u8(x, **kw)
    out.fill_(SENTINEL)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
