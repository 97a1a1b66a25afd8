"""Colour match of decoded frames to their keyframes on the MI355X (csrc/colour_match.hip: tc_colour_stats, tc_colour_match)
against the float64 statement of tests/colour_match_ref.py, every case through both bindings (HipOps, TorchLibOps), whose
results must be the same bits:

  * the nine sums, exactly on grid inputs (every product a multiple of 2^-14) and within the bound of an n-term double sum on
    random ones; a frame's numbers do not depend on its batch, its slot, the frames asked for or the alignment of the clip;
  * the twelve coefficients within two fp32 ulps of the reference's; the apply pass bit for bit from the device's own
    coefficients with separate float32 operations on the host; in place; strength 0 and a frame against itself are exact;
  * `output.match_colour` end to end; placement into sentinel buffers of which every byte is compared; refusals write nothing;
    the three calls under a captured graph; the public timeline with and without `match` on the tiny model.

Shapes: the smallest at which the kernels can go wrong (b, t, h x w): (2, 3, 7 x 9) less than a wave, odd, planes on 4-byte
boundaries only; (2, 5, 24 x 40) a ragged tail of a 256-thread block; (1, 2, 128 x 160) ten parts per frame, so the fixed-order
sum over parts runs; (1, 1, 8 x 8) t = 1.  Nothing expected comes from the kernels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import colour_match_ref as ref
from conftest import load_golden
from test_gpu_pixel_front import tiny  # noqa: F401  (the tiny model with a tiny image tower, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
SHAPES = [(2, 3, 7, 9), (2, 5, 24, 40), (1, 2, 128, 160), (1, 1, 8, 8)]
IDS = ["2x3x7x9", "2x5x24x40", "1x2x128x160", "1x1x8x8"]
IDENTITY = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def tl():
    from tooncrafter_amd.torch_ops import TorchLibOps
    return TorchLibOps()


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """the seeded inputs of a shape and what the statement says of them, computed once and left unchanged: the clip, its two
    reference images (17 x 23: another size than the clip's) and the float64 sums of both"""
    b, t, h, w = shape
    make = ref.grid_frames if kind == "grid" else ref.frames
    x, ends = make(sum(shape), b, t, h, w), make(1 + sum(shape), b, 2, 17, 23)
    got = dict(x=x, ends=ends, stats=ref.frame_stats(x), ref=ref.frame_stats(ends))
    for v in got.values():
        v.setflags(write=False)
    return got


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                  # a copy: the cached inputs are read-only


def requests(t):
    """the (f0, nf, fstep) of the statistics tests that fit a clip of t frames"""
    return [r for r in ((0, t, 1), (0, 2, t - 1), (1, 1, 1)) if r[0] < t and (r[1] == 1 or (r[2] >= 1 and r[0] + (r[1] - 1) * r[2] <= t - 1))]


# ------------------------------------------------------------------------------------------------ statistics

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_statistics_are_exact_on_the_grid(hip, tl, shape):
    b, t, h, w = shape
    c = case(shape, "grid")
    assert (np.abs(c["x"]) > 1).any() and (np.abs(c["x"]) < 1).any()            # the clamp acts, and not everywhere
    x = dev(c["x"])
    for f0, nf, fstep in requests(t):
        want = torch.from_numpy(ref.frame_stats(c["x"], f0, nf, fstep))
        got = hip.colour_stats(x, frames=(f0, nf, fstep))
        assert got.dtype == torch.float64 and got.shape == (b, nf, 9)
        assert torch.equal(got.cpu(), want), (f0, nf, fstep)
        assert torch.equal(tl.colour_stats(x, frames=(f0, nf, fstep)), got)
    assert torch.equal(hip.colour_stats(x), hip.colour_stats(x, frames=(0, t, 1)))
    # a clip's numbers are those of a call on that clip alone, and of the same values one float off the 16-byte grid
    whole = hip.colour_stats(x)
    for i in range(b):
        assert torch.equal(hip.colour_stats(x[i:i + 1].contiguous()), whole[i:i + 1])
    shifted = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(x)
    assert torch.equal(hip.colour_stats(shifted), whole) and torch.equal(tl.colour_stats(shifted), whole)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_statistics_of_random_inputs_stay_within_the_bound_of_a_double_sum(hip, tl, shape):
    """|sum - ref| <= n 2^-53 sum |terms|: the worst case of an n-term double sum in any order, computed from the inputs.  The
    one-float shift changes the loads, not the order: the same bits."""
    b, t, h, w = shape
    c = case(shape, "random")
    x = dev(c["x"])
    bound = h * w * 2.0 ** -53 * np.abs(ref.terms(c["x"])).sum(axis=-1)           # (b, t, 9)
    got = hip.colour_stats(x)
    err = np.abs(got.cpu().numpy() - c["stats"])
    print(f"{shape}: worst |sum - ref| / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()
    assert torch.equal(tl.colour_stats(x), got)
    shifted = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
    shifted.copy_(x)
    assert torch.equal(hip.colour_stats(shifted), got)
    if t > 1:                                                                    # a frame's numbers, whichever frames are asked for
        assert torch.equal(hip.colour_stats(x, frames=(0, 2, t - 1)), got[:, [0, t - 1]])
        assert torch.equal(hip.colour_stats(x, frames=(1, 1, 1)), got[:, 1:2])


# ------------------------------------------------------------------------------------------------ coefficients, apply

def device_match(be, c, method, strength, out=None, x=None):
    x = dev(c["x"]) if x is None else x
    src, two = be.colour_stats(x), be.colour_stats(dev(c["ends"]), frames=(0, 2, 1))
    return (x, *be.colour_match(x, src, two, 17 * 23, method, strength, out=out))


@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("method", ["mkl", "mean_std"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_coefficients_are_within_two_ulps_of_the_statement(hip, tl, shape, method, strength):
    b, t, h, w = shape
    c = case(shape, "random")
    for i in range(b):
        for f in range(t):
            assert ref.cond(ref.moments(c["stats"][i, f], h * w)[1]) <= 1e3
    want = ref.coefs(c["stats"], c["ref"], h * w, 17 * 23, method, strength).astype(np.float32).astype(np.float64)
    _, _, co = device_match(hip, c, method, strength)
    assert co.shape == (b, t, 12) and co.dtype == torch.float32
    err = np.abs(co.cpu().numpy().astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
    print(f"{shape} {method} {strength}: worst coefficient error {err.max() * 2 ** 22:.3g} x 2^-22")
    assert (err <= 2.0 ** -22).all()
    assert torch.equal(device_match(tl, c, method, strength)[2], co)
    assert torch.equal(hip.colour_match(dev(c["x"]), hip.colour_stats(dev(c["x"])), hip.colour_stats(dev(c["ends"])), 17 * 23,
                                        ref.METHODS[method], strength)[1], co)    # the method by its code


def host_apply(x, co):
    """y_k = ((o_k + a_k0 r) + a_k1 g) + a_k2 b with separate torch CPU float32 multiplies and adds, in that order"""
    c = x.cpu().clamp(-1.0, 1.0)
    co = co.cpu()
    r, g, bl = c[:, 0], c[:, 1], c[:, 2]                                          # (b, t, h, w)
    k = [co[:, :, j, None, None] for j in range(12)]
    rows = []
    for i in range(3):
        y = k[9 + i] + k[3 * i] * r
        y = y + k[3 * i + 1] * g
        rows.append(y + k[3 * i + 2] * bl)
    return torch.stack(rows, dim=1)


@pytest.mark.parametrize("method", ["mkl", "mean_std"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_is_the_stated_float32_arithmetic_bit_for_bit(hip, tl, shape, method):
    c = case(shape, "random")
    x, out, co = device_match(hip, c, method, 0.75)
    want = host_apply(x, co)
    assert out.dtype == torch.float32 and out.shape == x.shape and torch.equal(out.cpu(), want)
    assert (want.abs() > 1).any()                                                 # not clamped on the way out
    x2, out2, co2 = device_match(tl, c, method, 0.75)
    assert torch.equal(out2, out) and torch.equal(co2, co)
    for be in (hip, tl):                                                          # in place: the same bits
        mine = x.clone()
        _, res, co3 = device_match(be, c, method, 0.75, out=mine, x=mine)
        assert res is mine and torch.equal(mine, out) and torch.equal(co3, co)
    shifted = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)      # 4-byte loads and stores
    shifted.copy_(x)
    _, res, _ = device_match(hip, c, method, 0.75, out=shifted, x=shifted)
    assert torch.equal(res, out)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_identities(hip, tl, shape):
    c = case(shape, "random")
    x = dev(c["x"])
    clamped = x.clamp(-1.0, 1.0)
    for be in (hip, tl):
        for method in ("mkl", "mean_std"):
            _, out, co = device_match(be, c, method, 0.0)
            assert torch.equal(out, clamped) and np.array_equal(co.cpu().numpy(), np.broadcast_to(IDENTITY, co.shape))
        # a frame against its own statistics (t = 1, the same image in both slots)
        one = x[:, :, :1].contiguous()
        src = be.colour_stats(one)
        two = be.colour_stats(torch.cat([one, one], dim=2), frames=(0, 2, 1))
        assert torch.equal(two[:, :1], src) and torch.equal(two[:, 1:], src)
        out, co = be.colour_match(one, src, two, shape[2] * shape[3], "mean_std", 1.0)
        assert torch.equal(out, one.clamp(-1.0, 1.0)) and np.array_equal(co.cpu().numpy(), np.broadcast_to(IDENTITY, co.shape))


def test_match_colour_end_to_end_against_the_statement(hip, tl):
    """output.match_colour on (2, 5, 24 x 40) against the float64 reference: per value 4 x 2^-22 x (1 + sum_k |A'_row k|) --
    the coefficient tolerance times the input range, plus the fp32 rounding of the apply -- from the REFERENCE's coefficients"""
    from tooncrafter_amd import ops, output
    c = case((2, 5, 24, 40), "random")
    for method in ("mkl", "mean_std"):
        for strength in (1.0, 0.5):
            want, co = ref.match(c["x"], c["ends"], method, strength)
            bound = 4 * 2.0 ** -22 * (1.0 + np.abs(co[..., :9]).reshape(2, 5, 3, 3).sum(axis=-1))      # (b, t, k)
            bound = bound.transpose(0, 2, 1)[:, :, :, None, None]
            got = []
            for be in (hip, tl):
                prev = ops.set_backend(be)
                try:
                    got.append(output.match_colour(dev(c["x"]), dev(c["ends"]), output.ColourMatch(method, strength)))
                finally:
                    ops.set_backend(prev)
            err = np.abs(got[0].cpu().numpy().astype(np.float64) - want)
            print(f"{method} {strength}: worst error / bound = {(err / bound).max():.3g}")
            assert (err <= bound).all() and torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------ placement, refusals

def test_results_land_inside_sentinel_buffers_and_nowhere_else(hip):
    from tooncrafter_amd import _lib
    shape = (2, 3, 7, 9)
    b, t, h, w = shape
    c = case(shape, "random")
    x, guard = dev(c["x"]), 256
    stream = torch.cuda.current_stream().cuda_stream

    def carve(nbytes):
        buf = torch.full((guard + nbytes + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
        return buf, buf[guard:guard + nbytes]
    sbuf, stats = carve(b * t * 9 * 8)
    p = _lib.TcColourStatsParams(x=x.data_ptr(), b=b, t=t, h=h, w=w, f0=0, nf=t, fstep=1, stats=stats.data_ptr())
    p.workspace_bytes = hip.lib.tc_colour_stats_workspace(C.byref(p))
    assert p.workspace_bytes == b * t * 72
    wbuf, ws = carve(p.workspace_bytes)
    p.workspace = ws.data_ptr()
    _lib.check(hip.lib.tc_colour_stats(C.byref(p), stream), "tc_colour_stats")
    src = hip.colour_stats(x)
    two = hip.colour_stats(dev(c["ends"]))
    for buf, inner, want in ((sbuf, stats, src), (wbuf, ws, None)):
        got = buf.cpu().numpy()
        assert (got[:guard] == SENTINEL).all() and (got[-guard:] == SENTINEL).all()
        if want is not None:
            assert np.array_equal(inner.cpu().numpy().view(np.float64).reshape(b, t, 9), want.cpu().numpy())
    obuf, out = carve(x.numel() * 4)
    cbuf, coefs = carve(b * t * 12 * 4)
    m = _lib.TcColourMatchParams(x=x.data_ptr(), out=out.data_ptr(), b=b, t=t, h=h, w=w, src=src.data_ptr(), ref=two.data_ptr(),
                                 ref_pixels=17 * 23, method=1, strength=1.0, coefs=coefs.data_ptr())
    _lib.check(hip.lib.tc_colour_match(C.byref(m), stream), "tc_colour_match")
    want_out, want_co = hip.colour_match(x, src, two, 17 * 23, "mkl", 1.0)
    for buf, inner, want in ((obuf, out, want_out), (cbuf, coefs, want_co)):
        got = buf.cpu().numpy()
        assert (got[:guard] == SENTINEL).all() and (got[-guard:] == SENTINEL).all()
        assert np.array_equal(inner.cpu().numpy().view(np.float32), want.cpu().numpy().reshape(-1))
    assert not (want_out.cpu().numpy().view(np.uint8) == SENTINEL).all()


def test_refused_requests_write_nothing(hip):
    from tooncrafter_amd import _lib
    from tooncrafter_amd._lib import TooncrafterHipError
    shape = (2, 3, 7, 9)
    b, t, h, w = shape
    c = case(shape, "random")
    x = dev(c["x"])
    src, two = hip.colour_stats(x), hip.colour_stats(dev(c["ends"]))
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    room = buf[256:]

    def stats_rc(**kw):
        p = _lib.TcColourStatsParams(x=x.data_ptr(), b=b, t=t, h=h, w=w, f0=0, nf=t, fstep=1, stats=room.data_ptr(),
                                     workspace=room.data_ptr() + 4096, workspace_bytes=b * t * 72)
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib.tc_colour_stats(C.byref(p), stream)

    def match_rc(**kw):
        p = _lib.TcColourMatchParams(x=x.data_ptr(), out=room.data_ptr(), b=b, t=t, h=h, w=w, src=src.data_ptr(), ref=two.data_ptr(),
                                     ref_pixels=17 * 23, method=1, strength=1.0, coefs=room.data_ptr() + 8192)
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib.tc_colour_match(C.byref(p), stream)
    assert stats_rc(nf=t + 1) == -1 and stats_rc(f0=1) == -1 and stats_rc(nf=2, fstep=0) == -1 and stats_rc(f0=t, nf=1) == -1
    assert stats_rc(stats=room.data_ptr() + 4) == -2 and stats_rc(workspace=room.data_ptr() + 4100) == -2
    assert stats_rc(workspace_bytes=b * t * 72 - 1) == -4 and stats_rc(workspace=None) == -4
    assert match_rc(method=2) == -1 and match_rc(strength=1.5) == -1 and match_rc(strength=float("nan")) == -1
    assert match_rc(ref_pixels=0) == -1 and match_rc(coefs=None) == -1
    assert match_rc(x=room.data_ptr() + 4, out=room.data_ptr()) == -1             # a partial overlap
    assert match_rc(src=src.data_ptr() + 4) == -2 and match_rc(ref=two.data_ptr() + 4) == -2
    for bad in (dict(method="lab"), dict(strength=-0.5), dict(ref_pixels=0)):
        kw = dict(ref_pixels=17 * 23, method="mkl", strength=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip.colour_match(x, src, two, **kw)
    with pytest.raises(ValueError):
        hip.colour_match(x, src.float(), two, 17 * 23, "mkl", 1.0)
    with pytest.raises(ValueError):
        hip.colour_stats(x.transpose(3, 4))                                        # not contiguous
    with pytest.raises((ValueError, TooncrafterHipError)):
        hip.colour_match(x, src, two, 17 * 23, "mkl", 1.0, out=x.view(-1)[1:])
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ graph capture

@pytest.mark.parametrize("binding", ["ctypes", "torch"])
def test_match_colour_replays_from_a_captured_graph(hip, tl, binding):
    """the three calls of match_colour captured once and replayed on changed inputs: no allocation outside the caching allocator,
    no synchronisation, no host read of device memory"""
    from tooncrafter_amd import ops, output
    shape = (2, 5, 24, 40)
    first, second = case(shape, "random"), case(shape, "grid")
    m = output.ColourMatch("mkl", 0.75)
    prev = ops.set_backend(hip if binding == "ctypes" else tl)
    try:
        eager = output.match_colour(dev(second["x"]), dev(second["ends"]), m)
        video, ends = dev(first["x"]), dev(first["ends"])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            output.match_colour(video, ends, m)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = output.match_colour(video, ends, m)
        video.copy_(dev(second["x"]))
        ends.copy_(dev(second["ends"]))
        out.fill_(7.0)
        gr.replay()
        torch.cuda.synchronize()
    finally:
        ops.set_backend(prev)
    assert torch.equal(out, eager) and not torch.equal(eager, dev(second["x"]).clamp(-1, 1))


# ------------------------------------------------------------------------------------------------ the public path

def test_timeline_with_and_without_a_match(tiny):  # noqa: F811
    """three keyframes, two segments.  match=None is the call without the keyword, byte for byte.  With mean_std the video is the
    matched clips in the writer's bytes, and frames 0 and t - 1 of every matched clip have their keyframe's mean and variances
    within the property's bound eps (1 + |A|_2^2) + 1e-12: the seam property on the device (the last frame of segment 0 and
    frame 0 of segment 1 share keyframe 1)."""
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd import ops, output
    model, _ = tiny
    fr = load_golden("pixel_front.npz")
    h, w = (int(v) for v in fr["e2e.size"])
    a, b = fr["e2e.src"][0][:36, :52], fr["e2e.src"][1][:36, :52]
    kf = torch.from_numpy(np.ascontiguousarray(np.stack([a, b, a[::-1, ::-1]]))).to(DEV)
    shape, seeds, t = [1, 4, 4, h // 8, w // 8], [51, 52], 4
    m = output.ColourMatch("mean_std")

    def plan(s):
        return pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=s)
    with torch.no_grad():
        plain = pipeline.synthesize_timeline_u8(model, kf, shape, size=(h, w), plan=plan(seeds), fs=10)
        none = pipeline.synthesize_timeline_u8(model, kf, shape, size=(h, w), plan=plan(seeds), fs=10, match=None)
        video = pipeline.synthesize_timeline_u8(model, kf, shape, size=(h, w), plan=plan(seeds), fs=10, match=m)
        assert torch.equal(plain, none) and video.shape == plain.shape == (7, h, w, 3) and not torch.equal(video, plain)
        pieces = []
        for i, s in enumerate(seeds):
            cond = pipeline.Conditions.from_uint8(model, kf[i:i + 1], kf[i + 1:i + 2], size=(h, w), t=t, prompts=None, fs=10, guided=True,
                                                  three_way=False, image_branch=True, hold_endpoints=True)
            assert cond.ends_px.shape == (1, 3, 2, h, w)
            decoded = pipeline.decode_spliced(model, pipeline.sample(model, cond, plan([s]), shape), cond.refs).to(torch.float32)
            matched = output.match_colour(decoded, cond.ends_px, m)
            pieces.append(ops.frames_to_u8(matched, frames=(0, t))[0])
            want, co = ref.match(decoded.cpu().numpy(), cond.ends_px.cpu().numpy(), "mean_std", 1.0)
            ends, y = cond.ends_px.cpu().numpy(), matched.cpu().numpy()
            for f, e in ((0, 0), (t - 1, 1)):
                gain = co[0, f, :9].reshape(3, 3)
                bound = ref.EPS * (1.0 + np.linalg.norm(gain, 2) ** 2) + 1e-12
                (my, cy), (mk, ck) = ref.plain_moments(y[0, :, f]), ref.plain_moments(ref.clamp(ends[0, :, e]))
                print(f"segment {i} frame {f}: |mean - keyframe's| {np.abs(my - mk).max():.3g}, |var - keyframe's| "
                      f"{np.abs(np.diag(cy - ck)).max():.3g}, bound {bound:.3g}, gains {np.diag(gain)}")
                assert np.abs(my - mk).max() <= bound and np.abs(np.diag(cy - ck)).max() <= bound
    assert torch.equal(video, torch.cat([pieces[0], pieces[1][1:]]))
