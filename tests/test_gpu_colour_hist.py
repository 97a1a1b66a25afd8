"""Histogram colour transfer on the MI355X (csrc/colour_hist.hip: tc_colour_hist, tc_colour_transfer) against the numpy statement
of tests/colour_hist_ref.py, through both bindings (HipOps, TorchLibOps), whose results must be the same bits:

  * histograms equal to the statement's bincount: every shape, a frame subset, a clip on 4-byte boundaries only, constant,
    two-tone and edge-value clips, a workspace and a result buffer full of garbage;
  * tables bit for bit at every frame index (sources and references with empty bins, a single-bin reference, a single-bin
    source); the apply pass bit for bit at strengths 0, 0.75 and 1, with and without a base, in place;
  * the exact consequences on the device: strength 0, self-match, the whole-bin shift;
  * `output.match_colour` for "hm" and "hm_mkl_hm" within the bound of the MKL stage; placement into sentinel buffers; refusals
    write nothing; a captured graph; the public timeline with match=ColourMatch("hm") on the tiny model.

Shapes (b = 2, t = 5): 17 x 23 (4-byte loads, one part), 24 x 40 (16-byte loads, one part), 50 x 83 (4-byte loads, five parts
with a tail), 48 x 64 (16-byte loads, three parts).  Reference images are 19 x 29, so ref_pixels != h * w.  Nothing expected
comes from the kernels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import colour_hist_ref as ref
import colour_match_ref as cm
from conftest import load_golden
from test_colour_hist_cpu import COMPOUND_SEEDS
from test_gpu_pixel_front import tiny  # noqa: F401  (the tiny model with a tiny image tower, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
SHAPES = [(2, 5, 17, 23), (2, 5, 24, 40), (2, 5, 50, 83), (2, 5, 48, 64)]
IDS = ["17x23", "24x40", "50x83", "48x64"]
REF_HW = (19, 29)
REF_PIXELS = 19 * 29


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def tl():
    from tooncrafter_amd.torch_ops import TorchLibOps
    return TorchLibOps()


def single_bin(b, t, h, w, value):
    return np.full((b, 3, t, h, w), value, np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, kind="toon"):
    """the seeded inputs of a shape and what the statement says of them, computed once and left unchanged: the clip, its two
    reference images, the histograms of both and the tables"""
    b, t, h, w = shape
    x, ends = ref.toon_frames(sum(shape), b, t, h, w), ref.toon_frames(1 + sum(shape), b, 2, *REF_HW)
    if kind == "single_bin_reference":
        ends = single_bin(b, 2, *REF_HW, -0.2)
    if kind == "single_bin_source":
        x = single_bin(b, t, h, w, 0.3)
    got = dict(x=x, ends=ends, hist=ref.hist(x), ref=ref.hist(ends))
    got["table"] = ref.table(got["hist"], got["ref"], h * w, REF_PIXELS)[0]
    for v in got.values():
        v.setflags(write=False)
    return got


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                  # a copy: the cached inputs are read-only


def shifted_copy(x):
    """the same values one float off the 16-byte grid"""
    s = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
    assert s.data_ptr() % 16 == 4
    s.copy_(x)
    return s


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ------------------------------------------------------------------------------------------------ histograms

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_histograms_equal_the_statements_bincount(hip, tl, shape):
    b, t, h, w = shape
    c = case(shape)
    assert (np.abs(c["x"]) > 1).any() and (c["hist"] == 0).sum() > c["hist"].size // 2     # the clamp acts; most bins are empty
    x = dev(c["x"])
    got = hip.colour_hist(x)
    assert got.dtype == torch.int32 and got.shape == (b, t, 3, 1024)
    assert torch.equal(got.cpu(), torch.from_numpy(np.array(c["hist"]))) and torch.equal(tl.colour_hist(x), got)
    for f0, nf, fstep in ((1, 2, 3), (0, 2, t - 1), (t - 1, 1, 1)):               # a frame subset
        want = torch.from_numpy(ref.hist(c["x"], f0, nf, fstep))
        assert torch.equal(hip.colour_hist(x, frames=(f0, nf, fstep)).cpu(), want), (f0, nf, fstep)
        assert torch.equal(tl.colour_hist(x, frames=(f0, nf, fstep)).cpu(), want), (f0, nf, fstep)
    s = shifted_copy(x)                                                          # 4-byte loads only
    assert torch.equal(hip.colour_hist(s), got) and torch.equal(tl.colour_hist(s), got)


@pytest.mark.parametrize("shape", [(2, 5, 17, 23), (2, 5, 24, 40), (2, 5, 48, 64)], ids=["17x23", "24x40", "48x64"])
def test_histograms_of_flat_two_tone_and_edge_value_clips(hip, shape):
    """the contents that send whole waves into one bin (the one-add path), and the values at the ends of the range"""
    b, t, h, w = shape
    flat = single_bin(b, t, h, w, 0.3)
    two = flat.copy()
    two[:, :, :, h // 2:] = -0.61
    two[:, 1, :, :, : w // 3] = 2.0                                                # and a third tone in one channel, cut along x
    edge = np.resize(ref.EDGE_VALUES, (b, 3, t, h, w)).astype(np.float32)
    for name, x in (("flat", flat), ("two-tone", two), ("edge", edge)):
        want = ref.hist(x)
        assert want.sum() == b * t * 3 * h * w
        assert torch.equal(hip.colour_hist(dev(x)).cpu(), torch.from_numpy(want)), name
        assert torch.equal(hip.colour_hist(shifted_copy(dev(x))).cpu(), torch.from_numpy(want)), name
    assert (ref.hist(flat) > 0).sum() == b * t * 3 and np.isnan(edge).any() and np.isinf(edge).any()


def carve(nbytes, guard=256):
    buf = torch.full((guard + nbytes + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[guard:guard + nbytes]


def guards_intact(buf, guard=256):
    got = buf.cpu().numpy()
    return bool((got[:guard] == SENTINEL).all() and (got[-guard:] == SENTINEL).all())


def test_garbage_in_workspace_and_result_changes_nothing_and_guards_stay(hip):
    from tooncrafter_amd import _lib
    shape = (2, 5, 50, 83)
    b, t, h, w = shape
    c = case(shape)
    x = dev(c["x"])
    stream = torch.cuda.current_stream().cuda_stream
    hbuf, hist = carve(b * t * 3 * 1024 * 4)
    p = _lib.TcColourHistParams(x=x.data_ptr(), b=b, t=t, h=h, w=w, f0=0, nf=t, fstep=1, hist=hist.data_ptr())
    p.workspace_bytes = hip.lib.tc_colour_hist_workspace(C.byref(p))
    assert p.workspace_bytes == b * t * 3 * 5 * 1024 * 4
    wbuf, ws = carve(p.workspace_bytes)
    p.workspace = ws.data_ptr()
    for fill in (SENTINEL, 0x7F):                                                  # two kinds of garbage, the second over the first result
        ws.fill_(fill)
        hist.fill_(fill)
        _lib.check(hip.lib.tc_colour_hist(C.byref(p), stream), "tc_colour_hist")
        assert np.array_equal(hist.cpu().numpy().view(np.int32).reshape(b, t, 3, 1024), c["hist"])
        assert guards_intact(hbuf) and guards_intact(wbuf)


# ------------------------------------------------------------------------------------------------ tables, apply

def device_transfer(be, c, strength, base=None, out=None, x=None):
    x = dev(c["x"]) if x is None else x
    src, two = be.colour_hist(x), be.colour_hist(dev(c["ends"]), frames=(0, 2, 1))
    return (x, *be.colour_transfer(x, src, two, REF_PIXELS, strength, base=base, out=out))


@pytest.mark.parametrize("kind", ["toon", "single_bin_reference", "single_bin_source"])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_tables_are_the_statements_bit_for_bit(hip, tl, shape, kind):
    b, t, h, w = shape
    c = case(shape, kind)
    assert (c["ref"] == 0).any() and (c["hist"] == 0).any() and c["table"].any()
    _, _, table = device_transfer(hip, c, 1.0)
    assert table.dtype == torch.float32 and table.shape == (b, t, 3, 1024)
    got, want = table.cpu().numpy(), c["table"]
    off = got.view(np.uint32) != want.view(np.uint32)
    print(f"{shape} {kind}: {int(off.sum())} of {off.size} entries differ, worst |difference| {np.abs(got - want).max():.3g}")
    assert not off.any()
    assert torch.equal(device_transfer(tl, c, 1.0)[2], table)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_is_the_stated_float32_arithmetic_bit_for_bit(hip, tl, shape):
    c = case(shape)
    base_np = ref.toon_frames(77 + sum(shape), *shape)
    x, base = dev(c["x"]), dev(base_np)
    for strength in (0.0, 0.75, 1.0):
        for with_base in (False, True):
            want = ref.apply(c["x"], c["table"], strength, base_np if with_base else None)
            _, out, table = device_transfer(hip, c, strength, base=base if with_base else None)
            assert out.dtype == torch.float32 and out.shape == x.shape and same_bits(table, c["table"])
            assert same_bits(out, want), (strength, with_base)
            assert torch.equal(device_transfer(tl, c, strength, base=base if with_base else None)[1], out)
            for be in (hip, tl):                                                  # in place: the same bits
                mine = x.clone()
                _, res, _ = device_transfer(be, c, strength, base=base if with_base else None, out=mine, x=mine)
                assert res is mine and torch.equal(mine, out)
            if strength == 0.75:                                                  # 4-byte loads and stores
                s, sb = shifted_copy(x), shifted_copy(base)
                _, res, _ = device_transfer(hip, c, strength, base=sb if with_base else None, out=s, x=s)
                assert torch.equal(res, out)


@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_exact_consequences_on_the_device(hip, tl, shape):
    b, t, h, w = shape
    c = case(shape)
    x = dev(c["x"])
    clamped = x.clamp(-1.0, 1.0)
    other = dev(ref.toon_frames(5, b, t, h, w))
    for be in (hip, tl):
        # strength 0: clamp(x), or clamp(base)
        assert torch.equal(device_transfer(be, c, 0.0)[1], clamped)
        assert torch.equal(device_transfer(be, c, 0.0, base=other)[1], other.clamp(-1.0, 1.0))
        # self-match: the clip's frames all one image, the references that image (at its own size, and four to a reference)
        one = x[:, :, :1].expand(b, 3, t, h, w).contiguous()
        own = be.colour_hist(one)
        for mult in (1, 4):
            two = (own[:, :2] * mult).contiguous()
            for strength in (1.0, 0.75):
                out, table = be.colour_transfer(one, own, two, h * w * mult, strength)
                assert not table.any() and torch.equal(out, one.clamp(-1.0, 1.0)), (mult, strength)
        # whole-bin shift: 64 bins, nothing clipped: the reference comes back bit for bit
        g = ref.grid_frames(7 + h, b, 1, h, w)
        target = (g + np.float32(0.125)).astype(np.float32)
        gx, gt = dev(g), dev(np.concatenate([target, target], axis=2))
        out, table = be.colour_transfer(gx, be.colour_hist(gx), be.colour_hist(gt), h * w, 1.0)
        assert same_bits(out, target)
        assert set(np.unique(table.cpu().numpy())) == {np.float32(0.0), np.float32(0.125)}


@pytest.mark.parametrize("method", ["hm", "hm_mkl_hm"])
def test_match_colour_end_to_end_against_the_statement(hip, tl, method):
    """output.match_colour on (2, 5, 24 x 40) clips against 19 x 29 keyframes: per value within 4 x 2^-22 x (1 + sum_k |A'_row k|) of
    the reference, the bound of the existing MKL end-to-end test from the REFERENCE's MKL coefficients (A' = I for "hm", which
    has no MKL stage).  The histogram stages add no error of their own, but a difference inside that bound after the MKL stage
    can move a value across a bin edge, and then the two table entries either side of the edge change: such pixels are
    counted, must lie in `ref.touched`, and must stay below 1 % of the pixels of every frame (the seeds: the CPU test
    test_compound_seeds_keep_bin_crossings_below_one_percent)."""
    from tooncrafter_amd import ops, output
    for seed in COMPOUND_SEEDS:
        video, ends = cm.frames(seed, 2, 5, 24, 40), cm.frames(100 + seed, 2, 2, *REF_HW)
        for strength in (1.0, 0.75):
            want = ref.match(video, ends, method, strength)
            bound = want.get("bound", np.full((2, 3, 5, 1, 1), 4 * 2.0 ** -22 * 2.0))
            allowed = ref.touched(want["mid"], bound) if method == "hm_mkl_hm" else np.zeros(video.shape, bool)
            got = []
            for be in (hip, tl):
                prev = ops.set_backend(be)
                try:
                    got.append(output.match_colour(dev(video), dev(ends), output.ColourMatch(method, strength)))
                finally:
                    ops.set_backend(prev)
            err = np.abs(got[0].cpu().numpy().astype(np.float64) - want["out"])
            past = err > bound
            share = past.any(axis=1).reshape(2, 5, -1).mean(axis=-1)
            print(f"{method} seed {seed} strength {strength}: worst error / bound outside the counted pixels "
                  f"{(err / bound)[~past].max():.3g}; pixels past the bound {int(past.any(axis=1).sum())} of {2 * 5 * 24 * 40}, "
                  f"worst share of a frame {share.max():.4f}")
            assert not (past & ~allowed).any() and share.max() <= 0.01
            assert torch.equal(got[0], got[1])
            assert not np.array_equal(want["out"], ref.clamp(video))


# ------------------------------------------------------------------------------------------------ placement, refusals

def test_transfer_lands_inside_sentinel_buffers_and_nowhere_else(hip):
    from tooncrafter_amd import _lib
    shape = (2, 5, 17, 23)
    b, t, h, w = shape
    c = case(shape)
    x = dev(c["x"])
    src, two = hip.colour_hist(x), hip.colour_hist(dev(c["ends"]))
    stream = torch.cuda.current_stream().cuda_stream
    obuf, out = carve(x.numel() * 4)
    tbuf, table = carve(b * t * 3 * 1024 * 4)
    p = _lib.TcColourTransferParams(x=x.data_ptr(), base=None, out=out.data_ptr(), b=b, t=t, h=h, w=w, src=src.data_ptr(),
                                    ref=two.data_ptr(), ref_pixels=REF_PIXELS, strength=1.0, table=table.data_ptr())
    _lib.check(hip.lib.tc_colour_transfer(C.byref(p), stream), "tc_colour_transfer")
    assert guards_intact(obuf) and guards_intact(tbuf)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.apply(c["x"], c["table"], 1.0).view(np.uint32).reshape(-1))
    assert np.array_equal(table.cpu().numpy().view(np.uint32), c["table"].view(np.uint32).reshape(-1))


def test_refused_requests_write_nothing(hip):
    from tooncrafter_amd import _lib
    from tooncrafter_amd._lib import TooncrafterHipError
    shape = (2, 5, 17, 23)
    b, t, h, w = shape
    c = case(shape)
    x = dev(c["x"])
    src, two = hip.colour_hist(x), hip.colour_hist(dev(c["ends"]))
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((1 << 20,), SENTINEL, dtype=torch.uint8, device=DEV)
    room = buf[256:]
    one = 3 * 1024 * 4

    def hist_rc(**kw):
        p = _lib.TcColourHistParams(x=x.data_ptr(), b=b, t=t, h=h, w=w, f0=0, nf=t, fstep=1, hist=room.data_ptr(),
                                    workspace=room.data_ptr() + (1 << 19), workspace_bytes=b * t * one)
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib.tc_colour_hist(C.byref(p), stream)

    def transfer_rc(**kw):
        p = _lib.TcColourTransferParams(x=x.data_ptr(), base=None, out=room.data_ptr(), b=b, t=t, h=h, w=w, src=src.data_ptr(),
                                        ref=two.data_ptr(), ref_pixels=REF_PIXELS, strength=1.0, table=room.data_ptr() + (1 << 19))
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib.tc_colour_transfer(C.byref(p), stream)
    assert hist_rc(nf=t + 1) == -1 and hist_rc(f0=1) == -1 and hist_rc(nf=2, fstep=0) == -1 and hist_rc(f0=t, nf=1) == -1
    assert hist_rc(hist=room.data_ptr() + 2) == -2 and hist_rc(workspace=room.data_ptr() + (1 << 19) + 2) == -2
    assert hist_rc(workspace_bytes=b * t * one - 1) == -4 and hist_rc(workspace=None) == -4
    assert transfer_rc(strength=1.5) == -1 and transfer_rc(strength=float("nan")) == -1
    assert transfer_rc(ref_pixels=0) == -1 and transfer_rc(table=None) == -1
    assert transfer_rc(x=room.data_ptr() + 4, out=room.data_ptr()) == -1          # a partial overlap with x
    assert transfer_rc(base=room.data_ptr()) == -1 and transfer_rc(base=room.data_ptr() + 64) == -1     # out is, or overlaps, base
    assert transfer_rc(src=src.data_ptr() + 2) == -2 and transfer_rc(ref=two.data_ptr() + 2) == -2
    assert transfer_rc(ref_pixels=2 ** 26 + 1) == -3
    for bad in (dict(strength=-0.5), dict(ref_pixels=0), dict(ref_pixels=2 ** 26 + 1)):
        kw = dict(ref_pixels=REF_PIXELS, strength=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip.colour_transfer(x, src, two, **kw)
    with pytest.raises(ValueError):
        hip.colour_transfer(x, src.float(), two, REF_PIXELS, 1.0)
    with pytest.raises(ValueError):
        hip.colour_transfer(x, src, two, REF_PIXELS, 1.0, base=x[:, :, :1].contiguous())
    with pytest.raises(ValueError):
        hip.colour_hist(x.transpose(3, 4))                                         # not contiguous
    with pytest.raises((ValueError, TooncrafterHipError)):
        hip.colour_transfer(x, src, two, REF_PIXELS, 1.0, out=x.view(-1)[1:])
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ graph capture

@pytest.mark.parametrize("method", ["hm", "hm_mkl_hm"])
@pytest.mark.parametrize("binding", ["ctypes", "torch"])
def test_match_colour_replays_from_a_captured_graph(hip, tl, binding, method):
    """the calls of match_colour captured once and replayed on changed inputs: no allocation outside the caching allocator, no
    synchronisation, no host read of device memory"""
    from tooncrafter_amd import ops, output
    shape = (2, 5, 24, 40)
    first = dict(x=cm.frames(21, *shape), ends=cm.frames(22, 2, 2, *REF_HW))
    second = case(shape)
    m = output.ColourMatch(method, 0.75)
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

RANKS = tuple((2 * k + 1) / 20 for k in range(10))                               # ten fixed ranks: 0.05, 0.15, ... 0.95


def quantile_bins(counts):
    """the bin of rank r of a histogram (1024,), for the ten RANKS: the smallest j with sum_{i <= j} counts_i >= r * total"""
    cum = np.cumsum(np.asarray(counts, np.int64))
    return np.array([int(np.searchsorted(cum, r * cum[-1], side="left")) for r in RANKS])


def test_timeline_seam_has_the_inner_keyframes_quantiles(tiny):  # noqa: F811
    """three keyframes, two segments, match=ColourMatch("hm").  The video is the transferred clips in the writer's bytes; the
    last frame of segment 0 and frame 0 of segment 1, transferred, have per-channel histograms whose quantiles at the ten RANKS
    lie within one bin of the inner keyframe's: the seam does not step.  The statement alone, run on the decoded clips, meets
    the same, and the device's clips are the statement's bit for bit.
    The keyframes: 8-bit keyframes at model size hold one code in every fourth bin, a transferred frame lands on the bins
    its keyframe occupies, and at a rank where the keyframe's quantile function steps from one code to the next the two
    can sit either side of that step.  So the keyframes are the golden crops at a sixteenth of their contrast around mid
    grey: 17 well-filled codes, and the ten ranks stay clear of the steps (the statement alone, on the tiny model's decoded
    clips: off by 134 to 222 bins before the transfer, by at most 1 after, also with noise of 0.01 added to the decoded clip;
    with the crops at full contrast, 235 sparse codes, it is off by 3 to 4 bins after)."""
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd import ops, output
    model, _ = tiny
    fr = load_golden("pixel_front.npz")
    h, w = (int(v) for v in fr["e2e.size"])
    a, b = fr["e2e.src"][0][:36, :52], fr["e2e.src"][1][:36, :52]
    full = np.stack([a, b, a[::-1, ::-1]]).astype(np.float64)
    kf = torch.from_numpy(np.clip(np.round(128 + (full - 128) / 16), 0, 255).astype(np.uint8)).to(DEV)
    shape, seeds, t = [1, 4, 4, h // 8, w // 8], [51, 52], 4
    m = output.ColourMatch("hm")

    def plan(s):
        return pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=s)
    with torch.no_grad():
        video = pipeline.synthesize_timeline_u8(model, kf, shape, size=(h, w), plan=plan(seeds), fs=10, match=m)
        assert video.shape == (7, h, w, 3)
        pieces = []
        for i, s in enumerate(seeds):
            cond = pipeline.Conditions.from_uint8(model, kf[i:i + 1], kf[i + 1:i + 2], size=(h, w), t=t, prompts=None, fs=10, guided=True,
                                                  three_way=False, image_branch=True, hold_endpoints=True)
            decoded = pipeline.decode_spliced(model, pipeline.sample(model, cond, plan([s]), shape), cond.refs).to(torch.float32)
            matched = output.match_colour(decoded, cond.ends_px, m)
            pieces.append(ops.frames_to_u8(matched, frames=(0, t))[0])
            ends = cond.ends_px.cpu().numpy()
            want = ref.transfer(decoded.cpu().numpy(), ends, 1.0)[0]
            assert same_bits(matched, want)
            f, e = ((t - 1, 1), (0, 0))[i]                                        # the frame at the seam and the inner keyframe's slot
            key = ref.hist(ends)[0, e]
            for name, y in (("device", matched.cpu().numpy()), ("statement", want)):
                before, after = ref.hist(decoded.cpu().numpy())[0, f], ref.hist(y)[0, f]
                for k in range(3):
                    was = np.abs(quantile_bins(before[k]) - quantile_bins(key[k])).max()
                    off = np.abs(quantile_bins(after[k]) - quantile_bins(key[k])).max()
                    print(f"segment {i} frame {f} channel {k} ({name}): quantiles off the keyframe's by {was} bins before, {off} after")
                    assert off <= 1
    assert torch.equal(video, torch.cat([pieces[0], pieces[1][1:]]))
