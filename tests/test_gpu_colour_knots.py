"""Colour match through knots and its gain limit on the MI355X (tc_colour_match_knots, tc_colour_transfer_knots: the coefficient
kernel of csrc/colour_match.hip, the table kernel of csrc/colour_hist.hip, the course of csrc/colour_course.h) against the
statement of tests/colour_knots_ref.py, every case through both bindings (HipOps, TorchLibOps), whose results must be the same
bits:

  * knots {0, t - 1} without a limit are the old entry points bit for bit: coefficients, tables, outputs; with t = 1 and two
    clips (2, 1, 8 x 8) the old entry points still step two reference images per clip;
  * the tables of every knot set equal the statement bit for bit; the coefficients of every knot set, limited or not, lie within
    relative 2^-22 of the statement rounded to fp32, and the apply pass is the stated fp32 arithmetic on the device's own
    coefficients, bit for bit;
  * the limited map on the device: eigenvalues inside [1 / g, g], the means still matched; the exact consequences; refusals
    write nothing; the knots calls under a captured graph; `synthesize(keyframes=, match=ColourMatch(targets="pinned"))`.

Shapes (b, t, h x w): (2, 5, 7 x 9) less than a wave, odd, planes on 4-byte boundaries only; (2, 6, 24 x 40) a ragged tail of a
256-thread block, twelve frames in all; (1, 1, 8 x 8) t = 1; (1, 64, 8 x 8) as many knots as frames, and a full 64-thread block
of the coefficient kernel.  References are 17 x 23.  Nothing expected comes from the kernels.

The limited map (g = 4) against the statement: the second Jacobi decomposition costs nothing measurable -- the Jacobi statement
and the same map by numpy.linalg.eigh differ by 2.85e-15 relative (1.2e-8 x 2^-22) on these cases
(tests/test_colour_knots_cpu.py measures and asserts it), so the bound stays the project's 2^-22."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import colour_hist_ref as ch
import colour_knots_ref as ref
import colour_match_ref as cm
from conftest import load_golden
from test_gpu_colour_match import host_apply
from test_gpu_pixel_front import shim_frames, tiny  # noqa: F401  (the tiny model with a tiny image tower, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
M = ref.REF_HW[0] * ref.REF_HW[1]
G = 4.0
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
    """the seeded inputs of a shape (ref.inputs) and what the statement says of them, computed once and left unchanged"""
    x, refs = ref.inputs(shape, kind)
    got = dict(x=x, refs=refs)
    if kind in ("toon", "grid"):
        got.update(hist=ch.hist(x), ref_hist=ch.hist(refs))
    else:
        got.update(stats=cm.frame_stats(x), ref_stats=cm.frame_stats(refs))
    for v in got.values():
        v.setflags(write=False)
    return got


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                  # a copy: the cached inputs are read-only


def device_stats(be, c, nk):
    x, refs = dev(c["x"]), dev(c["refs"][:, :, :nk])
    return x, be.colour_stats(x), be.colour_stats(refs)


def device_hists(be, c, nk):
    x, refs = dev(c["x"]), dev(c["refs"][:, :, :nk])
    return x, be.colour_hist(x), be.colour_hist(refs)


# ------------------------------------------------------------------------------------------------ 1. the old entry points

@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_the_two_ends_without_a_limit_are_the_old_entry_points_bit_for_bit(hip, tl, shape):
    b, t, h, w = shape
    knots = (0, t - 1) if t > 1 else (0,)
    c, toon = case(shape, "random"), case(shape, "toon")
    for be in (hip, tl):
        x, src, some = device_stats(be, c, len(knots))
        two = some if t > 1 else torch.cat([some, some], dim=1)                   # t = 1: the old call reads the first of two
        for method in ("mkl", "mean_std"):
            for strength in (1.0, 0.5):
                old_out, old_co = be.colour_match(x, src, two, M, method, strength)
                new_out, new_co = be.colour_match(x, src, some, M, method, strength, knots=knots, max_gain=0.0)
                assert torch.equal(new_co, old_co) and torch.equal(new_out, old_out), (type(be).__name__, method, strength)
                if t > 1:                                                         # a limit of None with knots, knots of None with a limit of 0
                    assert torch.equal(be.colour_match(x, src, two, M, method, strength, knots=knots)[1], old_co)
                    assert torch.equal(be.colour_match(x, src, two, M, method, strength, max_gain=0)[1], old_co)
        x, hsrc, hsome = device_hists(be, toon, len(knots))
        htwo = hsome if t > 1 else torch.cat([hsome, hsome], dim=1)
        for strength in (1.0, 0.5):
            old_out, old_tab = be.colour_transfer(x, hsrc, htwo, M, strength)
            new_out, new_tab = be.colour_transfer(x, hsrc, hsome, M, strength, knots=knots)
            assert torch.equal(new_tab, old_tab) and torch.equal(new_out, old_out), (type(be).__name__, strength)
            base = x.flip(2).contiguous()
            assert torch.equal(be.colour_transfer(x, hsrc, hsome, M, strength, base=base, knots=knots)[0],
                               be.colour_transfer(x, hsrc, htwo, M, strength, base=base)[0])


def four_references(make, seed):
    """(2, 3, 2, 17, 23): two reference images per clip, each with an offset and a contrast of its own"""
    refs = make(seed, 2, 2, *ref.REF_HW).astype(np.float64)
    for (i, j), (gain, offset) in {(0, 0): (1.0, -0.3), (0, 1): (0.45, 0.35), (1, 0): (0.7, 0.15), (1, 1): (0.3, -0.1)}.items():
        refs[i, :, j] = gain * refs[i, :, j] + offset
    return refs.astype(np.float32)


def test_the_old_entry_points_step_two_reference_images_per_clip_when_t_is_1(hip, tl):
    """t = 1: only the first of a clip's two reference images is a knot, but the old entry points still take two per clip, so
    clip 1's target is row 2 of `ref`, not row 1.  Two clips (every other t = 1 case has one, where the stride is multiplied by
    zero) against four clearly different images.  The expectation is the numpy statements' alone: the old ones on both images,
    which equal the knots statement on the first; the device must meet it through the old call and through knots=(0,) on
    ref[:, :1], with the same bits."""
    b, t, h, w = shape = (2, 1, 8, 8)
    x_np, refs_np = cm.frames(sum(shape), *shape), four_references(cm.frames, sum(shape) + 1)
    tx_np, trefs_np = ch.toon_frames(sum(shape), *shape), four_references(ch.toon_frames, sum(shape) + 1)
    stats, ref_stats = cm.frame_stats(x_np), cm.frame_stats(refs_np)
    hist, ref_hist = ch.hist(tx_np), ch.hist(trefs_np)
    want_tab, _ = ch.table(hist, ref_hist, h * w, M)
    assert np.array_equal(want_tab.view(np.int32), ref.table(hist, ref_hist[:, :1], (0,), h * w, M)[0].view(np.int32))
    strided = ref.table(hist[1:], ref_hist[:1, 1:], (0,), h * w, M)[0]              # clip 1 against row 1: a stride of one
    assert np.abs(want_tab[1] - strided[0]).max() > 0.05
    want_out = ch.apply(tx_np, want_tab, 0.75)
    want_co = {}
    for method in ("mkl", "mean_std"):
        want = cm.coefs(stats, ref_stats, h * w, M, method, 0.75)
        assert np.array_equal(want, ref.coefs(stats, ref_stats[:, :1], (0,), h * w, M, method, 0.75))
        strided = ref.coefs(stats[1:], ref_stats[:1, 1:], (0,), h * w, M, method, 0.75)
        assert np.abs(want[1] - strided[0]).max() > 0.05
        want_co[method] = want.astype(np.float32).astype(np.float64)
    for i in range(b):
        assert cm.cond(cm.moments(stats[i, 0], h * w)[1]) <= 1e3
    for be in (hip, tl):
        x, two = dev(tx_np), be.colour_hist(dev(trefs_np))
        src = be.colour_hist(x)
        assert two.shape == (2, 2, 3, 1024) and np.array_equal(two.cpu().numpy(), ref_hist)
        out, tab = be.colour_transfer(x, src, two, M, 0.75)
        assert np.array_equal(tab.cpu().numpy().view(np.int32), want_tab.view(np.int32)), type(be).__name__
        assert np.array_equal(out.cpu().numpy().view(np.int32), want_out.view(np.int32)), type(be).__name__
        out1, tab1 = be.colour_transfer(x, src, two[:, :1].contiguous(), M, 0.75, knots=(0,))
        assert torch.equal(tab1, tab) and torch.equal(out1, out), type(be).__name__
        x, two = dev(x_np), be.colour_stats(dev(refs_np))
        src = be.colour_stats(x)
        assert two.shape == (2, 2, 9)
        for method in ("mkl", "mean_std"):
            out, co = be.colour_match(x, src, two, M, method, 0.75)
            err = np.abs(co.cpu().numpy().astype(np.float64) - want_co[method]) / np.maximum(1.0, np.abs(want_co[method]))
            print(f"{type(be).__name__} {method}: worst coefficient error {err.max() * 2 ** 22:.3g} x 2^-22")
            assert (err <= 2.0 ** -22).all(), (type(be).__name__, method)
            assert torch.equal(out.cpu(), host_apply(x, co)), (type(be).__name__, method)
            out1, co1 = be.colour_match(x, src, two[:, :1].contiguous(), M, method, 0.75, knots=(0,))
            assert torch.equal(co1, co) and torch.equal(out1, out), (type(be).__name__, method)


# ------------------------------------------------------------------------------------------------ 2. tables

@pytest.mark.parametrize("kind", ["toon", "grid"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_tables_of_every_knot_set_equal_the_statement_bit_for_bit(hip, tl, shape, kind):
    b, t, h, w = shape
    c = case(shape, kind)
    for knots in ref.KNOT_SETS[t]:
        nk = len(knots)
        want, _ = ref.table(c["hist"], c["ref_hist"][:, :nk], knots, h * w, M)
        x, hsrc, hrefs = device_hists(hip, c, nk)
        assert np.array_equal(hsrc.cpu().numpy(), c["hist"]) and np.array_equal(hrefs.cpu().numpy(), c["ref_hist"][:, :nk])
        out, tab = hip.colour_transfer(x, hsrc, hrefs, M, 0.75, knots=knots)
        assert tab.shape == (b, t, 3, 1024) and tab.dtype == torch.float32
        assert np.array_equal(tab.cpu().numpy().view(np.int32), want.view(np.int32)), knots
        assert np.array_equal(out.cpu().numpy().view(np.int32), ch.apply(c["x"], want, 0.75).view(np.int32)), knots
        out2, tab2 = tl.colour_transfer(x, hsrc, hrefs, M, 0.75, knots=knots)
        assert torch.equal(tab2, tab) and torch.equal(out2, out)
        mine = x.clone()                                                          # in place, through either binding's out=
        assert torch.equal(tl.colour_transfer(mine, hsrc, hrefs, M, 0.75, out=mine, knots=knots)[0], out)


# ------------------------------------------------------------------------------------------------ 3. - 5. coefficients

def check_coefficients(hip, tl, shape, kind, method, strength, max_gain):
    """the device's coefficients of every knot set within relative 2^-22 of the statement rounded to fp32 (inputs with
    cond <= 1e3), the same bits through both bindings, and the apply pass from them bit for bit; returns them per knot set"""
    b, t, h, w = shape
    c = case(shape, kind)
    for i in range(b):
        for f in range(t):
            assert cm.cond(cm.moments(c["stats"][i, f], h * w)[1]) <= 1e3
    got = {}
    for knots in ref.KNOT_SETS[t]:
        nk = len(knots)
        want = ref.coefs(c["stats"], c["ref_stats"][:, :nk], knots, h * w, M, method, strength, max_gain or 0.0)
        want = want.astype(np.float32).astype(np.float64)
        x, src, refs = device_stats(hip, c, nk)
        out, co = hip.colour_match(x, src, refs, M, method, strength, knots=knots, max_gain=max_gain)
        assert co.shape == (b, t, 12) and co.dtype == torch.float32
        err = np.abs(co.cpu().numpy().astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
        print(f"{shape} {kind} {method} {strength} g={max_gain} {knots if nk < 8 else nk}: worst coefficient error "
              f"{err.max() * 2 ** 22:.3g} x 2^-22")
        assert (err <= 2.0 ** -22).all(), knots
        assert torch.equal(out.cpu(), host_apply(x, co)), knots
        out2, co2 = tl.colour_match(x, src, refs, M, method, strength, knots=knots, max_gain=max_gain)
        assert torch.equal(co2, co) and torch.equal(out2, out)
        got[knots] = co.cpu().numpy().astype(np.float64)
    return got


@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("method", ["mkl", "mean_std"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_coefficients_of_every_knot_set_are_within_the_bound_of_the_statement(hip, tl, shape, method, strength):
    check_coefficients(hip, tl, shape, "random", method, strength, None)


@pytest.mark.parametrize("kind", ["flat", "steep"])
@pytest.mark.parametrize("method", ["mkl", "mean_std"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_the_limited_map_meets_the_same_bound_and_keeps_gains_and_means(hip, tl, shape, method, kind):
    """g = 4 on the gain-limit case ("flat": unlimited gains above 4 g; "steep": the reverse, below 1 / (4 g); both checked on the
    CPU).  The bound is the 2^-22 of the unlimited map: Jacobi against LAPACK on the same limited map differ by 2.85e-15 relative
    (1.2e-8 x 2^-22) on these cases, so nothing is widened.  At strength 1, on the DEVICE's coefficients: the eigenvalues of the
    symmetrised A' lie in [1 / g, g] up to a relative 2^-20, and o' + A' m_s equals m_t within 2^-20 max(1, |m_t|) -- twelve fp32
    roundings of numbers below 2 g weigh 2^-24 each."""
    b, t, h, w = shape
    check_coefficients(hip, tl, shape, kind, method, 0.5, G)
    got = check_coefficients(hip, tl, shape, kind, method, 1.0, G)
    c = case(shape, kind)
    for knots, co in got.items():
        a = co[..., :9].reshape(b, t, 3, 3)
        lam = np.linalg.eigvalsh(0.5 * (a + a.transpose(0, 1, 3, 2)))
        assert lam.min() >= (1 / G) * (1 - 2.0 ** -20) and lam.max() <= G * (1 + 2.0 ** -20), (knots, lam.min(), lam.max())
        for i in range(b):
            moments = [cm.moments(c["ref_stats"][i, k], M) for k in range(len(knots))]
            for f in range(t):
                ms, mt = cm.moments(c["stats"][i, f], h * w)[0], ref.target(moments, knots, f)[0]
                assert (np.abs(co[i, f, 9:] + a[i, f] @ ms - mt) <= 2.0 ** -20 * np.maximum(1.0, np.abs(mt))).all(), (knots, i, f)


# ------------------------------------------------------------------------------------------------ 6. exact consequences

@pytest.mark.parametrize("shape", ref.SHAPES[:2], ids=ref.IDS[:2])
def test_exact_consequences(hip, tl, shape):
    b, t, h, w = shape
    c = case(shape, "random")
    for be in (hip, tl):
        x = dev(c["x"])
        clamped = x.clamp(-1.0, 1.0)
        src, hsrc = be.colour_stats(x), be.colour_hist(x)
        # a knot frame whose reference is that frame itself comes back as clamp(x)
        for knots in ref.KNOT_SETS[t]:
            own = x[:, :, list(knots)].contiguous()
            out, co = be.colour_match(x, src, be.colour_stats(own), h * w, "mean_std", 1.0, knots=knots)
            out2, tab = be.colour_transfer(x, hsrc, be.colour_hist(own), h * w, 1.0, knots=knots)
            for k in knots:
                assert np.array_equal(co[:, k].cpu().numpy(), np.broadcast_to(IDENTITY, (b, 12)))
                assert not tab[:, k].any() and torch.equal(out[:, :, k], clamped[:, :, k]) and torch.equal(out2[:, :, k], clamped[:, :, k])
        # knots {1, 3}, frames 0 and 1 with the same pixels: the same coefficients and tables
        twin = x.clone()
        twin[:, :, 0] = twin[:, :, 1]
        refs = dev(c["refs"][:, :, :2])
        for method in ("mkl", "mean_std"):
            co = be.colour_match(twin, be.colour_stats(twin), be.colour_stats(refs), M, method, 1.0, knots=(1, 3), max_gain=G)[1]
            assert torch.equal(co[:, 0], co[:, 1]) and not torch.equal(co[:, 1], co[:, 2])
        tab = be.colour_transfer(twin, be.colour_hist(twin), be.colour_hist(refs), M, 1.0, knots=(1, 3))[1]
        assert torch.equal(tab[:, 0], tab[:, 1]) and not torch.equal(tab[:, 1], tab[:, 2])
        # MEAN_STD with g = 1 is the exact mean shift: A' = I, o' = fp32(s (m_t - m_s)); on the frames that take one knot itself
        # m_t is that knot's mean bit for bit, between two knots it is one double rounding away from the statement's
        knots = ref.KNOT_SETS[t][1]
        three = be.colour_stats(dev(c["refs"][:, :, :3]))
        sums, ref_sums = src.cpu().numpy(), three.cpu().numpy()                    # the device's own sums: exact means exact
        for s in (1.0, 0.5):
            out, co = be.colour_match(x, src, three, M, "mean_std", s, knots=knots, max_gain=1.0)
            co = co.cpu().numpy()
            assert np.array_equal(co[..., :9], np.broadcast_to(IDENTITY[:9], co[..., :9].shape))
            for i in range(b):
                moments = [cm.moments(ref_sums[i, k], M) for k in range(3)]
                for f in range(t):
                    want = s * (ref.target(moments, knots, f)[0] - cm.moments(sums[i, f], h * w)[0])
                    if ref.course(knots, f)[1]:
                        assert np.array_equal(co[i, f, 9:], want.astype(np.float32)), (i, f)
                    else:
                        assert (np.abs(co[i, f, 9:] - want) <= 2.0 ** -22 * np.maximum(1.0, np.abs(want))).all(), (i, f)
            assert torch.equal(out.cpu(), host_apply(x, torch.from_numpy(co)))
        # strength 0 returns clamp(x)
        for method in ("mkl", "mean_std"):
            out, co = be.colour_match(x, src, three, M, method, 0.0, knots=knots, max_gain=G)
            assert torch.equal(out, clamped) and np.array_equal(co.cpu().numpy(), np.broadcast_to(IDENTITY, co.shape))
        assert torch.equal(be.colour_transfer(x, hsrc, be.colour_hist(dev(c["refs"][:, :, :3])), M, 0.0, knots=knots)[0], clamped)


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refused_requests_write_nothing(hip):
    from tooncrafter_amd import _lib
    shape = (2, 5, 7, 9)
    b, t, h, w = shape
    c = case(shape, "random")
    x, src, three = device_stats(hip, c, 3)
    hsrc, h3 = hip.colour_hist(x), hip.colour_hist(dev(c["refs"][:, :, :3]))
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((1 << 17,), SENTINEL, dtype=torch.uint8, device=DEV)
    room = buf[256:]

    def match_rc(knots=(0, 2, 4), **kw):
        p = _lib.TcColourMatchKnotsParams(x=x.data_ptr(), out=room.data_ptr(), b=b, t=t, h=h, w=w, src=src.data_ptr(), ref=three.data_ptr(),
                                          ref_pixels=M, method=1, strength=1.0, coefs=room.data_ptr() + 8192, nk=len(knots), max_gain=G)
        p.knot[:len(knots)] = knots
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib.tc_colour_match_knots(C.byref(p), stream)

    def transfer_rc(knots=(0, 2, 4), **kw):
        p = _lib.TcColourTransferKnotsParams(x=x.data_ptr(), base=None, out=room.data_ptr(), b=b, t=t, h=h, w=w, src=hsrc.data_ptr(),
                                             ref=h3.data_ptr(), ref_pixels=M, strength=1.0, table=room.data_ptr() + 8192, nk=len(knots))
        p.knot[:len(knots)] = knots
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib.tc_colour_transfer_knots(C.byref(p), stream)
    for rc in (match_rc, transfer_rc):
        assert rc(nk=0) == -1 and rc(nk=-1) == -1 and rc(nk=65) == -1
        for knots in ((0, 2, 2), (0, 4, 2), (2, 0, 4), (0, 2, 5), (-1, 2, 4), (5,)):
            assert rc(knots=knots) == -1, knots
        assert rc(strength=1.5) == -1 and rc(strength=float("nan")) == -1 and rc(ref_pixels=0) == -1 and rc(t=0) == -1
        assert rc(x=room.data_ptr() + 4, out=room.data_ptr()) == -1               # a partial overlap
    for g in (-1.0, 0.5, float("inf"), float("nan")):
        assert match_rc(max_gain=g) == -1, g
    assert match_rc(method=2) == -1 and match_rc(coefs=None) == -1 and transfer_rc(table=None) == -1
    assert match_rc(src=src.data_ptr() + 4) == -2 and match_rc(ref=three.data_ptr() + 4) == -2
    assert transfer_rc(src=hsrc.data_ptr() + 2) == -2 and transfer_rc(ref=h3.data_ptr() + 2) == -2
    assert transfer_rc(table=room.data_ptr() + 8194) == -2 and transfer_rc(ref_pixels=2 ** 26 + 1) == -3
    for bad in (dict(knots=(0, 2, 2)), dict(knots=(0, 2, 5)), dict(knots=(0, 4)), dict(max_gain=0.5), dict(max_gain=float("nan"))):
        kw = dict(knots=(0, 2, 4), max_gain=G)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip.colour_match(x, src, three, M, "mkl", 1.0, **kw)
    for knots in ((0, 2, 2), (0, 2, 5), (0, 4)):
        with pytest.raises(ValueError):
            hip.colour_transfer(x, hsrc, h3, M, 1.0, knots=knots)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ 8. graph capture

@pytest.mark.parametrize("binding", ["ctypes", "torch"])
def test_the_knots_calls_replay_from_a_captured_graph(hip, tl, binding):
    """match_colour with an inner target and a gain limit under "hm_mkl_hm" (both knots calls, nine launches) captured once and
    replayed on changed inputs: the knots are host values in the kernel arguments, nothing is read back"""
    from tooncrafter_amd import ops, output
    shape = (2, 6, 24, 40)
    first, second = case(shape, "random"), case(shape, "toon")
    m = output.ColourMatch("hm_mkl_hm", 0.75, max_gain=G)

    def parts(c):
        return dev(c["x"]), dev(c["refs"][:, :, :2]), dev(c["refs"][:, :, 2])
    prev = ops.set_backend(hip if binding == "ctypes" else tl)
    try:
        v2, e2, i2 = parts(second)
        eager = output.match_colour(v2, e2, m, inner={2: i2})
        video, ends, inner = parts(first)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            output.match_colour(video, ends, m, inner={2: inner})
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = output.match_colour(video, ends, m, inner={2: inner})
        video.copy_(v2)
        ends.copy_(e2)
        inner.copy_(i2)
        out.fill_(7.0)
        gr.replay()
        torch.cuda.synchronize()
    finally:
        ops.set_backend(prev)
    assert torch.equal(out, eager) and not torch.equal(eager, v2.clamp(-1, 1))
    assert not torch.equal(eager, output.match_colour(v2, e2, output.ColourMatch("hm_mkl_hm", 0.75)))


# ------------------------------------------------------------------------------------------------ 9. the public path

def test_synthesize_matches_pinned_frames_to_the_images_they_were_pinned_to(tiny):  # noqa: F811
    """`synthesize(keyframes={2: px}, match=ColourMatch("mkl", targets="pinned"))` is `match_colour` with inner={2: px} on the
    unmatched seeded clip, bit for bit; it differs from targets="ends", which is the call of the parent's signature,
    ColourMatch("mkl")."""
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd import output
    model, _ = tiny
    fr = load_golden("pixel_front.npz")
    h, w = (int(v) for v in fr["e2e.size"])
    first, last = (shim_frames(fr["e2e.crop_u8"])[i].to(DEV) for i in range(2))    # (3, h, w) each, in [-1, 1]
    videos = torch.zeros(1, 3, 4, h, w, device=DEV)
    videos[0, :, 0], videos[0, :, 3] = first, last
    px = (0.6 * first.flip(-1) + 0.2)[None].contiguous()                           # another image: other means, other contrast
    shape = [1, 4, 4, h // 8, w // 8]

    def run(**kw):
        plan = pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=[61])
        return pipeline.synthesize(model, videos, shape, plan=plan, fs=10, keyframes={2: px}, **kw)[:, 0]
    with torch.no_grad():
        plain = run()
        pinned = run(match=output.ColourMatch("mkl", targets="pinned"))
        ends = run(match=output.ColourMatch("mkl", targets="ends"))
        parent = run(match=output.ColourMatch("mkl"))
        two = torch.stack([videos[:, :, 0], videos[:, :, 3]], dim=2)
        assert torch.equal(pinned, output.match_colour(plain, two, output.ColourMatch("mkl"), inner={2: px}))
        assert torch.equal(ends, parent) and torch.equal(parent, output.match_colour(plain, two, output.ColourMatch("mkl")))
        assert not torch.equal(pinned, ends) and torch.equal(pinned[:, :, [0, 3]], ends[:, :, [0, 3]])
        limited = run(match=output.ColourMatch("mkl", max_gain=1.0, targets="pinned"))
        assert torch.equal(limited, output.match_colour(plain, two, output.ColourMatch("mkl", max_gain=1.0), inner={2: px}))
        assert not torch.equal(limited, pinned)
