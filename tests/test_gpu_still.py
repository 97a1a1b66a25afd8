"""tc_still_map and tc_still_composite on the MI355X (csrc/still.hip) against the numpy statement of tests/still_ref.py, bit for
bit in mask, alpha and dist and in every composited frame; a captured graph of the two ops; and one run of the tiny model with
`still=`.  The shapes are the smallest at which the kernels can go wrong: 2 x 3 and 3 x 5 cells (a block of the scan is 16 cells
wide, so both are partial blocks), D larger than the map, and one 40 x 64 map (four scan blocks per cell row, 2560 cells in LDS)."""
import contextlib
import ctypes
import hashlib
import sys

import numpy as np
import pytest
import torch

import still_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR8 = np.float32(8) / np.float32(127.5)

# sha256 of the seeded tiny-model clip of `seeded_clip` without `still`, taken from the parent commit's tree on the MI355X
PARENT_CLIP_SHA256 = "b5340345d9dd79b9eb284a15bf855a2eed4cf3ada32295b0eeab01caa4c14ec2"


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def model(tiny_sd):
    from test_host_logic_cpu import _tiny_model_cfg
    from tooncrafter_amd.utils import instantiate_from_config
    m = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=_tiny_model_cfg())).eval()
    m.load_state_dict(tiny_sd, strict=False)
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the map, bit for bit

def still_pair(b, hh, ww, seed=0):
    """two equal keyframes per clip: all still at any tau"""
    x = np.random.default_rng(seed).uniform(-1, 1, (b, 3, 1, hh, ww)).astype(np.float32)
    return np.ascontiguousarray(x.repeat(2, axis=2))


def poke(ends, places, clip=0, ch=0, by=0.5):
    for y, x in places:
        ends[clip, ch, 1, y, x] = ends[clip, ch, 0, y, x] + (by if ends[clip, ch, 0, y, x] < 0 else -by)
    return ends


def case(name, hh, ww):
    """(ends, tau) of a named case at hh x ww"""
    e, tau = still_pair(1, hh, ww, seed=len(name)), 8
    if name.startswith("corner"):
        k = int(name[-1])
        poke(e, [((hh - 1) * (k // 2), (ww - 1) * (k % 2))])
    elif name == "row_7":
        poke(e, [(3, 7)])
    elif name == "row_8":
        poke(e, [(3, 8)])
    elif name == "col_7":
        poke(e, [(7, 13)])
    elif name == "col_8":
        poke(e, [(8, 13)])
    elif name in ("channel_1", "channel_2"):
        poke(e, [(hh - 3, ww // 2)], ch=int(name[-1]))
    elif name in ("at_thr", "above_thr"):
        e[:] = 0.0
        e[0, 1, 0, hh - 1, 2] = THR8 if name == "at_thr" else np.nextafter(THR8, np.float32(1))
    elif name == "nan":
        e[0, 2, 1, 9, ww - 1] = np.nan
    elif name == "nan_both":
        e[0, 0, :, 9, 1] = np.nan
    elif name == "clamped_equal":
        e[0, 0, :, 0, 0] = (1.5, 3.0)
        e[0, 1, :, 5, 9] = (-2.0, -1.0)
        e[0, 2, :, hh - 1, ww - 1] = (np.inf, 1.0)
        e[0, 2, :, 8, 8] = (-np.inf, -7.0)
    elif name == "clamped_apart":
        e[0, 0, :, 8, 8] = (1.5, -1.5)
    elif name == "all_still":
        pass
    elif name == "all_moved":
        e[:, :, 1] = -e[:, :, 0] + np.where(np.abs(e[:, :, 0]) < 0.25, np.float32(0.5), np.float32(0))
    elif name == "tau_0":
        tau = 0
        e[0, 0, 1, 1, 1] = np.nextafter(e[0, 0, 0, 1, 1], np.float32(2))            # one ulp apart: moved at tau 0
    elif name == "tau_255":
        tau = 255
        e[0, 0, :, 0, 0] = (1.0, -1.0)                                              # 2 apart: thr = 2, not moved
        e[0, 1, :, hh - 1, ww - 1] = (np.nan, 0.0)                                  # only a NaN moves at tau 255
    elif name == "scattered":
        rng = np.random.default_rng(hh * ww)
        poke(e, [(int(rng.integers(hh)), int(rng.integers(ww))) for _ in range(max(2, hh * ww // 4096))], ch=1)
    else:
        raise KeyError(name)
    return e, tau


CASES = ["corner_0", "corner_1", "corner_2", "corner_3", "row_7", "row_8", "col_7", "col_8", "channel_1", "channel_2", "at_thr",
         "above_thr", "nan", "nan_both", "clamped_equal", "clamped_apart", "all_still", "all_moved", "tau_0", "tau_255", "scattered"]
RULES = [(0, 1), (1, 2), (2, 3), (0, 3), (2, 1)]                                    # (grow, feather): D = 2 .. 6, larger than 2 x 3 cells


def check_map(hip, ends, tau, grow, feather, tag):
    want = ref.still_map(ends, tau, grow, feather)
    got = hip.still_map(torch.from_numpy(ends).to(DEV), tau=tau, grow=grow, feather=feather)
    b, hh, ww = ends.shape[0], ends.shape[3], ends.shape[4]
    assert [tuple(v.shape) for v in got] == [(b, 1, 1, hh // 8, ww // 8), (b, hh, ww), (b, hh // 8, ww // 8)], tag
    assert [v.dtype for v in got] == [torch.float32, torch.float32, torch.uint8], tag
    for name, g, w in zip(("mask", "alpha", "dist"), got, want):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (tag, name)
    return want


@pytest.mark.parametrize("size", [(16, 24), (24, 40)])
@pytest.mark.parametrize("name", CASES)
def test_still_map_is_bit_exact(hip, name, size):
    ends, tau = case(name, *size)
    moved = ref.moved_cells(ends, tau)
    expect = {"at_thr": 0, "clamped_equal": 0, "all_still": 0, "nan_both": 1, "above_thr": 1, "nan": 1, "clamped_apart": 1, "tau_0": 1,
              "tau_255": 1, "all_moved": moved.size}                                # the statement says what the case is meant to show
    if name in expect:
        assert moved.sum() == expect[name], name
    if name in ("row_7", "row_8", "col_7", "col_8"):                                # either side of a cell edge: another cell
        assert [v.tolist() for v in moved[0].nonzero()] == {"row_7": [[0], [0]], "row_8": [[0], [1]], "col_7": [[0], [1]], "col_8": [[1], [1]]}[name]
    for grow, feather in RULES:
        check_map(hip, ends, tau, grow, feather, (name, size, grow, feather))


def test_still_map_keeps_the_clips_of_a_batch_apart(hip):
    parts = [case("corner_3", 24, 40)[0], case("all_still", 24, 40)[0], case("col_8", 24, 40)[0]]
    ends = np.ascontiguousarray(np.concatenate(parts))
    for grow, feather in ((1, 2), (0, 1)):
        mask, alpha, dist = check_map(hip, ends, 8, grow, feather, ("batch", grow, feather))
        for i, part in enumerate(parts):
            one = ref.still_map(part, 8, grow, feather)
            assert np.array_equal(mask[i], one[0][0]) and np.array_equal(alpha[i], one[1][0]) and np.array_equal(dist[i], one[2][0])
        assert (dist[1] == grow + feather + 1).all() and (alpha[1] == 1).all() and not (dist[0] == dist[2]).all()


@pytest.mark.parametrize("name,grow,feather", [("scattered", 1, 2), ("corner_3", 2, 29), ("all_still", 1, 2)])
def test_still_map_at_320x512(hip, name, grow, feather):
    ends, tau = case(name, 320, 512)
    _, alpha, dist = check_map(hip, ends, tau, grow, feather, (name, 320, 512))
    if name == "scattered":
        assert 0 < (alpha == 1).mean() < 1 and 0 < (alpha == 0).mean() < 1 and (dist == 0).sum() >= 2
    if name == "corner_3":                                                          # D = 32: the distance runs over the whole map
        assert dist[0, 39, 63] == 0 and dist[0, 39, 40] == 23 and dist[0, 0, 0] == 32 and dist[0, 8, 63] == 31


def test_still_map_refuses_shapes_that_are_no_multiple_of_8_without_a_launch(hip):
    from tooncrafter_amd import _lib
    guard = torch.full((4096,), 7.0, device=DEV)
    marks = torch.full((64,), 9, dtype=torch.uint8, device=DEV)
    ends = torch.zeros(1, 3, 2, 24, 40, device=DEV)
    for hh, ww in ((20, 40), (24, 36), (23, 39), (4, 4)):
        p = _lib.TcStillMapParams(ends=ends.data_ptr(), b=1, h=hh, w=ww, tau=8, grow=1, feather=2, mask=guard.data_ptr(),
                                  alpha=guard[1024:].data_ptr(), dist=marks.data_ptr())
        assert hip.lib.tc_still_map(ctypes.byref(p), torch.cuda.current_stream().cuda_stream) == -3, (hh, ww)       # TC_ESHAPE
        with pytest.raises(ValueError):
            hip.still_map(torch.zeros(1, 3, 2, hh, ww, device=DEV))
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all()) and bool((marks == 9).all()), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ 2. the composite, bit for bit

def composite_inputs(b, t, hh, ww, seed):
    rng = np.random.default_rng(seed)
    video = rng.uniform(-1.2, 1.2, (b, 3, t, hh, ww)).astype(np.float32)
    ends = rng.uniform(-1, 1, (b, 3, 2, hh, ww)).astype(np.float32)
    alpha = rng.uniform(0, 1, (b, hh, ww)).astype(np.float32)
    alpha[:, :, : ww // 3] = 0.0                                                    # whole groups of four at 0 ...
    alpha[:, : hh // 2, -(ww // 3):] = 1.0                                          # ... and at 1
    alpha[:, hh - 1, ::3] = 0.0                                                     # ... and 0, 1 and between inside one group
    alpha[:, hh - 1, 1::3] = 1.0
    zero = np.broadcast_to((alpha == 0)[:, None, None], ends.shape)
    ends = np.where(zero & (rng.random(ends.shape) < 0.3), np.float32("nan"), ends).astype(np.float32)    # NaN keyframes under alpha 0
    return video, ends, alpha


def guarded(shape, value=12345.0):
    n = int(np.prod(shape))
    guard = torch.full((n + 64,), value, device=DEV)
    return guard, guard[32:32 + n].view(shape)


@pytest.mark.parametrize("t,frames", [(2, None), (3, None), (16, None), (16, (5, 7)), (3, (2, 1)), (3, (0, 1))])
def test_still_composite_is_bit_exact(hip, t, frames):
    b, hh, ww = 2, 16, 24
    video, ends, alpha = composite_inputs(b, t, hh, ww, seed=t)
    f0, nf = (0, t) if frames is None else frames
    want = ref.composite(video, ends, alpha, f0, nf)
    assert not np.isnan(want).any() and np.isnan(ends).any()
    zero, one = np.broadcast_to((alpha == 0)[:, None, None], want.shape), (alpha == 1)[:, None]
    assert np.array_equal(want[zero], video[zero])                                  # alpha 0: v's bits
    with np.errstate(invalid="ignore"):
        for j in range(f0, f0 + nf):                                                # alpha 1: key's bits
            key = ends[:, :, 0] + (np.float32(j) / np.float32(t - 1)) * (ends[:, :, 1] - ends[:, :, 0])
            sel = np.broadcast_to(one, key.shape)
            assert np.array_equal(want[:, :, j][sel], key[sel])
    dv, de, da = (torch.from_numpy(v).to(DEV) for v in (video, ends, alpha))
    fresh = hip.still_composite(dv, de, da, frames=frames)                          # out of place: a new tensor
    assert fresh.data_ptr() != dv.data_ptr() and torch.equal(fresh.cpu(), torch.from_numpy(want)) and torch.equal(dv.cpu(), torch.from_numpy(video))
    guard, out = guarded(video.shape)                                               # out of place into sentinel-filled memory
    res = hip.still_composite(dv, de, da, frames=frames, out=out)
    assert res is out
    inside = torch.ones(t, dtype=torch.bool)
    inside[f0:f0 + nf] = False
    assert torch.equal(out[:, :, f0:f0 + nf].cpu(), torch.from_numpy(want[:, :, f0:f0 + nf]))
    assert bool((out[:, :, inside] == 12345.0).all())                               # frames outside the range are not written
    assert bool((guard[:32] == 12345.0).all()) and bool((guard[-32:] == 12345.0).all())
    guard, held = guarded(video.shape)                                              # in place, sentinels around the clip
    held.copy_(dv)
    res = hip.still_composite(held, de, da, frames=frames, out=held)
    assert res is held and torch.equal(held.cpu(), torch.from_numpy(want))
    assert bool((guard[:32] == 12345.0).all()) and bool((guard[-32:] == 12345.0).all())
    assert torch.equal(de.cpu().view(torch.int32), torch.from_numpy(ends).view(torch.int32)) and torch.equal(da.cpu(), torch.from_numpy(alpha))


def test_still_composite_follows_the_map(hip):
    """alpha as tc_still_map gives it, through clip.still_map and output.hold_still"""
    from tooncrafter_amd import clip, output
    ends, tau = case("col_8", 24, 40)
    rng = np.random.default_rng(4)
    ends = np.ascontiguousarray(np.concatenate([ends, case("all_still", 24, 40)[0]]))
    ends[:, :, 1] += (rng.uniform(-0.01, 0.01, ends[:, :, 1].shape)).astype(np.float32)     # below tau: still, but not equal
    video = rng.uniform(-1, 1, (2, 3, 4, 24, 40)).astype(np.float32)
    rule = clip.StillRegions(tau=8, grow=0, feather=1)
    want_map = ref.still_map(ends, 8, 0, 1)
    assert 0 < (want_map[1] == 1).mean() < 1 and (want_map[1][1] == 1).all()
    mask, alpha, dist = clip.still_map(torch.from_numpy(ends).to(DEV), rule)
    assert torch.equal(alpha.cpu(), torch.from_numpy(want_map[1])) and torch.equal(mask.cpu(), torch.from_numpy(want_map[0]))
    dv = torch.from_numpy(video).to(DEV)
    got = output.hold_still(dv, torch.from_numpy(ends).to(DEV), alpha)
    assert torch.equal(got.cpu(), torch.from_numpy(ref.composite(video, ends, want_map[1]))) and torch.equal(dv.cpu(), torch.from_numpy(video))
    again = output.hold_still(dv, torch.from_numpy(ends).to(DEV), alpha, inplace=True)
    assert again.data_ptr() == dv.data_ptr() and torch.equal(dv, got)


def test_still_composite_refuses_an_overlapping_out(hip):
    from tooncrafter_amd import _lib
    b, t, hh, ww = 1, 2, 8, 8
    n = b * 3 * t * hh * ww
    flat = torch.full((6 * n,), 7.0, device=DEV)
    video, ends = flat[:n].view(b, 3, t, hh, ww), flat[2 * n:3 * n].view(b, 3, 2, hh, ww)
    alpha = flat[4 * n:4 * n + hh * ww].view(b, hh, ww)
    for out in (flat[4:n + 4], flat[n - 4:2 * n - 4], flat[n + 64:2 * n + 64], flat[3 * n + 32:4 * n + 32]):
        with pytest.raises(_lib.TooncrafterHipError, match="TC_EINVAL"):            # over video (not exactly), over ends, over alpha
            hip.still_composite(video, ends, alpha, out=out.view(b, 3, t, hh, ww))
    with pytest.raises(_lib.TooncrafterHipError, match="TC_EALIGN"):
        hip.still_composite(video, ends, alpha, out=flat[n + 1:2 * n + 1].view(b, 3, t, hh, ww))
    with pytest.raises(ValueError):
        hip.still_composite(video, ends, alpha, frames=(1, 2))
    torch.cuda.synchronize()
    assert bool((flat == 7.0).all()), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ 3. a captured graph

def test_a_captured_graph_of_both_ops_replays_on_changed_bytes(hip):
    b, t, hh, ww = 2, 3, 24, 40
    ends = torch.zeros(b, 3, 2, hh, ww, device=DEV)
    video = torch.zeros(b, 3, t, hh, ww, device=DEV)
    hip.still_composite(video, ends, hip.still_map(ends, tau=8, grow=1, feather=1)[1])        # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mask, alpha, dist = hip.still_map(ends, tau=8, grow=1, feather=1)
        out = hip.still_composite(video, ends, alpha)
    for seed, name in ((1, "corner_0"), (2, "col_8")):
        he = np.ascontiguousarray(np.concatenate([case(name, hh, ww)[0], case("nan", hh, ww)[0]]))
        hv = np.random.default_rng(seed).uniform(-1, 1, (b, 3, t, hh, ww)).astype(np.float32)
        ends.copy_(torch.from_numpy(he).to(DEV))
        video.copy_(torch.from_numpy(hv).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [v.clone() for v in (mask, alpha, dist, out)]
        eager = hip.still_map(ends, tau=8, grow=1, feather=1)
        eager = (*eager, hip.still_composite(video, ends, eager[1]))
        want = ref.still_map(he, 8, 1, 1)
        for name_, r, e, w in zip(("mask", "alpha", "dist", "out"), replayed, eager, (*want, ref.composite(hv, he, want[1]))):
            assert torch.equal(r.view(torch.uint8), e.view(torch.uint8)), name_     # the same bytes as the eager calls
            assert torch.equal(r.cpu().view(torch.uint8), torch.from_numpy(w).view(torch.uint8)), name_


# ------------------------------------------------------------------------------------------------ 4. the tiny model

@contextlib.contextmanager
def stubbed(model):
    """the tiny model with the stub embedders of the pinned tests and a deterministic encoder posterior"""
    sys.path.insert(0, GOLDEN)
    try:
        import pipeline_stubs as stubs
    finally:
        sys.path.remove(GOLDEN)
    from tooncrafter_amd.lvdm import autoencoder as my_ae
    saved = model.embedder, model.image_proj_model, my_ae.DiagonalGaussianDistribution.sample
    model.embedder, model.image_proj_model = stubs.StubEmbedder(), stubs.StubImageProj(4)
    model.get_learned_conditioning = lambda prompts: stubs.stub_text(prompts, DEV)
    my_ae.DiagonalGaussianDistribution.sample = lambda self, noise=None: self.mean
    try:
        yield
    finally:
        model.embedder, model.image_proj_model, my_ae.DiagonalGaussianDistribution.sample = saved
        del model.get_learned_conditioning


def seeded_videos():
    """(1, 3, 4, 64, 64): the last frame is the first with a 16 x 16 patch redrawn in the top left corner: 2 x 2 of 8 x 8 cells"""
    gen = torch.Generator().manual_seed(91)
    videos = torch.randn(1, 3, 4, 64, 64, generator=gen).clamp(-1, 1)
    videos[:, :, 3] = videos[:, :, 0]
    videos[:, :, 3, :16, :16] = torch.randn(1, 3, 16, 16, generator=gen).clamp(-1, 1)
    return videos.to(DEV)


def seeded_clip(model, **kw):
    """one seeded three-step clip of the tiny model; the keywords of `synthesize` beyond the parent commit's go in `kw`"""
    from tooncrafter_amd import clip as pipeline
    plan = pipeline.SamplingPlan(steps=3, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=[20261021])
    with stubbed(model), torch.no_grad():
        return pipeline.synthesize(model, seeded_videos(), [1, 4, 4, 8, 8], plan=plan, fs=10, **kw)


def clip_sha256(video):
    return hashlib.sha256(video.detach().to(torch.float32).contiguous().cpu().numpy().tobytes()).hexdigest()


def test_tiny_model_holds_the_still_pixels_and_is_the_parents_clip_without_still(model):
    from tooncrafter_amd import clip as pipeline
    rule = pipeline.StillRegions()
    plain = seeded_clip(model)
    none = seeded_clip(model, still=None)
    print("seeded clip sha256:", clip_sha256(plain))
    assert torch.equal(plain, none) and clip_sha256(none) == PARENT_CLIP_SHA256
    held = seeded_clip(model, still=rule)
    assert tuple(held.shape) == (1, 1, 3, 4, 64, 64) and torch.isfinite(held).all()
    videos = seeded_videos()
    ends = torch.stack([videos[:, :, 0], videos[:, :, 3]], dim=2).cpu().numpy()
    _, alpha, dist = ref.still_map(ends, rule.tau, rule.grow, rule.feather)
    full = torch.from_numpy(alpha == 1)[:, None, None].expand(1, 3, 4, 64, 64)
    assert dist[0, :2, :2].max() == 0 and (alpha == 1).sum() == 64 * 64 - 44 * 44 and (alpha == 0).sum() == 28 * 28
    key = ref.composite(np.zeros((1, 3, 4, 64, 64), np.float32), ends, np.ones((1, 64, 64), np.float32))     # alpha 1 everywhere: key
    held, plain = held[:, 0].float().cpu(), plain[:, 0].float().cpu()
    assert torch.equal(held[full], torch.from_numpy(key)[full])                     # every pixel whose alpha is 1 is key, bit for bit
    zero = torch.from_numpy(alpha == 0)[:, None, None].expand(1, 3, 4, 64, 64)
    assert not torch.equal(held[zero], plain[zero])                                 # the pins changed what was sampled
    only = seeded_clip(model, still=pipeline.StillRegions(pin=False))[:, 0].float().cpu()       # composite alone: the parent's pixels at alpha 0
    assert torch.equal(only[zero], plain[zero]) and torch.equal(only[full], torch.from_numpy(key)[full])
