"""tc_frame_deltas on the MI355X (csrc/frame_delta.hip) against the numpy statement of tests/frame_delta_ref.py, torch.equal
throughout: the four formats at sizes from one sample to several parts per image, pitched and offset surfaces (the 16-byte and
the byte-load path), every n / lag / tau, random and flat content, sentinels round the results and a dirty workspace, a sum
past 2^31, the three layouts of one picture, a captured graph, both bindings, and the timeline that acts on the labels."""
import ctypes

import numpy as np
import pytest
import torch

import frame_delta_ref as ref
from conftest import load_golden
from test_gpu_pixel_front import tiny  # noqa: F401  (the tiny model with a tiny image tower, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODES = {"rgb24": 0, "i420": 1, "nv12": 2, "p010": 3}
# name -> (h, w, pitch quantum, gap after every plane, base offset); P010 doubles an odd base
LAYOUTS = {"one": (1, 1, 1, 0, 0), "tiny": (3, 5, 1, 0, 0), "pitched": (37, 53, 64, 96, 0), "parts": (130, 1030, 1, 0, 0),
           "parts16": (130, 1040, 16, 0, 0), "offset": (37, 53, 64, 96, 1)}


@pytest.fixture(scope="module")
def hip():
    from tooncrafter_amd.ops import HipOps
    return HipOps()


def layout(fmt, name, n):
    h, w, quantum, gap, base = LAYOUTS[name]
    if fmt == "p010":
        base *= 2
    lay, total = ref.packed(fmt, n, h, w, base=base, pitch_quantum=quantum, gap=gap)
    return h, w, lay, total + total % 2                      # an even number of bytes: the buffer is viewed as words for P010


def surfaces(buf, fmt, n, h, w, lay):
    """the device views of a flat uint8 device buffer that the layout describes: (n, h, w, 3) frames or a Planes"""
    from tooncrafter_amd import clip
    if fmt == "rgb24":
        return torch.as_strided(buf, (n, h, w, 3), (lay["stride_y"], lay["pitch_y"], 3, 1), lay["y"])
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt == "p010":
        words = buf.view(torch.uint16)
        y = torch.as_strided(words, (n, h, w), (lay["stride_y"] // 2, lay["pitch_y"] // 2, 1), lay["y"] // 2)
        c = torch.as_strided(words, (n, ch, cw, 2), (lay["stride_c"] // 2, lay["pitch_c"] // 2, 2, 1), lay["c0"] // 2)
        return clip.Planes(y, (c,), "p010")
    y = torch.as_strided(buf, (n, h, w), (lay["stride_y"], lay["pitch_y"], 1), lay["y"])
    if fmt == "nv12":
        return clip.Planes(y, (torch.as_strided(buf, (n, ch, cw, 2), (lay["stride_c"], lay["pitch_c"], 2, 1), lay["c0"]),), "nv12")
    return clip.Planes(y, tuple(torch.as_strided(buf, (n, ch, cw), (lay["stride_c"], lay["pitch_c"], 1), lay[k]) for k in ("c0", "c1")), "i420")


def content(kind, seed, total, n):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, total, dtype=np.uint8)
    if kind == "toon":                                       # long runs of a few values: the merged adds of the histogram
        return np.repeat(rng.choice(np.array([3, 4, 90, 200, 255], np.uint8), total // 97 + 1), 97)[:total].copy()
    return np.full(total, 17 + 40 * (seed % 5), np.uint8)    # flat: every byte of the buffer the same


def check(hip, fmt, name, n, kind, combos, seed=0):
    h, w, lay, total = layout(fmt, name, n)
    host = content(kind, seed, total, n)
    if kind == "flat":                                       # n flat images, each its own value
        for i in range(n):
            for key, stride in (("y", "stride_y"), ("c0", "stride_c"), ("c1", "stride_c")):
                if key in lay:
                    host[lay[key] + i * lay[stride]:lay[key] + (i + 1) * lay[stride]] = (37 * i + 11) % 256
    comps = ref.components(host, fmt, n, h, w, lay)
    x = surfaces(torch.from_numpy(host).to(DEV), fmt, n, h, w, lay)
    for lag, tau in combos:
        want_delta, want_hist = ref.deltas(comps, lag, tau)
        delta, hist = hip.frame_deltas(x, lag=lag, tau=tau)
        assert delta.dtype == torch.int64 and hist.dtype == torch.int32 and delta.is_cuda and hist.is_cuda
        assert delta.shape == (max(n - lag, 0), 3, 3) and hist.shape == (n, 3, 64)
        assert torch.equal(hist.cpu(), torch.from_numpy(want_hist)), (fmt, name, n, lag, tau, kind)
        assert torch.equal(delta.cpu(), torch.from_numpy(want_delta)), (fmt, name, n, lag, tau, kind)


ALL = [(lag, tau) for lag in (1, 2) for tau in (0, 8, 255)]


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_equal_to_the_statement_at_every_n_lag_and_tau(hip, fmt, name):
    for n in (1, 2, 3, 7):
        check(hip, fmt, name, n, "random", ALL, seed=n)


@pytest.mark.parametrize("name", ["tiny", "pitched", "parts", "offset"])
@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_flat_and_toon_images(hip, fmt, name):
    check(hip, fmt, name, 2, "flat", [(1, 0), (1, 8), (1, 255)])
    check(hip, fmt, name, 3, "flat", [(1, 8), (2, 8)])
    check(hip, fmt, name, 3, "toon", [(1, 8), (2, 0)], seed=3)


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_sentinels_round_the_results_and_a_dirty_workspace(hip, fmt):
    """the raw entry point: hist and delta in the middle of sentinel-filled buffers, the workspace full of garbage, twice with
    different garbage"""
    from tooncrafter_amd import _lib
    n, lag, tau = 3, 1, 8
    h, w, lay, total = layout(fmt, "pitched", n)
    host = content("random", 9, total, n)
    buf = torch.from_numpy(host).to(DEV)
    want_delta, want_hist = ref.deltas(ref.components(host, fmt, n, h, w, lay), lag, tau)
    pad = 256
    for round_ in range(2):
        hist = torch.full((pad + n * 3 * 64 + pad,), -77 - round_, dtype=torch.int32, device=DEV)
        delta = torch.full((pad + (n - lag) * 9 + pad,), -99 - round_, dtype=torch.int64, device=DEV)
        p = _lib.TcFrameDeltaParams(y=buf.data_ptr() + lay["y"], c0=buf.data_ptr() + lay["c0"] if "c0" in lay else None,
                                    c1=buf.data_ptr() + lay["c1"] if "c1" in lay else None, image_stride_y=lay["stride_y"],
                                    image_stride_c=lay["stride_c"], pitch_y=lay["pitch_y"], pitch_c=lay["pitch_c"], format=CODES[fmt],
                                    n=n, h=h, w=w, lag=lag, tau=tau, hist=hist.data_ptr() + 4 * pad, delta=delta.data_ptr() + 8 * pad)
        need = hip.lib.tc_frame_deltas_workspace(ctypes.byref(p))
        assert need > 0
        ws = torch.randint(-2 ** 31, 2 ** 31 - 1, (need // 4 + pad,), dtype=torch.int32, device=DEV,
                           generator=torch.Generator(DEV).manual_seed(round_))
        before = ws.clone()
        p.workspace, p.workspace_bytes = ws.data_ptr(), need
        _lib.check(hip.lib.tc_frame_deltas(ctypes.byref(p), torch.cuda.current_stream().cuda_stream), "tc_frame_deltas")
        assert torch.equal(hist[pad:-pad].view(n, 3, 64).cpu(), torch.from_numpy(want_hist))
        assert torch.equal(delta[pad:-pad].view(n - lag, 3, 3).cpu(), torch.from_numpy(want_delta))
        assert (hist[:pad] == -77 - round_).all() and (hist[-pad:] == -77 - round_).all()
        assert (delta[:pad] == -99 - round_).all() and (delta[-pad:] == -99 - round_).all()
        assert torch.equal(ws[need // 4:], before[need // 4:])                    # nothing past the bytes that were asked for


def test_sums_past_two_to_the_31_are_exact(hip):
    """two 2304 x 4096 packed images, all 0 and all 255: sad = 255 * 2304 * 4096 = 2 406 481 920 per component"""
    h, w = 2304, 4096
    x = torch.zeros((2, h, w, 3), dtype=torch.uint8, device=DEV)
    x[1] = 255
    delta, hist = hip.frame_deltas(x, lag=1, tau=8)
    s = h * w
    assert 255 * s > 2 ** 31
    assert delta.cpu().tolist() == [[[255 * s, s, 2 * s]] * 3]
    want = torch.zeros(2, 3, 64, dtype=torch.int32)
    want[0, :, 0], want[1, :, 63] = s, s
    assert torch.equal(hist.cpu(), want)


def test_one_picture_as_i420_nv12_and_p010_gives_equal_tables(hip):
    from tooncrafter_amd import clip
    n, h, w = 3, 37, 53
    ch, cw = (h + 1) // 2, (w + 1) // 2
    rng = np.random.default_rng(12)
    y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))
    both = np.stack([cb, cr], axis=-1)
    dev = lambda *planes: [torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in planes]          # noqa: E731
    tables = []
    for fmt, planes in (("i420", dev(y, cb, cr)), ("nv12", dev(y, both))):
        tables.append(hip.frame_deltas(clip.Planes(planes[0], tuple(planes[1:]), fmt), lag=1, tau=8))
    for noise in (False, True):                              # v << 8, then with anything in the low eight bits
        wide = dev(*((v.astype(np.uint16) << 8) | rng.integers(0, 256 if noise else 1, v.shape).astype(np.uint16) for v in (y, both)))
        tables.append(hip.frame_deltas(clip.Planes(wide[0], (wide[1],), "p010"), lag=1, tau=8))
    assert tables[0][0].any() and tables[0][1].sum() == n * (h * w + 2 * ch * cw)
    for delta, hist in tables[1:]:
        assert torch.equal(delta, tables[0][0]) and torch.equal(hist, tables[0][1])


def test_a_captured_graph_replays_on_changed_bytes(hip):
    n, h, w = 3, 130, 1030
    ch, cw = (h + 1) // 2, (w + 1) // 2
    from tooncrafter_amd import clip
    rng = np.random.default_rng(21)
    y = torch.zeros((n, h, w), dtype=torch.uint8, device=DEV)
    c = torch.zeros((n, ch, cw, 2), dtype=torch.uint8, device=DEV)
    planes = clip.Planes(y, (c,), "nv12")
    hip.frame_deltas(planes, lag=1, tau=8)                                        # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        delta, hist = hip.frame_deltas(planes, lag=1, tau=8)
    for _ in range(2):
        hy, hc = rng.integers(0, 256, (n, h, w), dtype=np.uint8), rng.integers(0, 256, (n, ch, cw, 2), dtype=np.uint8)
        y.copy_(torch.from_numpy(hy).to(DEV))
        c.copy_(torch.from_numpy(hc).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        comps = [hy.reshape(n, -1), hc[..., 0].reshape(n, -1), hc[..., 1].reshape(n, -1)]
        want_delta, want_hist = ref.deltas(comps, 1, 8)
        assert torch.equal(delta.cpu(), torch.from_numpy(want_delta)) and torch.equal(hist.cpu(), torch.from_numpy(want_hist))


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_both_bindings_return_equal_tensors(hip, fmt):
    from tooncrafter_amd import clip, ops
    from tooncrafter_amd.torch_ops import TorchLibOps
    n = 3
    h, w, lay, total = layout(fmt, "pitched", n)
    x = surfaces(torch.from_numpy(content("random", 4, total, n)).to(DEV), fmt, n, h, w, lay)
    a, b = hip.frame_deltas(x, lag=2, tau=3), TorchLibOps().frame_deltas(x, lag=2, tau=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (1, 3, 3)
    prev = ops.set_backend(TorchLibOps())
    try:
        c = clip.frame_deltas(x, lag=2, tau=3)
    finally:
        ops.set_backend(prev)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ------------------------------------------------------------------------------------------------ labels and the timeline

@pytest.fixture(scope="module")
def g():
    return load_golden("pixel_front.npz")


@pytest.fixture(scope="module")
def shot_keyframes(g):
    """Four uint8 keyframes: a dark picture (the fixture's first frame over four), the same moved by a few pixels, an unrelated
    picture (random bytes over the whole range), and that one moved.  By the numpy statement and the default rule the segments
    are ("tween", "cut", "tween"): checked here on the CPU before anything runs on the device."""
    from tooncrafter_amd import clip as pipeline
    dark = g["e2e.src"][0] // 4
    other = np.random.default_rng(7).integers(0, 256, dark.shape, dtype=np.uint8)
    kf = np.stack([dark, np.roll(dark, (3, 5), axis=(0, 1)), other, np.roll(other, (3, 5), axis=(0, 1))])
    n, h, w, _ = kf.shape
    lay, _ = ref.packed("rgb24", n, h, w)
    table, _ = ref.deltas(ref.components(kf.reshape(-1), "rgb24", n, h, w, lay), 1, pipeline.ShotRule().tau)
    want = pipeline.label_shots(table.tolist(), ref.samples("rgb24", h, w))
    assert want.labels == ("tween", "cut", "tween"), want
    return torch.from_numpy(kf).to(DEV), want


def plan_with(seeds):
    from tooncrafter_amd import clip as pipeline
    return pipeline.SamplingPlan(steps=2, eta=1.0, scale=7.5, spacing="uniform_trailing", rescale=0.7, seeds=seeds)


def test_find_shots_labels_the_cut(shot_keyframes):
    from tooncrafter_amd import clip as pipeline
    kf, want = shot_keyframes
    found = pipeline.find_shots(kf)
    assert found == want and found.distinct() == [0, 1, 2, 3]
    still = pipeline.find_shots(torch.cat([kf[:2], kf[1:2], kf[2:]]))              # a keyframe held once
    assert still.labels == ("tween", "hold", "cut", "tween") and still.distinct() == [0, 1, 3, 4]
    assert still.moved[1] == still.mad[1] == still.hist[1] == 0.0


@pytest.mark.parametrize("fmt", ["rgb24", "nv12"])
def test_the_timeline_skips_the_cut_and_samples_the_rest(tiny, shot_keyframes, g, fmt):  # noqa: F811
    from tooncrafter_amd import clip as pipeline
    from tooncrafter_amd import ops
    model, _ = tiny
    kf, _ = shot_keyframes
    h, w = (int(v) for v in g["e2e.size"])
    shape, seeds, t = [1, 4, 4, h // 8, w // 8], [11, 12, 13], 4
    with torch.no_grad():
        video = pipeline.synthesize_timeline_u8(model, kf, shape, size=(h, w), plan=plan_with(seeds), fs=10, out_fmt=fmt,
                                                shots=pipeline.ShotRule())
        by_hand = pipeline.synthesize_timeline_u8(model, kf, shape, size=(h, w), plan=plan_with(seeds), fs=10, out_fmt=fmt,
                                                  shots=pipeline.ShotPlan(("tween", "cut", "tween")))
        parts = {i: pipeline.synthesize_u8(model, kf[i:i + 1], kf[i + 1:i + 2], shape, size=(h, w), plan=plan_with([seeds[i]]), fs=10,
                                           out_fmt=fmt)[0] for i in (0, 2)}
        # the front end followed by the writer, per keyframe
        px = pipeline.frames_from_uint8(kf, (h, w), [(0, i) for i in range(4)], 4)
        still = ops.frames_to_u8(px, fmt=fmt)[0]
    assert video.shape == ((10, h, w, 3) if fmt == "rgb24" else (10, h * w * 3 // 2)) and video.dtype == torch.uint8
    assert torch.equal(video, by_hand)
    assert torch.equal(video[:t], parts[0]) and torch.equal(video[2 * (t - 1) + 1:], parts[2][1:])         # sampled: the calls they replace
    assert torch.equal(video[t], still[1]) and torch.equal(video[t + 1], still[1]) and torch.equal(video[t + 2], still[2])
    assert not torch.equal(still[1], still[2]) and not torch.equal(parts[0][-1], still[1])
