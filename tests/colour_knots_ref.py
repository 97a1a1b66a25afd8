"""The course through knots and the gain limit (include/tooncrafter_hip.h: tc_colour_match_knots, tc_colour_transfer_knots)
restated in numpy float64 and numpy integers, on top of tests/colour_match_ref.py and tests/colour_hist_ref.py.  Nothing here is
shared with the product.

Knots: nk reference images at strictly increasing frame indices k_0 < ... < k_{nk-1} in [0, t).  Course of frame f: f <= k_0 takes
knot 0 itself, f >= k_{nk-1} the last knot itself; otherwise j is the last knot with k_j <= f and w = (f - k_j) / (k_{j+1} - k_j);
a frame on a knot takes that knot itself.  Linear methods: m_t = (1 - w) m_j + w m_{j+1}, C_t likewise.  Histogram transfer:
T = q_j + w (q_{j+1} - q_j).
Gain limit g (0: none; else >= 1), on A before o and before the strength: mean_std clamps the diagonal to [1 / g, g]; mkl
symmetrises A, decomposes it by the same Jacobi, clamps the eigenvalues to [1 / g, g] and rebuilds V diag V^T, always."""
import numpy as np

import colour_hist_ref as ch
import colour_match_ref as cm

F32 = np.float32


def course(knots, f):
    """(j, single, w) of frame f: `single` -- the target is knot j itself (w = 0); otherwise between knots j and j + 1 at w"""
    j = 0
    for i in range(1, len(knots)):
        if knots[i] <= f:
            j = i
    single = f <= knots[j] or j == len(knots) - 1
    w = 0.0 if single else np.float64(f - knots[j]) / np.float64(knots[j + 1] - knots[j])
    return j, single, w


def target(moments, knots, f):
    """(m_t, C_t) of frame f from the knots' [(m, C), ...]"""
    j, single, w = course(knots, f)
    if single:
        return moments[j]
    (m0, c0), (m1, c1) = moments[j], moments[j + 1]
    return (1.0 - w) * m0 + w * m1, (1.0 - w) * c0 + w * c1


def limit(a, method, g, eig=cm.jacobi):
    """A held inside the gain limit g (0: as it is)"""
    if not g:
        return a
    lo = 1.0 / g
    if method == "mkl":
        lam, v = eig(0.5 * (a + a.T))
        return (v * np.clip(lam, lo, g)) @ v.T
    return np.diag(np.clip(np.diag(a), lo, g))


def frame_map(ms, cs, mt, ct, method, strength, max_gain=0.0, eig=cm.jacobi):
    """(A', o', A) of one frame in float64, before the rounding to fp32; A is the limited map at strength 1"""
    a = cm.mkl_with(eig, cs, ct) if method == "mkl" else cm.mean_std(cs, ct)
    a = limit(a, method, max_gain, eig)
    o = mt - a @ ms
    return np.eye(3) + strength * (a - np.eye(3)), strength * o, a


def coefs(src, ref, knots, n, ref_pixels, method, strength, max_gain=0.0, eig=cm.jacobi):
    """src (b, t, 9), ref (b, nk, 9) -> (b, t, 12) float64: A' row-major, then o' (not yet rounded to fp32)"""
    b, t, _ = src.shape
    assert ref.shape[1] == len(knots)
    out = np.empty((b, t, 12))
    for i in range(b):
        moments = [cm.moments(ref[i, k], ref_pixels) for k in range(len(knots))]
        for f in range(t):
            ms, cs = cm.moments(src[i, f], n)
            a, o, _ = frame_map(ms, cs, *target(moments, knots, f), method, strength, max_gain, eig)
            out[i, f, :9], out[i, f, 9:] = a.reshape(9), o
    return out


def unlimited_gain(src, ref, knots, n, ref_pixels, method):
    """the largest eigenvalue of the symmetrised unlimited map of every frame: (b, t)"""
    co = coefs(src, ref, knots, n, ref_pixels, method, 1.0)[..., :9].reshape(*src.shape[:2], 3, 3)
    return np.linalg.eigvalsh(0.5 * (co + co.transpose(0, 1, 3, 2)))[..., -1]


def table(src, ref, knots, n, m):
    """src (b, t, 3, 1024), ref (b, nk, 3, 1024) counts -> (D (b, t, 3, 1024) float32, T float64 of the same shape, NaN where the
    source bin is empty)"""
    b, t = src.shape[:2]
    assert ref.shape[1] == len(knots)
    d, big = np.zeros((b, t, 3, ch.BINS), F32), np.full((b, t, 3, ch.BINS), np.nan)
    centre = np.arange(ch.BINS, dtype=np.float64) + 0.5
    for i in range(b):
        for f in range(t):
            j, single, w = course(knots, f)
            for k in range(3):
                s = src[i, f, k]
                tt = ch.quantile(s, ref[i, j, k], n, m)[0]
                if not single:
                    qb = ch.quantile(s, ref[i, j + 1, k], n, m)[0]
                    tt = tt + w * (qb - tt)
                on = s > 0
                big[i, f, k, on] = tt[on]
                d[i, f, k, on] = ((tt[on] - centre[on]) / 512.0).astype(F32)
    return d, big


def match(video, refs, knots, method, strength, max_gain=0.0):
    """the linear match of `video` (b, 3, t, h, w) against `refs` (b, 3, nk, H, W) at `knots`: (float64 clip, coefficients)"""
    co = coefs(cm.frame_stats(video), cm.frame_stats(refs), knots, video.shape[3] * video.shape[4], refs.shape[3] * refs.shape[4],
               method, strength, max_gain)
    return cm.apply64(video, co), co


def transfer(x, refs, knots, strength, base=None):
    """one histogram stage: x against the images of `refs` (b, 3, nk, H, W) at `knots` -> (float32 clip, D)"""
    d, _ = table(ch.hist(x), ch.hist(refs), knots, x.shape[3] * x.shape[4], refs.shape[3] * refs.shape[4])
    return ch.apply(x, d, strength, base), d


def compound(video, refs, knots, strength, max_gain=0.0):
    """"hm_mkl_hm" through the knots: (float32 clip, the MKL stage's result rounded to float32)"""
    first = transfer(video, refs, knots, 1.0)[0]
    mid = match(first, refs, knots, "mkl", 1.0, max_gain)[0].astype(F32)
    return transfer(mid, refs, knots, strength, base=video)[0], mid


def stack_targets(ends, t, inner):
    """`output.match_colour`'s targets: (knots, images (b, 3, nk, H, W)) from the endpoints (b, 3, 2, H, W) and {index: image}"""
    images = {0: ends[:, :, 0]}
    if t > 1:
        images[t - 1] = ends[:, :, 1]
    images.update(inner or {})
    knots = tuple(sorted(images))
    return knots, np.stack([images[k] for k in knots], axis=2)


# ---------------------------------------------------------------- inputs

KNOT_SETS = {1: [(0,)], 5: [(0, 4), (0, 2, 4), (1, 3), (2,)], 6: [(0, 5), (0, 2, 5), (1, 4), (3,)], 64: [tuple(range(64))]}
SHAPES = [(2, 5, 7, 9), (2, 6, 24, 40), (1, 1, 8, 8), (1, 64, 8, 8)]
IDS = ["2x5x7x9", "2x6x24x40", "1x1x8x8", "1x64x8x8"]
REF_HW = (17, 23)


def flat_frames(seed, b, t, h, w, spread=(0.002, 0.005)):
    """cm.frames with a spread of a few thousandths: near-flat frames (a fade, a held background), whose unlimited gains against
    references of spread 0.25 .. 0.6 run to tens"""
    return cm.frames(seed, b, t, h, w, spread=spread)


def inputs(shape, kind):
    """(clip (b, 3, t, h, w), reference images (b, 3, nmax, 17, 23)) of a shape, seeded by it; a knot set of nk knots uses the first
    nk reference images.  kind: "random" (cm.frames), "flat" (a near-flat clip against cm.frames references: the gain-limit
    case), "steep" (the reverse: gains far below 1), "toon" (ch.toon_frames), "grid" (ch.grid_frames)"""
    b, t, h, w = shape
    nmax, seed = max(len(k) for k in KNOT_SETS[t]), sum(shape)
    if kind in ("toon", "grid"):
        make = ch.toon_frames if kind == "toon" else ch.grid_frames
        return make(seed, b, t, h, w), make(seed + 1, b, nmax, *REF_HW)
    clip = (flat_frames if kind == "flat" else cm.frames)(seed, b, t, h, w)
    return clip, (flat_frames if kind == "steep" else cm.frames)(seed + 1, b, nmax, *REF_HW)
