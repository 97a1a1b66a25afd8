"""The histogram colour transfer (include/tooncrafter_hip.h: tc_colour_hist, tc_colour_transfer) restated with numpy integers,
float64 and float32.  Nothing here is shared with the product; the tests compare the kernels with these functions and these
functions with each other.

c = clamp(x, -1, 1) in fp32 (a NaN becomes -1);  bin(c) = min(1023, floor((c + 1) * 512)) in fp32.
Histogram of a frame: 3 x 1024 counts.  Transfer of frame f of t, per channel, with s the frame's counts over n pixels and
a, b the two references' over m pixels each:
  P_i = 2 S_i - s_i (S inclusive);  for r in {a, b}: A_j = sum_{i < j} r_i, j the smallest index in [1, 1024] with
  A_j 2n >= P_i m,  q_r = (j - 1) + (P_i m - A_{j-1} 2n) / (r_{j-1} 2n);  w = f / (t - 1) (0 for t = 1),  T = q_a + w (q_b - q_a),
  frame t - 1 of a clip with t > 1: T = q_b;  D[i] = float32((T - (i + 0.5)) / 512) where s_i > 0, else +0.
Apply in fp32, every operation rounded on its own: v = c + D[bin(c)], y = beta + s (v - beta), beta = c or clamp(base)."""
import numpy as np

import colour_match_ref as cm

BINS = 1024
F32 = np.float32


def clamp(x):
    x = np.asarray(x, F32)
    return np.where(np.isnan(x), F32(-1.0), np.minimum(np.maximum(x, F32(-1.0)), F32(1.0))).astype(F32)


def bins(x):
    """bin index of every value of x (any shape), int64"""
    u = (clamp(x) + F32(1.0)).astype(F32)
    v = (u * F32(512.0)).astype(F32)
    return np.minimum(BINS - 1, np.floor(v).astype(np.int64))


def hist(x, f0=0, nf=None, fstep=1):
    """(b, 3, t, h, w) -> the counts of frames f0, f0 + fstep, ... (nf of them; None: all from f0): (b, nf, 3, 1024) int32"""
    x = np.asarray(x)
    b, _, t = x.shape[:3]
    nf = (t - f0 + fstep - 1) // fstep if nf is None else nf
    out = np.empty((b, nf, 3, BINS), np.int32)
    for i in range(b):
        for j in range(nf):
            f = f0 + j * (fstep if nf > 1 else 1)
            for k in range(3):
                out[i, j, k] = np.bincount(bins(x[i, k, f]).reshape(-1), minlength=BINS)
    return out


def ranks(s):
    """midpoint ranks P_i = 2 S_i - s_i of counts s (1024,), int64"""
    s = np.asarray(s, np.int64)
    return 2 * np.cumsum(s) - s


def quantile(s, r, n, m):
    """(q (1024,) float64 in bin units, j (1024,) int64) of the midpoint ranks of source counts s (over n pixels) in the
    reference counts r (over m pixels); entries of unoccupied source bins mean nothing"""
    s, r = np.asarray(s, np.int64), np.asarray(r, np.int64)
    p = ranks(s)
    cum = np.concatenate([[0], np.cumsum(r)])                                   # A_0 .. A_1024
    pm, n2 = p * m, 2 * n
    j = np.clip(np.searchsorted(cum * n2, pm, side="left"), 1, BINS)            # the smallest j with A_j 2n >= P m
    num, den = pm - cum[j - 1] * n2, r[j - 1] * n2
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (j - 1).astype(np.float64) + num.astype(np.float64) / den.astype(np.float64)
    return q, j


def course(qa, qb, f, t):
    if t > 1 and f == t - 1:
        return qb
    w = np.float64(f) / np.float64(t - 1) if t > 1 else np.float64(0.0)
    return qa + w * (qb - qa)


def table(src, ref, n, m):
    """src (b, t, 3, 1024), ref (b, 2, 3, 1024) counts -> (D (b, t, 3, 1024) float32, T float64 of the same shape, NaN where the
    source bin is empty)"""
    b, t = src.shape[:2]
    d, big = np.zeros((b, t, 3, BINS), F32), np.full((b, t, 3, BINS), np.nan)
    centre = np.arange(BINS, dtype=np.float64) + 0.5
    for i in range(b):
        for f in range(t):
            for k in range(3):
                s = src[i, f, k]
                qa, qb = quantile(s, ref[i, 0, k], n, m)[0], quantile(s, ref[i, 1, k], n, m)[0]
                tt = course(qa, qb, f, t)
                on = s > 0
                big[i, f, k, on] = tt[on]
                d[i, f, k, on] = ((tt[on] - centre[on]) / 512.0).astype(F32)
    return d, big


def apply(x, d, strength, base=None):
    """the apply pass in float32: x (b, 3, t, h, w), d (b, t, 3, 1024) -> (b, 3, t, h, w) float32"""
    c = clamp(x)
    s = F32(strength)
    beta = c if base is None else clamp(base)
    lut = np.take_along_axis(d.transpose(0, 2, 1, 3), bins(x).reshape(*c.shape[:3], -1), axis=3).reshape(c.shape)
    v = (c + lut).astype(F32)
    diff = (v - beta).astype(F32)
    return (beta + (s * diff).astype(F32)).astype(F32)


def transfer(x, ends, strength, base=None):
    """one histogram stage: x against the two images of `ends` (b, 3, 2, H, W) -> (float32 clip, D)"""
    d, _ = table(hist(x), hist(ends), x.shape[3] * x.shape[4], ends.shape[3] * ends.shape[4])
    return apply(x, d, strength, base), d


def mkl_bound(co):
    """the per-value bound of the existing MKL end-to-end test, from the stage's float64 coefficients (b, t, 12): (b, 3, t, 1, 1)"""
    b, t = co.shape[:2]
    return (4 * 2.0 ** -22 * (1.0 + np.abs(co[..., :9]).reshape(b, t, 3, 3).sum(axis=-1))).transpose(0, 2, 1)[:, :, :, None, None]


def match(video, ends, method, strength, mkl_shift=0.0):
    """`output.match_colour` for "hm" and "hm_mkl_hm": a dict with `out` (float32), and for the compound `mid` (the MKL stage's
    result rounded to float32), `bound` (mkl_bound of its coefficients).  mkl_shift moves every MKL coefficient by
    mkl_shift * max(1, |coefficient|): what the device's coefficient tolerance allows."""
    if method == "hm":
        return dict(out=transfer(video, ends, strength)[0])
    first = transfer(video, ends, 1.0)[0]
    co = cm.coefs(cm.frame_stats(first), cm.frame_stats(ends), video.shape[3] * video.shape[4], ends.shape[3] * ends.shape[4], "mkl", 1.0)
    mid = cm.apply64(first, co + mkl_shift * np.maximum(1.0, np.abs(co))).astype(F32)
    return dict(out=transfer(mid, ends, strength, base=video)[0], mid=mid, bound=mkl_bound(co))


def touched(mid, margin):
    """Values of the MKL stage's result `mid` (b, 3, t, h, w) whose last-stage displacement can differ when `mid` moves by up to
    `margin` (broadcastable): a value within margin of a bin edge can change bins, which changes the counts, and so the ranks
    and table entries, of exactly the two bins either side of that edge; every value in those two bins is touched.  Boolean,
    of mid's shape."""
    c = clamp(mid).astype(np.float64)
    u = (c + 1.0) * 512.0
    i = bins(mid)
    reach = np.broadcast_to(np.asarray(margin, np.float64) * 512.0, c.shape)
    low, high = (u - i <= reach) & (i > 0), (i + 1 - u <= reach) & (i < BINS - 1)
    out = np.zeros(c.shape, bool)
    b, _, t = c.shape[:3]
    for n in range(b):
        for k in range(3):
            for f in range(t):
                ii = i[n, k, f]
                hit = np.zeros(BINS + 2, bool)
                for edge, side in ((low[n, k, f], -1), (high[n, k, f], 1)):
                    hit[ii[edge] + 1] = True
                    hit[ii[edge] + 1 + side] = True
                out[n, k, f] = hit[ii + 1]
    return out


# ---------------------------------------------------------------- inputs

def toon_frames(seed, b, t, h, w, levels=12):
    """A seeded (b, 3, t, h, w) fp32 clip of toon-like content: per frame and channel a few flat levels under a bent tone curve,
    plus a little noise and a few values outside [-1, 1]; many bins stay empty."""
    rng = np.random.default_rng(seed)
    out = np.empty((b, 3, t, h, w), F32)
    for i in range(b):
        for f in range(t):
            for k in range(3):
                lv = np.sort(rng.uniform(-1.1, 1.1, levels))
                pick = rng.integers(0, levels, (h, w))
                gamma = rng.uniform(0.7, 1.4)
                v = np.sign(lv[pick]) * np.abs(lv[pick]) ** gamma + rng.normal(0.0, 0.01, (h, w))
                out[i, k, f] = v.astype(F32)
    return out


def grid_frames(seed, b, t, h, w, lo=100, hi=800):
    """A seeded clip on the bin centres (2k + 1) / 2048 - 1 with k in [lo, hi): nothing near the ends of the range"""
    rng = np.random.default_rng(seed)
    k = rng.integers(lo, hi, (b, 3, t, h, w))
    return ((2 * k + 1) / 2048.0 - 1.0).astype(F32)


EDGE_VALUES = np.array([-np.inf, -2.0, -1.0, np.nextafter(F32(-1.0), F32(0.0)), np.nextafter(F32(1.0 / 512 - 1), F32(-2.0)), 1.0 / 512 - 1,
                        -0.0, 0.0, np.nextafter(F32(0.0), F32(-1.0)), np.nextafter(F32(1.0), F32(0.0)), 1.0, 2.0, np.inf, np.nan], F32)
EDGE_BINS = np.array([0, 0, 0, 0, 0, 1, 512, 512, 512, 1023, 1023, 1023, 1023, 0])
