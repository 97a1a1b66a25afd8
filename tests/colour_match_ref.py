"""The colour match (include/tooncrafter_hip.h: tc_colour_stats, tc_colour_match) restated in numpy float64.  Nothing here is
shared with the product; the tests compare the kernels with these functions and these functions with each other.

All statistics are of c = clip(x, -1, 1).  Per frame, nine sums over its n pixels: r, g, b, rr, rg, rb, gg, gb, bb.
m = S1 / n, C = S2 / n - m m^T.  Target of frame f of t: w = f / (t - 1) (0 for t = 1), m_t = (1 - w) m0 + w m1, C_t likewise.
eps = 2^-16 on every diagonal that is inverted or rooted.
  mean_std:  A = diag(sqrt((C_t[k][k] + eps) / (C_s[k][k] + eps)))
  mkl:       S = C_s + eps I, T = C_t + eps I, A = S^-1/2 (S^1/2 T S^1/2)^1/2 S^-1/2; roots by cyclic Jacobi, eight sweeps;
             eigenvalues of S clamped below at eps / 2, of the middle matrix at 0; the middle matrix symmetrised first.
o = m_t - A m_s;  A' = I + s (A - I), o' = s o;  coefs = A' row-major, then o', each rounded to fp32 once.
Apply in fp32: y_k = ((o'_k + A'_k0 r) + A'_k1 g) + A'_k2 b on the clamped inputs, every operation rounded on its own."""
import numpy as np

EPS = 2.0 ** -16
METHODS = {"mean_std": 0, "mkl": 1}
PAIRS = ((0, 1), (0, 2), (1, 2))


def clamp(x):
    return np.clip(x, -1.0, 1.0)


def terms(x):
    """(b, 3, t, h, w) -> the nine per-pixel terms (b, t, 9, h * w) in float64, of the clamped values"""
    c = clamp(np.asarray(x)).astype(np.float64)
    b, _, t, h, w = c.shape
    r, g, bl = (c[:, k].reshape(b, t, h * w) for k in range(3))
    return np.stack([r, g, bl, r * r, r * g, r * bl, g * g, g * bl, bl * bl], axis=2)


def frame_stats(x, f0=0, nf=None, fstep=1):
    """the nine sums of frames f0, f0 + fstep, ... (nf of them; None: all from f0): (b, nf, 9) float64"""
    t = np.asarray(x).shape[2]
    nf = (t - f0 + fstep - 1) // fstep if nf is None else nf
    frames = [f0 + j * (fstep if nf > 1 else 1) for j in range(nf)]
    return terms(x)[:, frames].sum(axis=-1)


def moments(s, n):
    """nine sums over n pixels -> (m (3,), C (3, 3))"""
    s = np.asarray(s, np.float64)
    m = s[:3] / n
    second = np.array([[s[3], s[4], s[5]], [s[4], s[6], s[7]], [s[5], s[7], s[8]]]) / n
    return m, second - np.outer(m, m)


def target(m0, c0, m1, c1, f, t):
    w = f / (t - 1) if t > 1 else 0.0
    return (1.0 - w) * m0 + w * m1, (1.0 - w) * c0 + w * c1


def jacobi(a, sweeps=8):
    """eigenvalues and eigenvectors (columns) of a symmetric 3 x 3: cyclic Jacobi over PAIRS, a fixed number of sweeps"""
    a = np.array(a, np.float64)
    v = np.eye(3)
    for _ in range(sweeps):
        for p, q in PAIRS:
            if a[p, q] == 0.0:
                continue
            with np.errstate(over="ignore"):              # a vanishing a[p][q]: theta = +-inf, the rotation is the identity
                theta = (a[q, q] - a[p, p]) / (2.0 * a[p, q])
                tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(tt * tt + 1.0)
            s = tt * c
            rot = np.eye(3)
            rot[p, p] = rot[q, q] = c
            rot[p, q], rot[q, p] = s, -s
            a = rot.T @ a @ rot
            a = 0.5 * (a + a.T)
            a[p, q] = a[q, p] = 0.0
            v = v @ rot
    return np.diag(a).copy(), v


def mkl_with(eig, cs, ct):
    """the Monge-Kantorovich map with `eig`: a symmetric matrix -> (eigenvalues, eigenvectors in columns)"""
    lam, v = eig(cs + EPS * np.eye(3))
    root = np.sqrt(np.maximum(lam, EPS / 2))
    half, ihalf = (v * root) @ v.T, (v / root) @ v.T
    mid = half @ (ct + EPS * np.eye(3)) @ half
    lam, v = eig(0.5 * (mid + mid.T))
    return ihalf @ ((v * np.sqrt(np.maximum(lam, 0.0))) @ v.T) @ ihalf


def mkl(cs, ct):
    return mkl_with(jacobi, cs, ct)


def mkl_eigh(cs, ct):
    """the same map by LAPACK's eigensolver: the independent statement the Jacobi one is checked against"""
    return mkl_with(np.linalg.eigh, cs, ct)


def mean_std(cs, ct):
    return np.diag(np.sqrt((np.diag(ct) + EPS) / (np.diag(cs) + EPS)))


def frame_map(ms, cs, mt, ct, method, strength):
    """(A', o') of one frame in float64, before the rounding to fp32"""
    a = mkl(cs, ct) if method == "mkl" else mean_std(cs, ct)
    o = mt - a @ ms
    return np.eye(3) + strength * (a - np.eye(3)), strength * o


def coefs(src, ref, n, ref_pixels, method, strength):
    """src (b, t, 9), ref (b, 2, 9) -> (b, t, 12) float64: A' row-major, then o' (not yet rounded to fp32)"""
    b, t, _ = src.shape
    out = np.empty((b, t, 12))
    for i in range(b):
        (m0, c0), (m1, c1) = moments(ref[i, 0], ref_pixels), moments(ref[i, 1], ref_pixels)
        for f in range(t):
            ms, cs = moments(src[i, f], n)
            a, o = frame_map(ms, cs, *target(m0, c0, m1, c1, f, t), method, strength)
            out[i, f, :9], out[i, f, 9:] = a.reshape(9), o
    return out


def apply64(x, co):
    """y = o' + A' clamp(x) in float64 with coefficients co (b, t, 12): the end-to-end reference"""
    c = clamp(np.asarray(x)).astype(np.float64)
    a, o = co[..., :9].reshape(*co.shape[:2], 3, 3), co[..., 9:]
    return np.einsum("btkj,bjthw->bkthw", a, c) + o.transpose(0, 2, 1)[:, :, :, None, None]


def match(video, ends, method, strength):
    """(matched clip in float64, coefficients (b, t, 12) in float64) of `video` (b, 3, t, h, w) against `ends` (b, 3, 2, H, W)"""
    co = coefs(frame_stats(video), frame_stats(ends), video.shape[3] * video.shape[4], ends.shape[3] * ends.shape[4], method, strength)
    return apply64(video, co), co


def plain_moments(y):
    """(m, C) of one frame y (3, h, w) in float64 WITHOUT a clamp: what the match property speaks of"""
    y = np.asarray(y, np.float64).reshape(3, -1)
    m = y.mean(axis=1)
    return m, y @ y.T / y.shape[1] - np.outer(m, m)


# ---------------------------------------------------------------- inputs

def frames(seed, b, t, h, w, spread=(0.25, 0.6)):
    """A seeded (b, 3, t, h, w) fp32 clip whose frames have well-conditioned colour statistics: per frame, three independent
    unit-variance planes (a smooth ramp plus noise) mixed by a random rotation times gains in `spread` and another rotation,
    around a random mean; a few percent of the values leave [-1, 1], so the clamp acts.  cond(C + eps I) stays far below 1e3
    (the tests assert it on what they use)."""
    rng = np.random.default_rng(seed)
    out = np.empty((b, 3, t, h, w), np.float32)
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    for i in range(b):
        for f in range(t):
            base = rng.standard_normal((3, h, w)) * 0.8 + np.stack([yy, xx, yy * xx]) * rng.uniform(0.5, 1.0, (3, 1, 1))
            q1, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            q2, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            mix = q1 @ np.diag(rng.uniform(*spread, 3)) @ q2
            mean = rng.uniform(-0.4, 0.4, 3)
            out[i, :, f] = (np.einsum("kj,jhw->khw", mix, base) + mean[:, None, None]).astype(np.float32)
    return out


def grid_frames(seed, b, t, h, w):
    """A seeded clip on the grid k / 128, k in [-128, 128], with about one value in eight outside [-1, 1] (also multiples of
    1 / 128): every product of two clamped values is a multiple of 2^-14, so the nine sums are exact in any order."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-128, 129, (b, 3, t, h, w))
    far = rng.integers(0, 8, k.shape) == 0
    k = np.where(far, np.sign(k + 0.5) * rng.integers(129, 400, k.shape), k)
    return (k / 128.0).astype(np.float32)


def cond(c):
    lam = np.linalg.eigvalsh(c + EPS * np.eye(3))
    return lam[-1] / lam[0]
