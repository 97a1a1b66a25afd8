"""The rule of tc_still_map and tc_still_composite (include/tooncrafter_hip.h) in numpy.  It shares no code with the kernels:
the distance is taken by repeated 3 x 3 dilation, the upsampling from per-axis index and weight tables.  tests/test_still_cpu.py
checks this statement against a brute-force definition (exhaustive search over cells, the upsampling in Fractions)."""
import numpy as np

CELL = 8
MAX_DIST = 32


def clamp(v):
    """to [-1, 1]; a NaN stays a NaN"""
    v = np.asarray(v, dtype=np.float32)
    return np.where(v < np.float32(-1), np.float32(-1), np.where(v > np.float32(1), np.float32(1), v)).astype(np.float32)


def moved_cells(ends, tau):
    """(b, h, w) bool of (b, 3, 2, H, W) fp32 keyframes: a cell has moved if any pixel of it has in any channel"""
    ends = np.asarray(ends, dtype=np.float32)
    b, c, two, hh, ww = ends.shape
    assert (c, two) == (3, 2) and hh % CELL == 0 and ww % CELL == 0
    thr = np.float32(tau) / np.float32(127.5)
    with np.errstate(invalid="ignore"):
        diff = np.abs(clamp(ends[:, :, 0]) - clamp(ends[:, :, 1]))              # fp32, the subtraction rounded on its own
        pixel = ~(diff <= thr)                                                   # a NaN fails the comparison: moved
    return pixel.any(axis=1).reshape(b, hh // CELL, CELL, ww // CELL, CELL).any(axis=(2, 4))


def distance(moved, cap):
    """min(cap, Chebyshev distance in cells to the nearest moved cell of the same clip), (b, h, w) uint8: the ball of radius k is
    the map dilated k times by a 3 x 3 square, nothing moved outside the image"""
    reach = np.asarray(moved, dtype=bool)
    d = np.zeros(reach.shape, dtype=np.int64)
    for _ in range(cap):
        d += ~reach
        p = np.pad(reach, ((0, 0), (1, 1), (1, 1)))
        h, w = reach.shape[1:]
        reach = np.any([p[:, i:i + h, j:j + w] for i in range(3) for j in range(3)], axis=0)
    return d.astype(np.uint8)


def taps(n):
    """per pixel of an axis of n cells: the two cells and their weights in sixteenths (centres at 8 i + 3.5, edges replicated)"""
    p = np.arange(n * CELL)
    i, r = p // CELL, p % CELL
    low = r < 4
    i0 = np.where(low, np.maximum(i - 1, 0), i)
    i1 = np.where(low, i, np.minimum(i + 1, n - 1))
    w1 = np.where(low, 2 * r + 9, 2 * r - 7)
    return i0, i1, 16 - w1, w1


def upsample_n(a):
    """(b, h, w) integer cell weights -> (b, 8 h, 8 w) exact integers in units of 1 / 256"""
    a = np.asarray(a, dtype=np.int64)
    y0, y1, wy0, wy1 = taps(a.shape[1])
    x0, x1, wx0, wx1 = taps(a.shape[2])
    rows = wy0[None, :, None] * a[:, y0, :] + wy1[None, :, None] * a[:, y1, :]
    return wx0[None, None, :] * rows[:, :, x0] + wx1[None, None, :] * rows[:, :, x1]


def still_map(ends, tau, grow, feather):
    """(mask (b, 1, 1, h, w) fp32, alpha (b, H, W) fp32, dist (b, h, w) uint8)"""
    cap = grow + feather + 1
    assert 0 <= tau <= 255 and grow >= 0 and feather >= 1 and cap <= MAX_DIST
    d = distance(moved_cells(ends, tau), cap)
    mask = (d > grow).astype(np.float32)[:, None, None]
    a = np.clip(d.astype(np.int64) - grow - 1, 0, feather)
    alpha = upsample_n(a).astype(np.float32) / np.float32(256 * feather)
    return np.ascontiguousarray(mask), np.ascontiguousarray(alpha, dtype=np.float32), np.ascontiguousarray(d)


def composite(video, ends, alpha, f0=0, nf=None):
    """out (b, 3, t, H, W) fp32: frames f0 .. f0 + nf - 1 of `video` held to the keyframes by alpha, the others as they are.  Every
    operation is one numpy call on fp32 arrays: rounded on its own."""
    video, ends, alpha = (np.asarray(v, dtype=np.float32) for v in (video, ends, alpha))
    t = video.shape[2]
    nf = t - f0 if nf is None else nf
    out = video.copy()
    e0, e1, a = ends[:, :, 0], ends[:, :, 1], alpha[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        span = e1 - e0
        for j in range(f0, f0 + nf):
            s = np.float32(j) / np.float32(t - 1)
            key = e0 + s * span
            v = video[:, :, j]
            out[:, :, j] = np.where(a == 0, v, np.where(a == 1, key, v + a * (key - v)))
    return out
