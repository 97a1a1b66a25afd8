"""A numpy statement of the pixel back end (tc_resize_tables_filter, tc_frames_to_u8; include/tooncrafter_hip.h), written from
the rules alone: it imports nothing from the package.  tests/test_pixel_back_cpu.py checks it against Pillow and the host
table builder against it; tests/test_gpu_pixel_back.py checks the kernels against it and the fixture."""
import math

import numpy as np

FILTERS = ("bilinear", "bicubic", "lanczos", "box")           # TC_RESIZE_* = the index
FORMATS = ("rgb24", "i420", "nv12")                           # TC_PIXFMT_* = the index
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0, "box": 0.5}


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


FILTER_FN = {"bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos, "box": _box}


def tables(filter, n_in, n_out):
    """(bounds [n_out, 2] = (xmin, count), coefs [n_out, kmax]) int32 of one axis n_in -> n_out: Pillow's precompute_coeffs
    and normalize_coeffs_8bpc in Python floats (IEEE doubles): the argument of the filter is a product with 1 / fs, the
    weights are summed in tap order, int() truncates toward zero."""
    fn, scale = FILTER_FN[filter], n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    kmax = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds, coefs = np.zeros((n_out, 2), np.int32), np.zeros((n_out, kmax), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            if total != 0.0:
                v = v / total
            coefs[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx] = (xmin, xmax - xmin)
    return bounds, coefs


def resample_pass(img, n_out, axis, filter):
    """one pass over `axis` of a uint8 array: clip(((1 << 21) + sum k * src) >> 22, 0, 255), the shift arithmetic"""
    bounds, coefs = tables(filter, img.shape[axis], n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.int64)
    for xx, (xmin, cnt) in enumerate(bounds):
        acc = np.tensordot(coefs[xx, :cnt].astype(np.int64), src[xmin:xmin + cnt], axes=1)
        assert np.abs(acc).max(initial=0) < (1 << 31) - (1 << 21)              # the kernel's int32 sum holds it
        out[xx] = np.clip(((1 << 21) + acc) >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize(img, oh, ow, filter):
    """(..., h, w, c) uint8 -> (..., oh, ow, c): horizontal pass, then vertical; a pass whose size does not change is skipped"""
    if img.shape[-2] != ow:
        img = resample_pass(img, ow, img.ndim - 2, filter)
    if img.shape[-3] != oh:
        img = resample_pass(img, oh, img.ndim - 3, filter)
    return img


def to_u8(x):
    """(b, 3, t, h, w) fp32 -> (b, t, h, w, 3) uint8: clamp, (v + 1) / 2, * 255, truncate -- each operation rounded to fp32"""
    v = np.clip(np.asarray(x, np.float32), np.float32(-1), np.float32(1))
    v = (v + np.float32(1)) / np.float32(2)
    v = v * np.float32(255)
    assert v.dtype == np.float32
    return np.ascontiguousarray(v.astype(np.uint8).transpose(0, 2, 3, 4, 1))


def yuv420(rgb):
    """(..., h, w, 3) uint8, h and w even -> Y (..., h, w), Cb, Cr (..., h / 2, w / 2) uint8: BT.601 limited range in integers,
    chroma from the sums over each 2 x 2 block"""
    p = rgb.astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (16829 * r + 33039 * g + 6416 * b + (16 << 16) + (1 << 15)) >> 16
    h, w = r.shape[-2:]
    rs, gs, bs = (c.reshape(*c.shape[:-2], h // 2, 2, w // 2, 2).sum(axis=(-3, -1)) for c in (r, g, b))
    cb = (-9714 * rs - 19070 * gs + 28784 * bs + (128 << 18) + (1 << 17)) >> 18
    cr = (28784 * rs - 24103 * gs - 4681 * bs + (128 << 18) + (1 << 17)) >> 18
    assert min(y.min(initial=0), cb.min(initial=0), cr.min(initial=0)) >= 0     # every shifted quantity is non-negative
    return tuple(np.clip(v, 0, 255).astype(np.uint8) for v in (y, cb, cr))


def frame_bytes(fmt, oh, pitch):
    plane = pitch * oh
    return plane if fmt == "rgb24" else plane + (2 * (pitch // 2) * (oh // 2) if fmt == "i420" else pitch * (oh // 2))


def place(buf, frame, fmt, pitch):
    """write one (oh, ow, 3) uint8 RGB frame into the 1-D uint8 `buf` (a view starting at the frame's first byte) as
    tc_frames_to_u8 lays it out; only the addressed bytes are touched"""
    oh, ow = frame.shape[:2]
    if fmt == "rgb24":
        rows = buf[:pitch * oh].reshape(oh, pitch)
        rows[:, :3 * ow] = frame.reshape(oh, 3 * ow)
        return
    y, cb, cr = yuv420(frame)
    buf[:pitch * oh].reshape(oh, pitch)[:, :ow] = y
    chroma = buf[pitch * oh:]
    if fmt == "i420":
        cp = pitch // 2
        chroma[:cp * (oh // 2)].reshape(oh // 2, cp)[:, :ow // 2] = cb
        chroma[cp * (oh // 2):2 * cp * (oh // 2)].reshape(oh // 2, cp)[:, :ow // 2] = cr
    else:
        rows = chroma[:pitch * (oh // 2)].reshape(oh // 2, pitch)
        rows[:, 0:ow:2] = cb
        rows[:, 1:ow:2] = cr


def packed(frames, fmt):
    """(..., oh, ow, 3) uint8 RGB frames -> what frames_to_u8 returns without `out`: the frames themselves for rgb24,
    (..., oh * ow * 3 / 2) planes otherwise"""
    if fmt == "rgb24":
        return frames
    oh, ow = frames.shape[-3:-1]
    flat = frames.reshape(-1, oh, ow, 3)
    out = np.zeros((len(flat), oh * ow * 3 // 2), np.uint8)
    for i, f in enumerate(flat):
        place(out[i], f, fmt, ow)
    return out.reshape(*frames.shape[:-3], -1)
