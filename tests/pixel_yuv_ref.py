"""A numpy statement of the planar-YUV front end (tc_yuv_matrix, tc_frames_from_yuv; include/tooncrafter_hip.h), written from
the rules alone: it imports nothing from the package.  Two statements of the colour conversion stand here, the integer one
the kernel must equal bit for bit and an independent one in double (the same standards' matrices, floor(v + 0.5), clipped)
that bounds what the 16-bit fixed point costs.  tests/test_pixel_yuv_cpu.py checks one against the other and the host
matrix builder against the table; tests/test_gpu_pixel_yuv.py checks the kernels against the integer statement."""
import math

import numpy as np

STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}         # (Kr, Kb)
FORMATS = {"i420": 1, "nv12": 2, "p010": 3}                              # TC_PIXFMT_*
SITINGS = ("nearest", "center", "left")                                  # TC_CHROMA_* = the index
# {cy, crv, cgu, cgv, cbu} of the issue's table, computed there from the rule below
TABLE = {
    ("bt601", "limited", 8): (76309, 104597, 25675, 53279, 132201), ("bt601", "limited", 10): (19077, 26149, 6419, 13320, 33050),
    ("bt601", "full", 8): (65536, 91881, 22553, 46802, 116130), ("bt601", "full", 10): (16336, 22903, 5622, 11666, 28947),
    ("bt709", "limited", 8): (76309, 117489, 13975, 34925, 138438), ("bt709", "limited", 10): (19077, 29372, 3494, 8731, 34610),
    ("bt709", "full", 8): (65536, 103206, 12276, 30679, 121609), ("bt709", "full", 10): (16336, 25726, 3060, 7647, 30313),
}


def gains(standard, range_, bits):
    """the five real coefficients (Y gain, Cr -> R, Cb -> G, Cr -> G, Cb -> B) and (yoff, coff), in Python floats"""
    kr, kb = STANDARDS[standard]
    kg = 1.0 - kr - kb
    q = 2 ** (bits - 8)
    if range_ == "limited":
        gy, s, yoff = 255.0 / (219.0 * q), 255.0 / (224.0 * q), 16 * q
    else:
        gy = s = 255.0 / (2 ** bits - 1)
        yoff = 0
    return (gy, 2 * (1 - kr) * s, 2 * kb * (1 - kb) / kg * s, 2 * kr * (1 - kr) / kg * s, 2 * (1 - kb) * s), (yoff, 128 * q)


def matrix(standard, range_, bits):
    """m = [cy, crv, cgu, cgv, cbu, yoff, coff]: floor(v * 65536 + 0.5) of the gains"""
    v, offs = gains(standard, range_, bits)
    return [int(math.floor(x * 65536 + 0.5)) for x in v] + list(offs)


def to_rgb(y, cb, cr, m):
    """integer statement: arrays of samples (any integer dtype, one shape) -> (..., 3) uint8; int64 here, and the assert is the
    header's claim that int32 holds every sum"""
    cy, crv, cgu, cgv, cbu, yoff, coff = (int(v) for v in m)
    c, d, e = y.astype(np.int64) - yoff, cb.astype(np.int64) - coff, cr.astype(np.int64) - coff
    sums = (cy * c + crv * e, cy * c - cgu * d - cgv * e, cy * c + cbu * d)
    assert max(np.abs(s).max(initial=0) for s in sums) < 1 << 27
    return np.stack([np.clip((s + 32768) >> 16, 0, 255) for s in sums], axis=-1).astype(np.uint8)


def to_rgb_double(y, cb, cr, standard, range_, bits):
    """the independent statement: the real matrix in double, floor(v + 0.5), clipped"""
    (gy, rv, gu, gv, bu), (yoff, coff) = gains(standard, range_, bits)
    c, d, e = y.astype(np.float64) - yoff, cb.astype(np.float64) - coff, cr.astype(np.float64) - coff
    vals = (gy * c + rv * e, gy * c - gu * d - gv * e, gy * c + bu * d)
    return np.stack([np.clip(np.floor(v + 0.5), 0, 255) for v in vals], axis=-1).astype(np.uint8)


def upsample(c, sh, sw, siting):
    """(..., ch, cw) chroma samples -> (..., sh, sw) at the source bit depth; indices clamped to the plane, shifts arithmetic"""
    c = c.astype(np.int64)
    ch, cw = c.shape[-2:]
    assert (ch, cw) == ((sh + 1) // 2, (sw + 1) // 2)
    ys, xs = np.arange(sh)[:, None], np.arange(sw)[None, :]
    j, i = ys >> 1, xs >> 1

    def at(jj, ii):
        return c[..., np.clip(jj, 0, ch - 1), np.clip(ii, 0, cw - 1)]
    if siting == "nearest":
        return at(j, i)
    jn = np.where(ys & 1, j + 1, j - 1)
    if siting == "center":
        i2 = np.where(xs & 1, i + 1, i - 1)
        return (9 * at(j, i) + 3 * at(j, i2) + 3 * at(jn, i) + at(jn, i2) + 8) >> 4
    assert siting == "left"
    even = (3 * at(j, i) + at(jn, i) + 2) >> 2
    odd = (3 * at(j, i) + 3 * at(j, i + 1) + at(jn, i) + at(jn, i + 1) + 4) >> 3
    return np.where(xs & 1, odd, even)


def samples(planes, fmt):
    """(y, cb, cr) sample arrays of n images from the stored planes: fmt "i420": (y, cb, cr); "nv12" / "p010": (y, cbcr) with
    cbcr (n, ch, cw, 2); p010 words are read as uint16 and shifted down by six"""
    if fmt == "i420":
        y, cb, cr = planes
        return y, cb, cr
    y, cbcr = planes
    if fmt == "p010":
        y, cbcr = y.view(np.uint16) >> 6, cbcr.view(np.uint16) >> 6
    return y, cbcr[..., 0], cbcr[..., 1]


def rgb_image(planes, fmt, m, siting):
    """the packed RGB image (n, sh, sw, 3) uint8 that tc_frames_from_yuv's result is tc_frames_from_u8 of"""
    y, cb, cr = samples(planes, fmt)
    sh, sw = y.shape[-2:]
    return to_rgb(y, upsample(cb, sh, sw, siting), upsample(cr, sh, sw, siting), m)


def random_planes(rng, n, sh, sw, fmt, low_bits=False):
    """random planes of n (sh, sw) pictures in the storage of `fmt`; p010: 10-bit samples in the upper bits of uint16 words,
    the low six zero or (low_bits) random"""
    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    if fmt == "i420":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, sh, sw), (n, ch, cw), (n, ch, cw)))
    if fmt == "nv12":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, sh, sw), (n, ch, cw, 2)))
    out = []
    for s in ((n, sh, sw), (n, ch, cw, 2)):
        words = rng.integers(0, 1024, s).astype(np.uint16) << 6
        if low_bits:
            words |= rng.integers(0, 64, s).astype(np.uint16)
        out.append(words)
    return tuple(out)
