"""A numpy statement of planar frames out in a named colour (tc_yuv_out_matrix, tc_frames_to_yuv; include/tooncrafter_hip.h),
written from the rules alone: it imports nothing from the package.  The resize tables and the 8-bit value / resample steps are
tests/pixel_back_ref.py's; what stands here is the forward matrix, the 16-bit value and resample of the P010 path, the colour
step with both sitings and the layout.  All integer work is int64; the asserts are the header's claims about what the
kernel's narrower sums hold.  An independent float64 statement of the standards bounds what the fixed point costs.
tests/test_pixel_colour_cpu.py checks the host code against this file, tests/test_gpu_pixel_colour.py the kernels."""
import math

import numpy as np

import pixel_back_ref as back

STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}         # (Kr, Kb)
FORMATS = {"i420": 1, "nv12": 2, "p010": 3}                              # TC_PIXFMT_*
SITINGS = {"center": 1, "left": 2}                                       # TC_CHROMA_*
# the issue's check points: (standard, range, bits) -> m
TABLE = {
    ("bt601", "limited", 8): [16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 16, 128],
    ("bt709", "limited", 8): [11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639, 16, 128],
    ("bt601", "full", 8): [19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329, 0, 128],
    ("bt709", "limited", 10): [47678, 160389, 16192, -26280, -88410, 114690, 114690, -104174, -10516, 64, 512],
}


def depth(bits):
    """(bits of the RGB samples, F, top code) of an output depth"""
    bits_in = 8 if bits == 8 else 16
    return bits_in, 8 + bits_in, (1 << bits) - 1


def gains(range_, bits):
    """(gy, gc, yoff, coff): code values per unit of an RGB SAMPLE, and the offsets"""
    bits_in, _, top = depth(bits)
    inmax, q = (1 << bits_in) - 1, 1 << (bits - 8)
    if range_ == "limited":
        return 219 * q / inmax, 224 * q / inmax, 16 * q, 128 * q
    return top / inmax, top / inmax, 0, 128 * q


def out_matrix(standard, range_, bits):
    """m = [yr, yg, yb, ur, ug, ub, vr, vg, vb, yoff, coff] by the header's rule, in Python floats (IEEE doubles)"""
    kr, kb = STANDARDS[standard]
    gy, gc, yoff, coff = gains(range_, bits)
    one = float(1 << depth(bits)[1])

    def r(v):
        return int(math.floor(v * one + 0.5))
    yr, yb = r(kr * gy), r(kb * gy)
    yg = r(gy) - yr - yb
    ub = vr = r(gc / 2)
    ur = r(-kr / (2 * (1 - kb)) * gc)
    vb = r(-kb / (2 * (1 - kr)) * gc)
    return [yr, yg, yb, ur, -(ub + ur), ub, vr, -(vr + vb), vb, yoff, coff]


def codes_double(rgb, standard, range_, bits):
    """the independent statement: (..., 3) RGB samples -> real-valued (Y, Cb, Cr) code values of one pixel, in float64, from
    the standards' own formulas (Y' = Kr R' + Kg G' + Kb B', Pb = (B' - Y') / (2 (1 - Kb)), Pr likewise); not rounded"""
    kr, kb = STANDARDS[standard]
    bits_in, _, top = depth(bits)
    p = rgb.astype(np.float64) / ((1 << bits_in) - 1)
    yp = kr * p[..., 0] + (1 - kr - kb) * p[..., 1] + kb * p[..., 2]
    pb, pr = (p[..., 2] - yp) / (2 * (1 - kb)), (p[..., 0] - yp) / (2 * (1 - kr))
    q = 1 << (bits - 8)
    sy, sc, yoff = (219 * q, 224 * q, 16 * q) if range_ == "limited" else (top, top, 0)
    return yoff + sy * yp, 128 * q + sc * pb, 128 * q + sc * pr


def to_u16(x):
    """(b, 3, t, h, w) fp32 -> (b, t, h, w, 3) uint16: clamp, (v + 1) / 2, * 65535, floor(s + 0.5) -- each operation rounded to
    fp32"""
    v = np.clip(np.asarray(x, np.float32), np.float32(-1), np.float32(1))
    v = (v + np.float32(1)) / np.float32(2)
    v = v * np.float32(65535)
    v = np.floor(v + np.float32(0.5))
    assert v.dtype == np.float32
    return np.ascontiguousarray(v.astype(np.uint16).transpose(0, 2, 3, 4, 1))


def resample_pass16(img, n_out, axis, filter):
    """one pass over `axis` of a uint16 array with the 8-bit tables: clip(((1 << 21) + sum k * src) >> 22, 0, 65535) in int64"""
    bounds, coefs = back.tables(filter, img.shape[axis], n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.int64)
    for xx, (xmin, cnt) in enumerate(bounds):
        acc = np.tensordot(coefs[xx, :cnt].astype(np.int64), src[xmin:xmin + cnt], axes=1)
        out[xx] = np.clip(((1 << 21) + acc) >> 22, 0, 65535)
    return np.moveaxis(out, 0, axis).astype(np.uint16)


def resize16(img, oh, ow, filter):
    """(..., h, w, c) uint16 -> (..., oh, ow, c): horizontal pass, then vertical; a pass whose size does not change is skipped"""
    if img.shape[-2] != ow:
        img = resample_pass16(img, ow, img.ndim - 2, filter)
    if img.shape[-3] != oh:
        img = resample_pass16(img, oh, img.ndim - 3, filter)
    return img


def rgb_frames(x, size, filter, bits):
    """the resized RGB frames (b, t, oh, ow, 3) the colour step reads: uint8 for 8-bit output, uint16 for P010"""
    img = back.to_u8(x) if bits == 8 else to_u16(x)
    if size is None:
        return img
    return back.resize(img, size[0], size[1], filter) if bits == 8 else resize16(img, size[0], size[1], filter)


def yuv420(rgb, m, siting, bits):
    """(..., h, w, 3) RGB samples (uint8 for bits 8, uint16 for bits 10), h and w even -> codes Y (..., h, w), Cb, Cr
    (..., h / 2, w / 2) as int64 by the matrix m; siting "center": 2 x 2 sums, shift F + 2; "left": columns 2 bx - 1 (clamped to
    0), 2 bx, 2 bx + 1 of both rows weighted 1 2 1, shift F + 3"""
    _, F, top = depth(bits)
    m = [int(v) for v in m]
    p = rgb.astype(np.int64)
    h, w = p.shape[-3:-1]
    assert h % 2 == 0 and w % 2 == 0
    y = (m[0] * p[..., 0] + m[1] * p[..., 1] + m[2] * p[..., 2] + (m[9] << F) + (1 << (F - 1))) >> F
    rows = p[..., 0::2, :, :] + p[..., 1::2, :, :]                                # both rows of a block row: (..., h / 2, w, 3)
    if siting == "center":
        sums, s = rows[..., 0::2, :] + rows[..., 1::2, :], 2
    else:
        assert siting == "left"
        x0 = np.arange(0, w, 2)
        sums, s = rows[..., np.maximum(x0 - 1, 0), :] + 2 * rows[..., x0, :] + rows[..., x0 + 1, :], 3
    shift = F + s
    chroma = []
    for k in (m[3:6], m[6:9]):
        raw = k[0] * sums[..., 0] + k[1] * sums[..., 1] + k[2] * sums[..., 2] + (m[10] << shift) + (1 << (shift - 1))
        if bits == 8:
            assert np.abs(raw).max(initial=0) <= 1 << 27                          # the kernel's int32 sum holds it
        chroma.append(np.clip(raw >> shift, 0, top))
    return np.clip(y, 0, top), chroma[0], chroma[1]


def frame_bytes(fmt, oh, pitch):
    """bytes of one frame with rows `pitch` bytes apart; "p010" is NV12's rule with its own pitch"""
    return back.frame_bytes("nv12" if fmt == "p010" else fmt, oh, pitch)


def place(buf, frame, fmt, pitch, m, siting):
    """write one (oh, ow, 3) RGB frame into the 1-D uint8 `buf` (a view starting at the frame's first byte) as tc_frames_to_yuv
    lays it out, `pitch` in bytes; fmt "p010": little-endian words of code << 6; only the addressed bytes are touched"""
    oh, ow = frame.shape[:2]
    wide = fmt == "p010"
    y, cb, cr = yuv420(frame, m, siting, 10 if wide else 8)
    if wide:
        def store(rows, vals):                                                    # rows: (n, pitch) bytes; vals: (n, k) codes
            words = (vals.astype(np.uint16) << 6)
            rows[:, 0:2 * vals.shape[1]:2] = (words & 0xFF).astype(np.uint8)
            rows[:, 1:2 * vals.shape[1]:2] = (words >> 8).astype(np.uint8)
        store(buf[:pitch * oh].reshape(oh, pitch), y)
        store(buf[pitch * oh:pitch * oh + pitch * (oh // 2)].reshape(oh // 2, pitch), np.stack([cb, cr], axis=-1).reshape(oh // 2, ow))
        return
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


def packed(frames, fmt, m, siting):
    """(..., oh, ow, 3) RGB frames -> what frames_to_yuv returns without `out`: (..., oh * ow * 3 / 2) bytes, twice that for
    "p010" """
    oh, ow = frames.shape[-3:-1]
    flat = frames.reshape(-1, oh, ow, 3)
    es = 2 if fmt == "p010" else 1
    out = np.zeros((len(flat), oh * ow * 3 // 2 * es), np.uint8)
    for i, f in enumerate(flat):
        place(out[i], f, fmt, ow * es, m, siting)
    return out.reshape(*frames.shape[:-3], -1)
