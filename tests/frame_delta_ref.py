"""The rule of tc_frame_deltas (include/tooncrafter_hip.h) in numpy integers, from byte buffers with pitches.  It shares no code
with the kernel or with `ops`: a surface is a flat uint8 array, a plane is (offset, pitch, image stride) in bytes."""
import numpy as np

BINS = 64
FORMATS = ("rgb24", "i420", "nv12", "p010")


def rows(buf, off, n, nrows, row_bytes, pitch, stride):
    """(n, nrows, row_bytes) bytes of a pitched plane of n images"""
    at = off + stride * np.arange(n)[:, None, None] + pitch * np.arange(nrows)[None, :, None] + np.arange(row_bytes)[None, None, :]
    return np.asarray(buf, np.uint8)[at]


def components(buf, fmt, n, h, w, lay):
    """The three components of n images as (n, S_c) arrays of 8-bit values.  lay: byte offsets y / c0 / c1, pitch_y / pitch_c,
    stride_y / stride_c."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt == "rgb24":
        p = rows(buf, lay["y"], n, h, 3 * w, lay["pitch_y"], lay["stride_y"])
        out = [p[:, :, k::3] for k in range(3)]
    elif fmt == "i420":
        out = [rows(buf, lay["y"], n, h, w, lay["pitch_y"], lay["stride_y"]),
               rows(buf, lay["c0"], n, ch, cw, lay["pitch_c"], lay["stride_c"]),
               rows(buf, lay["c1"], n, ch, cw, lay["pitch_c"], lay["stride_c"])]
    elif fmt == "nv12":
        c = rows(buf, lay["c0"], n, ch, 2 * cw, lay["pitch_c"], lay["stride_c"])
        out = [rows(buf, lay["y"], n, h, w, lay["pitch_y"], lay["stride_y"]), c[:, :, 0::2], c[:, :, 1::2]]
    elif fmt == "p010":                                       # little-endian words: the upper byte is the odd one
        c = rows(buf, lay["c0"], n, ch, 4 * cw, lay["pitch_c"], lay["stride_c"])
        out = [rows(buf, lay["y"], n, h, 2 * w, lay["pitch_y"], lay["stride_y"])[:, :, 1::2], c[:, :, 1::4], c[:, :, 3::4]]
    else:
        raise ValueError(fmt)
    return [v.reshape(n, -1) for v in out]


def samples(fmt, h, w):
    c = h * w if fmt == "rgb24" else ((h + 1) // 2) * ((w + 1) // 2)
    return (h * w, c, c)


def deltas(comps, lag, tau):
    """(delta (max(n - lag, 0), 3, 3) int64: sad, changed, hist_l1; hist (n, 3, 64) int32) of `components`' result"""
    n = comps[0].shape[0]
    hist = np.zeros((n, 3, BINS), np.int64)
    for c in range(3):
        for i in range(n):
            hist[i, c] = np.bincount(comps[c][i] >> 2, minlength=BINS)
    delta = np.zeros((max(n - lag, 0), 3, 3), np.int64)
    for p in range(n - lag):
        for c in range(3):
            d = np.abs(comps[c][p].astype(np.int64) - comps[c][p + lag].astype(np.int64))
            delta[p, c] = (d.sum(), (d > tau).sum(), np.abs(hist[p, c] - hist[p + lag, c]).sum())
    return delta, hist.astype(np.int32)


def packed(fmt, n, h, w, base=0, pitch_quantum=1, gap=0):
    """A layout for n images one after the other: planes of an image in order (y, c0, c1), rows padded to a multiple of
    `pitch_quantum` bytes, `gap` unused bytes after every plane (so the chroma planes sit at offsets of their own and an image
    stride is larger than a plane), everything shifted by `base` bytes.  Returns (lay, total bytes)."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    up = lambda v: -(-v // pitch_quantum) * pitch_quantum                                      # noqa: E731
    row_y = {"rgb24": 3 * w, "i420": w, "nv12": w, "p010": 2 * w}[fmt]
    row_c = {"rgb24": 0, "i420": cw, "nv12": 2 * cw, "p010": 4 * cw}[fmt]
    pitch_y, pitch_c = up(row_y), up(row_c)
    stride_y, stride_c = h * pitch_y + gap, ch * pitch_c + gap
    lay = dict(y=base, pitch_y=pitch_y, pitch_c=pitch_c, stride_y=stride_y, stride_c=stride_c)
    end = base + n * stride_y
    if fmt != "rgb24":
        lay["c0"] = end + gap
        end = lay["c0"] + n * stride_c
    if fmt == "i420":
        lay["c1"] = end + gap
        end = lay["c1"] + n * stride_c
    return lay, end + gap
