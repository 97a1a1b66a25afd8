#!/usr/bin/env python3
"""Writes tests/golden/pixel_back.npz: a small decoded clip and what PIL makes of its uint8 frames, the expected output of
tc_frames_to_u8 (tests/test_gpu_pixel_back.py) bit for bit.

  x            (2, 3, 3, 20, 32) fp32: two clips of three frames -- gradients, hard-edged bars at -1.3 / +1.3 (beyond the clamp,
               so that bicubic and Lanczos overshoot clips at 0 and 255) and a patch of noise
  <filter>.<oh>x<ow>   (2, 3, oh, ow, 3) uint8: PIL.Image.resize of every frame of clamp -> (v + 1) / 2 -> * 255 -> uint8 with
               Image.BICUBIC / LANCZOS / BILINEAR / BOX

Nothing of the reference tree is involved.  The input is seeded.  Run anywhere PIL is installed (CPU):
    python tests/golden/make_pixel_back_golden.py [--out FILE]
"""
import argparse
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pixel_back.npz")

SHAPE = (2, 3, 3, 20, 32)
FILTERS = ("bicubic", "lanczos", "bilinear", "box")
SIZES = [(46, 72),        # non-integer upscale on both axes
         (14, 22),        # downscale: the filter is stretched (fs > 1)
         (20, 50),        # horizontal pass only
         (34, 32)]        # vertical pass only


def clip():
    b, c, t, h, w = SHAPE
    rng = np.random.default_rng(7100)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    x = np.empty(SHAPE, np.float32)
    for i in range(b):
        for f in range(t):
            for ch in range(c):
                ramp = xx * np.float32((ch + 1) / (3.0 * w)) + yy * np.float32((f + 1) / (3.0 * h))          # 0 .. 2
                x[i, ch, f] = ramp * np.float32(1.1) - np.float32(1.1 - 0.05 * i)
            # hard edges beyond the clamp: a bright and a dark bar that move with the frame, one colour channel left out
            x[i, :, f, 3 + f:8 + f, 4 + 3 * i:15 + 3 * i] = 1.3
            x[i, (i + f) % 3, f, 3 + f:8 + f, 4 + 3 * i:15 + 3 * i] = -1.3
            x[i, :, f, 11:18, 20 + f:23 + f] = -1.3
            x[i, :, f, 12:19, 26] = 1.3                                         # a line one pixel wide
            x[i, :, f, 10 + i:16 + i, 2:10] = rng.uniform(-1.2, 1.2, (c, 6, 8)).astype(np.float32)
    return x


def to_u8(x):
    """inference.py:148-153 in fp32: clamp, (v + 1) / 2, * 255, truncation; (b, 3, t, h, w) -> (b, t, h, w, 3)"""
    v = np.clip(x, np.float32(-1), np.float32(1))
    v = ((v + np.float32(1)) / np.float32(2)) * np.float32(255)
    assert v.dtype == np.float32
    return np.ascontiguousarray(v.astype(np.uint8).transpose(0, 2, 3, 4, 1))


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    x = clip()
    assert x.min() < -1 and x.max() > 1
    u8 = to_u8(x)
    out = {"x": x}
    for name in FILTERS:
        flt = getattr(Image, name.upper())
        for oh, ow in SIZES:
            out[f"{name}.{oh}x{ow}"] = np.stack([np.stack([np.asarray(Image.fromarray(fr).resize((ow, oh), flt)) for fr in cl]) for cl in u8])
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
