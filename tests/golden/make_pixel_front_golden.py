#!/usr/bin/env python3
"""Writes tests/golden/pixel_front.npz: what the script's image transform makes of random uint8 images, the expected output
of tc_frames_from_u8 (tests/test_gpu_pixel_front.py) bit for bit.

The transform is the one the reference's `load_data_prompts` composes (scripts/evaluation/inference.py:64-69: Resize(min(size)),
CenterCrop(size), ToTensor, Normalize(0.5, 0.5)), run here through the classes of `tooncrafter_amd.dropin`'s torchvision shim,
i.e. PIL's 8-bit BILINEAR resample and crop and torch's fp32 division: nothing of the reference tree is involved.  Inputs are
seeded.  Run anywhere PIL is installed (CPU):
    python tests/golden/make_pixel_front_golden.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pixel_front.npz")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (name, target (H, W), source (sh, sw)): one way to go wrong each
CASES = [("down_odd_crop", (16, 24), (37, 53)),        # non-integer downscale on both axes, odd crop
         ("up_2tap", (16, 24), (5, 7)),                # upscale: the 2-tap filter, bounds clamped at both ends
         ("crop_only", (16, 24), (16, 40)),            # the shorter side fits already: no resize
         ("half", (16, 24), (32, 48)),                 # exact 2 : 1
         ("portrait_k19", (16, 24), (200, 131)),       # portrait, 19 taps on the long axis
         ("bars_even", (16, 32), (30, 30)),            # the crop is wider than the image: zero bars, even shortfall
         ("half_even_top", (16, 24), (21, 40)),        # top = round(2.5) = 2
         ("one_wide", (16, 24), (64, 1))]              # a source one pixel wide
MULTI = ((16, 24), (37, 53), 3)                        # three images of one size for the pitch / slot case
E2E = ((64, 64), (37, 53), 2)                          # the two keyframes of the end-to-end test (the tiny model's frame size)


def transform(size):
    from tooncrafter_amd import dropin
    dropin._install_torchvision_shim()
    from torchvision import transforms
    return transforms.Compose([transforms.Resize(min(size)), transforms.CenterCrop(size), transforms.ToTensor(),
                               transforms.Normalize(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))]), \
        transforms.Compose([transforms.Resize(min(size)), transforms.CenterCrop(size)])


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    out = {}
    for i, (name, size, src) in enumerate(CASES):
        rng = np.random.default_rng(5200 + i)
        img = rng.integers(0, 256, (*src, 3), dtype=np.uint8)
        out[f"{name}.src"] = img
        out[f"{name}.size"] = np.array(size)
        out[f"{name}.y"] = transform(size)[0](Image.fromarray(img)).numpy()
    size, src, n = MULTI
    imgs = np.random.default_rng(5300).integers(0, 256, (n, *src, 3), dtype=np.uint8)
    out["multi.src"], out["multi.size"] = imgs, np.array(size)
    out["multi.y"] = np.stack([transform(size)[0](Image.fromarray(im)).numpy() for im in imgs])
    # the end-to-end keyframes: only the resized, cropped bytes are stored (the frames are their ToTensor / Normalize, which
    # the test applies with the same torch operations)
    size, src, n = E2E
    imgs = np.random.default_rng(5400).integers(0, 256, (n, *src, 3), dtype=np.uint8)
    out["e2e.src"], out["e2e.size"] = imgs, np.array(size)
    out["e2e.crop_u8"] = np.stack([np.asarray(transform(size)[1](Image.fromarray(im)), dtype=np.uint8) for im in imgs])
    for k, v in out.items():
        if k.endswith(".y"):
            assert v.dtype == np.float32 and v.shape[-3] == 3
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
