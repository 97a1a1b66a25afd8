#!/usr/bin/env python3
"""What a decoder's keyframes cost on the way in: `clip.frames_from_planes` (tc_frames_from_yuv: chroma upsample, integer
YCbCr -> RGB, PIL's 8-bit resample, crop, value) for two 1080 x 1920 surfaces -> frames 0 and 15 of a 320 x 512 x 16 clip tensor,
NV12 and P010, against the host path it replaces: device -> host copy of the planes, the numpy statement of the same conversion
(tests/pixel_yuv_ref.py), PIL's BILINEAR resize and the crop, ToTensor / Normalize in torch, host -> device copy.
HIP events for the device path, the host clock (with synchronisation) for the host path; `--runs` runs of each after one
warm-up.  Both paths give the same bits, which the script checks before it times anything.

    python scripts/pixel_yuv_timing.py [--runs 5] [--out profiles/pixel_yuv_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def half_even(d):
    q = d >> 1
    return q + 1 if (d & 1) and (q & 1) else q


def host_path(planes, fmt, size, t, resized):
    """the same frames by way of the host: copies, numpy, PIL"""
    import pixel_yuv_ref as ref
    from PIL import Image
    (h, w), (rh, rw) = size, resized
    host = (planes.y.cpu().numpy(),) + tuple(c.cpu().numpy() for c in planes.chroma)
    rgb = ref.rgb_image(host, fmt, ref.matrix(planes.standard, planes.range, 10 if fmt == "p010" else 8), planes.siting)
    videos = torch.zeros(1, 3, t, h, w)
    top, left = half_even(rh - h), half_even(rw - w)
    for i, f in enumerate((0, t - 1)):
        img = Image.fromarray(rgb[i]).resize((rw, rh), Image.BILINEAR).crop((left, top, left + w, top + h))
        x = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).to(torch.float32).div(255.0)
        videos[0, :, f] = (x - 0.5) / 0.5
    return videos.to(planes.y.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    import pixel_yuv_ref as ref
    from tooncrafter_amd import clip, ops
    dev, size, t, (sh, sw) = "cuda", (320, 512), 16, (1080, 1920)
    resized = ops.resized_size(sh, sw, *size)
    slots = [(0, 0), (0, t - 1)]
    res = {"what": "two 1080x1920 planar keyframes -> frames 0 and 15 of a 320x512x16f fp32 clip tensor, ms", "runs": args.runs}
    try:
        import PIL  # noqa: F401
        with_host = True
    except ImportError:
        with_host = False
    for fmt in ("nv12", "p010"):
        y, *chroma = (torch.from_numpy(a).to(dev) for a in ref.random_planes(np.random.default_rng(12), 2, sh, sw, fmt))
        planes = clip.Planes(y, tuple(chroma), fmt)
        got = clip.frames_from_planes(planes, size, slots, t)                    # warm-up: code object, tables, allocator
        torch.cuda.synchronize()
        if with_host:
            assert torch.equal(got, host_path(planes, fmt, size, t, resized)), fmt
        ms = {"frames_from_planes": []}
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            clip.frames_from_planes(planes, size, slots, t)
            b.record()
            torch.cuda.synchronize()
            ms["frames_from_planes"].append(a.elapsed_time(b))
        if with_host:
            ms["host: copies + numpy + PIL"] = []
            for _ in range(args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_path(planes, fmt, size, t, resized)
                torch.cuda.synchronize()
                ms["host: copies + numpy + PIL"].append((time.perf_counter() - t0) * 1e3)
        res[fmt] = {k: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
