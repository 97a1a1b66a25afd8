#!/usr/bin/env python3
"""What conditioning costs beside a clip: `Conditions.build` (fp32 frames in; ATen pad / conv2d / interpolate in front of the
image tower) against `Conditions.from_uint8` (uint8 frames in; tc_frames_from_u8 + tc_clip_patches) on the full-size model
-- ViT-H/14 towers, the 512 Resampler, the first-stage encoder -- at 320 x 512 x 16 frames, from two 720 x 1280 keyframes.
HIP events, 5 runs of each after one warm-up, alternating.  Where PIL imports, the host transform the uint8 path replaces
(device -> host copy, PIL resize + crop, ToTensor / Normalize, host -> device copy) is timed on the host clock as well.
Weights are random (timing only).  `--clip-seconds S` adds each figure's share of a clip of S seconds (bench.py's
ms_per_step / 1000 of the same visit).

    python scripts/pixel_front_timing.py [--clip-seconds 1.9] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def full_model(device):
    import bench
    from tooncrafter_amd.lvdm.condition import FrozenOpenCLIPEmbedder, FrozenOpenCLIPImageEmbedderV2
    from tooncrafter_amd.lvdm.resampler import Resampler
    model = bench.build_model(device)
    model.cond_stage_model = FrozenOpenCLIPEmbedder(layer="penultimate").eval().to(device)
    model.embedder = FrozenOpenCLIPImageEmbedderV2().eval().to(device)
    model.image_proj_model = Resampler(dim=1024, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280,
                                       output_dim=1024, ff_mult=4, video_length=16).eval().to(device)
    return model


def host_transform(first, last, size, t):
    """the script's transform as a caller without the device path runs it on frames it holds on the device"""
    import numpy as np
    from PIL import Image
    from tooncrafter_amd import dropin
    dropin._install_torchvision_shim()
    from torchvision import transforms
    tf = transforms.Compose([transforms.Resize(min(size)), transforms.CenterCrop(size), transforms.ToTensor(),
                             transforms.Normalize(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))])
    videos = torch.zeros(first.shape[0], 3, t, *size)
    for i in range(first.shape[0]):
        videos[i, :, 0] = tf(Image.fromarray(np.asarray(first[i].cpu())))
        videos[i, :, t - 1] = tf(Image.fromarray(np.asarray(last[i].cpu())))
    return videos.to(first.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip-seconds", type=float, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd import clip
    dev, size, t = "cuda", (320, 512), 16
    model = full_model(dev)
    gen = torch.Generator().manual_seed(11)
    first, last = (torch.randint(0, 256, (1, 720, 1280, 3), dtype=torch.uint8, generator=gen).to(dev) for _ in range(2))
    videos = clip.frames_from_uint8(torch.cat([first, last]), size, [(0, 0), (0, t - 1)], t)

    paths = {"Conditions.build": lambda: clip.Conditions.build(model, videos, fs=10),
             "Conditions.from_uint8": lambda: clip.Conditions.from_uint8(model, first, last, size=size, t=t, fs=10)}
    ms = {k: [] for k in paths}
    with torch.no_grad():
        for k, fn in paths.items():                              # warm-up: code objects, packing, allocator
            fn()
        torch.cuda.synchronize()
        for _ in range(args.runs):
            for k, fn in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[k].append(a.elapsed_time(b))
        try:
            import PIL  # noqa: F401
            host_transform(first, last, size, t)
            ms["host PIL transform + copies"] = []
            for _ in range(args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_transform(first, last, size, t)
                torch.cuda.synchronize()
                ms["host PIL transform + copies"].append((time.perf_counter() - t0) * 1e3)
        except ImportError:
            pass
    res = {"what": "conditioning of one 320x512x16f clip from two 720x1280 keyframes, full-size towers, ms",
           "runs": args.runs, "clip_seconds": args.clip_seconds}
    for k, v in ms.items():
        res[k] = {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)}
        if args.clip_seconds:
            res[k]["share_of_clip"] = res[k]["median_ms"] / 1e3 / args.clip_seconds
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
