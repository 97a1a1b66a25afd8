#!/usr/bin/env python3
"""What the output edge costs for one decoded (1, 3, 16, 320, 512) clip, to yuv420p planes on the host, at the model's size and
at 640 x 1024 (bicubic):

  new    tc_frames_to_u8 to I420 on the device (value, PIL's 8-bit resample, integer BT.601), then the copy to the host;
  today  tc_video_to_u8, the copy to the host, PIL.Image.resize of every frame, mp4.rgb_to_yuv420 of every frame.

HIP events around each path (the host work of `today` lies between the two records), median of 20 runs after a warm-up, and the
bytes each path copies from the device.  The clip is random (timing only).  No threshold: the kernels run once per clip.

    python scripts/pixel_back_timing.py [--runs 20] [--out profiles/pixel_back_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs):
    fn()                                                         # warm-up: code objects, tables, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": sorted(ms)[len(ms) // 2], "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_back_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd import mp4
    from tooncrafter_amd.ops import HipOps
    hip = HipOps()
    x = (torch.rand(1, 3, 16, 320, 512, generator=torch.Generator().manual_seed(17)) * 2.4 - 1.2).to("cuda")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    res = {"what": "one (1, 3, 16, 320, 512) fp32 clip -> yuv420p planes on the host, ms (HIP events, host work included)",
           "runs": args.runs}
    for oh, ow in ((320, 512), (640, 1024)):
        size = None if (oh, ow) == (320, 512) else (oh, ow)

        def new():
            return hip.frames_to_u8(x, size=size, filter="bicubic", fmt="i420").cpu()

        def today():
            frames = hip.video_to_uint8(x).cpu().numpy()[0]
            if size is not None:
                frames = [np.asarray(Image.fromarray(f).resize((ow, oh), Image.BICUBIC)) for f in frames]
            return [mp4.rgb_to_yuv420(f) for f in frames]
        entry = {"new_i420": timed(new, args.runs), "new_bytes_copied": 16 * oh * ow * 3 // 2,
                 "today_bytes_copied": 16 * 320 * 512 * 3}
        entry["today_rgb_host_pil_yuv"] = timed(today, args.runs) if size is None or Image is not None else None
        res[f"{oh}x{ow}"] = entry
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
