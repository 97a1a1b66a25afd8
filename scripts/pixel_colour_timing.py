#!/usr/bin/env python3
"""What naming the colour costs on the device: 16 frames of 320 x 512 to 1080 x 1920 planes (bicubic), for

  u8_nv12            tc_frames_to_u8 NV12: BT.601 limited, centre siting, its own kernel -- the path before tc_frames_to_yuv;
  yuv_nv12_601c      tc_frames_to_yuv NV12 with the same matrix and siting (the general kernel on the same work);
  yuv_nv12_709l      tc_frames_to_yuv NV12, BT.709 limited, left siting (six resized pixels per chroma sample);
  yuv_p010_709l      tc_frames_to_yuv P010, BT.709 limited, left siting (16-bit samples, int64 sums).

HIP events around each call (into a preallocated buffer, nothing copied to the host), median of the runs after a warm-up; all
four in one process, so the general kernel is judged against tc_frames_to_u8 in the same run.  The clip is random (timing
only).  No threshold: the kernels run once per clip batch.

    python scripts/pixel_colour_timing.py [--runs 20] [--out profiles/pixel_colour_timing.json]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_colour_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd.ops import HipOps
    from tooncrafter_amd.output import Colour
    hip = HipOps()
    x = (torch.rand(1, 3, 16, 320, 512, generator=torch.Generator().manual_seed(17)) * 2.4 - 1.2).to("cuda")
    oh, ow = 1080, 1920
    frame = oh * ow * 3 // 2
    out8 = torch.empty(16 * frame, dtype=torch.uint8, device="cuda")
    out16 = torch.empty(2 * 16 * frame, dtype=torch.uint8, device="cuda")
    kw = dict(size=(oh, ow), filter="bicubic", fmt="nv12")
    paths = {
        "u8_nv12": lambda: hip.frames_to_u8(x, out=out8, strides=(ow, frame, 16 * frame), **kw),
        "yuv_nv12_601c": lambda: hip.frames_to_yuv(x, colour=Colour("bt601", "limited", "center"), out=out8, strides=(ow, frame, 16 * frame), **kw),
        "yuv_nv12_709l": lambda: hip.frames_to_yuv(x, colour=Colour("bt709", "limited", "left"), out=out8, strides=(ow, frame, 16 * frame), **kw),
        "yuv_p010_709l": lambda: hip.frames_to_yuv(x, colour=Colour("bt709", "limited", "left", 10), out=out16,
                                                   strides=(2 * ow, 2 * frame, 32 * frame), **kw),
    }
    res = {"what": "one (1, 3, 16, 320, 512) fp32 clip -> 16 planar frames of 1080 x 1920 on the device, bicubic, ms (HIP events)",
           "runs": args.runs}
    for name, fn in paths.items():
        res[name] = timed(fn, args.runs)
    res["general_over_u8"] = res["yuv_nv12_601c"]["median_ms"] / res["u8_nv12"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
