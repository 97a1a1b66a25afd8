#!/usr/bin/env python3
"""What the colour match costs on the device, on one (1, 3, 16, 320, 512) fp32 clip (the product shape), for

  stats_clip         tc_colour_stats of all 16 frames (two launches: per-part sums, their sum);
  stats_ends         tc_colour_stats of the two keyframes, a (1, 3, 2, 320, 512) tensor;
  match_mean_std     tc_colour_match, per-channel mean / std (two launches: coefficients, apply), statistics given;
  match_mkl          tc_colour_match, the Monge-Kantorovich map (the 3 x 3 solve in the coefficient launch), statistics given;
  match_colour_mkl   output.match_colour: the three calls together, as `match=` runs them;
  video_to_u8        tc_video_to_u8 of the same clip: the yardstick, the pass every clip already pays on its way out.

HIP events around each call, median of the runs after a warm-up; all in one process.  The clip is random (timing only).  The
streaming passes read 31.5 MB (stats) and read and write 31.5 MB each (apply); the achieved rate is printed next to the time.
No threshold: the passes run once per clip batch.

    python scripts/colour_match_timing.py [--runs 50] [--out profiles/colour_match_timing.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs):
    for _ in range(3):                                           # warm-up: code objects, allocator
        fn()
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
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_match_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd import ops, output
    from tooncrafter_amd.ops import HipOps
    hip = HipOps()
    gen = torch.Generator().manual_seed(23)
    x = (torch.rand(1, 3, 16, 320, 512, generator=gen) * 2.4 - 1.2).to("cuda")
    ends = (torch.rand(1, 3, 2, 320, 512, generator=gen) * 1.6 - 0.8).to("cuda")
    out = torch.empty_like(x)
    src, ref = hip.colour_stats(x), hip.colour_stats(ends)
    pixels = 320 * 512
    prev = ops.set_backend(hip)
    paths = {
        "stats_clip": lambda: hip.colour_stats(x),
        "stats_ends": lambda: hip.colour_stats(ends),
        "match_mean_std": lambda: hip.colour_match(x, src, ref, pixels, "mean_std", 1.0, out=out),
        "match_mkl": lambda: hip.colour_match(x, src, ref, pixels, "mkl", 1.0, out=out),
        "match_colour_mkl": lambda: output.match_colour(x, ends, output.ColourMatch("mkl")),
        "video_to_u8": lambda: hip.video_to_uint8(x),
    }
    clip_bytes = x.numel() * 4
    moved = {"stats_clip": clip_bytes, "match_mean_std": 2 * clip_bytes, "match_mkl": 2 * clip_bytes, "video_to_u8": clip_bytes + clip_bytes // 4}
    res = {"what": "colour match of one (1, 3, 16, 320, 512) fp32 clip to two 320 x 512 keyframes on the device, ms (HIP events)",
           "runs": args.runs}
    try:
        for name, fn in paths.items():
            res[name] = timed(fn, args.runs)
            if name in moved:
                res[name]["gb_per_s"] = moved[name] / res[name]["median_ms"] / 1e6
    finally:
        ops.set_backend(prev)
    res["match_colour_over_video_to_u8"] = res["match_colour_mkl"]["median_ms"] / res["video_to_u8"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
