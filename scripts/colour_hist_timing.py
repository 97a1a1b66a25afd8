#!/usr/bin/env python3
"""What the histogram colour transfer costs on the device, on one (1, 3, 16, 320, 512) fp32 clip (the product shape) against two
320 x 512 keyframes, for

  hist_noise         tc_colour_hist of all 16 frames of a noise clip: lanes of a wave in different bins;
  hist_flat          ... of a flat clip: every lane of every wave in ONE bin (same-address LDS atomics, the one-add path);
  hist_two_tone      ... of a clip with half of every frame one value and half another: waves in one bin, two bins per block;
  hist_ends          tc_colour_hist of the two keyframes;
  transfer           tc_colour_transfer of the noise clip (two launches: 48 tables, the apply pass), histograms given;
  match_colour_hm    output.match_colour with "hm": three calls, as `match=` runs them;
  match_colour_hm_mkl_hm  ... with the compound: nine calls;
  stats_clip         tc_colour_stats of the same clip in the same process: the yardstick, a streaming pass of the same bytes.

HIP events around each call, median of the runs after a warm-up, with the range; all in one process.  The histogram and the
statistics read 31.5 MB, the apply pass reads and writes 31.5 MB each; the achieved rate is printed next to the time.  No
threshold: the passes run once per clip batch, beside a decoder pass of tens of milliseconds.

    python scripts/colour_hist_timing.py [--runs 50] [--out profiles/colour_hist_timing.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_hist_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd import ops, output
    from tooncrafter_amd.ops import HipOps
    hip = HipOps()
    gen = torch.Generator().manual_seed(23)
    noise = (torch.rand(1, 3, 16, 320, 512, generator=gen) * 2.4 - 1.2).to("cuda")
    flat = torch.full_like(noise, 0.3)
    two_tone = flat.clone()
    two_tone[:, :, :, 160:] = -0.61
    ends = (torch.rand(1, 3, 2, 320, 512, generator=gen) * 1.6 - 0.8).to("cuda")
    out = torch.empty_like(noise)
    src, ref = hip.colour_hist(noise), hip.colour_hist(ends)
    pixels = 320 * 512
    assert int(hip.colour_hist(flat).max()) == pixels and int((hip.colour_hist(two_tone) > 0).sum()) == 16 * 3 * 2
    prev = ops.set_backend(hip)
    paths = {
        "hist_noise": lambda: hip.colour_hist(noise),
        "hist_flat": lambda: hip.colour_hist(flat),
        "hist_two_tone": lambda: hip.colour_hist(two_tone),
        "hist_ends": lambda: hip.colour_hist(ends),
        "transfer": lambda: hip.colour_transfer(noise, src, ref, pixels, 1.0, out=out),
        "match_colour_hm": lambda: output.match_colour(noise, ends, output.ColourMatch("hm")),
        "match_colour_hm_mkl_hm": lambda: output.match_colour(noise, ends, output.ColourMatch("hm_mkl_hm")),
        "stats_clip": lambda: hip.colour_stats(noise),
    }
    clip_bytes = noise.numel() * 4
    moved = {"hist_noise": clip_bytes, "hist_flat": clip_bytes, "hist_two_tone": clip_bytes, "transfer": 2 * clip_bytes, "stats_clip": clip_bytes}
    res = {"what": "histogram colour transfer of one (1, 3, 16, 320, 512) fp32 clip to two 320 x 512 keyframes on the device, ms (HIP events)",
           "runs": args.runs}
    try:
        for name, fn in paths.items():
            res[name] = timed(fn, args.runs)
            if name in moved:
                res[name]["gb_per_s"] = moved[name] / res[name]["median_ms"] / 1e6
    finally:
        ops.set_backend(prev)
    res["hist_flat_over_hist_noise"] = res["hist_flat"]["median_ms"] / res["hist_noise"]["median_ms"]
    res["hist_noise_over_stats_clip"] = res["hist_noise"]["median_ms"] / res["stats_clip"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
