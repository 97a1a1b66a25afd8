#!/usr/bin/env python3
"""What targets at inner frames and the gain limit cost on the device, on one (1, 3, 16, 320, 512) fp32 clip (the product
shape) against 320 x 512 keyframes: `output.match_colour` for every method

  <method>_ends          the two endpoints, no limit: the old entry points (tc_colour_match / tc_colour_transfer);
  <method>_2knots        the same two targets through the knots calls (a limit of 0 / knots {0, 15} spelled out);
  <method>_3knots        a third target pinned at frame 7 (`inner={7: image}`): three reference images in one statistics or
                         histogram call, the course through three knots;
  <method>_ends_gain     the two endpoints with max_gain = 4 (linear methods and the compound's MKL stage);
  <method>_3knots_gain   both.

HIP events around each call, median of the runs after a warm-up, with the range; all in one process, beside the parent's
figures in profiles/colour_hist_timing.json (match_colour_hm, match_colour_hm_mkl_hm) and profiles/colour_match_timing.json.
The expectation: equal times within the run-to-run spread -- the apply passes are unchanged, the coefficient kernel is one
thread per frame and the table kernel one block per frame and channel; a third target adds one 320 x 512 image to the
reference pass.  No threshold.

    python scripts/colour_knots_timing.py [--runs 50] [--out profiles/colour_knots_timing.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_knots_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd import ops, output
    from tooncrafter_amd.ops import HipOps
    hip = HipOps()
    gen = torch.Generator().manual_seed(23)
    noise = (torch.rand(1, 3, 16, 320, 512, generator=gen) * 2.4 - 1.2).to("cuda")
    ends = (torch.rand(1, 3, 2, 320, 512, generator=gen) * 1.6 - 0.8).to("cuda")
    inner = {7: (torch.rand(1, 3, 320, 512, generator=gen) * 1.2 - 0.6).to("cuda")}
    two = {0: ends[:, :, 0].contiguous()}                        # an inner target ON an endpoint: the knots route, two knots

    def path(method, gain=None, pinned=None):
        m = output.ColourMatch(method, max_gain=gain)
        return lambda: output.match_colour(noise, ends, m, inner=pinned)
    paths = {}
    for method in output.COLOUR_MATCH_METHODS:
        paths[f"{method}_ends"] = path(method)
        paths[f"{method}_2knots"] = path(method, pinned=two)
        paths[f"{method}_3knots"] = path(method, pinned=inner)
        if method != "hm":
            paths[f"{method}_ends_gain"] = path(method, gain=4.0)
            paths[f"{method}_3knots_gain"] = path(method, gain=4.0, pinned=inner)
    res = {"what": "output.match_colour of one (1, 3, 16, 320, 512) fp32 clip to 320 x 512 keyframes on the device with 2 and 3 knots, "
                   "with and without max_gain = 4, ms (HIP events)", "runs": args.runs}
    prev = ops.set_backend(hip)
    try:
        for name, fn in paths.items():
            res[name] = timed(fn, args.runs)
    finally:
        ops.set_backend(prev)
    for method in output.COLOUR_MATCH_METHODS:
        res[f"{method}_3knots_over_ends"] = res[f"{method}_3knots"]["median_ms"] / res[f"{method}_ends"]["median_ms"]
        res[f"{method}_2knots_over_ends"] = res[f"{method}_2knots"]["median_ms"] / res[f"{method}_ends"]["median_ms"]
        if method != "hm":
            res[f"{method}_gain_over_ends"] = res[f"{method}_ends_gain"]["median_ms"] / res[f"{method}_ends"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
