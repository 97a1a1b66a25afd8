#!/usr/bin/env python3
"""What tc_still_map and tc_still_composite cost on the device at b = 1, 320 x 512, t = 16, and what the same quantities cost
written with torch operators on the same GPU.

  map         ops.still_map(ends, tau 8, grow 1, feather 2): three launches                              against `torch_map`:
              clamp, difference, threshold, `max_pool2d` 8 x 8 for the cells, D dilations by `max_pool2d` 3 x 3 for the capped
              distance, bilinear `interpolate` x 8 for alpha (floating point: equal to 1e-6, mask and dist exactly);
  composite   ops.still_composite over all 16 frames, into a second tensor and in place               against `torch_composite`:
              key = e0 + s (e1 - e0), where(alpha == 0, v, where(alpha == 1, key, v + alpha (key - v))) (bit for bit).

The keyframes are a still background with a redrawn region of 96 x 128 pixels, so that alpha has its three kinds of pixel.  The
results are checked against the torch statements before anything is timed.

HIP events around `--inner` calls in a row, per-call time = window / inner, median over `--runs` windows after a warm-up, with
the range; all in one process, the arms alternating window by window.  The HBM bound is the bytes a call must read and write
once (map: the keyframes in, alpha, mask and dist out; composite: clip in and out, keyframes and alpha in) at 6.3 TB/s, the
achievable rate; the in-place composite skips the pixels whose alpha is 0, its bound is quoted for the full clip all the same.
No threshold is fixed in advance: the torch statement in the same process is the yardstick.

    python scripts/still_timing.py [--runs 30] [--inner 20] [--out profiles/still_timing.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TB_S = 6.3


def torch_map(ends, tau, grow, feather):
    """(mask (b, 1, 1, h, w), alpha (b, H, W), dist (b, h, w) uint8) of (b, 3, 2, H, W) keyframes in torch operators"""
    cap = grow + feather + 1
    thr = float(torch.tensor(float(tau), dtype=torch.float32) / torch.tensor(127.5, dtype=torch.float32))
    c = ends.clamp(-1.0, 1.0)
    pixel = (~((c[:, :, 0] - c[:, :, 1]).abs() <= thr)).any(dim=1, keepdim=True).to(torch.float32)
    reach = F.max_pool2d(pixel, 8)
    d = torch.zeros_like(reach)
    for _ in range(cap):
        d += 1.0 - reach
        reach = F.max_pool2d(reach, 3, stride=1, padding=1)
    a = (d - grow - 1).clamp(0, feather) / feather
    alpha = F.interpolate(a, scale_factor=8, mode="bilinear", align_corners=False)
    return (d > grow).to(torch.float32).unsqueeze(1), alpha[:, 0], d[:, 0].to(torch.uint8)


def torch_composite(video, ends, alpha):
    t = video.shape[2]
    s = (torch.arange(t, dtype=torch.float32, device=video.device) / torch.tensor(float(t - 1), device=video.device)).view(1, 1, t, 1, 1)
    e0, e1, a = ends[:, :, :1], ends[:, :, 1:], alpha[:, None, None]
    key = e0 + s * (e1 - e0)
    return torch.where(a == 0, video, torch.where(a == 1, key, video + a * (key - video)))


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def timed(fns, runs, inner):
    """the arms of `fns` alternating, window by window"""
    for fn in fns.values():                                      # warm-up: code objects, allocator
        window(fn, 3)
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            ms[name].append(window(fn, inner))
    return {name: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}


def inputs(b, t, hh, ww, device):
    gen = torch.Generator().manual_seed(31)
    first = torch.rand(b, 3, hh, ww, generator=gen) * 2 - 1
    last = first.clone()
    last[:, :, 100:196, 200:328] = torch.rand(b, 3, 96, 128, generator=gen) * 2 - 1
    ends = torch.stack([first, last], dim=2).contiguous().to(device)
    video = (torch.rand(b, 3, t, hh, ww, generator=gen) * 2 - 1).to(device)
    return ends, video


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "still_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd.ops import HipOps
    hip = HipOps()
    b, t, hh, ww, rule = 1, 16, 320, 512, dict(tau=8, grow=1, feather=2)
    ends, video = inputs(b, t, hh, ww, "cuda")
    mask, alpha, dist = hip.still_map(ends, **rule)
    want = torch_map(ends, **rule)
    assert torch.equal(mask, want[0]) and torch.equal(dist, want[2]) and float((alpha - want[1]).abs().max()) <= 1e-6
    assert torch.equal(hip.still_composite(video, ends, alpha), torch_composite(video, ends, alpha))
    out, held = torch.empty_like(video), video.clone()
    res = {"what": f"tc_still_map and tc_still_composite at b = {b}, {hh} x {ww}, t = {t} against the same quantities in torch operators, "
                   f"ms per call (HIP events round {args.inner} calls)", "runs": args.runs, "inner": args.inner,
           "hbm_tb_per_s_for_the_bound": HBM_TB_S, "rule": rule,
           "alpha_share": {"zero": float((alpha == 0).float().mean()), "one": float((alpha == 1).float().mean())}}
    plane, cells = hh * ww * 4, (hh // 8) * (ww // 8)
    r = timed({"hip": lambda: hip.still_map(ends, **rule), "torch": lambda: torch_map(ends, **rule)}, args.runs, args.inner)
    r["bytes"] = b * (7 * plane + 5 * cells)
    res["map"] = r
    r = timed({"hip": lambda: hip.still_composite(video, ends, alpha, out=out),
               "hip_in_place": lambda: hip.still_composite(held, ends, alpha, out=held),
               "torch": lambda: torch_composite(video, ends, alpha)}, args.runs, args.inner)
    r["bytes"] = b * (2 * 3 * t + 6 + 1) * plane
    res["composite"] = r
    for r in (res["map"], res["composite"]):
        r["hbm_bound_ms"] = r["bytes"] / (HBM_TB_S * 1e9)
        r["hip_over_hbm_bound"] = r["hip"]["median_ms"] / r["hbm_bound_ms"]
        r["hip"]["gb_per_s"] = r["bytes"] / r["hip"]["median_ms"] / 1e6
        r["torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
