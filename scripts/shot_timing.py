#!/usr/bin/env python3
"""What tc_frame_deltas costs on the device, and what the same quantities cost written with torch on the same GPU, for

  nv12_1080p   16 NV12 surfaces of 1920 x 1080 (49.8 MB): what a hardware decoder leaves for 16 keyframes;
  rgb_320x512  16 packed RGB frames of 320 x 512 (7.9 MB): keyframes at the model's size;

each on noise (lanes of a wave in different bins) and on flat images (every lane in ONE bin: the one-add path of the
histogram).  `hip` is one ops.frame_deltas call (two launches, lag 1, tau 8); `torch` is `torch_statement` below: the absolute
difference, its sum and its count over a threshold per component, and a bincount histogram per image and component.  The two
are checked equal before anything is timed.

HIP events around `--inner` calls in a row, per-call time = window / inner, median over `--runs` windows after a warm-up, with
the range; all in one process, the two arms alternating window by window.  Bytes: every sample is read once as `a` (n images)
and once as `b` (n - 1 images); the second read of an image follows the first closely and may come from cache, so the HBM bound
is quoted for n images at 6.3 TB/s (the achievable rate) and the rate for the (2n - 1) images the kernel asks for.  No
threshold is fixed in advance: the torch statement in the same process is the yardstick.

    python scripts/shot_timing.py [--runs 30] [--inner 20] [--out profiles/shot_timing.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TB_S = 6.3


def torch_statement(comps, tau):
    """(delta (n - 1, 3, 3) int64, hist (n, 3, 64) int32) of three (n, S_c) uint8 components, lag 1, in torch operators"""
    n = comps[0].shape[0]
    delta, hist = [], []
    rows = 64 * torch.arange(n, device=comps[0].device).view(n, 1)
    for v in comps:
        d = (v[:-1].to(torch.int16) - v[1:].to(torch.int16)).abs()
        h = torch.bincount(((v >> 2).to(torch.int64) + rows).view(-1), minlength=64 * n).view(n, 64)
        delta.append(torch.stack([d.sum(dim=1, dtype=torch.int64), (d > tau).sum(dim=1), (h[:-1] - h[1:]).abs().sum(dim=1)], dim=1))
        hist.append(h.to(torch.int32))
    return torch.stack(delta, dim=1), torch.stack(hist, dim=1)


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def timed_pair(fns, runs, inner):
    """the arms of `fns` alternating, window by window"""
    for fn in fns.values():                                      # warm-up: code objects, allocator
        window(fn, 3)
    ms = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            ms[name].append(window(fn, inner))
    return {name: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shot_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    from tooncrafter_amd import clip
    from tooncrafter_amd.ops import HipOps
    hip = HipOps()
    gen = torch.Generator().manual_seed(29)
    n, tau = 16, 8

    def nv12(flat):
        y = torch.randint(0, 256, (n, 1080, 1920), dtype=torch.uint8, generator=gen)
        c = torch.randint(0, 256, (n, 540, 960, 2), dtype=torch.uint8, generator=gen)
        if flat:
            y[:], c[:] = torch.arange(n, dtype=torch.uint8).view(n, 1, 1) * 9, torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1) * 5
        y, c = y.to("cuda"), c.to("cuda")
        return clip.Planes(y, (c,), "nv12"), [y.view(n, -1), c[..., 0].reshape(n, -1), c[..., 1].reshape(n, -1)], y.numel() + c.numel()

    def rgb(flat):
        x = torch.randint(0, 256, (n, 320, 512, 3), dtype=torch.uint8, generator=gen)
        if flat:
            x[:] = torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1) * 9
        x = x.to("cuda")
        return x, [x[..., k].reshape(n, -1) for k in range(3)], x.numel()
    res = {"what": "tc_frame_deltas (lag 1, tau 8) of 16 images against the same quantities in torch operators, ms per call (HIP events "
                   f"round {args.inner} calls)", "runs": args.runs, "inner": args.inner, "hbm_tb_per_s_for_the_bound": HBM_TB_S}
    for name, make in (("nv12_1080p", nv12), ("rgb_320x512", rgb)):
        for kind in ("noise", "flat"):
            frames, comps, nbytes = make(kind == "flat")
            got, want = hip.frame_deltas(frames, lag=1, tau=tau), torch_statement(comps, tau)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, kind)
            r = timed_pair({"hip": lambda: hip.frame_deltas(frames, lag=1, tau=tau), "torch": lambda: torch_statement(comps, tau)},
                           args.runs, args.inner)
            r["image_bytes"] = nbytes
            r["bytes_asked_for"] = nbytes * (2 * n - 1) // n
            r["hbm_bound_ms"] = nbytes / (HBM_TB_S * 1e9)
            r["hip"]["gb_per_s_of_bytes_asked_for"] = r["bytes_asked_for"] / r["hip"]["median_ms"] / 1e6
            r["hip_over_hbm_bound"] = r["hip"]["median_ms"] / r["hbm_bound_ms"]
            r["torch_over_hip"] = r["torch"]["median_ms"] / r["hip"]["median_ms"]
            res[f"{name}_{kind}"] = r
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
