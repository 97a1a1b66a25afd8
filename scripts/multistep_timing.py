#!/usr/bin/env python3
"""What the second-order multistep sampler costs and saves.

(1) The step kernel: tc_ddim_step_ms (history given, corr != 0) against tc_ddim_step on the same operands, at the clip's
latent (1, 4, 16, 40, 64) and at B = 2, in the clip's configuration (two-way guidance 7.5, rescale 0.7, eta = 1 noise), in one
process.  Each figure is the time of one call inside a captured graph of `--calls` back-to-back calls (device time, no host
launch cost), and the same loop launched eagerly (what a Python caller sees); HIP events, `--runs` windows of each after a
warm-up, the two kernels alternating.
(2) The clip: `SamplingPlan(steps=20, order=2)` against `SamplingPlan(steps=50, order=1)`, sampler plus the spliced decode,
on the full-size model with random weights as bench.py builds it (timing only: random weights say nothing about quality).

    python scripts/multistep_timing.py [--runs 7] [--calls 200] [--clip-runs 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SC = dict(cfg_scale=7.5, guidance_rescale=0.7, sqrt_ac=0.6, sqrt_1m_ac=0.8, sqrt_a_prev=0.7, dir_coef=0.5, sigma=0.3, x0_rescale=0.98)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


def kernel_timing(runs, calls):
    from tooncrafter_amd import ops
    be = ops.backend()
    out = {}
    for b in (1, 2):
        g = torch.Generator().manual_seed(3 + b)
        x, ec, eu, nz, hist = (torch.randn(b, 4, 16, 40, 64, generator=g).cuda() for _ in range(5))
        loops = {"tc_ddim_step": lambda: [be.ddim_step(x, ec, eu, nz, **SC) for _ in range(calls)],
                 "tc_ddim_step_ms": lambda: [be.ddim_step_ms(x, ec, eu, nz, hist, corr=0.4, **SC) for _ in range(calls)]}
        graphs = {}
        for k, fn in loops.items():                              # warm-up, then one captured graph of `calls` calls per kernel
            fn()
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                fn()
            graphs[k].replay()
        torch.cuda.synchronize()
        us = {(k, how): [] for k in loops for how in ("graph", "eager")}
        for _ in range(runs):
            for k in loops:
                us[k, "graph"].append(timed(graphs[k].replay) * 1e3 / calls)
                us[k, "eager"].append(timed(loops[k]) * 1e3 / calls)
        res = {f"{k} {how} us_per_call": stats(v) for (k, how), v in us.items()}
        for how in ("graph", "eager"):
            res[f"ms_over_first_order {how}"] = (res[f"tc_ddim_step_ms {how} us_per_call"]["median"] /
                                                 res[f"tc_ddim_step {how} us_per_call"]["median"])
        out[f"B={b}"] = res
        print(json.dumps({f"kernel B={b}": res}), flush=True)
    return out


def clip_timing(clip_runs):
    import bench
    from tooncrafter_amd import clip
    model = bench.build_model("cuda")
    inp = bench.make_inputs("cuda", seed=0)
    cond = clip.Conditions({"c_crossattn": [inp["cond"]], "c_concat": [inp["c_concat"]]},
                           {"c_crossattn": [inp["uncond"]], "c_concat": [inp["c_concat"]]}, None, inp["refs"], inp["fs"])
    plans = {"steps=50 order=1": clip.SamplingPlan(steps=50, order=1), "steps=20 order=2": clip.SamplingPlan(steps=20, order=2)}

    def one(plan):
        latents = clip.sample(model, cond, plan, [1, 4, 16, 40, 64], x_T=inp["x_T"])
        video = clip.decode_spliced(model, latents, cond.refs)
        assert bool(torch.isfinite(video).all())
        return video

    ms = {k: [] for k in plans}
    with torch.no_grad():
        one(clip.SamplingPlan(steps=3, order=2))                 # warm-up: code objects, packing, graphs, allocator
        one(clip.SamplingPlan(steps=2, order=1))
        torch.cuda.synchronize()
        for _ in range(clip_runs):
            for k, plan in plans.items():
                ms[k].append(timed(lambda: one(plan)))
                print(json.dumps({"clip": k, "ms": ms[k][-1]}), flush=True)
    res = {f"{k} clip_ms": stats(v) for k, v in ms.items()}
    res["clip_time_ratio"] = res["steps=20 order=2 clip_ms"]["median"] / res["steps=50 order=1 clip_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--clip-runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    res = {"what": "tc_ddim_step_ms vs tc_ddim_step (us per call) and the clip at 20 corrected steps vs 50 DDIM steps (ms), "
                   "320x512x16f, random weights", "runs": args.runs, "calls": args.calls, "clip_runs": args.clip_runs}
    res["kernel"] = kernel_timing(args.runs, args.calls)
    res["clip"] = clip_timing(args.clip_runs)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
