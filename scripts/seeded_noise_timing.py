"""One step's noise draw, seeded against unseeded, on the GPU: `ops.randn_clips(seeds, shape, stream, scale=temperature)` (one
tc_randn_clips launch) against what the unseeded sampler runs for the same operand (`torch.randn(shape)` from the device
generator, times the temperature).  HIP events around `--iters` back-to-back draws, median of `--repeats` after a warm-up, the
two alternating.  Prints one JSON line.

    python scripts/seeded_noise_timing.py [--batch 1] [--iters 200] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tooncrafter_amd import ops  # noqa: E402


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / iters          # microseconds per draw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    shape = (a.batch, 4, 16, 40, 64)
    seeds = list(range(1, a.batch + 1))
    paths = {"seeded": lambda t: ops.randn_clips(seeds, shape, 7, scale=t),
             "unseeded": lambda t: torch.randn(shape, device="cuda") if t == 1.0 else torch.randn(shape, device="cuda") * t}
    out = {"shape": list(shape), "iters": a.iters, "repeats": a.repeats, "binding": getattr(ops.backend(), "binding", "ctypes")}
    for temperature in (1.0, 0.9):
        runs = {k: [] for k in paths}
        for rep in range(a.repeats + 1):
            for name, fn in paths.items():
                us = timed(lambda: fn(temperature), a.iters)
                if rep:                                       # the first round is the warm-up
                    runs[name].append(us)
        for name, v in runs.items():
            out[f"{name}_us_t{temperature}"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
