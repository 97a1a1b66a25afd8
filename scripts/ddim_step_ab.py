#!/usr/bin/env python3
"""A/B of the DDIM step between two builds of libtooncrafter_hip.so in ONE process: the kernel part of
scripts/multistep_timing.py (same operands, scalars, graph of `calls` calls, eager loop, HIP events), the two libraries
alternating inside every run.   python scripts/ddim_step_ab.py PARENT.so BRANCH.so OUT.json [runs] [calls]"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from multistep_timing import SC, stats, timed  # noqa: E402
from tooncrafter_amd import _lib  # noqa: E402
from tooncrafter_amd.ops import HipOps  # noqa: E402


def backend(path):
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.tc_abi_version() == _lib.TC_ABI_VERSION
    be = HipOps()
    be.lib = lib
    return be, lib.tc_build_info().decode()


def main():
    parent, branch, out_path = sys.argv[1:4]
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    calls = int(sys.argv[5]) if len(sys.argv) > 5 else 200
    bes, info = {}, {}
    for who, path in (("parent", parent), ("branch", branch)):
        bes[who], info[who] = backend(path)
    res = {"runs": runs, "calls": calls, "build_info": info}
    for b in (1, 2):
        g = torch.Generator().manual_seed(3 + b)
        x, ec, eu, nz, hist = (torch.randn(b, 4, 16, 40, 64, generator=g).cuda() for _ in range(5))
        loops = {}
        for who, be in bes.items():
            loops[who, "tc_ddim_step"] = lambda be=be: [be.ddim_step(x, ec, eu, nz, **SC) for _ in range(calls)]
            loops[who, "tc_ddim_step_ms"] = lambda be=be: [be.ddim_step_ms(x, ec, eu, nz, hist, corr=0.4, **SC) for _ in range(calls)]
        # the two builds agree bit for bit on these operands
        for k in ("tc_ddim_step", "tc_ddim_step_ms"):
            a, c = loops["parent", k]()[-1], loops["branch", k]()[-1]
            assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), k
        graphs = {}
        for k, fn in loops.items():
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
        r = {f"{who} {k} {how} us_per_call": dict(stats(v), runs=v) for ((who, k), how), v in us.items()}
        for k in ("tc_ddim_step", "tc_ddim_step_ms"):
            p, n = r[f"parent {k} graph us_per_call"], r[f"branch {k} graph us_per_call"]
            s = (p["max"] - p["min"]) / p["median"]
            r[f"{k} graph criterion"] = {"parent_spread_s": s, "bound_us": p["median"] * (1 + s), "branch_median_us": n["median"],
                                         "met": n["median"] <= p["median"] * (1 + s)}
        res[f"B={b}"] = r
        print(json.dumps({f"B={b}": {k: (v if "criterion" in k else v["median"]) for k, v in r.items()}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
