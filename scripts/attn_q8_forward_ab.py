#!/usr/bin/env python3
"""Same-process forward A/B of TC_FP8_ATTN on the full-size UNet (one forward of the 16-frame clip, TC_FP8=1 in both arms).  Each arm gets a fresh backend with its switch set, one eager warm-up forward, then its own captured hipGraph; the
arms' replays are timed alternately.  The two arms' outputs must differ: two graphs of the same kernels would not.

    python scripts/attn_q8_forward_ab.py [rounds]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bench  # noqa: E402
import fullsize_cases as fc  # noqa: E402
from tooncrafter_amd import ops, synth  # noqa: E402
from tooncrafter_amd.torch_ops import TorchLibOps  # noqa: E402
from tooncrafter_amd.utils import instantiate_from_config  # noqa: E402


def build_model():
    with torch.device("meta"):
        model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=bench.MODEL_PARAMS))
    model = model.to_empty(device="cuda").eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(synth.synth_tensor(name, tuple(p.shape), 1234, "cpu"))
        bufs = bench.instantiate_schedule()
        for name, b in model.named_buffers():
            b.copy_(bufs[name].to("cuda"))
    return model


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    model = build_model()
    un = model.model.diffusion_model
    inp = fc.inputs()
    ctx, fs = inp["cond"].to("cuda"), inp["fs"].to("cuda")
    ts = torch.tensor([fc.UNET_T], device="cuda")
    parts = [inp["x_T"].to("cuda"), inp["c_concat"].to("cuda")]
    arms = {}
    for name, on in (("fp8", False), ("fp8+attn8", True)):
        be = TorchLibOps()
        be.fp8, be.fp8_attn = "linear", on
        ops.set_backend(be)
        with torch.no_grad():
            un(None, ts, context=ctx, fs=fs, x_parts=parts)                   # eager: weight quantisation, caches
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                un(None, ts, context=ctx, fs=fs, x_parts=parts)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = un(None, ts, context=ctx, fs=fs, x_parts=parts)
        arms[name] = (g, out, dict(be.fp8_calls))
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for name, (g, _, _) in arms.items():
            g.replay()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / 5)
    ya, yb = arms["fp8"][1].float(), arms["fp8+attn8"][1].float()
    d = float((ya - yb).norm() / ya.norm())
    print(f"# {torch.cuda.get_device_name(0)}; full-size UNet, one 16-frame forward, hipGraph replay, "
          f"{rounds} alternating rounds of 5 replays")
    for name in arms:
        t = sorted(times[name])
        print(f"{name:10s} median {t[len(t) // 2]:7.2f} ms  min {t[0]:7.2f} ms  all {' '.join(f'{x:.2f}' for x in times[name])}  "
              f"fp8_calls at capture {arms[name][2]}")
    ma, mb = sorted(times["fp8"])[rounds // 2], sorted(times["fp8+attn8"])[rounds // 2]
    print(f"speed-up of TC_FP8_ATTN=1 over TC_FP8=1 alone: x{ma / mb:.4f}; outputs differ by rel-L2 {d:.3e}")
    assert arms["fp8+attn8"][2]["attn_q8"] > 0 and arms["fp8"][2]["attn_q8"] == 0
    assert d > 0, "the two arms computed the same thing: the switch did not reach the captured graph"


if __name__ == "__main__":
    main()
