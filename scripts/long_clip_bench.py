#!/usr/bin/env python3
"""Long clips (the reference's --video_length N) on the full-size model at 320 x 512: what a clip of T frames costs, and
what the temporal self-attention costs in it.

    python scripts/long_clip_bench.py                     # clips + per-level kernel times, T in {16, 24, 32, 64}
    python scripts/long_clip_bench.py --forward 32        # 5 guided UNet forwards at T = 32 only (run under rocprofv3)
    python scripts/long_clip_bench.py --stats DIR         # temporal-attention share of a rocprofv3 --stats run in DIR

Reported per T:
  * DDIM-50 clip (CFG 7.5, batched guidance, hipGraph replay, two decodes + splice, as bench.py's clip) frames / s;
  * tc_attn_temporal per call at each UNet level (B = 2: the guided batch), HIP events over 50 calls; at T = 16 that is
    the VALU kernel of csrc/attention.hip, above it csrc/attention_temporal_long.hip;
  * the attention's share of one guided forward, from HIP events around every attention_temporal call of the forward.
The context is 77 text + 256 image tokens at every T (the reference's image projection yields 256 whatever N is; at
T = 16 that is the per-frame split, above it the shared-image-token route).  T = 16 takes bench.py's routes unchanged
(levels 0-3 fused: tb_fused / qkv_attn); the other lengths take the GEMM + tc_attn_temporal route at every level.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from tooncrafter_amd import clip as clip_api, ops, synth  # noqa: E402
from tooncrafter_amd.lvdm.ddim import DDIMSampler  # noqa: E402

DEV = "cuda"
H, W = 40, 64
LEVELS = [(0, 320, H * W), (1, 640, H * W // 4), (2, 1280, H * W // 16), (3, 1280, H * W // 64)]   # (level, C, hw)


def inputs(t, seed=7):
    inp = synth.synth_inputs(1, t, H, W, n_img_tokens_per_frame=0, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in ("cond", "uncond"):
        inp[k] = torch.cat([inp[k], torch.randn(1, 256, inp[k].shape[2], generator=g)], 1)
    d = {k: v.to(DEV) for k, v in inp.items()}
    d["refs"] = [r.to(DEV) for r in synth.synth_ref_context(1, H, W, ch=128, seed=seed + 100)]
    return d


def run_clip(model, sampler, inp, t, steps):
    cond = {"c_crossattn": [inp["cond"]], "c_concat": [inp["c_concat"]]}
    uc = {"c_crossattn": [inp["uncond"]], "c_concat": [inp["c_concat"]]}
    samples, _ = sampler.sample(S=steps, conditioning=cond, batch_size=1, shape=(4, t, H, W), verbose=False,
                                unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0, cfg_img=None,
                                mask=None, x0=None, fs=inp["fs"], timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                                x_T=inp["x_T"], unconditional_conditioning_img_nonetext=None)
    return clip_api.decode_spliced(model, samples, inp["refs"])


def clip_fps(model, t, clips):
    sampler = DDIMSampler(model)
    inp = inputs(t)
    model._cfg_state = None
    with torch.no_grad():
        run_clip(model, sampler, inp, t, 2)                     # graph capture of this shape, decoder graphs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(clips):
            video = run_clip(model, sampler, inp, t, 50)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert torch.isfinite(video).all()
    return clips * t / dt, dt / clips


def kernel_times(t, reps=50):
    hip = ops.backend()
    out = {}
    for lvl, c, hw in LEVELS:
        heads = c // 64
        qkv = torch.randn(2 * t * hw, 3 * c, device=DEV).to(torch.bfloat16)
        for _ in range(3):
            hip.attention_temporal(qkv, b=2, t=t, hw=hw, heads=heads)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            hip.attention_temporal(qkv, b=2, t=t, hw=hw, heads=heads)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / reps
        flop = 4.0 * 2 * hw * heads * t * t * 64                 # q k^T and p v
        byts = 2 * t * hw * (3 * c + c) * 2.0
        out[f"level{lvl}"] = dict(c=c, hw=hw, us=round(us, 2), tflops=round(flop / us * 1e-6, 3),
                                  gbs=round(byts / us * 1e-3, 1))
    return out


def forward_share(model, t, reps=3):
    """HIP events around the whole guided forward and around every attention_temporal call inside it."""
    inp = inputs(t)
    un = model.model.diffusion_model
    be = ops.backend()
    orig = be.attention_temporal
    rec = []

    def attn(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = orig(*a, **kw)
        e1.record()
        rec.append((e0, e1))
        return r
    x2 = torch.cat([inp["x_T"]] * 2)
    cc2 = torch.cat([inp["c_concat"]] * 2)
    ctx2 = torch.cat([inp["cond"], inp["uncond"]])
    fs2 = torch.cat([inp["fs"]] * 2)
    ts = torch.tensor([601, 601], device=DEV)
    with torch.no_grad():
        un(None, ts, context=ctx2, fs=fs2, x_parts=[x2, cc2])
        be.attention_temporal = attn
        try:
            tot = 0.0
            for _ in range(reps):
                f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                f0.record()
                un(None, ts, context=ctx2, fs=fs2, x_parts=[x2, cc2])
                f1.record()
                torch.cuda.synchronize()
                tot += f0.elapsed_time(f1)
        finally:
            be.attention_temporal = orig
    attn_ms = sum(a.elapsed_time(b) for a, b in rec) / reps
    return dict(forward_ms=round(tot / reps, 2), attn_calls=len(rec) // reps, attn_ms=round(attn_ms, 3),
                attn_share=round(attn_ms / (tot / reps), 4))


def stats_share(d):
    """Temporal-attention kernels' share of all kernel time in a rocprofv3 --kernel-trace --stats directory."""
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {d}")
    rows = list(csv.DictReader(open(files[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    attn = [r for r in rows if "attn_temporal" in r["Name"]]
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]
    return dict(file=os.path.relpath(files[0], d), total_ms=round(tot * 1e-6, 2),
                temporal_attention={r["Name"][:80]: dict(calls=int(r["Calls"]), ms=round(float(r["TotalDurationNs"]) * 1e-6, 3))
                                    for r in attn},
                temporal_attention_share=round(sum(float(r["TotalDurationNs"]) for r in attn) / tot, 4),
                top=[(r["Name"][:80], int(r["Calls"]), round(float(r["Percentage"]), 2)) for r in top])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 24, 32, 64])
    ap.add_argument("--clips", type=int, default=2, help="timed DDIM-50 clips per T")
    ap.add_argument("--forward", type=int, metavar="T", help="only 5 guided forwards at T (for a rocprofv3 run)")
    ap.add_argument("--stats", metavar="DIR", help="only parse a rocprofv3 --stats directory")
    ap.add_argument("--out", help="also write the JSON result here")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats_share(a.stats), indent=1))
        return
    model = bench.build_model(DEV)
    if a.forward:
        r = forward_share(model, a.forward, reps=5)
        print(json.dumps(dict(frames=a.forward, **r)))
        return
    res = {"device": torch.cuda.get_device_name(0), "h": H * 8, "w": W * 8, "by_frames": {}}
    for t in a.frames:
        fps, s = clip_fps(model, t, a.clips)
        r = dict(clip_frames_per_s=round(fps, 3), s_per_clip=round(s, 3), attention_per_call=kernel_times(t),
                 forward=forward_share(model, t))
        res["by_frames"][str(t)] = r
        print(json.dumps({"frames": t, **r}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
