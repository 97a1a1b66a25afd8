#!/usr/bin/env python3
"""Long clips (the reference's --video_length N) on the full-size model at 320 x 512: what a clip of T frames costs, and
what the temporal self-attention costs in it.

    python scripts/long_clip_bench.py                     # clips + per-level kernel times, T in {16, 24, 32, 64}
    python scripts/long_clip_bench.py --forward 32        # 5 guided UNet forwards at T = 32 only (run under rocprofv3)
    python scripts/long_clip_bench.py --stats DIR         # temporal-attention share of a rocprofv3 --stats run in DIR
    python scripts/long_clip_bench.py --qkv-attn          # per call: one-launch qkv + attention vs tc_gemm_bf16 + tc_attn_temporal
    python scripts/long_clip_bench.py --forward-ab 32 64  # guided forward, TC_QKV_ATTN=0 against 2, same process

Reported per T:
  * DDIM-50 clip (CFG 7.5, batched guidance, hipGraph replay, two decodes + splice, as bench.py's clip) frames / s;
  * tc_attn_temporal per call at each UNet level (B = 2: the guided batch), HIP events over 50 calls; at T = 16 that is
    the VALU kernel of csrc/attention.hip, above it csrc/attention_temporal_long.hip;
  * the attention's share of one guided forward, from HIP events around every attention_temporal call of the forward.
The context is 77 text + 256 image tokens at every T (the reference's image projection yields 256 whatever N is; at
T = 16 that is the per-frame split, above it the shared-image-token route).  T = 16 takes bench.py's routes unchanged
(one launch per temporal self-attention: qkv_attn); the other lengths take the one launch of qkv_attn_long where
TC_QKV_ATTN admits the shape and the GEMM + tc_attn_temporal route elsewhere (TC_QKV_ATTN=0: everywhere).
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


def _time_calls(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def qkv_attn_table(frames, reps=50):
    """tc_temporal_qkv_attn (csrc/qkv_attn_long.hip, TC_QKV_ATTN=2) against tc_gemm_bf16 + tc_attn_temporal per call, at
    the four level geometries, B = 2 (the guided batch): HIP events over `reps` calls, both arms in this process, each arm
    measured twice (fused, two launches, fused, two launches).  A cell is AHEAD only if the slower fused repeat beats the
    faster two-launch repeat by more than the larger of the two arms' repeat-to-repeat spreads: the rule the library's
    default (mode 1) is set by."""
    from tooncrafter_amd.ops import HipOps
    os.environ["TC_QKV_ATTN"] = "2"
    hip = HipOps()                                              # ctypes for both arms, every result into a fixed buffer
    lines = ["# one-launch qkv + temporal attention vs tc_gemm_bf16 + tc_attn_temporal, per call, B = 2",
             f"# {torch.cuda.get_device_name(0)}; {hip.lib.tc_build_info().decode()}; HIP events over {reps} calls, us",
             "# ahead = (min two launches - max fused) / min two launches; spread = max over the arms of |rep1 - rep2| / min",
             f"{'C':>5} {'hw':>5} {'T':>3} {'TT':>3} | {'fused 1':>9} {'fused 2':>9} | {'gemm+attn 1':>11} {'gemm+attn 2':>11} | "
             f"{'ahead %':>8} {'spread %':>8} | verdict"]
    for lvl, c, hw in LEVELS:
        heads = c // 64
        g = torch.Generator(device=DEV).manual_seed(lvl)
        w = (torch.randn(3 * c, c, device=DEV, generator=g) * c ** -0.5).to(torch.bfloat16)
        for t in frames:
            x = torch.randn(2 * t * hw, c, device=DEV, generator=g).to(torch.bfloat16)
            kw = dict(b=2, t=t, hw=hw, heads=heads)
            if not hip.temporal_qkv_attn_eligible(b=2, t=t, hw=hw, c=c, heads=heads):
                raise SystemExit(f"C = {c}, hw = {hw}, T = {t}: not eligible with TC_QKV_ATTN=2")
            out = torch.empty(2 * t * hw, c, device=DEV, dtype=torch.bfloat16)
            qkv = torch.empty(2 * t * hw, 3 * c, device=DEV, dtype=torch.bfloat16)
            fused = lambda: hip.temporal_qkv_attn(x, w, None, out=out, **kw)
            out2 = torch.empty_like(out)
            from tooncrafter_amd import _lib
            stream = torch.cuda.current_stream().cuda_stream

            def two():                                          # the raw entry: a fixed output buffer, as the fused arm has
                hip.gemm(x, w, out=qkv)
                _lib.check(hip.lib.tc_attn_temporal(qkv.data_ptr(), out2.data_ptr(), 2, t, hw, heads, 0.125, stream), "tc_attn_temporal")
            for fn in (fused, two):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            f1, t1, f2, t2 = _time_calls(fused, reps), _time_calls(two, reps), _time_calls(fused, reps), _time_calls(two, reps)
            ahead = (min(t1, t2) - max(f1, f2)) / min(t1, t2)
            spread = max(abs(f1 - f2) / min(f1, f2), abs(t1 - t2) / min(t1, t2))
            ok = ahead > spread
            lines.append(f"{c:>5} {hw:>5} {t:>3} {32 if t <= 32 else 64:>3} | {f1:>9.2f} {f2:>9.2f} | {t1:>11.2f} {t2:>11.2f} | "
                         f"{100 * ahead:>+8.2f} {100 * spread:>8.2f} | {'AHEAD' if ok else 'not ahead'}")
            print(lines[-1], flush=True)
    return lines


def forward_ab(model, t, runs=6, rounds=3):
    """Guided (B = 2) UNet forward at T frames, TC_QKV_ATTN=0 against 2: per arm a fresh backend and a freshly captured
    graph, replayed alternately.  Reports whether the two arms' outputs are bit-identical and how many one-launch calls
    each arm's forward made: the kernel rounds exactly as the two launches do (tests/test_gpu_qkv_attn_long.py measures
    rel-L2 0 between them), so equal bits alone do not say that the switch failed -- equal call counts do.  The count is
    taken around the backend's Python method: it says that the host routed to tc_temporal_qkv_attn, not which kernel the
    library launched under it; that the two arms run different kernels shows in their different times."""
    inp = inputs(t)
    un = model.model.diffusion_model
    x2 = torch.cat([inp["x_T"]] * 2)
    cc2 = torch.cat([inp["c_concat"]] * 2)
    ctx2 = torch.cat([inp["cond"], inp["uncond"]])
    fs2 = torch.cat([inp["fs"]] * 2)
    ts = torch.tensor([601, 601], device=DEV)
    fwd = lambda: un(None, ts, context=ctx2, fs=fs2, x_parts=[x2, cc2])
    graphs, outs, calls, lines = {}, {}, {}, []
    prev = ops.backend()
    try:
        with torch.no_grad():
            for mode in ("0", "2"):
                os.environ["TC_QKV_ATTN"] = mode
                be = type(prev)()
                ops.set_backend(be)
                real, n = be.temporal_qkv_attn, []
                be.temporal_qkv_attn = lambda *a_, **k_: (n.append(1), real(*a_, **k_))[1]
                calls[mode] = n
                un.reset_conditioning()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    outs[mode] = fwd().clone()
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fwd()
                graphs[mode] = g
    finally:
        os.environ.pop("TC_QKV_ATTN", None)
        ops.set_backend(prev)
    same = torch.equal(outs["0"], outs["2"])
    rel = float((outs["2"].float() - outs["0"].float()).norm() / outs["0"].float().norm())
    n0, n2 = len(calls["0"]) // 2, len(calls["2"]) // 2         # eager run + capture
    lines.append(f"T = {t}: outputs TC_QKV_ATTN=0 vs 2: rel-L2 {rel:.3e}, bit-identical: {same}; one-launch calls per forward: "
                 f"{n0} vs {n2}" + ("   <-- THE SWITCH DID NOT TAKE EFFECT" if n0 == n2 else ""))

    def run(g):
        g.replay()
        torch.cuda.synchronize()
        return _time_calls(g.replay, runs) / 1000.0
    for g in graphs.values():
        run(g)
    ta, tb = [], []
    for rd in range(rounds):
        a, b = run(graphs["0"]), run(graphs["2"])
        ta.append(a)
        tb.append(b)
        lines.append(f"T = {t} round {rd}: two launches {a:8.3f} ms | one launch {b:8.3f} ms | one vs two {100.0 * (a / b - 1.0):+5.2f} %")
    ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
    lines.append(f"T = {t} median: two launches {ma:.3f} ms | one launch {mb:.3f} ms | one vs two {100.0 * (ma / mb - 1.0):+.2f} % "
                 f"per guided forward; spread of the rounds: two {100 * (max(ta) / min(ta) - 1):.2f} %, one {100 * (max(tb) / min(tb) - 1):.2f} %")
    for ln in lines:
        print(ln, flush=True)
    return lines


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
    ap.add_argument("--qkv-attn", action="store_true", help="only the per-call table one launch vs two (T from --qkv-frames)")
    ap.add_argument("--qkv-frames", type=int, nargs="+", default=[24, 32, 48, 64])
    ap.add_argument("--forward-ab", type=int, nargs="+", metavar="T", help="only the guided-forward A/B TC_QKV_ATTN=0 vs 2 at these T")
    ap.add_argument("--out", help="also write the result here (JSON; text for --qkv-attn / --forward-ab)")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats_share(a.stats), indent=1))
        return

    def write_text(lines):
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if a.qkv_attn:
        write_text(qkv_attn_table(a.qkv_frames))
        return
    model = bench.build_model(DEV)
    if a.forward_ab:
        lines = [f"# guided UNet forward (B = 2, 320 x 512), TC_QKV_ATTN=0 vs 2, graphs replayed alternately; {torch.cuda.get_device_name(0)}"]
        for t in a.forward_ab:
            lines += forward_ab(model, t)
        write_text(lines)
        return
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
