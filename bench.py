#!/usr/bin/env python3
"""Headline benchmark: interpolated frames/s of the ToonCrafter denoising hot path.

  python bench.py --gpus N --steps K --warmup W

One "step" = one clip through the hot path on every rank: DDIM-50 (CFG 7.5, eta 1,
uniform_trailing, guidance_rescale 0.7, dynamic rescale) over the 320-channel
spatio-temporal UNet at 16 x 40 x 64 latents, then the two dual-reference VideoDecoder
passes (16 frames, then the 14-frame re-decode whose two middle frames are spliced in,
reference scripts/evaluation/inference.py:244-270) -> (1, 3, 16, 320, 512) per clip.
Inputs (conditioning, c_concat, reference hidden states, noise source) are resident in
HBM when the timed region starts.  Clips shard over ranks with no data-path collective;
rank 0 gathers the decoded clips once at the end of every step (RCCL).  Weights are
synthetic (tooncrafter_amd/synth.py), generated on the device.

Every step runs a DIFFERENT clip (two resident input sets alternate), so the per-clip refresh of the
static CFG inputs, of the cross-attention K/V and of the decoder's reference K/V is inside the timed region.

`--gpus N` with N > 1 and no torchrun environment: this script launches its own N ranks
(python -m torch.distributed.run, 127.0.0.1) -- `python bench.py --gpus 8` works without a wrapper.
`--batched-decode B` measures BASELINE.json configs[3] (perframe_ae=False): B clips per GPU whose B*T frames
go through ONE decoder call (the only B>1-correct geometry of the dual-reference fusion).

A plain run sets up, warms up, times `--steps` steps and prints ONE JSON line (rank 0): metric, value, unit,
higher_is_better, dtype, ms_per_step (one timed step, wall clock) and the per-stage split of the timed steps.
`--dump-outputs DIR` then writes what the last timed step returned to its caller, as float32 .npy files:
  video.npy     : rank 0's decoded clip (clips_per_step, 3, 16, 320, 512), the fp32 tensor `step()` returns;
  frames_u8.npy : the writer-side uint8 clip (clips_per_step, 16, 320, 512, 3) that is gathered, as float32.
Each array keeps at most DUMP_BYTES_PER_ARRAY; a larger one (--batched-decode B > 1) is replaced by a fixed,
seeded sample of its flattened elements.  The DDIM noise source is seeded before the warm-up, so the same
arguments give the same inputs and noise on every run.

`--full` adds, after the timed region, everything the headline does not need: a lease calibration around
the timed region (`value_normalised`), per-rank evidence and a timed gather, the first-stage encoder, and
  roofline     : bf16 MFMA GEMM/implicit-conv kernel -- sum(algorithmic FLOP)/sum(duration) over
                 every launch of one B=2 UNet forward, HIP events on the launch stream;
  roofline_hbm : the GroupNorm(+SiLU) operator (HBM-bound): algorithmic bytes (2 B read + 2 B written per
                 element) / duration over every launch of the same forward;
  cpu_baseline : the CPU oracle (oracle/, fp32) timed on this host on a bounded sample -- ONE full-size UNet
                 forward and a 4-frame decode -- scaled to one clip by the unit counts (100 forwards, 30 frames).
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tooncrafter_amd import clip as clip_api, ops, synth  # noqa: E402

UNET_CFG = dict(in_channels=8, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
                num_res_blocks=2, channel_mult=[1, 2, 4, 4], dropout=0.1, num_head_channels=64,
                transformer_depth=1, context_dim=1024, use_linear=True, use_checkpoint=False, temporal_conv=True,
                temporal_attention=True, temporal_selfatt_only=True, use_relative_position=False,
                use_causal_attention=False, temporal_length=16, addition_attention=True,
                image_cross_attention=True, default_fs=24, fs_condition=True)
DD_CFG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
              num_res_blocks=2, attn_resolutions=[], dropout=0.0)
MODEL_PARAMS = dict(
    rescale_betas_zero_snr=True, parameterization="v", linear_start=0.00085, linear_end=0.012, num_timesteps_cond=1,
    timesteps=1000, first_stage_key="video", cond_stage_key="caption", cond_stage_trainable=False,
    conditioning_key="hybrid", image_size=[40, 64], channels=4, scale_by_std=False, scale_factor=0.18215,
    use_ema=False, uncond_type="empty_seq", use_dynamic_rescale=True, base_scale=0.7, fps_condition_type="fps",
    perframe_ae=True, loop_video=True,
    unet_config=dict(target="lvdm.modules.networks.openaimodel3d.UNetModel", params=UNET_CFG),
    first_stage_config=dict(target="lvdm.models.autoencoder.AutoencoderKL_Dualref",
                            params=dict(embed_dim=4, monitor="val/rec_loss", ddconfig=DD_CFG,
                                        lossconfig=dict(target="torch.nn.Identity"))),
    cond_stage_config=dict(target="torch.nn.Identity"), img_cond_stage_config=dict(target="torch.nn.Identity"),
    image_proj_stage_config=dict(target="torch.nn.Identity"))

# algorithmic work per clip, SURVEY.md 8(d) (1 MAC = 2 FLOP, counted on the reference modules)
TFLOP_UNET_FWD = 12.603
TFLOP_CLIP = 100 * TFLOP_UNET_FWD + 37.875 + 33.148
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md


def build_model(device):
    from tooncrafter_amd.utils import instantiate_from_config
    with torch.device("meta"):
        model = instantiate_from_config(dict(target="lvdm.models.ddpm3d.LatentVisualDiffusion", params=MODEL_PARAMS))
    bufs = {k: v for k, v in instantiate_schedule().items()}
    model = model.to_empty(device=device).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(synth.synth_tensor(name, tuple(p.shape), 1234, device))
        for name, b in model.named_buffers():
            b.copy_(bufs[name].to(device))
    model.model.diffusion_model.prepack()
    model.first_stage_model.decoder.prepack()
    return model


def instantiate_schedule():
    """The schedule buffers live on `meta` after the meta-device construction; rebuild them on CPU."""
    from tooncrafter_amd.lvdm.ddpm3d import DDPM
    import numpy as np

    class M(torch.nn.Module):
        pass
    m = M()
    m.rescale_betas_zero_snr, m.parameterization, m.v_posterior = True, "v", 0.0
    DDPM.register_schedule(m, beta_schedule="linear", timesteps=1000, linear_start=0.00085, linear_end=0.012)
    out = dict(m.named_buffers())
    out["scale_arr"] = torch.tensor(np.concatenate((np.linspace(1.0, 0.7, 400), np.full(1000, 0.7))),
                                    dtype=torch.float32)
    return out


def make_inputs(device, seed):
    inp = synth.synth_inputs(1, 16, 40, 64, seed=seed)
    refs = synth.synth_ref_context(1, 40, 64, ch=128, seed=seed + 100)
    d = {k: v.to(device) for k, v in inp.items()}
    d["refs"] = [r.to(device) for r in refs]
    return d


STAGE_EVENTS = []      # [(name, start, end)] HIP events of the timed steps: where a clip's time goes


def _log(msg):
    if os.environ.get("TC_BENCH_VERBOSE"):
        torch.cuda.synchronize()
        sys.stderr.write(f"[bench] {msg}\n")
        sys.stderr.flush()


def _mark():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def run_clip(model, sampler, inp, ddim_steps):
    """scripts/evaluation/inference.py:244-270, from resident conditioning to the decoded clip."""
    cond = {"c_crossattn": [inp["cond"]], "c_concat": [inp["c_concat"]]}
    uc = {"c_crossattn": [inp["uncond"]], "c_concat": [inp["c_concat"]]}
    e0 = _mark()
    samples, _ = sampler.sample(S=ddim_steps, conditioning=cond, batch_size=1, shape=(4, 16, 40, 64), verbose=False,
                                unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0,
                                cfg_img=None, mask=None, x0=None, fs=inp["fs"], timestep_spacing="uniform_trailing",
                                guidance_rescale=0.7, x_T=inp["x_T"], unconditional_conditioning_img_nonetext=None)
    e1 = _mark()
    mid_mark = []
    video = clip_api.decode_spliced(model, samples, inp["refs"], marks=lambda: mid_mark.append(_mark()))
    e2, e3 = mid_mark[0], _mark()
    STAGE_EVENTS.extend([("ddim_sampler", e0, e1), ("decode_16f", e1, e2), ("decode_14f_splice", e2, e3)])
    return video


class GemmProbe:
    """Brackets every tc_gemm_bf16 launch with HIP events on the launch stream and tallies its
    algorithmic FLOPs (2*M*N*K with the logical, un-padded K)."""

    def __init__(self, backend):
        self.b = backend
        self.orig = backend.gemm
        self.orig_ff = getattr(backend, "ff_geglu_fused", None)
        self.orig_tb = getattr(backend, "temporal_attn_fused", None)
        self.orig_tqa = getattr(backend, "temporal_qkv_attn", None)
        self.rec = []

    def __enter__(self):
        def ff(x, w1, b1, w2, b2, **kw):
            # the one-launch feed-forward (tc_ff_geglu_fused) IS the two GEMMs it replaces: counted with the family, at
            # the FLOPs of both products
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = self.orig_ff(x, w1, b1, w2, b2, **kw)
            e1.record()
            self.rec.append((e0, e1, 2.0 * x.shape[0] * (w1.shape[0] * w1.shape[1] + w2.shape[0] * w2.shape[1])))
            return out

        def tb(x, wqkv, bqkv, wo, bo, **kw):
            # the one-launch temporal self-attention (tc_temporal_attn_fused): counted with the family at the FLOPs of the
            # two projections it fuses (the 16 x 16 attentions in between were never part of the family)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = self.orig_tb(x, wqkv, bqkv, wo, bo, **kw)
            e1.record()
            self.rec.append((e0, e1, 2.0 * x.shape[0] * (wqkv.shape[0] * wqkv.shape[1] + wo.shape[0] * wo.shape[1])))
            return out

        def tqa(x, wqkv, bqkv=None, **kw):
            # the qkv projection + temporal attention launch of levels 1-3 (tc_temporal_qkv_attn, ABI 13): counted with the
            # family at the FLOPs of the projection it contains and at its WHOLE duration (the attentions included)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = self.orig_tqa(x, wqkv, bqkv, **kw)
            e1.record()
            self.rec.append((e0, e1, 2.0 * x.shape[0] * wqkv.shape[0] * wqkv.shape[1]))
            return out

        def gemm(a, w, bias=None, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = self.orig(a, w, bias, **kw)
            e1.record()
            out = res[0] if isinstance(res, tuple) else res          # gn_stats=True: (out, partial GroupNorm sums)
            conv = kw.get("conv")
            m = out.shape[0] if conv is None and kw.get("m") is None else (kw.get("m") or out.shape[0])
            self.rec.append((e0, e1, 2.0 * m * w.shape[0] * w.shape[1] * kw.get("batch", 1)))
            return res
        self.b.gemm = gemm
        if self.orig_ff is not None:
            self.b.ff_geglu_fused = ff
        if self.orig_tb is not None:
            self.b.temporal_attn_fused = tb
        if self.orig_tqa is not None:
            self.b.temporal_qkv_attn = tqa
        return self

    def __exit__(self, *a):
        self.b.gemm = self.orig
        if self.orig_ff is not None:
            self.b.ff_geglu_fused = self.orig_ff
        if self.orig_tb is not None:
            self.b.temporal_attn_fused = self.orig_tb
        if self.orig_tqa is not None:
            self.b.temporal_qkv_attn = self.orig_tqa

    def summary(self):
        torch.cuda.synchronize()
        ms = sum(e0.elapsed_time(e1) for e0, e1, _ in self.rec)
        fl = sum(f for _, _, f in self.rec)
        return len(self.rec), ms, fl


class NormProbe:
    """Brackets every tc_groupnorm call (its three launches) with HIP events; algorithmic bytes = 2 B read +
    2 B written per element."""

    def __init__(self, backend):
        self.b, self.orig, self.rec = backend, backend.groupnorm, []

    def __enter__(self):
        def groupnorm(x, *a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = self.orig(x, *a, **kw)
            e1.record()
            self.rec.append((e0, e1, 4.0 * x.numel()))
            # ABI 12: consumer weights this launch streams into the Infinity Cache beside its own work (ops.prefetch_list)
            pfl = self.b.prefetch_list(x.shape[0] if x.dim() == 2 else x.numel() // x.shape[-1], kw.get("prefetch")) \
                if hasattr(self.b, "prefetch_list") else []
            self.pf.append(sum(t.numel() * t.element_size() for t in pfl))
            return out
        self.pf = []
        self.b.groupnorm = groupnorm
        return self

    def __exit__(self, *a):
        self.b.groupnorm = self.orig

    def summary(self):
        torch.cuda.synchronize()
        return len(self.rec), sum(e0.elapsed_time(e1) for e0, e1, _ in self.rec), sum(f for _, _, f in self.rec)


PEAK_HBM_GBS = 8000.0          # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md


def guided_forward(model, inp):
    """The B = 2 (cond + uncond) UNet call of one DDIM step exactly as `apply_model_multi` issues it: with the shared
    prefix (lvdm/common.py: CfgShare) the latent-side inputs are handed over ONCE and `replicas=2`."""
    un = model.model.diffusion_model
    n = 1 if getattr(model, "cfg_share", False) else 2
    x, cc = torch.cat([inp["x_T"]] * n), torch.cat([inp["c_concat"]] * n)
    ctx2 = torch.cat([inp["cond"], inp["uncond"]])
    ts = torch.full((n,), 499, device=x.device, dtype=torch.long)
    fs = torch.cat([inp["fs"]] * n)
    return lambda: un(None, ts, context=ctx2, fs=fs, x_parts=[x, cc], replicas=2 if n == 1 else 1)


def measure_roofline_hbm(model, inp):
    fwd = guided_forward(model, inp)
    x2 = inp["x_T"]
    with torch.no_grad():
        fwd()
        torch.cuda.synchronize()
        big = torch.empty((8192, 8192), device=x2.device, dtype=torch.bfloat16).normal_()
        for _ in range(6):
            big @ big
        with NormProbe(ops.backend()) as probe:
            fwd()
        n, ms, by = probe.summary()
        pf_launches, pf_bytes = sum(1 for b in probe.pf if b), float(sum(probe.pf))
        # the same norms WITHOUT the weight-prefetch planes (ABI 12) riding on them: what the norm alone costs
        hipb = ops.backend()
        ms_plain = None
        if getattr(hipb, "prefetch_on", False) and pf_launches:
            hipb.prefetch_on = False
            try:
                fwd()
                with NormProbe(hipb) as probe0:
                    fwd()
                _, ms_plain, _ = probe0.summary()
            finally:
                hipb.prefetch_on = True
        # the decoder's GroupNorms, separately: one eager 16-frame decode (60 norms over 128..512-channel activations)
        dec = model.first_stage_model.decoder
        z16 = torch.randn(1, 4, 16, 40, 64, device=x2.device)
        was = dec.use_hipgraph
        dec.use_hipgraph = False
        try:
            dec.decode_clip(z16, inp["refs"], scale=1.0 / 0.18215)
            torch.cuda.synchronize()
            with NormProbe(ops.backend()) as dprobe:
                dec.decode_clip(z16, inp["refs"], scale=1.0 / 0.18215)
            dn, dms, dby = dprobe.summary()
        finally:
            dec.use_hipgraph = was
    gbs = by / (ms * 1e-3) / 1e9
    dgbs = dby / (dms * 1e-3) / 1e9
    name, tj = _pmc_file("r06_pmc_gn_traffic.json", "r05_pmc_gn_traffic.json", "r04_pmc_gn_traffic.json", "r03_pmc_gn_traffic.json")
    traffic = round(tj["traffic_bytes_per_launch"]) if tj is not None else None
    return {"bound": "hbm", "kernel": "tc_groupnorm (GroupNorm32 + SiLU over channels-last rows)",
            "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
            "traffic": traffic,
            "traffic_source": None if tj is None else f"profiles/{name}: (2*FETCH_SIZE + WRITE_SIZE) per tc_groupnorm call "
                                                      "of a B=2 UNet forward; a committed counter run",
            "launches": n, "avg_launch_us": round(ms * 1e3 / max(n, 1), 2),
            "algorithmic_gb_per_unet_fwd_b2": round(by / 1e9, 3), "ms_per_unet_fwd_b2": round(ms, 3),
            "weight_prefetch": None if ms_plain is None else {
                "what": "ABI 12: extra blocks of the GroupNorm launches in front of the small-M GEMMs (UNet levels 2 / 3 / middle) "
                        "stream those GEMMs' weights into the Infinity Cache; `achieved` / `frac` above count the norms' OWN "
                        "algorithmic bytes over their duration WITH that stream riding along (the product path)",
                "launches_carrying_it": pf_launches, "weight_gb_per_unet_fwd_b2": round(pf_bytes / 1e9, 3),
                "ms_per_unet_fwd_b2_without": round(ms_plain, 3),
                "frac_without": round(by / (ms_plain * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                "achieved_incl_weight_stream": round((by + pf_bytes) / (ms * 1e-3) / 1e9, 1)},
            "decoder_16f": {"launches": dn, "ms_per_decode": round(dms, 3), "algorithmic_gb_per_decode": round(dby / 1e9, 3),
                            "achieved": round(dgbs, 1), "frac": round(dgbs / PEAK_HBM_GBS, 4)}}


def _measured(fn, *a):
    """A measurement taken beside the headline must never cost it: on an exception the field carries the error instead."""
    try:
        return fn(*a)
    except Exception as e:                                           # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"[:300]}


def _pmc_file(*names):
    pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    for name in names:
        tp = os.path.join(pdir, name)
        if os.path.exists(tp):
            with open(tp) as f:
                return name, json.load(f)
    return None, None


def measure_roofline(model, inp):
    """GEMM family (tc_gemm_bf16: every Linear / implicit-GEMM convolution launch) over ONE CLIP: 50 batched-CFG
    B=2 UNet forwards + the 16-frame decode + the 14-frame re-decode.  One forward and one of each decode are
    bracketed launch by launch with HIP events on the launch stream (eager, so that every launch is visible);
    the clip figure composes them with the unit counts (50, 1, 1)."""
    un = model.model.diffusion_model
    dec = model.first_stage_model.decoder
    x2 = torch.cat([inp["x_T"]] * 2)
    cc2 = torch.cat([inp["c_concat"]] * 2)
    ctx2 = torch.cat([inp["cond"], inp["uncond"]])
    ts = torch.full((2,), 499, device=x2.device, dtype=torch.long)
    fs2 = torch.cat([inp["fs"]] * 2)
    z16 = torch.randn(1, 4, 16, 40, 64, device=x2.device)
    z14 = z16[:, :, [i for i in range(16) if i not in (1, 14)]].contiguous()

    def head_start():       # give the host a head start so that event gaps are not launch-bound
        big = torch.empty((8192, 8192), device=x2.device, dtype=torch.bfloat16).normal_()
        for _ in range(6):
            big @ big

    def probe(fn):
        fn()                                                            # warm (context / reference K/V cached)
        torch.cuda.synchronize()
        head_start()
        with GemmProbe(ops.backend()) as pr:
            fn()
        return pr.summary()

    was = dec.use_hipgraph
    dec.use_hipgraph = False
    try:
        with torch.no_grad():
            n_f, ms_f, fl_f = probe(guided_forward(model, inp))
            n_16, ms_16, fl_16 = probe(lambda: dec.decode_clip(z16, inp["refs"], scale=1.0 / 0.18215))
            n_14, ms_14, fl_14 = probe(lambda: dec.decode_clip(z14, inp["refs"], scale=1.0 / 0.18215))
    finally:
        dec.use_hipgraph = was
    n = 50 * n_f + n_16 + n_14
    ms = 50 * ms_f + ms_16 + ms_14
    fl = 50 * fl_f + fl_16 + fl_14
    achieved = fl / (ms * 1e-3) / 1e12
    unet_tfs = fl_f / (ms_f * 1e-3) / 1e12
    dec_tfs = (fl_16 + fl_14) / ((ms_16 + ms_14) * 1e-3) / 1e12
    # HBM-side bytes per launch come from a separate rocprofv3 --pmc run of the same forward (counters cannot
    # be read from inside this process); the committed summary of that run is quoted with its provenance
    traffic, traffic_src = None, None
    name, tj = _pmc_file("r06_pmc_unet_traffic.json", "r05_pmc_unet_traffic.json", "r04_pmc_unet_traffic.json", "r03_pmc_unet_traffic.json", "r02_pmc_unet_traffic.json", "r01_v6_pmc_unet_traffic.json")
    if tj is not None:
        traffic = round(tj["traffic_bytes_per_launch"])
        traffic_src = (f"profiles/{name}: (2*FETCH_SIZE + WRITE_SIZE) per tc_gemm_bf16 launch of a B=2 UNet forward, bytes; "
                       "L2-miss (fabric) traffic incl. Infinity-Cache hits; %.1f GB per B=2 forward vs %.1f GB algorithmic; "
                       "a committed counter run, not measured in this process"
                       % (tj["traffic_bytes_per_forward"] / 1e9, tj.get("algorithmic_bytes_per_b2_forward", 43.2e9) / 1e9))
    return {"bound": "mfma", "kernel": "tc_gemm_bf16 family (gemm_kernel / gemm16 / gemm_wide / gemm_ws / gemm8: Linear and "
                                       "implicit-GEMM convolutions, all gather modes; tc_ff_geglu_fused / tc_temporal_attn_fused / tc_temporal_qkv_attn counted at the "
                                       "FLOPs of the projections each contains and at its whole duration), UNet + decoder launches of one clip",
            "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_src,
            "launches": n, "avg_launch_us": round(ms * 1e3 / max(n, 1), 2),
            "composition": "50 x (B=2 UNet forward) + decode 16f + decode 14f",
            "algorithmic_tflop_per_clip_gemm": round(fl / 1e12, 2), "gemm_ms_per_clip": round(ms, 1),
            "unet": {"launches": n_f, "algorithmic_tflop_per_unet_fwd_b2": round(fl_f / 1e12, 3),
                     "gemm_ms_per_unet_fwd_b2": round(ms_f, 3), "achieved": round(unet_tfs, 2),
                     "frac": round(unet_tfs / PEAK_BF16_TFLOPS, 4)},
            "decoder": {"launches": n_16 + n_14, "algorithmic_tflop_16f_plus_14f": round((fl_16 + fl_14) / 1e12, 3),
                        "gemm_ms_16f_plus_14f": round(ms_16 + ms_14, 3), "achieved": round(dec_tfs, 2),
                        "frac": round(dec_tfs / PEAK_BF16_TFLOPS, 4)}}


CALIB_REFERENCE = {"matmul_8192_bf16_tflops": 1200.0, "copy_1gib_gbs": 5200.0}      # the middle of what round 5's leases measured (1180-1241, 5080-5260)


def lease_calibration(device):
    """What THIS lease delivers on two fixed yardsticks, measured in-process right where it is called (bench.py calls it
    before and after the timed region): (i) a hipBLASLt 8192^3 bf16 product (torch.matmul -- calibration only, never on the
    product path), (ii) a 1 GiB device-to-device copy.  Leases of this pool differ by +-12 % on the same binary (docs/LAB_NOTEBOOK.md
    5.2, 5.5); these two numbers travel with the headline so that rounds can be compared: `value_normalised` =
    value x (reference matmul rate / measured matmul rate), the reference being a fixed constant (CALIB_REFERENCE)."""
    a = torch.empty((8192, 8192), device=device, dtype=torch.bfloat16).normal_()
    b = torch.empty((8192, 8192), device=device, dtype=torch.bfloat16).normal_()
    src = torch.empty(1 << 30, device=device, dtype=torch.uint8)
    dst = torch.empty_like(src)
    for _ in range(4):
        a @ b
    dst.copy_(src)
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    for _ in range(12):
        a @ b
    e[1].record()
    e[2].record()
    for _ in range(6):
        dst.copy_(src)
    e[3].record()
    torch.cuda.synchronize()
    mm = 12 * 2.0 * 8192 ** 3 / (e[0].elapsed_time(e[1]) * 1e-3) / 1e12
    cp = 6 * 2.0 * (1 << 30) / (e[2].elapsed_time(e[3]) * 1e-3) / 1e9
    return {"matmul_8192_bf16_tflops": round(mm, 1), "copy_1gib_gbs": round(cp, 1)}


def rocm_eager_baseline(model, inp):
    """SURVEY.md 8(d)'s secondary baseline: the reference's ARITHMETIC as plain PyTorch-ROCm eager code under
    torch.autocast(bfloat16) on this GPU (the reference itself runs under fp16 autocast, scripts/evaluation/inference.py:323;
    /root/reference does not exist on the GPU box, so the code that runs is oracle/ -- equal to the reference to 1e-5 by the
    committed checks tests/golden/check_fullsize_vs_reference.py / check_ddim50_vs_reference.py).  Bounded sample: 2 guided
    DDIM steps = 4 B=1 UNet forwards, and one 16-frame decode; one clip = 100 forwards + (16 + 14) / 16 decodes."""
    from oracle import decoder as odec
    from oracle import unet as ounet
    dev = inp["x_T"].device
    un, dec = model.model.diffusion_model, model.first_stage_model.decoder
    usd = {k: v.detach().float() for k, v in un.state_dict().items()}
    dsd = {k: v.detach().float() for k, v in dec.state_dict().items()}
    x = torch.cat([inp["x_T"], inp["c_concat"]], 1)
    ts = torch.tensor([499], device=dev)
    z = torch.randn(1, 4, 16, 40, 64, device=dev)

    def fwd(c):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return ounet.unet_forward(usd, UNET_CFG, x, ts, c, inp["fs"])

    def decode():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return odec.decode_first_stage(dsd, z, inp["refs"])
    with torch.no_grad():
        fwd(inp["cond"])                                   # warm: MIOpen / hipBLASLt solution selection
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            fwd(inp["cond"])
            fwd(inp["uncond"])
        torch.cuda.synchronize()
        t_fwd = (time.perf_counter() - t0) / 4
        decode()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        decode()
        torch.cuda.synchronize()
        t_dec = time.perf_counter() - t1
    clip_s = 100.0 * t_fwd + (16 + 14) / 16.0 * t_dec
    return {"value": round(16.0 / clip_s, 4), "unit": "frames/s", "kind": "oracle code (== reference arithmetic to 1e-5), PyTorch-ROCm eager, "
            "torch.autocast(bfloat16), same GPU", "unet_fwd_b1_ms": round(t_fwd * 1e3, 1), "decode_16f_ms": round(t_dec * 1e3, 1),
            "sample": "4 B=1 UNet forwards (2 guided DDIM steps) + one 16-frame decode; one clip = 100 forwards + 30/16 decodes"}


def other_binding_clip(args):
    """The headline runs on the binding BASELINE.json's north_star names -- PyTorch-ROCm custom ops (TORCH_LIBRARY(tooncrafter),
    csrc/torch_ops.cpp; the default since round 5).  This times the OTHER binding over the same C ABI (ctypes; or the custom ops
    if the headline ran under TC_BINDING=ctypes) on the same workload in a CHILD process (the binding is chosen when the operator
    backend is created): 2 timed clips after 1 warm-up, default flags otherwise."""
    import subprocess
    other = "ctypes" if getattr(ops.backend(), "binding", "ctypes") == "torch" else "torch"
    env = dict(os.environ, TC_BINDING=other)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.abspath(__file__), "--steps", "2", "--warmup", "1", "--ddim-steps", str(args.ddim_steps),
           "--full", "--no-cpu-baseline", "--no-roofline", "--no-extras"] + (["--fp8"] if args.fp8 else [])
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": f"rc {r.returncode}", "stderr_tail": r.stderr[-400:]}
        d = json.loads(line[-1])
        return {"binding": d.get("binding", other), "value": d["value"], "unit": d["unit"], "steps": d["steps"],
                "ms_per_step": d["ms_per_step"], "lease_calibration": d.get("lease_calibration", {}).get("after_timed_region")}
    except Exception as e:                                       # noqa: BLE001  (an extra must never cost the headline)
        return {"error": f"{type(e).__name__}: {e}"}


def host_handover(device, ms_per_clip):
    """What a caller that starts from HOST buffers adds to a clip: the two endpoint frames in (fp32 [1, 3, 2, 320, 512],
    pageable, like the reference's `videos.to("cuda")`, inference.py:223) and the uint8 clip out ([1, 16, 320, 512, 3],
    the f4 output path).  `value` is quoted with inputs resident in HBM; this is the PCIe-inclusive figure beside it."""
    try:
        frames = torch.randn(1, 3, 2, 320, 512)
        clip = torch.zeros((1, 16, 320, 512, 3), dtype=torch.uint8, device=device)

        def wall(fn, reps=5):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3
        h2d, d2h = wall(lambda: frames.to(device)), wall(lambda: clip.cpu())
        return {"frames_in_h2d_ms": round(h2d, 3), "clip_u8_out_d2h_ms": round(d2h, 3),
                "bytes_in": frames.numel() * 4, "bytes_out": clip.numel(),
                "frames_per_s_pcie_inclusive": round(16.0 / ((ms_per_clip + h2d + d2h) * 1e-3), 4)}
    except Exception as e:                                       # noqa: BLE001  (an extra must never cost the headline)
        return {"error": f"{type(e).__name__}: {e}"[:300]}


def measure_boundary(model, inp):
    """The boundary question (ctypes + hipGraph vs a per-op extension): wall time of ONE B=2 UNet forward and of
    ONE 16-frame decode, launched eagerly through ctypes (~1130 / ~1000 launches, host-paced) and as a hipGraph
    replay (one host call).  The product path always replays; the eager figures price what a lower-overhead
    per-op binding (TORCH_LIBRARY) could at most recover if the graphs did not exist."""
    un, dec = model.model.diffusion_model, model.first_stage_model.decoder
    x2, cc2 = torch.cat([inp["x_T"]] * 2), torch.cat([inp["c_concat"]] * 2)
    ctx2, fs2 = torch.cat([inp["cond"], inp["uncond"]]), torch.cat([inp["fs"]] * 2)
    ts = torch.full((2,), 499, device=x2.device, dtype=torch.long)
    z = torch.randn(1, 4, 16, 40, 64, device=x2.device)

    def wall(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    out = {}
    with torch.no_grad():
        un_fwd = guided_forward(model, inp)
        out["unet_fwd_b2_eager_ms"] = round(wall(un_fwd), 2)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            un_fwd()
        out["unet_fwd_b2_graph_ms"] = round(wall(g.replay), 2)
        was = dec.use_hipgraph
        dec.use_hipgraph = False
        out["decode_16f_eager_ms"] = round(wall(lambda: dec.decode_clip(z, inp["refs"], scale=1.0 / 0.18215), reps=2), 2)
        dec.use_hipgraph = was
        out["decode_16f_graph_ms"] = round(wall(lambda: dec.decode_clip(z, inp["refs"], scale=1.0 / 0.18215), reps=2), 2)
    return out


def cpu_baseline(model, inp):
    """Time the CPU oracle on ONE full-size UNet forward (the unit 94 % of the clip consists of) and
    compare its output with the HIP path on identical weights and inputs."""
    from oracle import unet as ounet
    un = model.model.diffusion_model
    t0 = time.time()
    torch.set_num_threads(min(64, os.cpu_count() or 1))
    sd = {k: v.detach().float().cpu() for k, v in un.state_dict().items()}
    x = torch.cat([inp["x_T"], inp["c_concat"]], 1).cpu()
    ts = torch.tensor([499])
    with torch.no_grad():
        t1 = time.time()
        y = ounet.unet_forward(sd, UNET_CFG, x, ts, inp["cond"].cpu(), inp["fs"].cpu())
        t_fwd = time.time() - t1
        yg = un(x.to(inp["x_T"].device), ts.to(inp["x_T"].device), context=inp["cond"], fs=inp["fs"])
        # decoder sample: 4 of the clip's frames at full resolution (cost is linear in frames)
        from oracle import decoder as odec
        dec = model.first_stage_model.decoder
        dsd = {k: v.detach().float().cpu() for k, v in dec.state_dict().items()}
        z4 = torch.randn(1, 4, 4, 40, 64, generator=torch.Generator().manual_seed(11))
        refs_cpu = [r.cpu() for r in inp["refs"]]
        t2 = time.time()
        d = odec.decode_first_stage(dsd, z4, refs_cpu)
        t_dec4 = time.time() - t2
        dg = dec.decode_clip(z4.to(inp["x_T"].device), inp["refs"], scale=1.0 / 0.18215)
    rel = float((yg.double().cpu() - y.double()).norm() / y.double().norm())
    rel_dec = float((dg.double().cpu() - d.double()).norm() / d.double().norm())
    clip_s = 100.0 * t_fwd + (16 + 14) / 4.0 * t_dec4
    return {"value": round(16.0 / clip_s, 6), "unit": "frames/s", "cores": torch.get_num_threads(),
            "host_cpus": os.cpu_count(), "kind": "port",
            "note": "the code timed is oracle/ (the reference tree does not travel to the GPU box); oracle == real reference to "
                    "6.7e-6 at full size and 1.3e-5 over DDIM-50 (committed checks: tests/golden/check_fullsize_vs_reference.py, "
                    "check_ddim50_vs_reference.py; profiles/r03_fullsize_golden_vs_reference.txt, r04_ddim50_oracle_vs_reference.txt)",
            "sample": f"fp32 CPU oracle: 1 full-size UNet forward (B=1, 12.603 TFLOP) {t_fwd:.1f} s + a 4-frame "
                      f"full-resolution decode {t_dec4:.1f} s; one clip = 100 forwards + (16+14)/4 such decodes",
            "unet_fwd_s": round(t_fwd, 2), "decode_4f_s": round(t_dec4, 2),
            "parity_rel_l2_hip_vs_oracle_full_size": round(rel, 5),
            "parity_rel_l2_hip_vs_oracle_decode_4f": round(rel_dec, 5), "prep_s": round(t1 - t0, 1)}


def run_clips_batched_decode(model, sampler, inps, ddim_steps):
    """BASELINE.json configs[3] (perframe_ae=False): B clips sampled one after the other (batch 1, the scripts
    assert bs == 1, inference.py:296), then ALL B*T frames through ONE decoder call with timesteps=T --
    the call the reference crashes on (ddpm3d.py:656-657) and the only geometry in which the dual-reference
    fusion indexes its per-clip K/V correctly for B > 1."""
    lat = []
    for inp in inps:
        cond = {"c_crossattn": [inp["cond"]], "c_concat": [inp["c_concat"]]}
        uc = {"c_crossattn": [inp["uncond"]], "c_concat": [inp["c_concat"]]}
        s, _ = sampler.sample(S=ddim_steps, conditioning=cond, batch_size=1, shape=(4, 16, 40, 64), verbose=False,
                              unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0, fs=inp["fs"],
                              timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=inp["x_T"])
        lat.append(s)
    samples = torch.cat(lat, 0)
    refs = inps[0]["refs_batched"]
    video = model.decode_first_stage(samples, ref_context=refs)
    idx = [i for i in range(samples.shape[2]) if i not in (1, samples.shape[2] - 2)]
    video2 = model.decode_first_stage(samples[:, :, idx].contiguous(), ref_context=refs)
    mid = video2.shape[2] // 2
    video[:, :, 7:9] = video2[:, :, mid - 1:mid + 1]
    return video


def rank_evidence(device, rank, local, world, clip_u8, gather_buf):
    """What a reader of the JSON line can check about the N-rank run without trusting it: every rank reports the GPU
    it really ran on (UUID / PCI address from the driver, host name) and a checksum of the LAST clip it produced; rank 0
    recomputes the checksums from the buffers the RCCL gather filled and times one more gather by itself.  All of it
    after the timed region.  At N = 1 the same keys are filled from the single rank (no collective)."""
    import socket
    props = torch.cuda.get_device_properties(device)
    me = {"rank": rank, "local_rank": local, "host": socket.gethostname(), "name": props.name,
          "uuid": str(getattr(props, "uuid", "")),
          "pci": "%04x:%02x:%02x" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", 0), getattr(props, "pci_device_id", 0)),
          "clip_checksum": int(clip_u8.to(torch.int64).sum().item())}
    if world == 1:
        return {"ranks_seen": 1, "devices": [me], "gather_verified": None, "gather_ms": None}
    everyone = [None] * world
    dist.all_gather_object(everyone, me)
    from tooncrafter_amd import dist as tcdist
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    tcdist.gather_clips(clip_u8, dst=0, out=gather_buf)
    torch.cuda.synchronize()
    gather_ms = (time.perf_counter() - t0) * 1e3
    if rank != 0:
        return {}
    seen = [int(b.to(torch.int64).sum().item()) for b in gather_buf]
    return {"ranks_seen": len({(d["host"], d["uuid"] or d["pci"]) for d in everyone}), "devices": everyone,
            "gather_verified": seen == [d["clip_checksum"] for d in everyone],
            "gather_ms": round(gather_ms, 3), "gather_bytes_per_rank": int(clip_u8.numel())}


def self_launch(args):
    """`python bench.py --gpus N` outside torchrun: start the N ranks ourselves, one process per GPU over
    RCCL on 127.0.0.1 (the analogue of the reference's scripts/evaluation/ddp_wrapper.py:29-47)."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < args.gpus and not args.launcher_selftest:
        # fail LOUDLY before any rendezvous: N ranks on fewer than N devices would otherwise sit in RCCL's init timeout
        sys.stderr.write(f"bench.py --gpus {args.gpus}: this box exposes {have} GPU(s); refusing to start {args.gpus} ranks\n")
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def supervise(args):
    """`--retry` only (off by default: a fault in the default run is a FAILED run, exit code and stderr intact).
    The measurement runs in a child process; if that process dies WITHOUT a result, scripts/gpu_health.py (plain
    PyTorch, none of this repo's code loaded) decides: box unhealthy -> the identical measurement is started again
    in a fresh process (up to three attempts); box healthy -> the failure is the code's, it is reported with the
    child's stderr and NOT retried.  A result from attempt > 1 carries `attempts` and `flagged`."""
    import subprocess
    argv = [a for a in sys.argv[1:] if a != "--retry"]
    for attempt in (1, 2, 3):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode == 0 and lines:
            d = json.loads(lines[-1])
            d["attempts"] = attempt
            if attempt > 1:
                d["flagged"] = f"{attempt - 1} earlier attempt(s) died on a lease whose plain-PyTorch health check also failed"
            print(json.dumps(d))
            return 0
        sys.stderr.write(f"[bench] attempt {attempt} ended with exit code {r.returncode} without a result\n")
        sys.stderr.write(r.stderr[-3000:])
        hc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gpu_health.py")], capture_output=True, text=True)
        if hc.returncode == 0:
            sys.stderr.write("[bench] scripts/gpu_health.py PASSES on this lease: the failure is this code's, not retried. "
                             "Re-run with TC_DEBUG_SYNC=1 to name the faulting entry point.\n")
            return r.returncode or 1
        sys.stderr.write("[bench] scripts/gpu_health.py also fails on this lease (box unhealthy): retrying\n")
    return 1


def launcher_selftest(args):
    """CPU check of the launcher + rendezvous + gather plumbing (tests/test_dist_cpu.py): every rank
    contributes one small 'clip', rank 0 gathers and prints the JSON line.  No GPU, gloo backend."""
    from tooncrafter_amd import dist as tcdist
    rank, world = tcdist.init(backend="gloo")
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    clip = torch.full((1, 3, 2, 4, 4), float(rank))
    got = tcdist.gather_clips(clip, dst=0)
    if world > 1:
        dist.barrier()
    if rank == 0:
        print(json.dumps({"selftest": "launcher", "n_gpus": world,
                          "gathered": [float(g.mean()) for g in got]}))
    if world > 1:
        dist.destroy_process_group()


DUMP_BYTES_PER_ARRAY = 30 << 20    # two arrays stay under 64 MB in all; one (1, 3, 16, 320, 512) fp32 clip is exactly this
NOISE_SEED = 20240607


def dump_outputs(out_dir, arrays):
    """Write each tensor as out_dir/<name>.npy in float32; one larger than DUMP_BYTES_PER_ARRAY becomes a fixed
    sample of its flattened elements (indices from a seeded generator, ascending), the same on every run."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().float()
        if a.numel() * 4 > DUMP_BYTES_PER_ARRAY:
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_BYTES_PER_ARRAY // 4]
            a = a.flatten()[idx.sort().values.to(a.device)]
        np.save(os.path.join(out_dir, name + ".npy"), a.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--batched-decode", type=int, default=0, metavar="B",
                    help="configs[3]: B clips per GPU per step, decoded in one call (perframe_ae=False)")
    ap.add_argument("--fp8", action="store_true",
                    help="configs[4]: MXFP8 (e4m3 + E8M0 block scales) operands on the qkv / GEGLU projections (TC_FP8=1; "
                         "export TC_FP8=all to add the convolutions)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure the lease calibration, per-rank evidence, encoder, roofline, "
                         "boundary, host handover, ROCm-eager baseline, other binding and CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline / boundary / handover probes")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the after-the-fact extras (ROCm-eager baseline, two clips through the other binding)")
    ap.add_argument("--launcher-selftest", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--retry", action="store_true",
                    help="supervise the run in a child process and repeat it ONLY if the lease itself is unhealthy "
                         "(scripts/gpu_health.py fails); off by default")
    ap.add_argument("--no-retry", action="store_true", help=argparse.SUPPRESS)      # accepted for old command lines
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.fp8:
        os.environ["TC_FP8"] = os.environ.get("TC_FP8", "1")      # read when the operator backend is created
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if args.launcher_selftest:
        return launcher_selftest(args)
    if args.retry and args.gpus == 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(supervise(args))

    from tooncrafter_amd import dist as tcdist
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if local >= torch.cuda.device_count():
        sys.exit(f"bench.py: LOCAL_RANK={local} but this box exposes {torch.cuda.device_count()} GPU(s) -- one process per GPU")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    rank, world = tcdist.init(backend="nccl", device=device)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert ops.backend().name == "hip"

    from tooncrafter_amd.lvdm.ddim import DDIMSampler
    model = build_model(device)
    sampler = DDIMSampler(model)
    bdec = args.batched_decode
    clips_per_step = bdec if bdec > 0 else 1
    # two resident input sets per rank: consecutive steps run DIFFERENT clips (per-clip refresh is timed)
    n_sets = 2 * clips_per_step
    inps = [make_inputs(device, seed=7 + rank + 1000 * j) for j in range(n_sets)]
    if bdec > 0:
        for j in (0, bdec):
            inps[j]["refs_batched"] = [torch.cat([inps[j + i]["refs"][l] for i in range(bdec)], 0) for l in range(5)]
    # what leaves a GPU is the writer-side uint8 clip (inference.py:146-153 on the device, tc_video_to_u8): 7.9 MB per
    # clip over xGMI instead of 31.5 MB fp32.  Every rank converts, also at N = 1 (equal work per GPU at every N).
    from tooncrafter_amd import output as tcout
    shape = (clips_per_step, 16, 320, 512, 3)
    gather_buf = [torch.empty(shape, device=device, dtype=torch.uint8) for _ in range(world)] \
        if rank == 0 and world > 1 else None
    counter = [0]
    last_u8 = [None]

    def step():
        k = counter[0] % 2
        counter[0] += 1
        with torch.no_grad():
            if bdec > 0:
                video = run_clips_batched_decode(model, sampler, inps[k * bdec:(k + 1) * bdec], args.ddim_steps)
            else:
                video = run_clip(model, sampler, inps[k], args.ddim_steps)
            frames_u8 = tcout.clip_to_uint8(video)                       # (b, T, H, W, 3) uint8, on the device
            last_u8[0] = frames_u8
            tcdist.gather_clips(frames_u8, dst=0, out=gather_buf)       # the one collective of the path
        return video

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    _log("model built")
    def calibrate():
        try:
            return lease_calibration(device)
        except Exception as e:                                           # noqa: BLE001  (calibration only: never fatal)
            return {"matmul_8192_bf16_tflops": None, "copy_1gib_gbs": None, "error": f"{type(e).__name__}: {e}"[:200]}
    calib_pre = calibrate() if rank == 0 and args.full else None
    torch.manual_seed(NOISE_SEED + rank)                                 # the DDIM noise (eta = 1) of every step
    for _ in range(args.warmup):
        step()
        _log("warmup step done")
    fence()
    STAGE_EVENTS.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        video = step()
    fence()
    _log("timed steps done")
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    finite = bool(torch.isfinite(video).all())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"video": video, "frames_u8": last_u8[0]})
    calib_post = calibrate() if rank == 0 and args.full else None
    evidence = rank_evidence(device, rank, local, world, last_u8[0], gather_buf) if args.full else {}

    result = None
    if rank == 0:
        frames = 16 * args.steps * world * clips_per_step
        result = {
            "metric": "interpolated frames/sec, 512x320x16f DDIM-50", "value": round(frames / dt, 4),
            "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if not args.fp8 else "fp8 e4m3 with E8M0 block scales (MXFP8) on the eligible GEMM operands, fp32 accumulate; bf16 elsewhere",
            "data": "synthetic",
            "config": {"workload": ("ToonCrafter_512 320x512x16f ddim_steps=%d CFG 7.5 bf16, %s; sampler + 16f decode "
                                    "+ 14f re-decode + splice; a different clip every step") % (
                                        args.ddim_steps,
                                        "1 clip per GPU, MXFP8 GEMM path (BASELINE.json configs[4])" if args.fp8 and bdec == 0 else
                                        "1 clip per GPU (BASELINE.json configs[1])" if bdec == 0 else
                                        f"{bdec} clips per GPU through one decode_first_stage call, perframe_ae=False (BASELINE.json configs[3]; grouped so that no activation exceeds 2 GiB)"),
                       "clips_per_step": world * clips_per_step,
                       "parallelism": f"dp{world} (independent clips, one RCCL gather)"},
            "effective_tflops_per_gpu": round(TFLOP_CLIP * args.steps * clips_per_step / dt, 1) if args.ddim_steps == 50 else None,
            "mfma_fraction_whole_clip": round(TFLOP_CLIP * args.steps * clips_per_step / dt / PEAK_BF16_TFLOPS, 4)
            if args.ddim_steps == 50 else None,
            "output_finite": finite,
            "binding": ("torch.ops.tooncrafter (TORCH_LIBRARY custom ops over the C ABI)" if getattr(ops.backend(), "binding", "ctypes") == "torch"
                        else "ctypes over the C ABI"),
            "binding_fallback": ops.binding_fallback(),        # None, or why the default custom-op layer was not taken
            **evidence,
        }
        if args.full:
            mms = [c["matmul_8192_bf16_tflops"] for c in (calib_pre, calib_post) if c.get("matmul_8192_bf16_tflops")]
            mm = sum(mms) / len(mms) if mms else None
            result["lease_calibration"] = {"before_timed_region": calib_pre, "after_timed_region": calib_post, "reference": CALIB_REFERENCE,
                                           "what": "hipBLASLt 8192^3 bf16 (torch.matmul) and a 1 GiB d2d copy, measured in this process on "
                                                   "rank 0; calibration only, not on the product path"}
            result["value_normalised"] = round(result["value"] * CALIB_REFERENCE["matmul_8192_bf16_tflops"] / mm, 4) if mm else None
        if args.fp8:
            result["fp8_gemm_calls"] = dict(ops.backend().fp8_calls)
        if STAGE_EVENTS:
            acc = {}
            for name, a, b in STAGE_EVENTS:
                acc[name] = acc.get(name, 0.0) + a.elapsed_time(b)
            result["stage_ms_per_clip"] = {k: round(v / args.steps, 2) for k, v in acc.items()}
    if world > 1:
        # the measurement is over: release the other ranks now -- what follows (encoder timing, roofline probes) is
        # rank 0 alone and must not sit inside anybody's collective timeout
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and args.full:
        # row f1 (not part of `value`): the first-stage encoder that produces z and the reference
        # hidden states, 16 frames at 320x512, reported so that "with encoder" can be derived
        frames = torch.rand((16, 3, 320, 512), device=device) * 2 - 1
        with torch.no_grad():
            model.first_stage_model.encode(frames, return_hidden_states=True)
            torch.cuda.synchronize()
            te = time.perf_counter()
            model.first_stage_model.encode(frames, return_hidden_states=True)
            torch.cuda.synchronize()
        enc_ms = (time.perf_counter() - te) * 1e3
        result["encoder_16f_ms"] = round(enc_ms, 2)
        _log("encoder done")
        result["frames_per_s_with_encoder"] = round(16.0 / (dt / args.steps / clips_per_step + enc_ms * 1e-3), 4)
    if rank == 0 and args.full and not args.no_roofline:
        result["roofline"] = _measured(measure_roofline, model, inps[0])
        if args.fp8 and "error" not in result["roofline"]:
            result["roofline"]["note"] = ("--fp8: the timed launches include the routed tc_gemm_mxfp8 ones; FLOPs are priced "
                                          "against the bf16 peak all the same (dense MX fp8 peak: ~4.66 PF/s measured)")
        _log("roofline done")
        result["roofline_hbm"] = _measured(measure_roofline_hbm, model, inps[0])
        _log("roofline_hbm done")
        result["boundary_host_overhead"] = _measured(measure_boundary, model, inps[0])
        _log("boundary done")
        result["host_handover"] = _measured(host_handover, device, dt / args.steps / clips_per_step * 1e3)
    if rank == 0 and world == 1 and args.full and not args.no_extras and bdec == 0:
        try:                                                         # an extra must never cost the headline
            result["rocm_eager_baseline"] = rocm_eager_baseline(model, inps[0])
        except Exception as e:                                       # noqa: BLE001
            result["rocm_eager_baseline"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        _log("rocm eager baseline done")
        result["binding_ab"] = other_binding_clip(args)
        _log("other binding clip done")
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        result["cpu_baseline"] = _measured(cpu_baseline, model, inps[0])
    if rank == 0:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
