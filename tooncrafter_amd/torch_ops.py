"""PyTorch-ROCm custom-op binding of the hot path: `torch.ops.tooncrafter.*` (csrc/torch_ops.cpp, TORCH_LIBRARY).

The same `extern "C"` entry points as the ctypes binding (ops.HipOps), registered as torch operators.  Each operator
is one C++ function under the CUDA(HIP) key and the Meta key: current-stream pickup and output allocation happen in
C++, and on the `meta` device the same function checks the request and infers the result without a GPU, so a trace
or export refuses what a launch would refuse.  `TorchLibOps` is a drop-in for `HipOps` and the default binding
(`ops.backend()`; `TC_BINDING=ctypes` selects the other, as does `ops.set_backend(HipOps())`).  Calls that use features
the functional op schema does not carry (an explicit `out=` buffer, batched GEMMs, accumulate) go through the
inherited ctypes methods.
"""
from __future__ import annotations

import os

import torch

from . import _lib
from ._lib import ACT_NONE
from .ops import HipOps, attn_scale

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libtooncrafter_torch.so")
_loaded = False


def load():
    """Register the `tooncrafter` operator namespace (idempotent).  Raises if the library is missing."""
    global _loaded
    if _loaded:
        return torch.ops.tooncrafter
    if not os.path.exists(LIB_PATH):
        raise _lib.TooncrafterHipError(f"{LIB_PATH} not found: build it with `python -m tooncrafter_amd.build`")
    torch.ops.load_library(LIB_PATH)
    got = int(torch.ops.tooncrafter.abi_version())
    if got != _lib.TC_ABI_VERSION:
        # fatal, not a reason to fall back to ctypes: the namespace is registered by now (TORCH_LIBRARY runs at dlopen), so
        # `torch.ops.tooncrafter.*` would resolve to the stale layer for anybody who calls it directly
        raise _lib.TooncrafterAbiError(f"{LIB_PATH} was built against ABI {got}, this tree is ABI {_lib.TC_ABI_VERSION}: "
                                       "rebuild with `python -m tooncrafter_amd.build`")
    _loaded = True
    return torch.ops.tooncrafter


def conv_list(conv):
    """ops.gemm's `conv` dict -> the 11-integer form of the op schema ([] = linear)."""
    if conv is None:
        return []
    return [1 if conv["kind"] == "3x3" else 2, conv["cin"], conv["frames"], conv.get("t_len", 1),
            conv.get("h_in", conv["h_out"]), conv.get("w_in", conv["w_out"]), conv["h_out"], conv["w_out"],
            conv.get("stride", 1), 1 if conv.get("upsample", False) else 0, conv.get("pad", 1)]


class TorchLibOps(HipOps):
    """HipOps with the arithmetic operators dispatched through `torch.ops.tooncrafter`."""

    name = "hip"          # the same kernels: callers that assert the HIP backend see it as such
    binding = "torch"

    def __init__(self):
        super().__init__()
        self.t = load()

    def gemm(self, a, w, bias=None, *, act=ACT_NONE, residual=None, row_bias=None, row_div=0, alpha=1.0, out_scale=1.0,
             out=None, out_f32=False, conv=None, batch=1, stride_a=0, stride_w=0, stride_c=0, m=None, a_norm_eps=None,
             gn_stats=False):
        # fp8 routing and the ABI 9 producer statistics (a second result; only when TC_GN_PART=1 can produce them) live in HipOps.gemm
        if out is not None or batch != 1 or m is not None or self.fp8 is not None or (gn_stats and self.gn_part):
            return super().gemm(a, w, bias, act=act, residual=residual, row_bias=row_bias, row_div=row_div, alpha=alpha,
                                out_scale=out_scale, out=out, out_f32=out_f32, conv=conv, batch=batch, stride_a=stride_a,
                                stride_w=stride_w, stride_c=stride_c, m=m, a_norm_eps=a_norm_eps, gn_stats=gn_stats)
        res = self.t.gemm(a, w, bias, residual, row_bias, int(row_div), int(act), float(alpha), float(out_scale),
                          bool(out_f32), conv_list(conv), -1.0 if a_norm_eps is None else float(a_norm_eps))
        return (res, None) if gn_stats else res                 # ResBlock / TemporalConvBlock always ask; no producer statistics here

    def quant_mxfp8(self, x, k=None):
        return self.t.quant_mxfp8(x, int(x.shape[1] if k is None else k))

    def attention(self, q, k, v, *, batch, heads, lq, lk, kv_bdiv=1, out=None, accumulate=False, scale=None,
                  k2=None, v2=None, lk2=0, kv2_bdiv=1):
        if out is not None or accumulate:
            return super().attention(q, k, v, batch=batch, heads=heads, lq=lq, lk=lk, kv_bdiv=kv_bdiv, out=out,
                                     accumulate=accumulate, scale=scale, k2=k2, v2=v2, lk2=lk2, kv2_bdiv=kv2_bdiv)
        return self.t.attention(q, k, v, batch, heads, lq, lk, kv_bdiv, attn_scale(scale),
                                k2, v2, int(lk2), int(kv2_bdiv))

    def attention_q8(self, q, k, v, *, batch, heads, lq, lk, scale=None):
        out = self.t.attention_q8(q, k, v, int(batch), int(heads), int(lq), int(lk), attn_scale(scale))
        self.fp8_calls["attn_q8"] += 1
        return out

    def attention_temporal(self, qkv, *, b, t, hw, heads, scale=None):
        return self.t.attention_temporal(qkv, b, t, hw, heads, attn_scale(scale))

    def attention_temporal_rel(self, qkv, rel_k, rel_v, *, b, t, hw, heads, max_rel, causal, scale=None):
        return self.t.attention_temporal_rel(qkv, rel_k, rel_v, int(b), int(t), int(hw), int(heads), int(max_rel), bool(causal),
                                             attn_scale(scale))

    def ff_geglu_fused(self, x, w1, b1, w2, b2, *, ln_eps=None):
        return self.t.ff_geglu_fused(x, w1, b1, w2, b2, -1.0 if ln_eps is None else float(ln_eps))

    def temporal_attn_fused(self, x, wqkv, bqkv, wo, bo, *, b, t, hw, heads, ln_eps=None, scale=None):
        return self.t.temporal_attn_fused(x, wqkv, bqkv, wo, bo, int(b), int(t), int(hw), int(heads),
                                          -1.0 if ln_eps is None else float(ln_eps), attn_scale(scale))

    def temporal_qkv_attn(self, x, wqkv, bqkv=None, *, b, t, hw, heads, scale=None, out=None):
        if out is not None:                                  # an explicit result buffer: the ctypes method (the op schema is functional)
            return super().temporal_qkv_attn(x, wqkv, bqkv, b=b, t=t, hw=hw, heads=heads, scale=scale, out=out)
        return self.t.temporal_qkv_attn(x, wqkv, bqkv, int(b), int(t), int(hw), int(heads), attn_scale(scale))

    def groupnorm(self, x, gamma, beta, *, samples, rows, eps, silu=False, part=None, prefetch=None, prefetch_linear=False):
        if part is not None:
            return super().groupnorm(x, gamma, beta, samples=samples, rows=rows, eps=eps, silu=silu, part=part, prefetch=prefetch,
                                     prefetch_linear=prefetch_linear)
        pfl = self.prefetch_list(x.shape[0], prefetch, linear=prefetch_linear)   # ABI 12: the consumer's weights ride on the launch
        if pfl:
            return self.t.groupnorm_pf(x, gamma, beta, samples, rows, float(eps), bool(silu), pfl)
        return self.t.groupnorm(x, gamma, beta, samples, rows, float(eps), bool(silu))

    def layernorm(self, x, gamma, beta, eps=1e-5, mx_for=None, prefetch=None):
        if mx_for is not None and self.fp8 is not None:
            return super().layernorm(x, gamma, beta, eps, mx_for=mx_for, prefetch=prefetch)
        pfl = self.prefetch_list(x.shape[0], prefetch, linear=True)
        if pfl:
            return self.t.layernorm_pf(x, gamma, beta, float(eps), pfl)
        return self.t.layernorm(x, gamma, beta, float(eps))

    def _step_op(self, what, parameterization, operands, want_x0, cfg_scale, cfg_img, *scalars):
        """`what` or its `_eps` form on `operands` and the step's nine scalars, which are marshalled here for every step."""
        if parameterization not in ("v", "eps"):
            raise NotImplementedError(f"{what}: parameterization {parameterization!r} (the fused step has 'v' and 'eps')")
        op = getattr(self.t, what if parameterization == "v" else what + "_eps")
        xp, x0 = op(*operands, float(cfg_scale), float(cfg_scale if cfg_img is None else cfg_img), *map(float, scalars))
        return xp, (x0 if want_x0 else None)

    def ddim_step(self, x, e_cond, e_uncond, noise, *, cfg_scale, guidance_rescale, sqrt_ac, sqrt_1m_ac, sqrt_a_prev,
                  dir_coef, sigma, x0_rescale, want_x0=True, e_uncond_img=None, cfg_img=None, parameterization="v"):
        return self._step_op("ddim_step", parameterization, (x, e_cond, e_uncond, noise, e_uncond_img), want_x0, cfg_scale, cfg_img,
                             guidance_rescale, sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef, sigma, x0_rescale)

    def ddim_step_ms(self, x, e_cond, e_uncond, noise, x0_hist, *, corr, cfg_scale, guidance_rescale, sqrt_ac, sqrt_1m_ac,
                     sqrt_a_prev, dir_coef, sigma, x0_rescale, want_x0=True, e_uncond_img=None, cfg_img=None,
                     parameterization="v", pred_x0=None):
        if pred_x0 is not None:                              # an explicit result buffer (the history in place): the ctypes method
            return super().ddim_step_ms(x, e_cond, e_uncond, noise, x0_hist, corr=corr, cfg_scale=cfg_scale,
                                        guidance_rescale=guidance_rescale, sqrt_ac=sqrt_ac, sqrt_1m_ac=sqrt_1m_ac,
                                        sqrt_a_prev=sqrt_a_prev, dir_coef=dir_coef, sigma=sigma, x0_rescale=x0_rescale,
                                        want_x0=want_x0, e_uncond_img=e_uncond_img, cfg_img=cfg_img,
                                        parameterization=parameterization, pred_x0=pred_x0)
        return self._step_op("ddim_step_ms", parameterization, (x, e_cond, e_uncond, noise, e_uncond_img, x0_hist, float(corr)),
                             want_x0, cfg_scale, cfg_img, guidance_rescale, sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef, sigma,
                             x0_rescale)

    def ddim_blend(self, x, x0, noise, mask, *, sqrt_ac=1.0, sqrt_1m_ac=0.0, out=None):
        if out is not None:                                 # an explicit result buffer (in place): the ctypes method
            return super().ddim_blend(x, x0, noise, mask, sqrt_ac=sqrt_ac, sqrt_1m_ac=sqrt_1m_ac, out=out)
        return self.t.ddim_blend(x, x0, noise, mask, float(sqrt_ac), float(sqrt_1m_ac))

    def frames_from_u8(self, images, size, slots, *, b, t, out=None):
        self._check_u8_images(images, "frames_from_u8: images")
        if out is not None or images.shape[0] > _lib.TC_FRAMES_U8_MAX:     # an explicit result buffer / several calls: the ctypes method
            return super().frames_from_u8(images, size, slots, b=b, t=t, out=out)
        (h, w), (sh, sw) = (int(v) for v in size), images.shape[1:3]
        return self.t.frames_from_u8(images, [int(s) for s in slots], int(b), int(t), h, w,
                                     *self._front_tables(sh, sw, h, w, images.device))

    def frames_from_yuv(self, planes, size, slots, *, b, t, out=None):
        lay, m, (h, w), slots, out = self._frames_yuv_args(planes, size, slots, b, t, out)
        if out is not None or lay["n"] > _lib.TC_FRAMES_U8_MAX:            # an explicit result buffer / several calls: the ctypes method
            return super().frames_from_yuv(planes, size, slots, b=b, t=t, out=out)
        c1 = planes.chroma[1] if len(planes.chroma) > 1 else None
        return self.t.frames_from_yuv(planes.y, planes.chroma[0], c1, lay["format"], m, _lib.TC_CHROMA_SITINGS[planes.siting], slots,
                                      int(b), int(t), h, w, *self._front_tables(lay["sh"], lay["sw"], h, w, planes.y.device))

    def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
        if out is not None or strides is not None:          # an explicit result buffer with its strides: the ctypes method
            return super().frames_to_u8(x, size, filter, fmt, frames, out=out, strides=strides)
        oh, ow, code, f0, nf, _, _ = self._frames_out_args(x, size, filter, fmt, frames)
        h, w = x.shape[3:]
        return self.t.frames_to_u8(x.contiguous(), oh, ow, code, f0, nf, *self._axis_tables(filter, w, ow, x.device),
                                   *self._axis_tables(filter, h, oh, x.device))

    def frames_to_yuv(self, x, size=None, filter="bicubic", fmt="nv12", colour=None, frames=None, out=None, strides=None):
        if out is not None or strides is not None:          # an explicit result buffer with its strides: the ctypes method
            return super().frames_to_yuv(x, size, filter, fmt, colour, frames, out=out, strides=strides)
        oh, ow, code, f0, nf, _, _, m, siting = self._frames_yuv_out_args(x, size, filter, fmt, colour, frames)
        h, w = x.shape[3:]
        return self.t.frames_to_yuv(x.contiguous(), oh, ow, code, f0, nf, siting, m, *self._axis_tables(filter, w, ow, x.device),
                                    *self._axis_tables(filter, h, oh, x.device))

    def colour_stats(self, x, frames=None):
        _, t, _, _ = self._colour_clip(x, "colour_stats: x")
        return self.t.colour_stats(x, *self._colour_frames(frames, t, "colour_stats"))

    def colour_match(self, x, src, ref, ref_pixels, method, strength, out=None, knots=None, max_gain=None):
        if out is not None:                                  # an explicit result buffer (in place): the ctypes method
            return super().colour_match(x, src, ref, ref_pixels, method, strength, out=out, knots=knots, max_gain=max_gain)
        _, knots, gain, code, strength, ref_pixels = self._colour_match_request(x, src, ref, ref_pixels, method, strength, knots, max_gain)
        if knots is None:
            return self.t.colour_match(x, src, ref, ref_pixels, code, strength)
        return self.t.colour_match_knots(x, src, ref, ref_pixels, code, strength, list(knots), gain)

    def colour_hist(self, x, frames=None):
        _, t, _, _ = self._colour_clip(x, "colour_hist: x")
        return self.t.colour_hist(x, *self._colour_frames(frames, t, "colour_hist"))

    def colour_transfer(self, x, src, ref, ref_pixels, strength, base=None, out=None, knots=None):
        if out is not None:                                  # an explicit result buffer (in place): the ctypes method
            return super().colour_transfer(x, src, ref, ref_pixels, strength, base=base, out=out, knots=knots)
        _, knots, strength, ref_pixels = self._colour_transfer_request(x, src, ref, ref_pixels, strength, base, knots)
        if knots is None:
            return self.t.colour_transfer(x, base, src, ref, ref_pixels, strength)
        return self.t.colour_transfer_knots(x, base, src, ref, ref_pixels, strength, list(knots))

    def clip_patches(self, x, *, size, patch, ld, mean, std, antialias=True):
        return self.t.clip_patches(x, int(size), int(patch), int(ld), [float(v) for v in mean], [float(v) for v in std], bool(antialias))

    def randn_clips(self, seeds, shape, stream, scale=1.0, out=None, raw=False):
        if out is not None:                                  # an explicit result buffer: the ctypes method
            return super().randn_clips(seeds, shape, stream, scale, out=out, raw=raw)
        seeds, shape, stream = self._randn_args(seeds, shape, stream)
        # the schema's int is an int64: a seed from 2^63 on goes over as its two's complement
        return self.t.randn_clips([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], list(shape), stream, float(scale), bool(raw))
