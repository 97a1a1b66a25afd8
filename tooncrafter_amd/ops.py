"""Tensor-level operators of the hot path, bound to the HIP C ABI.

PyTorch is plumbing here: it owns device memory (caching allocator, so outputs
are stream-ordered and hipGraph-capturable) and the current stream.  Every
arithmetic operation is a `tc_*` entry point of libtooncrafter_hip.so.

Data convention: activations are bf16 "rows" tensors `[M, C]` (channels-last:
M = B*T*H*W), possibly column-sliced views of a wider buffer (row stride =
`stride(0)`, unit column stride).  Weights are packed once by
`tooncrafter_amd.lvdm.packing`.

The functions below dispatch to the active backend object.  The only backend
the package ships is `HipOps`; tests may install a CPU emulation of the same
contract (tests/emu_ops.py) to exercise the host logic without a GPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_SILU, GATHER_CONV3x3, GATHER_CONVT3,
                   GATHER_LINEAR, TcAttnParams, TcAttnQ8Params, TcDdimBlendParams, TcDdimParams, TcFfParams, TcGemmMxParams, TcGemmParams, TcTbParams, TcTqaParams)

BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def attn_scale(scale) -> float:
    """The softmax scale of an attention call: the caller's, or 1 / sqrt(64) (every attention kernel has 64-wide heads)."""
    return float(64 ** -0.5 if scale is None else scale)


def _rows_view(t: torch.Tensor, dtype=BF16):
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != dtype:
        raise ValueError(f"expected a 2-D {dtype} rows tensor with unit column stride, got "
                         f"{tuple(t.shape)} {t.dtype} strides {t.stride()}")
    if not t.is_cuda:
        raise _lib.TooncrafterHipError("HIP operator called with a CPU tensor: the product path is GPU-only")
    return t


def _dev(t: Optional[torch.Tensor], dtype, what: str, contiguous: bool = True):
    """Pointer of a device operand, or raise: a CPU pointer handed to a kernel faults the GPU (and kills
    the process) instead of raising, so every tensor whose data_ptr() crosses the C ABI is checked here."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.TooncrafterHipError(f"{what}: expected a CUDA tensor, got "
                                       f"{getattr(t, 'device', type(t))}: the product path is GPU-only")
    if t.dtype != dtype:
        raise ValueError(f"{what}: expected {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous")
    return t.data_ptr()


def clip_seeds(seeds, b: int, what: str = "seeds"):
    """The per-clip seeds of a batch of `b` as a list of Python ints, or ValueError: one integer in [0, 2^64) per clip
    (tc_randn_clips keys Philox with the two 32-bit halves).  Host-only: callers check before anything is launched."""
    import numbers
    if isinstance(seeds, (str, bytes)) or not hasattr(seeds, "__len__"):
        raise ValueError(f"{what}: expected a sequence of {b} integers, got {type(seeds).__name__}")
    seeds = list(seeds)
    if len(seeds) != b:
        raise ValueError(f"{what}: {len(seeds)} seeds for a batch of {b} clips")
    for s in seeds:
        if isinstance(s, bool) or not isinstance(s, numbers.Integral) or not 0 <= int(s) < 1 << 64:
            raise ValueError(f"{what}: a seed is an integer in [0, 2^64), got {s!r}")
    return [int(s) for s in seeds]


def planes_layout(planes, what: str = "planes"):
    """The memory layout of n planar 4:2:0 images (`clip.Planes`) as tc_frames_from_yuv takes it, or ValueError: format code,
    n, sh, sw, the two pitches and image strides in bytes, and `wide` (2-byte samples).  Host-only: nothing is launched."""
    fmt = getattr(planes, "fmt", None)
    if fmt not in _lib.TC_YUV_FORMATS:
        raise ValueError(f"{what}: fmt {fmt!r}: one of {sorted(_lib.TC_YUV_FORMATS)}")
    if planes.standard not in _lib.TC_YUV_STANDARDS or planes.range not in _lib.TC_YUV_RANGES or planes.siting not in _lib.TC_CHROMA_SITINGS:
        raise ValueError(f"{what}: standard {planes.standard!r}, range {planes.range!r}, siting {planes.siting!r}: one of "
                         f"{sorted(_lib.TC_YUV_STANDARDS)}, {sorted(_lib.TC_YUV_RANGES)}, {sorted(_lib.TC_CHROMA_SITINGS)}")
    if planes.matrix is not None and (len(planes.matrix) != 7 or int(planes.matrix[0]) <= 0):
        raise ValueError(f"{what}: matrix {list(planes.matrix)}: seven integers (cy, crv, cgu, cgv, cbu, yoff, coff), cy > 0")
    wide = fmt == "p010"
    dtypes = (torch.uint16, torch.int16) if wide else (torch.uint8,)
    y, chroma = planes.y, tuple(planes.chroma) if isinstance(planes.chroma, (tuple, list)) else (planes.chroma,)
    if len(chroma) != (2 if fmt == "i420" else 1):
        raise ValueError(f"{what}: {fmt} has {2 if fmt == 'i420' else 1} chroma plane(s), got {len(chroma)}")
    for name, p in (("y", y),) + tuple((f"chroma[{i}]", c) for i, c in enumerate(chroma)):
        if not isinstance(p, torch.Tensor) or p.dtype not in dtypes:
            raise ValueError(f"{what}: {name}: expected a tensor of {' or '.join(str(d) for d in dtypes)} for {fmt}, got "
                             f"{getattr(p, 'dtype', type(p))}")
        if p.device != y.device:
            raise ValueError(f"{what}: {name} is on {p.device}, y on {y.device}")
    if y.dim() != 3 or 0 in y.shape:
        raise ValueError(f"{what}: y must be (n, h, w), got {tuple(y.shape)}")
    n, sh, sw = y.shape
    ch, cw = (sh + 1) // 2, (sw + 1) // 2
    cshape = (n, ch, cw) if fmt == "i420" else (n, ch, cw, 2)
    for i, c in enumerate(chroma):
        if tuple(c.shape) != cshape:
            raise ValueError(f"{what}: chroma[{i}] must be {cshape} for {fmt} with a {(sh, sw)} picture, got {tuple(c.shape)}")
    if fmt == "i420" and chroma[0].stride() != chroma[1].stride():
        raise ValueError(f"{what}: the Cb and Cr planes must share one pitch (strides {chroma[0].stride()}, {chroma[1].stride()})")

    def rows(p, row_elems, inner):
        """(pitch, image stride) in elements of a plane whose rows hold row_elems unit-stride elements"""
        if p.stride()[2:] != inner or p.stride(1) < row_elems or (n > 1 and p.stride(0) < p.shape[1] * p.stride(1)):
            raise ValueError(f"{what}: rows must have unit stride inside and may not overlap (shape {tuple(p.shape)}, strides {p.stride()})")
        return p.stride(1), p.stride(0) if n > 1 else p.shape[1] * p.stride(1)
    es = 2 if wide else 1
    pitch_y, stride_y = rows(y, sw, (1,))
    pitch_c, stride_c = rows(chroma[0], cw if fmt == "i420" else 2 * cw, (1,) if fmt == "i420" else (2, 1))
    return dict(format=_lib.TC_YUV_FORMATS[fmt], wide=wide, n=n, sh=sh, sw=sw, pitch_y=pitch_y * es, pitch_c=pitch_c * es,
                image_stride_y=stride_y * es, image_stride_c=stride_c * es)


class MxRows:
    """An activation that exists only as MXFP8 (e4m3 bytes + E8M0 block scales): what `layernorm(..., mx_for=...)`
    hands to the one GEMM that consumes it when the fp8 routing takes that GEMM."""

    def __init__(self, q, scales, k):
        self.q, self.scales, self.k = q, scales, k
        self.shape = (q.shape[0], k)
        self.device = q.device


class GnPart:
    """Partial GroupNorm sums a GEMM emitted beside its output (ABI 9): `sums` fp32 [row blocks, 2, N] (sum, sum of
    squares of the rounded outputs per block of `rows` rows and per column), `of` the output tensor they describe."""
    __slots__ = ("sums", "rows", "of")

    def __init__(self, sums, rows, of):
        self.sums, self.rows, self.of = sums, rows, of


class HipOps:
    """The product backend: ctypes calls into libtooncrafter_hip.so."""

    name = "hip"

    def __init__(self):
        import os
        self.lib = _lib.load()
        self._ws = {}
        self._resize_tables = {}
        # BASELINE.json configs[4]: TC_FP8 routes eligible GEMMs (see _fp8_eligible) through MXFP8 operands -- weights
        # quantised once, activations by tc_quant_mxfp8 in front of each GEMM.  TC_FP8=1 = "linear": the wide-N
        # projections (qkv, GEGLU), which carry most of the time gain at 2x the bf16 error of a UNet forward;
        # "all" adds the 3x3 / temporal convolutions (10x the bf16 error, profiles/r02_fp8_error_by_layer_class.txt);
        # "conv" | "conv3" | "convt" select those alone.
        mode = os.environ.get("TC_FP8", "0").lower()
        self.fp8 = None if mode in ("0", "", "off") else ("linear" if mode in ("1", "on") else mode)
        self.fp8_min_k = int(os.environ.get("TC_FP8_MIN_K", "640"))
        self.fp8_min_n = int(os.environ.get("TC_FP8_MIN_N", "1280"))
        self.fp8_max_cin = int(os.environ.get("TC_FP8_MAX_CIN", "1280"))
        self.fp8_min_cin = int(os.environ.get("TC_FP8_MIN_CIN", "0"))
        self.fp8_n_over_k = float(os.environ.get("TC_FP8_N_OVER_K", "2"))
        self.fp8_min_m = 1024
        self.fp8_decoder = os.environ.get("TC_FP8_DECODER", "0") == "1"
        self.fp8_fuse_ln = os.environ.get("TC_FP8_FUSE_LN", "1") != "0"     # LayerNorm emits MXFP8 for its fp8 consumer
        # ABI 14: TC_FP8_ATTN=1 runs the spatial self-attentions with lk >= fp8_attn_min_lk (640: UNet levels 0 and 1) on
        # int8 q k^T + MXFP8 P v (csrc/attention_q8.hip, spatial_attn_q8_eligible); independent of TC_FP8, off by default
        self.fp8_attn = os.environ.get("TC_FP8_ATTN", "0") == "1"
        self.fp8_attn_min_lk = int(os.environ.get("TC_FP8_ATTN_MIN_LK", "640"))
        self.fp8_calls = {"mx": 0, "bf16": 0, "attn_q8": 0}
        self._wq = {}
        # LayerNorm -> consumer GEMM fusion (ABI 8, gemm_ln_eligible); TC_FUSE_LN=0 keeps the separate launch (A/B runs)
        self.fuse_ln = os.environ.get("TC_FUSE_LN", "1") != "0"
        # ABI 9: GroupNorm statistics from the producing GEMM.  OFF by default: measured end to end (profiles/
        # r04_gn_part_ab.txt, same lease, alternating runs) GroupNorm loses 0.3-0.4 ms per guided forward (4.71 -> 4.39,
        # 6.08 -> 5.72 on a slow lease) and the producing convolutions gain 0.4-1.1 ms (their epilogues fold 160 rows per
        # column and end on two block barriers): 7.79 vs 7.79 frames/s on one lease, 6.63 vs 6.75 on the other
        # (a call that carries gn_part keeps the implicit-GEMM kernels: the halo-patch route, the default for the 3x3
        # convolutions of levels 0-2 since round 5, emits no statistics -- so TC_GN_PART=1 also moves those convolutions back,
        # which is the routing the figures above were measured on)
        self.gn_part = os.environ.get("TC_GN_PART", "0") == "1"
        # ABI 12: the norm in front of a GEMM streams that GEMM's weights into the Infinity Cache (tc_groupnorm_pf /
        # tc_layernorm_pf).  Inside a forward W is always cold (2.9 GB of parameters per forward, 256 MB of cache); that
        # costs the 1280-channel levels 7-29 % of their GEMM time and nothing where W is small beside A
        # (profiles/r05_cold_operand_probe.txt, r05_prefetch_premise_probe.txt) -- hence the row bound.  TC_PREFETCH=0: never.
        self.prefetch_on = os.environ.get("TC_PREFETCH", "1") != "0"
        self.prefetch_max_rows = int(os.environ.get("TC_PREFETCH_MAX_ROWS", "8192"))
        self.prefetch_min_bytes = 1 << 20
        self.prefetch_max_bytes = 96 << 20

    # ------------------------------------------------------------------ workspace
    def _workspace(self, nbytes: int, device) -> torch.Tensor:
        # stream-ordered scratch from the caching allocator (capture-safe)
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)

    # ------------------------------------------------------------------ GEMM family
    def gemm(self, a, w, bias=None, *, act=ACT_NONE, residual=None, row_bias=None, row_div=0,
             alpha=1.0, out_scale=1.0, out=None, out_f32=False, conv=None, batch=1,
             stride_a=0, stride_w=0, stride_c=0, m=None, a_norm_eps=None, gn_stats=False):
        """out[M, N'] = act(alpha * gather(a) @ w^T + bias + row_bias[m // row_div]) * out_scale + residual.

        gn_stats (ABI 9): the result is (out, GnPart | None) -- when the kernel this problem runs on can emit them
        (tc_gemm_gn_rows), per-row-block column sums of the rounded outputs, which `groupnorm(..., part=)` takes instead
        of reading the tensor once more for its statistics; None otherwise (the caller passes it on all the same).

        a_norm_eps (ABI 8): LayerNorm of the rows of `a` as a prologue of the product -- (x - mean) * rsqrt(var + eps)
        over the K columns; gamma / beta must already be folded into w / bias (lvdm.common.fold_layernorm).  Only for
        problems `gemm_ln_eligible` accepts (the weight-stationary K = 320 kernel).

        a: rows tensor (for conv modes the SOURCE rows, lda = a.stride(0));
        w: [N, K] bf16 contiguous; conv: None | dict(kind='3x3'|'t3', frames, t_len, h_in, w_in,
        h_out, w_out, stride, upsample, cin); batch>1: a/w/out are the first batch item views
        and stride_* the element strides between items."""
        mx_a = a if isinstance(a, MxRows) else None
        if mx_a is not None:
            if conv is not None or out is not None or batch != 1 or self.fp8 is None:
                raise ValueError("gemm: an MXFP8 activation feeds one plain linear GEMM of the fp8 route")
            a = mx_a.q                                   # shape / device bookkeeping below; never read as bf16
        else:
            a = _rows_view(a)
        if w.dtype != BF16 or w.dim() != 2 or w.stride(1) != 1:
            raise ValueError("w must be a [N, K] bf16 tensor with unit column stride")
        _dev(w, BF16, "gemm: w", contiguous=False)
        n, k = w.shape
        n_out = n // 2 if act == ACT_GEGLU else n
        p = TcGemmParams()
        if conv is None:
            mm = a.shape[0] if m is None else m
            p.gather = GATHER_LINEAR
            if a.shape[1] < k:
                raise ValueError(f"A has {a.shape[1]} columns, weight K = {k}")
        else:
            kind = conv["kind"]
            p.gather = GATHER_CONV3x3 if kind == "3x3" else GATHER_CONVT3
            p.cin = conv["cin"]
            p.frames = conv["frames"]
            p.t_len = conv.get("t_len", 1)
            p.h_out, p.w_out = conv["h_out"], conv["w_out"]
            p.h_in, p.w_in = conv.get("h_in", conv["h_out"]), conv.get("w_in", conv["w_out"])
            p.stride = conv.get("stride", 1)
            p.upsample = 1 if conv.get("upsample", False) else 0
            p.pad = conv.get("pad", 1)
            mm = p.frames * p.h_out * p.w_out
            need_rows = p.frames * p.h_in * p.w_in
            if a.shape[0] < need_rows:
                raise ValueError(f"conv source has {a.shape[0]} rows, geometry needs {need_rows}")
            if a.shape[1] < p.cin or k != (9 if kind == "3x3" else 3) * p.cin:
                raise ValueError(f"conv source has {a.shape[1]} channels / weight K = {k}, geometry says cin = {p.cin}")
        if out is None:
            out = torch.empty((mm, n_out), dtype=torch.float32 if out_f32 else BF16, device=a.device)
        else:
            _rows_view(out, torch.float32 if out_f32 else BF16)
            if out.shape[0] < mm or out.shape[1] != n_out:
                raise ValueError(f"out shape {tuple(out.shape)} != ({mm}, {n_out})")
        p.a, p.w, p.c = a.data_ptr(), w.data_ptr(), out.data_ptr()
        if bias is not None:
            if bias.numel() != n:
                raise ValueError("bias must be fp32 [N]")
            p.bias = _dev(bias, torch.float32, "gemm: bias")
        if row_bias is not None:
            if row_bias.dtype != torch.float32 or row_bias.dim() != 2 or row_bias.stride(1) != 1 \
                    or row_bias.shape[1] != n:
                raise ValueError("row_bias must be fp32 [R, N] with unit column stride")
            if row_div <= 0 or row_bias.shape[0] * row_div < mm:
                raise ValueError("row_bias / row_div do not cover M")
            p.row_bias = _dev(row_bias, torch.float32, "gemm: row_bias", contiguous=False)
            p.ldrb = row_bias.stride(0)
        if residual is not None:
            _rows_view(residual)
            if residual.shape[1] != n_out or residual.shape[0] < mm:
                raise ValueError("residual shape mismatch")
            p.residual = residual.data_ptr()
            p.ldr = residual.stride(0)
        p.m, p.n, p.k = mm, n, k
        p.lda, p.ldw, p.ldc = a.stride(0), w.stride(0), out.stride(0)
        p.row_div = row_div
        p.alpha, p.out_scale = float(alpha), float(out_scale)
        p.act, p.out_f32 = act, 1 if out_f32 else 0
        p.batch = batch
        p.stride_a, p.stride_w, p.stride_c = stride_a, stride_w, stride_c
        if a_norm_eps is not None:
            p.a_norm, p.a_norm_eps = 1, float(a_norm_eps)
            if mx_a is not None or self.fp8 is not None and self._fp8_eligible(p, conv is not None, n_out, batch):
                raise ValueError("gemm: a_norm_eps and the MXFP8 route exclude each other")
            if not self.lib.tc_gemm_ws_eligible(C.byref(p)):
                raise ValueError("gemm: a_norm_eps needs a problem the weight-stationary kernel takes (gemm_ln_eligible)")
        if self.fp8 is not None:
            if self._fp8_eligible(p, conv is not None, n_out, batch):
                self.fp8_calls["mx"] += 1
                self._gemm_mx(p, a, w, mx_a)
                return (out, None) if gn_stats else out
            if mx_a is not None:
                raise ValueError("gemm: MXFP8 activation handed to a GEMM the fp8 route does not take")
            self.fp8_calls["bf16"] += 1
        nbytes = self.lib.tc_gemm_workspace(C.byref(p))          # > 0 only for split-K candidates (low-res layers)
        if nbytes > 0:
            ws = self._workspace(nbytes, a.device)
            p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
        part = None
        if gn_stats and self.gn_part and out.is_contiguous():
            prow = self.lib.tc_gemm_gn_rows(C.byref(p))         # 160 / 128 / 0: the routing's own answer
            if prow > 0:
                part = GnPart(torch.empty(((mm + prow - 1) // prow, 2, n), dtype=torch.float32, device=a.device), prow, out)
                p.gn_part = part.sums.data_ptr()
        _lib.check(self.lib.tc_gemm_bf16(C.byref(p), _stream()), "tc_gemm_bf16")
        return (out, part) if gn_stats else out

    def gemm_ln_eligible(self, m, n, k, *, geglu=False, lda=None) -> bool:
        """Would `gemm(a[m, k], w[n, k], act=GEGLU if geglu, a_norm_eps=...)` be accepted, i.e. may the caller drop the
        LayerNorm launch in front of this projection?  ONE rule, the library's own (tc_gemm_ws_eligible); the MXFP8
        route keeps its LayerNorm -> MXFP8 fusion instead."""
        if not self.fuse_ln:
            return False
        p = TcGemmParams()
        p.gather, p.m, p.n, p.k = GATHER_LINEAR, int(m), int(n), int(k)
        p.lda, p.ldw = int(lda if lda is not None else k), int(k)
        p.act = ACT_GEGLU if geglu else ACT_NONE
        p.ldc = p.ldr = n // 2 if geglu else n
        p.alpha, p.out_scale, p.batch = 1.0, 1.0, 1
        return bool(self.lib.tc_gemm_ws_eligible(C.byref(p))) and not self._fp8_takes_linear(m, n, k, p.ldc)

    # ------------------------------------------------------------------ fused level-0 feed-forward (ABI 9)
    def _ff_params(self, m, c, hidden, ldx, ldo, ln_eps):
        p = TcFfParams()
        p.m, p.c, p.hidden, p.ldx, p.ldo = int(m), int(c), int(hidden), int(ldx), int(ldo)
        p.ln, p.ln_eps = (0, 0.0) if ln_eps is None else (1, float(ln_eps))
        return p

    def ff_fused_eligible(self, m, c, hidden, *, ldx=None) -> bool:
        """Would `ff_geglu_fused(x[m, c], w1[2 hidden, c], ...)` be accepted?  The library's own rule
        (tc_ff_geglu_fused_eligible: c = 320, hidden = 1280, TC_FF_FUSED != 0); never on the MXFP8 route, whose GEGLU
        projection is a different kernel with its own numerics."""
        if self.fp8 is not None:
            return False
        p = self._ff_params(m, c, hidden, c if ldx is None else ldx, c, 1e-5)
        return bool(self.lib.tc_ff_geglu_fused_eligible(C.byref(p)))

    def ff_geglu_fused(self, x, w1, b1, w2, b2, *, ln_eps=None):
        """out = x + w2 . GEGLU(w1 . LN(x) + b1) + b2 as ONE launch (reference attention.py:415-442 behind norm3): the hidden
        tensor never reaches HBM.  w1 / b1: the GEGLU projection exactly as `gemm(..., act=ACT_GEGLU)` takes it (with the
        LayerNorm's affine half folded in when ln_eps is given); ln_eps=None: x is taken as already normalised."""
        m, c = x.shape
        hidden = w2.shape[1]
        _dev(x, BF16, "ff_geglu_fused x", contiguous=False)
        for t, dt, what in ((w1, BF16, "w1"), (w2, BF16, "w2"), (b1, torch.float32, "b1"), (b2, torch.float32, "b2")):
            _dev(t, dt, "ff_geglu_fused " + what)
        if x.stride(1) != 1 or tuple(w1.shape) != (2 * hidden, c) or tuple(w2.shape) != (c, hidden) or b1.numel() != 2 * hidden \
                or b2.numel() != c:
            raise ValueError("ff_geglu_fused: x [m, c] rows, w1 [2 hidden, c], b1 [2 hidden], w2 [c, hidden], b2 [c]")
        out = torch.empty((m, c), dtype=BF16, device=x.device)
        p = self._ff_params(m, c, hidden, x.stride(0), c, ln_eps)
        p.x, p.w1, p.b1, p.w2, p.b2, p.out = (x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                              out.data_ptr())
        _lib.check(self.lib.tc_ff_geglu_fused(C.byref(p), _stream()), "tc_ff_geglu_fused")
        return out

    # ------------------------------------------------------------------ fused level-0 temporal self-attention (ABI 9)
    def _tb_params(self, b, t, hw, c, heads, ldx, ldo, ln_eps, scale):
        p = TcTbParams()
        p.b, p.t, p.hw, p.c, p.heads, p.ldx, p.ldo = int(b), int(t), int(hw), int(c), int(heads), int(ldx), int(ldo)
        p.ln, p.ln_eps = (0, 0.0) if ln_eps is None else (1, float(ln_eps))
        p.scale = attn_scale(scale)
        return p

    def temporal_attn_fused_eligible(self, *, b, t, hw, c, heads, ldx=None) -> bool:
        """Would `temporal_attn_fused` be accepted?  The library's own rule (tc_temporal_attn_fused_eligible: c = 320, 5 heads,
        16 frames, hw % 8 == 0, and TC_TB_FUSED=1 -- since round 6 the default route of level 0 is LayerNorm + `temporal_qkv_attn` +
        output projection, which measured ahead); never on the MXFP8 route."""
        if self.fp8 is not None:
            return False
        p = self._tb_params(b, t, hw, c, heads, c if ldx is None else ldx, c, 1e-5, None)
        return bool(self.lib.tc_temporal_attn_fused_eligible(C.byref(p)))

    def temporal_attn_fused(self, x, wqkv, bqkv, wo, bo, *, b, t, hw, heads, ln_eps=None, scale=None):
        """out = x + wo . Attn_frames(wqkv . LN(x) + bqkv) + bo as ONE launch (reference attention.py:81-144 over the frames of
        a pixel, TemporalTransformer attention.py:365-412): the qkv tensor and the attention output never reach HBM.  wqkv:
        the fused projection `gemm` takes in front of `attention_temporal` (LayerNorm's affine half folded in when ln_eps is
        given, bqkv = its bias; zeros otherwise)."""
        m, c = x.shape
        _dev(x, BF16, "temporal_attn_fused x", contiguous=False)
        for tns, dt, what in ((wqkv, BF16, "wqkv"), (wo, BF16, "wo"), (bqkv, torch.float32, "bqkv"), (bo, torch.float32, "bo")):
            _dev(tns, dt, "temporal_attn_fused " + what)
        if x.stride(1) != 1 or m != b * t * hw or tuple(wqkv.shape) != (3 * c, c) or tuple(wo.shape) != (c, c) \
                or bqkv.numel() != 3 * c or bo.numel() != c or c != heads * 64:
            raise ValueError("temporal_attn_fused: x [b*t*hw, c] rows, wqkv [3c, c], bqkv [3c], wo [c, c], bo [c], c = heads * 64")
        out = torch.empty((m, c), dtype=BF16, device=x.device)
        p = self._tb_params(b, t, hw, c, heads, x.stride(0), c, ln_eps, scale)
        p.x, p.wqkv, p.bqkv, p.wo, p.bo, p.out = (x.data_ptr(), wqkv.data_ptr(), bqkv.data_ptr(), wo.data_ptr(), bo.data_ptr(),
                                                  out.data_ptr())
        _lib.check(self.lib.tc_temporal_attn_fused(C.byref(p), _stream()), "tc_temporal_attn_fused")
        return out

    # ------------------------------------------------------------------ temporal qkv projection + attention, one launch (ABI 13)
    def _tqa_params(self, b, t, hw, c, heads, ldx, ldo, scale):
        p = TcTqaParams()
        p.b, p.t, p.hw, p.c, p.heads, p.ldx, p.ldo = int(b), int(t), int(hw), int(c), int(heads), int(ldx), int(ldo)
        p.scale = attn_scale(scale)
        return p

    def temporal_qkv_attn_eligible(self, *, b, t, hw, c, heads, ldx=None) -> bool:
        """Would `temporal_qkv_attn` be accepted?  The library's own rule (tc_temporal_qkv_attn_eligible: c = heads * 64;
        16 frames with hw % 8 == 0, or 17 .. 64 frames with hw % (128 / TT) == 0, TT = 32 | 64, where TC_QKV_ATTN admits
        the shape -- 0 never, 1 what measured ahead, 2 everything; any t is passed through, the library decides); never on
        the MXFP8 route (which quantises the projection's input)."""
        if self.fp8 is not None:
            return False
        p = self._tqa_params(b, t, hw, c, heads, c if ldx is None else ldx, c, None)
        return bool(self.lib.tc_temporal_qkv_attn_eligible(C.byref(p)))

    def temporal_qkv_attn(self, x, wqkv, bqkv=None, *, b, t, hw, heads, scale=None, out=None):
        """Attn_frames(x . wqkv^T + bqkv) -> [rows, c] as ONE launch: `gemm(x, wqkv, bqkv)` + `attention_temporal` without the
        [rows, 3c] tensor between them (reference attention.py:96-134 over the frames of a pixel, TemporalTransformer
        attention.py:365-412).  x: the projection's input (LayerNorm output) rows; the result feeds to_out.  `out` must
        not alias `x`."""
        m, c = x.shape
        _dev(x, BF16, "temporal_qkv_attn x", contiguous=False)
        _dev(wqkv, BF16, "temporal_qkv_attn wqkv")
        if bqkv is not None:
            _dev(bqkv, torch.float32, "temporal_qkv_attn bqkv")
        if x.stride(1) != 1 or m != b * t * hw or tuple(wqkv.shape) != (3 * c, c) or c != heads * 64 \
                or (bqkv is not None and bqkv.numel() != 3 * c):
            raise ValueError("temporal_qkv_attn: x [b*t*hw, c] rows, wqkv [3c, c], bqkv [3c] or None, c = heads * 64")
        if out is None:
            out = torch.empty((m, c), dtype=BF16, device=x.device)
        elif tuple(out.shape) != (m, c) or out.stride(1) != 1:
            raise ValueError("temporal_qkv_attn: out must be [b*t*hw, c] rows")
        else:
            _dev(out, BF16, "temporal_qkv_attn out", contiguous=False)
        p = self._tqa_params(b, t, hw, c, heads, x.stride(0), out.stride(0), scale)
        p.x, p.wqkv, p.bqkv, p.out = x.data_ptr(), wqkv.data_ptr(), (None if bqkv is None else bqkv.data_ptr()), out.data_ptr()
        _lib.check(self.lib.tc_temporal_qkv_attn(C.byref(p), _stream()), "tc_temporal_qkv_attn")
        return out

    # ------------------------------------------------------------------ MXFP8 GEMM path (configs[4])
    def quant_mxfp8(self, x, k=None):
        """bf16 rows [R, >=k] -> (e4m3 bytes [R, k], E8M0 scales [R, ceil(k/128)*4]); one scale per 32 K elements."""
        x = _rows_view(x)
        k = x.shape[1] if k is None else k
        if k % 32 or x.shape[1] < k:
            raise ValueError(f"quant_mxfp8: k = {k} must be a multiple of 32 and <= {x.shape[1]} columns")
        rows, lds = x.shape[0], (k + 127) // 128 * 4
        q = torch.empty((rows, k), dtype=torch.uint8, device=x.device)
        sc = torch.empty((rows, lds), dtype=torch.uint8, device=x.device)
        _lib.check(self.lib.tc_quant_mxfp8(x.data_ptr(), rows, k, x.stride(0), q.data_ptr(), q.stride(0),
                                           sc.data_ptr(), lds, _stream()), "tc_quant_mxfp8")
        return q, sc

    @contextlib.contextmanager
    def fp8_scope(self, name):
        """Modules whose output precision matters more than their time opt out of the fp8 routing: the VAE decoder
        writes the pixels (measured at full size: 1.3e-1 from the fp32 oracle with MXFP8 convolutions against 1.3e-2
        in bf16, for 3 ms per decode) -- TC_FP8_DECODER=1 opts it back in."""
        old = self.fp8
        if name == "decoder" and not self.fp8_decoder:
            self.fp8 = None
        try:
            yield
        finally:
            self.fp8 = old

    def _weight_mx(self, w):
        """Quantised copy of a packed weight matrix, made once per weight tensor (held while the tensor lives)."""
        import weakref
        ent = self._wq.get(id(w))
        if ent is None or ent[0]() is not w or ent[1] != w._version:
            q, sc = self.quant_mxfp8(w if w.stride(0) % 8 == 0 else w.contiguous())
            ent = (weakref.ref(w), w._version, q, sc)
            if id(w) not in self._wq:
                weakref.finalize(w, self._wq.pop, id(w), None)
            self._wq[id(w)] = ent
        return ent[2], ent[3]

    def _fp8_eligible(self, p, is_conv, n_out, batch) -> bool:
        if batch != 1 or n_out % 8 or p.k % 32 or p.m < self.fp8_min_m:
            return False
        # measured (profiles/r02_mx_gemm_bench.txt): with the activation quantiser in front, fp8 pays on the 3x3 /
        # temporal convolutions up to cin = 1280 (one quantisation feeds 9 / 3 taps) and on linear layers whose N is
        # large against K (qkv, GEGLU: N >= 2 K -- exactly the consumers of a LayerNorm, which then emits MXFP8
        # itself); short-K or narrow-N linear layers (out-projections, ff2: slower in fp8 even before the quantiser
        # pass, profiles/r02_mx_gemm_bench.txt) stay bf16
        if is_conv:
            kind = "conv3" if p.gather == GATHER_CONV3x3 else "convt"
            return self.fp8 in ("all", "conv", kind) and p.cin % 64 == 0 and self.fp8_min_cin <= p.cin <= self.fp8_max_cin
        return self.fp8 in ("all", "linear") and p.k >= self.fp8_min_k and p.n >= self.fp8_min_n \
            and p.n >= self.fp8_n_over_k * p.k

    def _fp8_takes_linear(self, m, n, k, n_out) -> bool:
        """Would the MXFP8 route take the plain linear GEMM a[m, k] . w[n, k]^T (n_out = n // 2 behind a GEGLU)?"""
        p = TcGemmParams(m=int(m), n=int(n), k=int(k), gather=GATHER_LINEAR)
        return self.fp8 is not None and self._fp8_eligible(p, False, n_out, 1)

    def _gemm_mx(self, p, a, w, mx_a=None):
        kc = p.cin if p.gather != GATHER_LINEAR else p.k
        rows = p.frames * p.h_in * p.w_in if p.gather == GATHER_CONV3x3 else p.m
        if mx_a is not None:
            if mx_a.k != kc:
                raise ValueError(f"gemm: MXFP8 activation has K = {mx_a.k}, weight K = {kc}")
            aq, asc = mx_a.q, mx_a.scales
        else:
            aq, asc = self.quant_mxfp8(a[:rows], kc)
        wq, wsc = self._weight_mx(w)
        px = TcGemmMxParams()
        px.g = p
        px.g.a, px.g.lda = aq.data_ptr(), aq.stride(0)
        px.g.w, px.g.ldw = wq.data_ptr(), wq.stride(0)
        px.a_scale, px.lda_s = asc.data_ptr(), asc.stride(0)
        px.w_scale, px.ldw_s = wsc.data_ptr(), wsc.stride(0)
        _lib.check(self.lib.tc_gemm_mxfp8(C.byref(px), _stream()), "tc_gemm_mxfp8")

    # ------------------------------------------------------------------ attention
    def attention(self, q, k, v, *, batch, heads, lq, lk, kv_bdiv=1, out=None, accumulate=False, scale=None,
                  k2=None, v2=None, lk2=0, kv2_bdiv=1):
        """q: [batch*lq, heads*64] rows view; k, v: [(batch//kv_bdiv)*lk, heads*64] rows views.
        out[batch*lq, heads*64] (+)= softmax(q k^T * scale) v per (batch, head)
        [+ softmax(q k2^T * scale) v2 when a second key/value set is given: two softmaxes, one launch]."""
        q, k, v = _rows_view(q), _rows_view(k), _rows_view(v)
        hd = heads * 64
        if q.shape != (batch * lq, hd) or k.shape[1] != hd or v.shape[1] != hd:
            raise ValueError("attention: head layout mismatch")
        kvb = (batch + kv_bdiv - 1) // kv_bdiv
        if k.shape[0] != kvb * lk or v.shape[0] != kvb * lk:
            raise ValueError("attention: K/V rows != kv_batches * lk")
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs out")
            out = torch.empty((batch * lq, hd), dtype=BF16, device=q.device)
        else:
            _rows_view(out)
        p = TcAttnParams()
        p.q, p.k, p.v, p.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
        p.batch, p.heads, p.lq, p.lk = batch, heads, lq, lk
        p.q_ss, p.k_ss, p.v_ss, p.o_ss = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
        p.q_sb, p.k_sb, p.v_sb, p.o_sb = lq * q.stride(0), lk * k.stride(0), lk * v.stride(0), lq * out.stride(0)
        p.kv_bdiv = kv_bdiv
        p.accumulate = 1 if accumulate else 0
        p.scale = attn_scale(scale)
        if k2 is not None:
            k2, v2 = _rows_view(k2), _rows_view(v2)
            kvb2 = (batch + kv2_bdiv - 1) // kv2_bdiv
            if lk2 <= 0 or k2.shape != (kvb2 * lk2, hd) or v2.shape != (kvb2 * lk2, hd):
                raise ValueError("attention: second K/V set must be [(batch//kv2_bdiv)*lk2, heads*64]")
            p.k2, p.v2, p.lk2, p.kv2_bdiv = k2.data_ptr(), v2.data_ptr(), lk2, kv2_bdiv
            p.k2_ss, p.v2_ss = k2.stride(0), v2.stride(0)
            p.k2_sb, p.v2_sb = lk2 * k2.stride(0), lk2 * v2.stride(0)
        _lib.check(self.lib.tc_attn_d64(C.byref(p), _stream()), "tc_attn_d64")
        return out

    def spatial_attn_q8_eligible(self, *, lk, kv_bdiv=1, k2=None, accumulate=False) -> bool:
        """Routing rule of the 8-bit spatial self-attention (ABI 14): the switch is on, it is a plain self-attention (one
        key/value set, no K/V batch sharing, no accumulate) and long enough (lk >= fp8_attn_min_lk)."""
        return self.fp8_attn and k2 is None and not accumulate and kv_bdiv == 1 and lk >= self.fp8_attn_min_lk

    def _q8_params(self, q, k, v, out, batch, heads, lq, lk, scale):
        hd = heads * 64
        if q.shape != (batch * lq, hd) or k.shape != (batch * lk, hd) or v.shape != (batch * lk, hd):
            raise ValueError("attention_q8: q must be [batch*lq, heads*64], k and v [batch*lk, heads*64]")
        p = TcAttnQ8Params()
        p.q, p.k, p.v, p.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
        p.batch, p.heads, p.lq, p.lk = batch, heads, lq, lk
        p.q_ss, p.k_ss, p.v_ss, p.o_ss = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
        p.q_sb, p.k_sb, p.v_sb, p.o_sb = lq * q.stride(0), lk * k.stride(0), lk * v.stride(0), lq * out.stride(0)
        p.scale = attn_scale(scale)
        return p

    def attention_q8(self, q, k, v, *, batch, heads, lq, lk, scale=None):
        """8-bit self-attention (ABI 14): out[batch*lq, heads*64] = softmax(q k^T * scale) v per (batch, head), q k^T on
        int8 operands and P v on MXFP8 -- tc_attn_q8_quant_kv into a workspace from the caching allocator, then
        tc_attn_d64_q8.  Rows views as for attention()."""
        q, k, v = _rows_view(q), _rows_view(k), _rows_view(v)
        out = torch.empty((batch * lq, heads * 64), dtype=BF16, device=q.device)
        p = self._q8_params(q, k, v, out, batch, heads, lq, lk, scale)
        ws = self._workspace(self.lib.tc_attn_q8_workspace(C.byref(p)), q.device)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        _lib.check(self.lib.tc_attn_q8_quant_kv(C.byref(p), _stream()), "tc_attn_q8_quant_kv")
        _lib.check(self.lib.tc_attn_d64_q8(C.byref(p), _stream()), "tc_attn_d64_q8")
        self.fp8_calls["attn_q8"] += 1
        return out

    def attention_temporal(self, qkv, *, b, t, hw, heads, scale=None):
        """qkv: contiguous [b*t*hw, 3*heads*64] with row = (b*T + t)*HW + p -> [b*t*hw, heads*64]."""
        qkv = _rows_view(qkv)
        cdim = heads * 64
        if not qkv.is_contiguous() or qkv.shape != (b * t * hw, 3 * cdim):
            raise ValueError("attention_temporal: qkv must be contiguous [b*t*hw, 3*C]")
        out = torch.empty((b * t * hw, cdim), dtype=BF16, device=qkv.device)
        _lib.check(self.lib.tc_attn_temporal(qkv.data_ptr(), out.data_ptr(), b, t, hw, heads,
                                             attn_scale(scale), _stream()),
                   "tc_attn_temporal")
        return out

    def attention_temporal_rel(self, qkv, rel_k, rel_v, *, b, t, hw, heads, max_rel, causal, scale=None):
        """attention_temporal with relative position and / or a causal mask (tc_attn_temporal_rel; reference
        attention.py:20-39, 103-124, 343-345, 376-390).  rel_k, rel_v: contiguous bf16 [2*max_rel + 1, 64] tables
        shared by the heads, or both None (mask only)."""
        qkv = _rows_view(qkv)
        cdim = heads * 64
        if not qkv.is_contiguous() or qkv.shape != (b * t * hw, 3 * cdim):
            raise ValueError("attention_temporal_rel: qkv must be contiguous [b*t*hw, 3*C]")
        for tab in (rel_k, rel_v):
            if tab is not None and (tab.dtype != BF16 or not tab.is_contiguous() or tab.device != qkv.device
                                    or tuple(tab.shape) != (2 * max_rel + 1, 64)):
                raise ValueError("attention_temporal_rel: a table must be contiguous bf16 [2*max_rel + 1, 64] on qkv's device")
        out = torch.empty((b * t * hw, cdim), dtype=BF16, device=qkv.device)
        p = _lib.TcAttnTemporalRelParams(qkv=qkv.data_ptr(), out=out.data_ptr(), rel_k=_ptr(rel_k), rel_v=_ptr(rel_v),
                                         b=b, t=t, hw=hw, heads=heads, max_rel=int(max_rel), causal=int(bool(causal)),
                                         scale=attn_scale(scale))
        _lib.check(self.lib.tc_attn_temporal_rel(C.byref(p), _stream()), "tc_attn_temporal_rel")
        return out

    # ------------------------------------------------------------------ norms
    def prefetch_list(self, x_rows: int, tensors, linear: bool = False):
        """Which of `tensors` (the packed weights of the GEMMs that consume a norm's output) the norm launch should
        stream ahead of them: ONE rule for both bindings.  Only when the consumer is a small-M GEMM (its weights are then a
        large share of its traffic), only tensors worth a request, at most TC_PREFETCH_MAX of them / 96 MB.
        `linear`: the tensors are [N, K] weights of plain linear layers over these x_rows rows.  With the MXFP8 routing on
        (opt-in, configs[4]) a consumer it takes reads a cached QUANTISED copy of W (`_weight_mx`), not this bf16 tensor:
        streaming the bf16 one would be up to 96 MB of traffic and cache pollution for data nobody reads, so
        those are left out -- per tensor for linear consumers, wholesale when the routing also takes convolutions."""
        if not self.prefetch_on or not tensors or x_rows > self.prefetch_max_rows:
            return []
        if self.fp8 is not None and not linear and self.fp8 != "linear":
            return []
        out, total = [], 0
        for t in tensors:
            if t is None or not isinstance(t, torch.Tensor) or not t.is_contiguous() or t.data_ptr() % 16:
                continue                                              # (a hint: what the ABI would refuse is simply not streamed)
            if linear and t.dim() == 2 and any(self._fp8_takes_linear(x_rows, *t.shape, n_out) for n_out in (t.shape[0], t.shape[0] // 2)):
                continue                                            # (a GEGLU weight's N_out is N / 2: either answer means "taken")
            nbytes = t.numel() * t.element_size()
            if nbytes < self.prefetch_min_bytes or total + nbytes > self.prefetch_max_bytes:
                continue
            out.append(t)
            total += nbytes
            if len(out) == _lib.TC_PREFETCH_MAX:
                break
        return out

    @staticmethod
    def _prefetch_struct(tensors):
        pf = _lib.TcPrefetch()
        for i, t in enumerate(tensors):
            if not t.is_cuda:
                raise _lib.TooncrafterHipError("prefetch: a CPU tensor in a norm's prefetch list: the product path is GPU-only")
            pf.ptr[i], pf.bytes[i] = t.data_ptr(), t.numel() * t.element_size()
        pf.n = len(tensors)
        return pf

    def groupnorm(self, x, gamma, beta, *, samples, rows, eps, silu=False, part=None, prefetch=None, prefetch_linear=False):
        """x: contiguous [samples*rows, C]; statistics over (rows, C/32) per (sample, group).  `part` (a GnPart from
        the gemm that produced x, or None): statistics from the producer's partial sums -- one pass over x, not two.
        `prefetch` (ABI 12): packed weights of the GEMMs that read the result (see prefetch_list)."""
        x = _rows_view(x)
        c = x.shape[1]
        if not x.is_contiguous() or x.shape[0] != samples * rows:
            raise ValueError("groupnorm: x must be contiguous [samples*rows, C]")
        if gamma.numel() != c or beta.numel() != c:
            raise ValueError("groupnorm: gamma/beta must have C elements")
        gp, bp = _dev(gamma, torch.float32, "groupnorm: gamma"), _dev(beta, torch.float32, "groupnorm: beta")
        y = torch.empty_like(x)
        nbytes = self.lib.tc_groupnorm_workspace(samples, rows, c)
        ws = self._workspace(nbytes, x.device)
        if part is not None and part.of is x and rows % part.rows == 0 and part.sums.shape[2] == c \
                and part.sums.shape[0] * part.rows == samples * rows:
            _lib.check(self.lib.tc_groupnorm_part(x.data_ptr(), y.data_ptr(), gp, bp, part.sums.data_ptr(), part.rows, samples,
                                                  rows, c, float(eps), 1 if silu else 0, ws.data_ptr(), nbytes, _stream()),
                       "tc_groupnorm_part")
            return y
        pfl = self.prefetch_list(x.shape[0], prefetch, linear=prefetch_linear)
        if pfl:
            pf = self._prefetch_struct(pfl)
            _lib.check(self.lib.tc_groupnorm_pf(x.data_ptr(), y.data_ptr(), gp, bp, samples, rows, c, float(eps), 1 if silu else 0,
                                                ws.data_ptr(), nbytes, C.byref(pf), _stream()), "tc_groupnorm_pf")
            return y
        _lib.check(self.lib.tc_groupnorm(x.data_ptr(), y.data_ptr(), gp, bp, samples,
                                         rows, c, float(eps), 1 if silu else 0, ws.data_ptr(), nbytes, _stream()),
                   "tc_groupnorm")
        return y

    def gn_conv(self, x, gamma, beta, w, bias=None, *, samples, rows, eps, conv, silu=True, part=None, prefetch_extra=(), **kw):
        """conv(act(GroupNorm(x))) with the epilogue of `gemm` (**kw: row_bias / row_div / residual / act / gn_stats / out_f32):
        the reference's pair lvdm/basics.py:76-87 -> nn.Conv2d / nn.Conv3d (openaimodel3d.py:154,179,255-266) as ONE host
        operator, two launches.  (Round 5 measured the alternative -- the convolution normalising its own operand, ABI 10 --
        at -4 % per clip and removed it: DESIGN.md 5.6.)  `part`: see groupnorm."""
        # ABI 12: the norm's launch brings the convolution's weights (and `prefetch_extra`: those of a GEMM right behind it,
        # e.g. a ResBlock's 1x1 skip convolution) into the Infinity Cache where that pays (prefetch_list)
        h = self.groupnorm(x, gamma, beta, samples=samples, rows=rows, eps=eps, silu=silu, part=part,
                           prefetch=[w, *prefetch_extra])
        return self.gemm(h, w, bias, conv=conv, **kw)

    def layernorm(self, x, gamma, beta, eps=1e-5, mx_for=None, prefetch=None):
        """`mx_for` = (N, N_out) of the packed weight of the ONE linear GEMM that consumes the result: when the fp8
        route takes that GEMM the row leaves as MXFP8 (an `MxRows`; the quantiser fused into its producer).
        `prefetch` (ABI 12): packed weights of the GEMMs behind the norm (see prefetch_list)."""
        x = _rows_view(x)
        if not x.is_contiguous():
            raise ValueError("layernorm: x must be contiguous")
        if gamma.numel() != x.shape[1] or beta.numel() != x.shape[1]:
            raise ValueError("layernorm: gamma/beta must have C elements")
        gp, bp = _dev(gamma, torch.float32, "layernorm: gamma"), _dev(beta, torch.float32, "layernorm: beta")
        if mx_for is not None and self.fp8_fuse_ln and self._fp8_takes_linear(x.shape[0], mx_for[0], x.shape[1], mx_for[1]):
            rows, k = x.shape
            lds = (k + 127) // 128 * 4
            q = torch.empty((rows, k), dtype=torch.uint8, device=x.device)
            sc = torch.empty((rows, lds), dtype=torch.uint8, device=x.device)
            _lib.check(self.lib.tc_layernorm_mxfp8(x.data_ptr(), q.data_ptr(), k, sc.data_ptr(), lds, gp, bp, rows, k,
                                                   float(eps), _stream()), "tc_layernorm_mxfp8")
            return MxRows(q, sc, k)
        y = torch.empty_like(x)
        pfl = self.prefetch_list(x.shape[0], prefetch, linear=True)
        if pfl:
            pf = self._prefetch_struct(pfl)
            _lib.check(self.lib.tc_layernorm_pf(x.data_ptr(), y.data_ptr(), gp, bp, x.shape[0], x.shape[1], float(eps),
                                                C.byref(pf), _stream()), "tc_layernorm_pf")
            return y
        _lib.check(self.lib.tc_layernorm(x.data_ptr(), y.data_ptr(), gp, bp,
                                         x.shape[0], x.shape[1], float(eps), _stream()), "tc_layernorm")
        return y

    def softmax_rows(self, s, n=None, causal_period=0):
        """fp32 scores [rows, ld] -> bf16 probabilities [rows, ld]: softmax over the first `n` columns
        (default: all), the padding columns [n, ld) written as zeros; `causal_period` > 0: row r attends
        columns 0..(r mod period) only."""
        if s.dtype != torch.float32 or s.dim() != 2 or not s.is_contiguous() or not s.is_cuda:
            raise ValueError("softmax_rows: contiguous fp32 CUDA [rows, n]")
        ld = s.shape[1]
        n = ld if n is None else int(n)
        p = torch.empty(s.shape, dtype=BF16, device=s.device)
        _lib.check(self.lib.tc_softmax_rows(s.data_ptr(), p.data_ptr(), s.shape[0], n, ld, ld, ld,
                                            int(causal_period), _stream()), "tc_softmax_rows")
        return p

    # ------------------------------------------------------------------ layout / elementwise
    def nchw_to_rows(self, x0, x1=None, *, c_pad, scale=1.0, out=None):
        """(B, C0, T, H, W) [+ (B, C1, T, H, W)] fp32 -> bf16 rows [(b t h w), c_pad] (into `out` when given)."""
        if x0.dtype != torch.float32 or x0.dim() != 5 or not x0.is_cuda:
            raise ValueError("nchw_to_rows: fp32 CUDA (B, C, T, H, W)")
        x0 = x0.contiguous()
        b, c0, t, h, w = x0.shape
        c1 = 0
        if x1 is not None:
            x1 = x1.contiguous()
            if not x1.is_cuda or x1.dtype != torch.float32 or x1.shape[0] != b or tuple(x1.shape[2:]) != (t, h, w):
                raise ValueError("nchw_to_rows: second tensor shape mismatch")
            c1 = x1.shape[1]
        if out is None:
            out = torch.empty((b * t * h * w, c_pad), dtype=BF16, device=x0.device)
        elif not out.is_contiguous() or _rows_view(out).shape != (b * t * h * w, c_pad):
            raise ValueError("nchw_to_rows: out must be a contiguous [(b t h w), c_pad] bf16 tensor")
        _lib.check(self.lib.tc_nchw_to_rows(x0.data_ptr(), c0, _ptr(x1), c1, out.data_ptr(), c_pad, b, t, h * w,
                                            float(scale), _stream()), "tc_nchw_to_rows")
        return out

    def rows_to_nchw(self, rows, *, c, b, t, h, w):
        if rows.dim() != 2 or rows.stride(1) != 1 or rows.dtype not in (BF16, torch.float32) or not rows.is_cuda:
            raise ValueError("rows_to_nchw: 2-D bf16/fp32 CUDA rows")
        out = torch.empty((b, c, t, h, w), dtype=torch.float32, device=rows.device)
        _lib.check(self.lib.tc_rows_to_nchw(rows.data_ptr(), 1 if rows.dtype == torch.float32 else 0,
                                            rows.stride(0), out.data_ptr(), c, b, t, h * w, _stream()),
                   "tc_rows_to_nchw")
        return out

    def concat_rows(self, a, b):
        a, b = _rows_view(a), _rows_view(b)
        if not a.is_contiguous() or not b.is_contiguous() or a.shape[0] != b.shape[0]:
            raise ValueError("concat_rows: contiguous inputs with equal rows")
        out = torch.empty((a.shape[0], a.shape[1] + b.shape[1]), dtype=BF16, device=a.device)
        _lib.check(self.lib.tc_concat_rows(a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], out.data_ptr(),
                                           a.shape[0], _stream()), "tc_concat_rows")
        return out

    def timestep_embedding(self, t, dim, ld=None):
        """t: fp32 or int64 [n] -> bf16 [n, ld] = [cos | sin | 0 pad] (int64: converted to fp32 in the kernel, like the
        reference's `timesteps[:, None].float()`, utils_diffusion.py:19-23)."""
        if t.dtype not in (torch.float32, torch.int64) or t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("timestep_embedding: contiguous fp32 / int64 CUDA [n]")
        ld = dim if ld is None else ld
        out = torch.empty((t.shape[0], ld), dtype=BF16, device=t.device)
        fn = self.lib.tc_timestep_embedding if t.dtype == torch.float32 else self.lib.tc_timestep_embedding_i64
        _lib.check(fn(t.data_ptr(), out.data_ptr(), t.shape[0], dim, ld, _stream()), "tc_timestep_embedding")
        return out

    def repeat_rows(self, x, n):
        """[rows, C] -> [n * rows, C]: n copies one after the other (x.repeat(n, 1) as one launch of this library)."""
        if x.dim() != 2 or not x.is_cuda or not x.is_contiguous() or (x.shape[1] * x.element_size()) % 16:
            raise ValueError("repeat_rows: contiguous CUDA [rows, C] with 16-byte rows")
        out = torch.empty((n * x.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
        _lib.check(self.lib.tc_repeat_rows(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1] * x.element_size(), n, _stream()),
                   "tc_repeat_rows")
        return out

    def silu_to_bf16(self, x):
        if x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("silu_to_bf16: contiguous fp32 CUDA")
        y = torch.empty(x.shape, dtype=BF16, device=x.device)
        _lib.check(self.lib.tc_silu_f32_to_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()),
                   "tc_silu_f32_to_bf16")
        return y

    def time_mix3(self, rows, w, bias, *, b, t, h, w_):
        """rows: fp32 [b*t*h*w_, ld>=3]; w: fp32 [3,3,3,1,1]; -> (b, 3, t, h, w_) fp32."""
        if rows.dtype != torch.float32 or rows.dim() != 2 or rows.stride(1) != 1 or not rows.is_cuda:
            raise ValueError("time_mix3: fp32 CUDA rows")
        if w.numel() != 27 or bias.numel() != 3:
            raise ValueError("time_mix3: w must have 27 elements, bias 3")
        wp, bp = _dev(w, torch.float32, "time_mix3: w"), _dev(bias, torch.float32, "time_mix3: bias")
        out = torch.empty((b, 3, t, h, w_), dtype=torch.float32, device=rows.device)
        _lib.check(self.lib.tc_time_mix3(rows.data_ptr(), rows.stride(0), wp, bp,
                                         out.data_ptr(), b, t, h * w_, _stream()), "tc_time_mix3")
        return out

    def video_to_uint8(self, video):
        """(b, 3, t, h, w) fp32 in [-1, 1] -> (b, t, h, w, 3) uint8: clamp, (x+1)/2*255, truncate, permute
        (scripts/evaluation/inference.py:148-153), on the device."""
        if video.dtype != torch.float32 or video.dim() != 5 or video.shape[1] != 3 or not video.is_cuda:
            raise ValueError("video_to_uint8: fp32 CUDA (b, 3, t, h, w)")
        video = video.contiguous()
        b, _, t, h, w = video.shape
        out = torch.empty((b, t, h, w, 3), dtype=torch.uint8, device=video.device)
        _lib.check(self.lib.tc_video_to_u8(video.data_ptr(), out.data_ptr(), b, t, h * w, _stream()), "tc_video_to_u8")
        return out

    def resized_size(self, sh, sw, h, w):
        """(rh, rw) of an (sh, sw) image under the script's Resize(min(h, w)) (tc_frames_from_u8_resized)."""
        rh, rw = C.c_int32(), C.c_int32()
        _lib.check(self.lib.tc_frames_from_u8_resized(int(sh), int(sw), int(h), int(w), C.byref(rh), C.byref(rw)),
                   "tc_frames_from_u8_resized")
        return rh.value, rw.value

    def resize_tables(self, n_in, n_out, device):
        """PIL's 8-bit BILINEAR tables of one axis on `device`: resize_tables_filter's bilinear case, as tc_resize_tables is
        tc_resize_tables_filter's."""
        return self.resize_tables_filter("bilinear", n_in, n_out, device)

    def resize_tables_filter(self, filter, n_in, n_out, device):
        """PIL's 8-bit tables of one axis for `filter` ("bilinear", "bicubic", "lanczos", "box") on `device`: (bounds [n_out, 2],
        coefs [n_out, kmax]) int32, built on the host by tc_resize_tables_filter and kept per (filter, n_in, n_out, device)."""
        key = (str(filter), int(n_in), int(n_out), torch.device(device))
        tabs = self._resize_tables.get(key)
        if tabs is None:
            if key[0] not in _lib.TC_RESIZE_FILTERS:
                raise ValueError(f"resize filter {filter!r}: one of {sorted(_lib.TC_RESIZE_FILTERS)}")
            code = _lib.TC_RESIZE_FILTERS[key[0]]
            kmax = self.lib.tc_resize_tables_filter(code, key[1], key[2], None, None, 0)
            _lib.check(min(kmax, 0), "tc_resize_tables_filter")
            bounds = torch.empty((key[2], 2), dtype=torch.int32)
            coefs = torch.empty((key[2], kmax), dtype=torch.int32)
            i32p = C.POINTER(C.c_int32)
            rc = self.lib.tc_resize_tables_filter(code, key[1], key[2], C.cast(bounds.data_ptr(), i32p), C.cast(coefs.data_ptr(), i32p),
                                                  coefs.numel())
            _lib.check(min(rc, 0), "tc_resize_tables_filter")
            tabs = self._resize_tables[key] = (bounds.to(key[3]), coefs.to(key[3]))
        return tabs

    def _axis_tables(self, filter, n_in, n_out, device):
        """(bounds, coefs) of one axis of a request, (None, None) where it keeps its size: that pass does not run."""
        return self.resize_tables_filter(filter, n_in, n_out, device) if n_out != n_in else (None, None)

    def _front_tables(self, sh, sw, h, w, device):
        """(h_bounds, h_coefs, v_bounds, v_coefs) of a front-end request for (sh, sw) images into (h, w) frames: both axes are
        resized or neither (tc_frames_from_u8_resized), then all four are None."""
        rh, rw = self.resized_size(sh, sw, h, w)
        return self._axis_tables("bilinear", sw, rw, device) + self._axis_tables("bilinear", sh, rh, device)

    @staticmethod
    def _set_tables(p, tabs):
        """A pair of axes (h_bounds, h_coefs, v_bounds, v_coefs, None for an axis that keeps its size) into any of the pixel
        path's params structs."""
        for axis, bounds, coefs in (("h", *tabs[:2]), ("v", *tabs[2:])):
            if bounds is not None:
                setattr(p, axis + "_bounds", bounds.data_ptr())
                setattr(p, axis + "_coefs", coefs.data_ptr())
                setattr(p, axis + "_kmax", coefs.shape[1])

    def _launch(self, entry, p, device):
        """The tail of an entry point whose params carry their workspace: query it, allocate, set, call, check."""
        p.workspace_bytes = getattr(self.lib, entry + "_workspace")(C.byref(p))
        ws = self._workspace(p.workspace_bytes, device)
        p.workspace = ws.data_ptr()
        _lib.check(getattr(self.lib, entry)(C.byref(p), _stream()), entry)

    def _front_launch(self, entry, p, slots, tabs, device, sources):
        """A front-end request, at most TC_FRAMES_U8_MAX images to a call: sources(i) gives the fields of `p` that point at
        image i, the first of a call's."""
        self._set_tables(p, tabs)
        for i in range(0, len(slots), _lib.TC_FRAMES_U8_MAX):
            part = slots[i:i + _lib.TC_FRAMES_U8_MAX]
            held = (C.c_int32 * len(part))(*part)
            p.n, p.slots = len(part), held
            for field, pointer in sources(i).items():
                setattr(p, field, pointer)
            self._launch(entry, p, device)

    @staticmethod
    def _front_args(what, n, size, slots, b, t, out):
        """The checked (h, w) and slots of a front-end request for n images; `out`, where given, is the clip tensor they name."""
        h, w = (int(v) for v in size)
        slots = [int(s) for s in slots]
        if len(slots) != n or any(s < 0 or s >= b * t for s in slots):
            raise ValueError(f"{what}: {n} images need {n} slots in [0, {b * t}), got {slots}")
        if out is not None:
            _dev(out, torch.float32, f"{what}: out")
            if tuple(out.shape) != (b, 3, t, h, w):
                raise ValueError(f"{what}: out must be ({b}, 3, {t}, {h}, {w}), got {tuple(out.shape)}")
        return (h, w), slots

    @staticmethod
    def _check_u8_images(images, what):
        """(n, sh, sw, 3) uint8, pixels packed (a row may be padded: stride(1) >= 3 * sw), on the device."""
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
            raise ValueError(f"{what}: expected a uint8 tensor, got {getattr(images, 'dtype', type(images))}")
        if images.dim() != 4 or images.shape[3] != 3 or 0 in images.shape:
            raise ValueError(f"{what}: expected (n, h, w, 3) images, got {tuple(images.shape)}")
        n, sh, sw, _ = images.shape
        if images.stride(3) != 1 or images.stride(2) != 3 or images.stride(1) < 3 * sw or (n > 1 and images.stride(0) < sh * images.stride(1)):
            raise ValueError(f"{what}: pixels must be packed HWC (strides {images.stride()})")
        if not images.is_cuda:
            raise _lib.TooncrafterHipError(f"{what}: expected a CUDA tensor: the product path is GPU-only")

    def frames_from_u8(self, images, size, slots, *, b, t, out=None):
        """uint8 (n, sh, sw, 3) images -> frames of a (b, 3, t, H, W) fp32 clip tensor, size = (H, W): the script's
        Resize(min(size)) / CenterCrop(size) / ToTensor / Normalize(0.5, 0.5) on PIL images (inference.py:64-69), bit for bit
        (tc_frames_from_u8).  Image i goes to frame slots[i] = batch * t + frame.  `out`: written in place, frames no slot names
        keep their contents; default: a new tensor, zero there."""
        self._check_u8_images(images, "frames_from_u8: images")
        n, sh, sw, _ = images.shape
        (h, w), slots = self._front_args("frames_from_u8", n, size, slots, b, t, out)
        if out is None:
            out = torch.zeros((b, 3, t, h, w), dtype=torch.float32, device=images.device)
        p = _lib.TcFramesU8Params(pitch=images.stride(1), image_stride=images.stride(0) if n > 1 else sh * images.stride(1),
                                  sh=sh, sw=sw, out=out.data_ptr(), b=b, t=t, h=h, w=w)
        self._front_launch("tc_frames_from_u8", p, slots, self._front_tables(sh, sw, h, w, images.device), images.device,
                           lambda i: {"src": images[i].data_ptr()})
        return out

    def yuv_matrix(self, standard="bt601", range="limited", bits=8):
        """The seven integers {cy, crv, cgu, cgv, cbu, yoff, coff} of a YCbCr -> RGB conversion (tc_yuv_matrix; host only):
        standard "bt601" | "bt709", range "limited" | "full", bits 8 | 10."""
        if standard not in _lib.TC_YUV_STANDARDS or range not in _lib.TC_YUV_RANGES:
            raise ValueError(f"yuv_matrix: standard {standard!r} (one of {sorted(_lib.TC_YUV_STANDARDS)}), "
                             f"range {range!r} (one of {sorted(_lib.TC_YUV_RANGES)})")
        m = (C.c_int32 * 7)()
        _lib.check(self.lib.tc_yuv_matrix(_lib.TC_YUV_STANDARDS[standard], _lib.TC_YUV_RANGES[range], int(bits), m), "tc_yuv_matrix")
        return list(m)

    def _frames_yuv_args(self, planes, size, slots, b, t, out):
        """The checked request of frames_from_yuv: (layout, matrix, (h, w), slots, out)."""
        lay = planes_layout(planes, "frames_from_yuv: planes")
        if not planes.y.is_cuda:
            raise _lib.TooncrafterHipError("frames_from_yuv: planes: expected CUDA tensors: the product path is GPU-only")
        (h, w), slots = self._front_args("frames_from_yuv", lay["n"], size, slots, b, t, out)
        m = self.yuv_matrix(planes.standard, planes.range, 10 if lay["wide"] else 8) if planes.matrix is None else [int(v) for v in planes.matrix]
        return lay, m, (h, w), slots, out

    def frames_from_yuv(self, planes, size, slots, *, b, t, out=None):
        """Planar 4:2:0 images (`clip.Planes`: I420, NV12 or P010, rows pitched as their strides say) -> frames of a
        (b, 3, t, H, W) fp32 clip tensor: chroma upsampled by `planes.siting`, YCbCr -> RGB in integers by the matrix of
        `planes.standard` / `planes.range` (or `planes.matrix`), then frames_from_u8's transform of that RGB image, bit for bit
        (tc_frames_from_yuv).  slots / out as in frames_from_u8."""
        lay, m, (h, w), slots, out = self._frames_yuv_args(planes, size, slots, b, t, out)
        sh, sw, dev = lay["sh"], lay["sw"], planes.y.device
        if out is None:
            out = torch.zeros((b, 3, t, h, w), dtype=torch.float32, device=dev)
        p = _lib.TcFramesYuvParams(image_stride_y=lay["image_stride_y"], image_stride_c=lay["image_stride_c"], pitch_y=lay["pitch_y"],
                                   pitch_c=lay["pitch_c"], format=lay["format"], siting=_lib.TC_CHROMA_SITINGS[planes.siting],
                                   m=(C.c_int32 * 7)(*m), sh=sh, sw=sw, out=out.data_ptr(), b=b, t=t, h=h, w=w)
        self._front_launch("tc_frames_from_yuv", p, slots, self._front_tables(sh, sw, h, w, dev), dev,
                           lambda i: dict(zip(("y", "c0", "c1"), (plane[i].data_ptr() for plane in (planes.y,) + planes.chroma))))
        return out

    @staticmethod
    def _frames_out_args(x, size, filter, fmt, frames, what="frames_to_u8"):
        """The checked request of frames_to_u8 (or of `what`, which shares its rules): (oh, ow, format code, f0, nf, bytes of a
        packed row, bytes of a packed frame)."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise ValueError(f"{what}: x: expected an fp32 tensor, got {getattr(x, 'dtype', type(x))}")
        if x.dim() != 5 or x.shape[1] != 3 or 0 in x.shape:
            raise ValueError(f"{what}: x must be (b, 3, t, h, w), got {tuple(x.shape)}")
        if fmt not in _lib.TC_PIXFMTS:
            raise ValueError(f"{what}: fmt {fmt!r}: one of {sorted(_lib.TC_PIXFMTS)}")
        if filter not in _lib.TC_RESIZE_FILTERS:
            raise ValueError(f"{what}: filter {filter!r}: one of {sorted(_lib.TC_RESIZE_FILTERS)}")
        t, h, w = x.shape[2:]
        oh, ow = (h, w) if size is None else (int(v) for v in size)
        if oh <= 0 or ow <= 0:
            raise ValueError(f"{what}: size {(oh, ow)}")
        f0, nf = (0, t) if frames is None else (int(v) for v in frames)
        if f0 < 0 or nf < 1 or f0 + nf > t:
            raise ValueError(f"{what}: frames (first, count) = {(f0, nf)} outside a clip of {t}")
        if fmt != "rgb24" and (oh % 2 or ow % 2):
            raise ValueError(f"{what}: {fmt} needs an even size, got {(oh, ow)}")
        if not x.is_cuda:
            raise _lib.TooncrafterHipError(f"{what}: x: expected a CUDA tensor: the product path is GPU-only")
        row = 3 * ow if fmt == "rgb24" else ow
        return oh, ow, _lib.TC_PIXFMTS[fmt], f0, nf, row, row * oh if fmt == "rgb24" else oh * ow * 3 // 2

    def frames_to_u8(self, x, size=None, filter="bicubic", fmt="rgb24", frames=None, out=None, strides=None):
        """Frames of the decoder's (b, 3, t, h, w) fp32 clips -> uint8 frames on the device (tc_frames_to_u8): tc_video_to_u8's
        value arithmetic, PIL's 8-bit two-pass resample to size = (oh, ow) with `filter` ("bilinear", "bicubic", "lanczos",
        "box"; None: the clip's own size, nothing resampled), then fmt "rgb24" (HWC), "i420" or "nv12" (BT.601 limited range, in
        integers).  frames = (first, count): which frames of every clip (None: all).
        Returns a new (b, nf, oh, ow, 3) tensor for rgb24, (b, nf, oh * ow * 3 / 2) for the planar formats.
        out: a contiguous uint8 device buffer written in place instead, frame first + j of clip i at byte
        i * clip_stride + j * frame_stride, rows `pitch` bytes apart, strides = (pitch, frame_stride, clip_stride) (None: packed);
        the bytes between rows, frames and clips keep their contents.  Returns `out`."""
        oh, ow, code, f0, nf, row, frame = self._frames_out_args(x, size, filter, fmt, frames)
        x = x.contiguous()
        b, _, t, h, w = x.shape
        pitch, frame_stride, clip_stride = (row, frame, nf * frame) if strides is None else (int(v) for v in strides)
        if out is None:
            if strides is not None:
                raise ValueError("frames_to_u8: strides describe an `out` buffer")
            out = torch.empty((b, nf, oh, ow, 3) if fmt == "rgb24" else (b, nf, frame), dtype=torch.uint8, device=x.device)
        else:
            _dev(out, torch.uint8, "frames_to_u8: out")
            if out.device != x.device:
                raise ValueError(f"frames_to_u8: out is on {out.device}, x on {x.device}")
        p = _lib.TcFramesOutParams(x=x.data_ptr(), out=out.data_ptr(), b=b, t=t, h=h, w=w, f0=f0, nf=nf, oh=oh, ow=ow, format=code,
                                   pitch=pitch, frame_stride=frame_stride, clip_stride=clip_stride)
        self._set_tables(p, self._axis_tables(filter, w, ow, x.device) + self._axis_tables(filter, h, oh, x.device))
        # the last byte the kernels may write: a frame's bytes by the header's rule, at the last place
        used = pitch * oh if fmt == "rgb24" else pitch * oh + (2 * (pitch // 2) * (oh // 2) if fmt == "i420" else pitch * (oh // 2))
        if pitch < row or frame_stride < used or (b > 1 and clip_stride < nf * frame_stride) or \
                (b - 1) * clip_stride + (nf - 1) * frame_stride + used > out.numel():
            raise ValueError(f"frames_to_u8: strides (pitch, frame, clip) = {(pitch, frame_stride, clip_stride)} do not fit {b} x {nf} "
                             f"frames of {used} bytes into an out of {out.numel()} bytes")
        self._launch("tc_frames_to_u8", p, x.device)
        return out

    def yuv_out_matrix(self, standard="bt601", range="limited", bits=8):
        """The eleven integers {yr, yg, yb, ur, ug, ub, vr, vg, vb, yoff, coff} of an RGB -> YCbCr conversion
        (tc_yuv_out_matrix; host only): standard "bt601" | "bt709", range "limited" | "full", bits 8 | 10 (10: for the 16-bit
        RGB of the P010 path)."""
        if standard not in _lib.TC_YUV_STANDARDS or range not in _lib.TC_YUV_RANGES:
            raise ValueError(f"yuv_out_matrix: standard {standard!r} (one of {sorted(_lib.TC_YUV_STANDARDS)}), "
                             f"range {range!r} (one of {sorted(_lib.TC_YUV_RANGES)})")
        m = (C.c_int32 * 11)()
        _lib.check(self.lib.tc_yuv_out_matrix(_lib.TC_YUV_STANDARDS[standard], _lib.TC_YUV_RANGES[range], int(bits), m),
                   "tc_yuv_out_matrix")
        return list(m)

    def _frames_yuv_out_args(self, x, size, filter, fmt, colour, frames):
        """The checked request of frames_to_yuv: _frames_out_args' tuple with P010's format code and doubled bytes for a 10-bit
        colour, then the matrix and the siting code."""
        what = "frames_to_yuv"
        if any(not hasattr(colour, a) for a in ("standard", "range", "siting", "bits")):
            raise ValueError(f"{what}: colour: expected an output.Colour, got {type(colour).__name__}")
        if fmt not in ("i420", "nv12"):
            raise ValueError(f"{what}: fmt {fmt!r}: a colour describes planar frames, 'i420' or 'nv12'")
        if colour.siting not in ("center", "left"):
            raise ValueError(f"{what}: siting {colour.siting!r}: chroma is produced 'center' or 'left'")
        if colour.bits not in (8, 10) or (colour.bits == 10 and fmt != "nv12"):
            raise ValueError(f"{what}: bits {colour.bits!r} with {fmt}: 8, or 10 with 'nv12' (P010)")
        oh, ow, code, f0, nf, row, frame = self._frames_out_args(x, size, filter, fmt, frames, what)
        m = self.yuv_out_matrix(colour.standard, colour.range, colour.bits)
        if colour.bits == 10:
            code, row, frame = _lib.TC_YUV_FORMATS["p010"], 2 * row, 2 * frame
        return oh, ow, code, f0, nf, row, frame, m, _lib.TC_CHROMA_SITINGS[colour.siting]

    def frames_to_yuv(self, x, size=None, filter="bicubic", fmt="nv12", colour=None, frames=None, out=None, strides=None):
        """frames_to_u8 for planar frames in a named colour (tc_frames_to_yuv): `colour` (an `output.Colour`) picks the integer
        RGB -> YCbCr matrix (standard, range), where the chroma samples sit ("center": 2 x 2 means; "left": H.264's default) and
        the depth -- bits 8 writes fmt "i420" / "nv12", bits 10 (fmt "nv12" only) P010: 16-bit words, code << 6, from a 16-bit
        RGB intermediate.  size / filter / frames / out / strides (bytes) as in frames_to_u8.
        Returns a new uint8 (b, nf, oh * ow * 3 / 2) tensor, (b, nf, oh * ow * 3) bytes for P010, or `out`."""
        oh, ow, code, f0, nf, row, frame, m, siting = self._frames_yuv_out_args(x, size, filter, fmt, colour, frames)
        x = x.contiguous()
        b, _, t, h, w = x.shape
        pitch, frame_stride, clip_stride = (row, frame, nf * frame) if strides is None else (int(v) for v in strides)
        if out is None:
            if strides is not None:
                raise ValueError("frames_to_yuv: strides describe an `out` buffer")
            out = torch.empty((b, nf, frame), dtype=torch.uint8, device=x.device)
        else:
            _dev(out, torch.uint8, "frames_to_yuv: out")
            if out.device != x.device:
                raise ValueError(f"frames_to_yuv: out is on {out.device}, x on {x.device}")
        p = _lib.TcFramesYuvOutParams(x=x.data_ptr(), out=out.data_ptr(), b=b, t=t, h=h, w=w, f0=f0, nf=nf, oh=oh, ow=ow, format=code,
                                      pitch=pitch, frame_stride=frame_stride, clip_stride=clip_stride, siting=siting,
                                      m=(C.c_int32 * 11)(*m))
        self._set_tables(p, self._axis_tables(filter, w, ow, x.device) + self._axis_tables(filter, h, oh, x.device))
        used = pitch * oh + (2 * (pitch // 2) * (oh // 2) if fmt == "i420" else pitch * (oh // 2))     # the header's frame bytes
        if pitch < row or frame_stride < used or (b > 1 and clip_stride < nf * frame_stride) or \
                (b - 1) * clip_stride + (nf - 1) * frame_stride + used > out.numel():
            raise ValueError(f"frames_to_yuv: strides (pitch, frame, clip) = {(pitch, frame_stride, clip_stride)} do not fit {b} x {nf} "
                             f"frames of {used} bytes into an out of {out.numel()} bytes")
        self._launch("tc_frames_to_yuv", p, x.device)
        return out

    def clip_patches(self, x, *, size, patch, ld, mean, std, antialias=True):
        """(B, 3, H, W) fp32 in [-1, 1] -> bf16 rows [B * (size / patch)^2, ld], the A operand of the CLIP image tower's
        patch-embedding GEMM: kornia's antialiased bicubic resize to (size, size), (x + 1) / 2, (x - mean) / std and the
        unfold (condition.py:322-330 of the reference and open_clip's conv1), columns from 3 * patch^2 on zero
        (tc_clip_patches)."""
        if _dev(x, torch.float32, "clip_patches: x") is None or x.dim() != 4 or x.shape[1] != 3 or 0 in x.shape:
            raise ValueError(f"clip_patches: x must be (B, 3, H, W), got {None if x is None else tuple(x.shape)}")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("clip_patches: mean and std have three entries")
        size, patch, ld = int(size), int(patch), int(ld)
        if patch <= 0 or size <= 0 or size % patch or ld < 3 * patch * patch:
            raise ValueError(f"clip_patches: size {size}, patch {patch}, ld {ld}")
        b, _, h, w = x.shape
        out = torch.empty((b * (size // patch) ** 2, ld), dtype=BF16, device=x.device)
        p = _lib.TcClipPatchesParams(x=x.data_ptr(), out=out.data_ptr(), b=b, h=h, w=w, size=size, patch=patch, ld=ld,
                                     antialias=1 if antialias else 0)
        p.mean[:], p.std[:] = [float(v) for v in mean], [float(v) for v in std]
        self._launch("tc_clip_patches", p, x.device)
        return out

    @staticmethod
    def _randn_args(seeds, shape, stream, what="randn_clips"):
        shape = tuple(int(v) for v in shape)
        if len(shape) < 1 or min(shape) <= 0:
            raise ValueError(f"{what}: shape (b, ...) with positive sizes, got {shape}")
        stream = int(stream)
        if not 0 <= stream < 1 << 32:
            raise ValueError(f"{what}: stream {stream} outside [0, 2^32)")
        return clip_seeds(seeds, shape[0], f"{what}: seeds"), shape, stream

    def randn_clips(self, seeds, shape, stream, scale=1.0, out=None, raw=False):
        """Gaussian noise of shape (b, ...), clip i drawn from seeds[i] alone (tc_randn_clips): Philox4x32-10 keyed by the
        seed, counter (element >> 2, 0, stream, 0), Box-Muller, times `scale`.  The row of a seed is the same bits in any
        batch, slot or process; the torch generator is not touched.  `stream` names the draw (lvdm/ddim.py numbers the
        sampler's).  `raw`: the Philox words themselves, as int32 bit patterns.  `out`: a contiguous fp32 (raw: fp32 or
        int32) device tensor of that shape to fill instead of a new one."""
        seeds, shape, stream = self._randn_args(seeds, shape, stream)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32 if raw else torch.float32, device="cuda")
        else:
            words_as_int = raw and getattr(out, "dtype", None) == torch.int32
            _dev(out, torch.int32 if words_as_int else torch.float32, "randn_clips: out")
            if tuple(out.shape) != shape:
                raise ValueError(f"randn_clips: out must be {shape}, got {tuple(out.shape)}")
        b = shape[0]
        held = (C.c_uint64 * b)(*seeds)
        p = _lib.TcRandnParams(out=out.data_ptr(), seeds=held, b=b, n=out.numel() // b, stream=stream, scale=float(scale),
                               raw=1 if raw else 0)
        _lib.check(self.lib.tc_randn_clips(C.byref(p), _stream()), "tc_randn_clips")
        return out

    def ddim_step(self, x, e_cond, e_uncond, noise, *, cfg_scale, guidance_rescale, sqrt_ac, sqrt_1m_ac,
                  sqrt_a_prev, dir_coef, sigma, x0_rescale, want_x0=True, e_uncond_img=None, cfg_img=None,
                  parameterization="v"):
        """One fused DDIM update.  With `e_uncond_img` the guidance is the three-way form of
        ddim_multiplecond.py:236 (cfg_img defaults to cfg_scale like the reference).  `parameterization` says what the
        model predicts: "v" (tc_ddim_step) or "eps" (tc_ddim_step_eps, ddim.py:234, 258)."""
        p, x_prev, x0 = HipOps._ddim_params("ddim_step", x, e_cond, e_uncond, noise, e_uncond_img, None, want_x0, parameterization,
                                            cfg_scale=cfg_scale, guidance_rescale=guidance_rescale, sqrt_ac=sqrt_ac,
                                            sqrt_1m_ac=sqrt_1m_ac, sqrt_a_prev=sqrt_a_prev, dir_coef=dir_coef, sigma=sigma,
                                            x0_rescale=x0_rescale, cfg_img=cfg_img)
        self._ddim_launch("tc_ddim_step", parameterization, p, p.b, x.device)
        return x_prev, x0

    def _ddim_launch(self, entry, parameterization, params, b, device):
        """The launch tail of a step after `_ddim_params`: the workspace, then `entry` or its `_eps` form on `params`."""
        if parameterization != "v":
            entry += "_eps"
        nbytes = self.lib.tc_ddim_workspace(b)
        ws = self._workspace(nbytes, device)
        _lib.check(getattr(self.lib, entry)(C.byref(params), ws.data_ptr(), nbytes, _stream()), entry)

    @staticmethod
    def _ddim_params(what, x, e_cond, e_uncond, noise, e_uncond_img, pred_x0, want_x0, parameterization, *, cfg_scale,
                     guidance_rescale, sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef, sigma, x0_rescale, cfg_img, also=()):
        """The checked TcDdimParams of a step and its two results: (p, x_prev, pred_x0).  `pred_x0`: the caller's tensor for
        that result, or None for a new one (no tensor at all when `want_x0` is false).  `also`: further operands to check."""
        if parameterization not in ("v", "eps"):
            raise NotImplementedError(f"{what}: parameterization {parameterization!r} (the fused step has 'v' and 'eps')")
        for tns in (x, e_cond, e_uncond, noise, e_uncond_img, pred_x0, *also):
            if tns is not None and (tns.dtype != torch.float32 or not tns.is_contiguous() or not tns.is_cuda):
                raise ValueError(f"{what}: contiguous fp32 CUDA tensors")
        b = x.shape[0]
        n = x.numel() // b
        x_prev = torch.empty_like(x)
        x0 = pred_x0 if pred_x0 is not None else (torch.empty_like(x) if want_x0 else None)
        p = TcDdimParams()
        p.x, p.e_cond, p.e_uncond, p.noise = x.data_ptr(), e_cond.data_ptr(), _ptr(e_uncond), _ptr(noise)
        p.x_prev, p.pred_x0 = x_prev.data_ptr(), _ptr(x0)
        p.b, p.n = b, n
        p.cfg_scale, p.guidance_rescale = float(cfg_scale), float(guidance_rescale)
        p.sqrt_ac, p.sqrt_1m_ac, p.sqrt_a_prev = float(sqrt_ac), float(sqrt_1m_ac), float(sqrt_a_prev)
        p.dir_coef, p.sigma, p.x0_rescale = float(dir_coef), float(sigma), float(x0_rescale)
        p.e_uncond_img = _ptr(e_uncond_img)
        p.cfg_img = float(cfg_scale if cfg_img is None else cfg_img)
        return p, x_prev, x0

    def ddim_step_ms(self, x, e_cond, e_uncond, noise, x0_hist, *, corr, cfg_scale, guidance_rescale, sqrt_ac, sqrt_1m_ac,
                     sqrt_a_prev, dir_coef, sigma, x0_rescale, want_x0=True, e_uncond_img=None, cfg_img=None,
                     parameterization="v", pred_x0=None):
        """`ddim_step` plus the second-order multistep term (tc_ddim_step_ms / tc_ddim_step_ms_eps):
        x_prev += corr * (x0u - x0_hist), x0u the prediction before `x0_rescale`, `x0_hist` the pred_x0 the previous step
        returned (None: no history) and `corr` the host scalar of DDIMSampler.multistep_corr.  With x0_hist None or corr 0
        the results are `ddim_step`'s bits.  `pred_x0`: a tensor to take that result -- it may be `x0_hist` itself (the
        history updated in place); any other overlap of it with `x0_hist` is refused (TC_EINVAL), as is a non-finite corr."""
        for tns in (x0_hist, pred_x0):
            if tns is not None and tns.shape != x.shape:
                raise ValueError(f"ddim_step_ms: shape {tuple(tns.shape)} against x {tuple(x.shape)}")
        p, x_prev, x0 = HipOps._ddim_params("ddim_step_ms", x, e_cond, e_uncond, noise, e_uncond_img, pred_x0, want_x0,
                                            parameterization, cfg_scale=cfg_scale, guidance_rescale=guidance_rescale,
                                            sqrt_ac=sqrt_ac, sqrt_1m_ac=sqrt_1m_ac, sqrt_a_prev=sqrt_a_prev, dir_coef=dir_coef,
                                            sigma=sigma, x0_rescale=x0_rescale, cfg_img=cfg_img, also=(x0_hist,))
        mp = _lib.TcDdimMsParams(base=p, x0_hist=_ptr(x0_hist), corr=float(corr))
        self._ddim_launch("tc_ddim_step_ms", parameterization, mp, p.b, x.device)
        return x_prev, x0

    def ddim_blend(self, x, x0, noise, mask, *, sqrt_ac=1.0, sqrt_1m_ac=0.0, out=None):
        """orig = sqrt_ac * x0 + sqrt_1m_ac * noise (noise None: x0 itself); result = orig * mask + (1 - mask) * x (mask None:
        orig) -- the pinned-frame blend of ddim.py:176-180, q_sample and stochastic_encode, every operation rounded on its own.
        Tensors of one shape (B, ...), fp32, contiguous.  `out` may be `x` itself (in place); default: a new tensor."""
        for tns in (x, x0, noise, mask, out):
            if tns is not None and (tns.dtype != torch.float32 or not tns.is_contiguous() or not tns.is_cuda):
                raise ValueError("ddim_blend: contiguous fp32 CUDA tensors")
        for tns in (x, noise, mask, out):
            if tns is not None and tns.shape != x0.shape:
                raise ValueError(f"ddim_blend: shape {tuple(tns.shape)} against x0 {tuple(x0.shape)}")
        if x0.dim() < 1:
            raise ValueError("ddim_blend: tensors of shape (B, ...)")
        if out is None:
            out = torch.empty_like(x0)
        b = x0.shape[0]
        p = TcDdimBlendParams()
        p.x, p.x0, p.noise, p.mask, p.out = _ptr(x), x0.data_ptr(), _ptr(noise), _ptr(mask), out.data_ptr()
        p.b, p.n = b, (x0.numel() // b if b else 0)
        p.sqrt_ac, p.sqrt_1m_ac = float(sqrt_ac), float(sqrt_1m_ac)
        _lib.check(self.lib.tc_ddim_blend(C.byref(p), _stream()), "tc_ddim_blend")
        return out

    # ------------------------------------------------------------------ colour match and histogram transfer (tc_colour_*)
    # The helpers state each check once for both families and both bindings (torch_ops.TorchLibOps marshals their results).
    @staticmethod
    def _colour_clip(x, what):
        """The (b, t, h, w) of a (b, 3, t, h, w) fp32 contiguous device clip, or raise."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.TooncrafterHipError(f"{what}: expected a CUDA tensor, got {getattr(x, 'device', type(x))}: the product "
                                           "path is GPU-only")
        if x.dtype != torch.float32 or x.dim() != 5 or x.shape[1] != 3 or x.numel() == 0 or not x.is_contiguous():
            raise ValueError(f"{what}: expected contiguous fp32 (b, 3, t, h, w), got {tuple(x.shape)} {x.dtype}")
        return x.shape[0], x.shape[2], x.shape[3], x.shape[4]

    @staticmethod
    def _colour_frames(frames, t, what):
        """The checked (f0, nf, fstep) of a statistics request on clips of t frames; None: every frame."""
        f0, nf, fstep = (0, t, 1) if frames is None else (int(v) for v in frames)
        if nf < 1 or not 0 <= f0 < t or (nf > 1 and (fstep < 1 or f0 + (nf - 1) * fstep > t - 1)):
            raise ValueError(f"{what}: frames (f0, nf, fstep) = {(f0, nf, fstep)} outside a clip of {t}")
        return f0, nf, fstep

    @staticmethod
    def _colour_knots(knots, max_gain, t, what):
        """The checked (knot indices, gain limit) of a knots call on clips of t frames.  knots None: the two ends ((0,) when
        t = 1); max_gain None: 0.0, no limit."""
        knots = ((0, t - 1) if t > 1 else (0,)) if knots is None else tuple(knots)
        if any(isinstance(k, bool) or not isinstance(k, int) for k in knots):
            raise ValueError(f"{what}: knots {knots!r}: frame indices")
        if not 1 <= len(knots) <= _lib.TC_TEMPORAL_MAX_FRAMES or knots[0] < 0 or knots[-1] >= t \
                or any(a >= b for a, b in zip(knots, knots[1:])):
            raise ValueError(f"{what}: knots {knots!r}: 1 .. {_lib.TC_TEMPORAL_MAX_FRAMES} strictly increasing frame indices in "
                             f"[0, {t})")
        gain = 0.0 if max_gain is None else float(max_gain)
        if isinstance(max_gain, bool) or not (gain == 0.0 or 1.0 <= gain < float("inf")):        # NaN fails the comparison too
            raise ValueError(f"{what}: max_gain {max_gain!r}: None or 0 (no limit), or a finite number >= 1")
        return knots, gain

    @staticmethod
    def _colour_refs(what, x, src, ref, knots, dtype, tail):
        """`src` (b, t, *tail) of the clip x and `ref` (b, rows, *tail) of its reference images -- one per knot, two when
        `knots` is None -- as contiguous device tensors of `dtype`, or raise."""
        b, t = x.shape[0], x.shape[2]
        for which, s, rows in (("src", src, t), ("ref", ref, 2 if knots is None else len(knots))):
            if not isinstance(s, torch.Tensor) or not s.is_cuda:
                raise _lib.TooncrafterHipError(f"{what}: {which}: expected a CUDA tensor: the product path is GPU-only")
            if s.dtype != dtype or s.shape != (b, rows) + tail or not s.is_contiguous():
                raise ValueError(f"{what}: {which}: expected contiguous {str(dtype)[6:]} {(b, rows) + tail}, got {tuple(s.shape)} "
                                 f"{s.dtype}")

    # (entry point, params struct) of a family towards the two ends, and of its knots form
    _COLOUR_MATCH = (("tc_colour_match", _lib.TcColourMatchParams), ("tc_colour_match_knots", _lib.TcColourMatchKnotsParams))
    _COLOUR_TRANSFER = (("tc_colour_transfer", _lib.TcColourTransferParams),
                        ("tc_colour_transfer_knots", _lib.TcColourTransferKnotsParams))

    def _colour_clip_call(self, forms, x, dims, out, knots, result, tail, fields):
        """The call of a checked clip request on x ((b, t, h, w) = dims): the first of `forms` (one of the pairs above) towards the
        two ends (knots None), the second through `knots`, with the further params `fields`.  `out` may be x itself; None: a new
        tensor.  Returns (out, the fp32 (b, t) + tail tensor that the params field `result` takes: coefficients or tables)."""
        if out is None:
            out = torch.empty_like(x)
        elif self._colour_clip(out, f"{forms[0][0][3:]}: out") != dims or out.device != x.device:
            raise ValueError(f"{forms[0][0][3:]}: out {tuple(out.shape)} against x {tuple(x.shape)}")
        b, t, h, w = dims
        res = torch.empty((b, t) + tail, dtype=torch.float32, device=x.device)
        fields[result] = res.data_ptr()
        entry, struct = forms[knots is not None]
        p = struct(x=x.data_ptr(), out=out.data_ptr(), b=b, t=t, h=h, w=w, **fields)
        if knots is not None:
            p.nk = len(knots)
            p.knot[:len(knots)] = knots
        _lib.check(getattr(self.lib, entry)(C.byref(p), _stream()), entry)
        return out, res

    @staticmethod
    def _colour_match_request(x, src, ref, ref_pixels, method, strength, knots, max_gain):
        """The checked request of a match on the clip x: ((b, t, h, w), knots, gain, method code, strength, ref_pixels).  The
        entry point is chosen here, once for both bindings: knots None (neither `knots` nor `max_gain` given) is tc_colour_match
        on the two ends; otherwise tc_colour_match_knots, an omitted `knots` spelled out as the two ends and an omitted
        `max_gain` as 0."""
        dims = HipOps._colour_clip(x, "colour_match: x")
        gain = 0.0
        if knots is not None or max_gain is not None:
            knots, gain = HipOps._colour_knots(knots, max_gain, dims[1], "colour_match")
        HipOps._colour_refs("colour_match", x, src, ref, knots, torch.float64, (_lib.TC_COLOUR_STATS,))
        code = _lib.TC_COLOUR_METHODS.get(method, method)
        if isinstance(code, bool) or code not in _lib.TC_COLOUR_METHODS.values():
            raise ValueError(f"colour_match: method {method!r}: one of {tuple(_lib.TC_COLOUR_METHODS)}")
        strength, ref_pixels = float(strength), int(ref_pixels)
        if not 0.0 <= strength <= 1.0 or ref_pixels <= 0:                      # NaN fails the comparison too
            raise ValueError(f"colour_match: strength {strength} outside [0, 1] or ref_pixels {ref_pixels} <= 0")
        return dims, knots, gain, code, strength, ref_pixels

    @staticmethod
    def _colour_transfer_request(x, src, ref, ref_pixels, strength, base, knots):
        """The checked request of a histogram transfer on the clip x: ((b, t, h, w), knots, strength, ref_pixels).  knots None
        is tc_colour_transfer on the two ends, otherwise tc_colour_transfer_knots."""
        dims = HipOps._colour_clip(x, "colour_transfer: x")
        if knots is not None:
            knots, _ = HipOps._colour_knots(knots, None, dims[1], "colour_transfer")
        HipOps._colour_refs("colour_transfer", x, src, ref, knots, torch.int32, (3, _lib.TC_COLOUR_BINS))
        if base is not None and (HipOps._colour_clip(base, "colour_transfer: base") != dims or base.device != x.device):
            raise ValueError(f"colour_transfer: base {tuple(base.shape)} against x {tuple(x.shape)}")
        strength, ref_pixels = float(strength), int(ref_pixels)
        if not 0.0 <= strength <= 1.0 or not 0 < ref_pixels <= 1 << 26 or dims[2] * dims[3] > 1 << 26:
            raise ValueError(f"colour_transfer: strength {strength} outside [0, 1], or ref_pixels {ref_pixels} or h * w "
                             f"{dims[2] * dims[3]} outside [1, 2^26]")
        return dims, knots, strength, ref_pixels

    def colour_stats(self, x, frames=None):
        """Nine float64 sums (r, g, b, rr, rg, rb, gg, gb, bb of the clamped values) per frame f0, f0 + fstep, ... (nf of them;
        frames = (f0, nf, fstep), None: all) of every clip of x (b, 3, t, h, w) fp32: (b, nf, 9), in a summation order fixed by
        h * w alone (tc_colour_stats)."""
        b, t, h, w = self._colour_clip(x, "colour_stats: x")
        f0, nf, fstep = self._colour_frames(frames, t, "colour_stats")
        stats = torch.empty((b, nf, _lib.TC_COLOUR_STATS), dtype=torch.float64, device=x.device)
        p = _lib.TcColourStatsParams(x=x.data_ptr(), b=b, t=t, h=h, w=w, f0=f0, nf=nf, fstep=fstep, stats=stats.data_ptr())
        self._launch("tc_colour_stats", p, x.device)
        return stats

    def colour_hist(self, x, frames=None):
        """3 x 1024 int32 counts (r, g, b; of the clamped values, bin = min(1023, floor((c + 1) * 512))) per frame f0, f0 + fstep,
        ... (nf of them; frames = (f0, nf, fstep), None: all) of every clip of x (b, 3, t, h, w) fp32: (b, nf, 3, 1024)
        (tc_colour_hist)."""
        b, t, h, w = self._colour_clip(x, "colour_hist: x")
        f0, nf, fstep = self._colour_frames(frames, t, "colour_hist")
        hist = torch.empty((b, nf, 3, _lib.TC_COLOUR_BINS), dtype=torch.int32, device=x.device)
        p = _lib.TcColourHistParams(x=x.data_ptr(), b=b, t=t, h=h, w=w, f0=f0, nf=nf, fstep=fstep, hist=hist.data_ptr())
        self._launch("tc_colour_hist", p, x.device)
        return hist

    def colour_match(self, x, src, ref, ref_pixels, method, strength, out=None, knots=None, max_gain=None):
        """x (b, 3, t, h, w) fp32 matched frame by frame to the course between two reference images per clip: `src` (b, t, 9) the
        statistics of x, `ref` (b, 2, 9) those of the reference images over `ref_pixels` pixels each, method "mkl" | "mean_std"
        (or its code), strength in [0, 1].  Returns (matched clip, coefs (b, t, 12) fp32: A' row-major, then o').  `out` may be
        `x` itself (in place); default: a new tensor (tc_colour_match).
        knots: strictly increasing frame indices, one per reference image -- `ref` is then (b, len(knots), 9) and the course
        runs through them; max_gain: a number >= 1 that limits the gain of the map (0: none).  With either given the call is
        tc_colour_match_knots (an omitted `knots` means the two ends); with both None it is tc_colour_match."""
        dims, knots, gain, code, strength, ref_pixels = self._colour_match_request(x, src, ref, ref_pixels, method, strength, knots,
                                                                                   max_gain)
        fields = dict(src=src.data_ptr(), ref=ref.data_ptr(), ref_pixels=ref_pixels, method=code, strength=strength)
        if knots is not None:
            fields["max_gain"] = gain
        return self._colour_clip_call(self._COLOUR_MATCH, x, dims, out, knots, "coefs", (12,), fields)

    def colour_transfer(self, x, src, ref, ref_pixels, strength, base=None, out=None, knots=None):
        """x (b, 3, t, h, w) fp32 carried channel by channel onto the course between the histograms of two reference images per
        clip: `src` (b, t, 3, 1024) the histograms of x, `ref` (b, 2, 3, 1024) those of the reference images over `ref_pixels`
        pixels each, strength in [0, 1] blending against clamp(x), or against clamp(base) when a `base` clip of x's shape is
        given.  Returns (transferred clip, table (b, t, 3, 1024) fp32: the displacement of every bin).  `out` may be `x` itself
        (in place); default: a new tensor (tc_colour_transfer).
        knots: strictly increasing frame indices, one per reference image -- `ref` is then (b, len(knots), 3, 1024) and the
        course runs through them (tc_colour_transfer_knots); None: tc_colour_transfer."""
        dims, knots, strength, ref_pixels = self._colour_transfer_request(x, src, ref, ref_pixels, strength, base, knots)
        fields = dict(base=None if base is None else base.data_ptr(), src=src.data_ptr(), ref=ref.data_ptr(), ref_pixels=ref_pixels,
                      strength=strength)
        return self._colour_clip_call(self._COLOUR_TRANSFER, x, dims, out, knots, "table", (3, _lib.TC_COLOUR_BINS), fields)

    def frame_deltas(self, frames_or_planes, lag=1, tau=8):
        """How much images p and p + lag of n keyframes differ, counted on the surfaces as they lie (tc_frame_deltas): `(n, h, w,
        3)` uint8 frames (rows may be padded) or a `clip.Planes` (I420, NV12, P010; the 8-bit value of a P010 sample is its upper
        byte).  Returns (delta (max(n - lag, 0), 3, 3) int64: per pair and component (Y, Cb, Cr or R, G, B) the sum of |a - b|, the
        number of samples with |a - b| > tau and the L1 distance of the two histograms; hist (n, 3, 64) int32: samples by
        value >> 2).  Exact integers, device tensors, no synchronisation."""
        lag, tau = int(lag), int(tau)
        if lag < 1 or not 0 <= tau <= 255:
            raise ValueError(f"frame_deltas: lag {lag} (at least 1), tau {tau} (0 .. 255)")
        if isinstance(frames_or_planes, torch.Tensor):
            x = frames_or_planes
            self._check_u8_images(x, "frame_deltas: frames")
            n, h, w, _ = x.shape
            fields = dict(y=x.data_ptr(), format=_lib.TC_PIXFMTS["rgb24"], pitch_y=x.stride(1),
                          image_stride_y=x.stride(0) if n > 1 else h * x.stride(1))
            device = x.device
        else:
            planes = frames_or_planes
            lay = planes_layout(planes, "frame_deltas: planes")
            if not planes.y.is_cuda:
                raise _lib.TooncrafterHipError("frame_deltas: planes: expected CUDA tensors: the product path is GPU-only")
            n, h, w = lay["n"], lay["sh"], lay["sw"]
            fields = dict(zip(("y", "c0", "c1"), (plane.data_ptr() for plane in (planes.y,) + tuple(planes.chroma))))
            fields.update({k: lay[k] for k in ("format", "pitch_y", "pitch_c", "image_stride_y", "image_stride_c")})
            device = planes.y.device
        hist = torch.empty((n, 3, _lib.TC_DELTA_BINS), dtype=torch.int32, device=device)
        delta = torch.empty((max(n - lag, 0), 3, 3), dtype=torch.int64, device=device)
        p = _lib.TcFrameDeltaParams(n=n, h=h, w=w, lag=lag, tau=tau, hist=hist.data_ptr(),
                                    delta=delta.data_ptr() if n > lag else None, **fields)
        self._launch("tc_frame_deltas", p, device)
        return delta, hist

    # ------------------------------------------------------------------ still regions (tc_still_map, tc_still_composite)
    @staticmethod
    def _still_ends(ends, what):
        """The (b, H, W) of (b, 3, 2, H, W) fp32 contiguous device keyframes with H and W multiples of the cell, or raise."""
        if not isinstance(ends, torch.Tensor) or not ends.is_cuda:
            raise _lib.TooncrafterHipError(f"{what}: expected a CUDA tensor, got {getattr(ends, 'device', type(ends))}: the product "
                                           "path is GPU-only")
        if ends.dtype != torch.float32 or ends.dim() != 5 or ends.shape[1:3] != (3, 2) or ends.numel() == 0 or not ends.is_contiguous():
            raise ValueError(f"{what}: expected contiguous fp32 (b, 3, 2, H, W), got {tuple(ends.shape)} {ends.dtype}")
        return ends.shape[0], ends.shape[3], ends.shape[4]

    @staticmethod
    def still_rule(tau, grow, feather, what="still_map"):
        """The checked (tau, grow, feather) of a still map: integers, tau in [0, 255], grow >= 0, feather >= 1 and
        grow + feather + 1 <= TC_STILL_MAX_DIST.  Host only."""
        import numbers
        for name, v in (("tau", tau), ("grow", grow), ("feather", feather)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                raise ValueError(f"{what}: {name} {v!r}: an integer")
        tau, grow, feather = int(tau), int(grow), int(feather)
        if not 0 <= tau <= 255 or grow < 0 or feather < 1 or grow + feather + 1 > _lib.TC_STILL_MAX_DIST:
            raise ValueError(f"{what}: tau {tau} (0 .. 255), grow {grow} (>= 0), feather {feather} (>= 1), grow + feather + 1 at most "
                             f"{_lib.TC_STILL_MAX_DIST}")
        return tau, grow, feather

    def still_map(self, ends, tau=8, grow=1, feather=2):
        """Where the two keyframes of every clip agree (tc_still_map; the rule: include/tooncrafter_hip.h): `ends` (b, 3, 2, H, W)
        fp32, H and W multiples of 8.  A pixel has moved if a channel differs by more than `tau` 8-bit code values, an 8 x 8
        cell if one of its pixels has; d is a cell's Chebyshev distance to the nearest moved cell, capped at grow + feather + 1.
        Returns (mask (b, 1, 1, H / 8, W / 8) fp32: 1 where d > grow; alpha (b, H, W) fp32: clamp(d - grow - 1, 0, feather) /
        feather upsampled bilinearly; dist (b, H / 8, W / 8) uint8: d).  Device tensors, no synchronisation."""
        tau, grow, feather = self.still_rule(tau, grow, feather)
        b, hh, ww = self._still_ends(ends, "still_map: ends")
        cell = _lib.TC_STILL_CELL
        if hh % cell or ww % cell:
            raise ValueError(f"still_map: ends of {(hh, ww)} pixels: multiples of {cell}")
        mask = torch.empty((b, 1, 1, hh // cell, ww // cell), dtype=torch.float32, device=ends.device)
        alpha = torch.empty((b, hh, ww), dtype=torch.float32, device=ends.device)
        dist = torch.empty((b, hh // cell, ww // cell), dtype=torch.uint8, device=ends.device)
        p = _lib.TcStillMapParams(ends=ends.data_ptr(), b=b, h=hh, w=ww, tau=tau, grow=grow, feather=feather, mask=mask.data_ptr(),
                                  alpha=alpha.data_ptr(), dist=dist.data_ptr())
        _lib.check(self.lib.tc_still_map(C.byref(p), _stream()), "tc_still_map")
        return mask, alpha, dist

    def still_composite(self, video, ends, alpha, frames=None, out=None):
        """`video` (b, 3, t, H, W) fp32 held to its keyframes `ends` (b, 3, 2, H, W) by the pixel weight `alpha` (b, H, W) in the
        frames (f0, nf) (None: all): with key = e0 + s (e1 - e0), s = j / (t - 1), frame j becomes v where alpha == 0 (bit for
        bit), key where alpha == 1 and v + alpha (key - v) between (tc_still_composite).  `out` may be `video` itself (in
        place); default: a new tensor, whose frames outside the range are copies of video's."""
        b, t, hh, ww = self._colour_clip(video, "still_composite: video")
        if self._still_ends(ends, "still_composite: ends") != (b, hh, ww) or ends.device != video.device:
            raise ValueError(f"still_composite: ends {tuple(ends.shape)} against video {tuple(video.shape)}")
        if not isinstance(alpha, torch.Tensor) or not alpha.is_cuda:
            raise _lib.TooncrafterHipError("still_composite: alpha: expected a CUDA tensor: the product path is GPU-only")
        if alpha.dtype != torch.float32 or alpha.shape != (b, hh, ww) or not alpha.is_contiguous() or alpha.device != video.device:
            raise ValueError(f"still_composite: alpha: expected contiguous fp32 {(b, hh, ww)}, got {tuple(alpha.shape)} {alpha.dtype}")
        f0, nf = (0, t) if frames is None else (int(v) for v in frames)
        if nf < 1 or not 0 <= f0 < t or f0 + nf > t:
            raise ValueError(f"still_composite: frames (f0, nf) = {(f0, nf)} outside a clip of {t}")
        if t < 2 or t > _lib.TC_TEMPORAL_MAX_FRAMES or hh % _lib.TC_STILL_CELL or ww % _lib.TC_STILL_CELL:
            raise ValueError(f"still_composite: clips of {t} frames (2 .. {_lib.TC_TEMPORAL_MAX_FRAMES}) of {(hh, ww)} pixels "
                             f"(multiples of {_lib.TC_STILL_CELL})")
        if out is None:
            out = torch.empty_like(video) if (f0, nf) == (0, t) else video.clone()
        elif self._colour_clip(out, "still_composite: out") != (b, t, hh, ww) or out.device != video.device:
            raise ValueError(f"still_composite: out {tuple(out.shape)} against video {tuple(video.shape)}")
        p = _lib.TcStillCompositeParams(video=video.data_ptr(), ends=ends.data_ptr(), alpha=alpha.data_ptr(), out=out.data_ptr(),
                                        b=b, t=t, h=hh, w=ww, f0=f0, nf=nf)
        _lib.check(self.lib.tc_still_composite(C.byref(p), _stream()), "tc_still_composite")
        return out


_backend = None


_binding_fallback = None


def binding_fallback():
    """None, or why the default custom-op binding was NOT taken and ctypes stepped in (bench.py prints it: a line that says
    `binding: ctypes` by accident must be tellable from one that was asked for)."""
    return _binding_fallback


def backend():
    """The operator set behind `ops.gemm(...)` etc.  Two bindings over the ONE C ABI (include/tooncrafter_hip.h):
      TC_BINDING=torch (default since round 5): PyTorch-ROCm custom ops, `torch.ops.tooncrafter.*` (csrc/torch_ops.cpp,
        TORCH_LIBRARY with CUDA + Meta keys) -- the binding BASELINE.json's north_star names;
      TC_BINDING=ctypes: the same entry points through ctypes.
    Bit-identical (tests/test_gpu_torch_ops.py) and equally fast (bench.py `binding_ab`; both replay hipGraphs).  Either way
    libtooncrafter_hip.so is mandatory: no kernel library, no backend (HipOps raises).  If only the custom-op layer
    (libtooncrafter_torch.so, host C++) is missing, the ctypes binding takes over with one line on stderr -- unless TC_BINDING=torch
    was asked for explicitly, which then fails."""
    global _backend
    if _backend is None:
        import os
        import sys
        want = os.environ.get("TC_BINDING", "").lower()
        if want in ("", "torch"):
            _lib.load()                                              # the kernel library first: its absence is fatal either way
            from . import torch_ops
            try:
                torch_ops.load()
            except _lib.TooncrafterAbiError:                         # a STALE op library: fatal (its namespace is registered already)
                raise
            except Exception as e:                                   # noqa: BLE001  (missing / unloadable op library)
                if want == "torch":
                    raise
                global _binding_fallback
                _binding_fallback = f"{type(e).__name__}: {e}"
                sys.stderr.write(f"[tooncrafter_amd] custom-op layer unavailable ({_binding_fallback}); using the ctypes binding\n")
                _backend = HipOps()
            else:
                _backend = torch_ops.TorchLibOps()
        elif want == "ctypes":
            _backend = HipOps()   # raises if libtooncrafter_hip.so is missing: no fallback
        else:
            raise ValueError(f"TC_BINDING={want!r}: expected 'torch' or 'ctypes'")
    return _backend


@contextlib.contextmanager
def fp8_scope(name):
    """`with ops.fp8_scope("decoder"):` -- see HipOps.fp8_scope; a no-op for backends without an fp8 path."""
    fn = getattr(backend(), "fp8_scope", None)
    if fn is None:
        yield
    else:
        with fn(name):
            yield


def set_backend(b):
    """Test hook: install another implementation of the operator contract."""
    global _backend
    prev, _backend = _backend, b
    return prev


def eligible(rule: str, *args, **kw) -> bool:
    """The backend's `<rule>_eligible(...)`: would it take that launch now?  A backend without the method does not offer the route."""
    return bool(getattr(backend(), rule + "_eligible", lambda *a, **k: False)(*args, **kw))


def __getattr__(name):   # ops.gemm(...) -> backend().gemm(...)
    if name.startswith("_"):
        raise AttributeError(name)
    return getattr(backend(), name)
