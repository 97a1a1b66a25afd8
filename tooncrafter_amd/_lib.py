"""ctypes binding of the C ABI declared in include/tooncrafter_hip.h.

The library is the product: if it is missing this module raises -- there is no
PyTorch or CPU fallback behind it.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libtooncrafter_hip.so")

TC_ABI_VERSION = 14
TC_TEMPORAL_MAX_FRAMES = 64      # include/tooncrafter_hip.h: the longest clip tc_attn_temporal takes
ACT_NONE, ACT_SILU, ACT_GELU, ACT_GEGLU = 0, 1, 2, 3
GATHER_LINEAR, GATHER_CONV3x3, GATHER_CONVT3 = 0, 1, 2

ERRORS = {-1: "TC_EINVAL (null pointer / bad size)", -2: "TC_EALIGN (16-byte alignment)",
          -3: "TC_ESHAPE (unsupported shape)", -4: "TC_EWORKSPACE (workspace too small)"}


class TcGemmParams(C.Structure):
    _fields_ = [
        ("a", C.c_void_p), ("w", C.c_void_p), ("c", C.c_void_p),
        ("bias", C.c_void_p), ("row_bias", C.c_void_p), ("residual", C.c_void_p),
        ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32),
        ("lda", C.c_int32), ("ldw", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32),
        ("ldrb", C.c_int32), ("row_div", C.c_int32),
        ("alpha", C.c_float), ("out_scale", C.c_float),
        ("act", C.c_int32), ("out_f32", C.c_int32),
        ("gather", C.c_int32), ("cin", C.c_int32), ("frames", C.c_int32), ("t_len", C.c_int32),
        ("h_out", C.c_int32), ("w_out", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32),
        ("stride", C.c_int32), ("upsample", C.c_int32), ("pad", C.c_int32),
        ("batch", C.c_int32),
        ("stride_a", C.c_int64), ("stride_w", C.c_int64), ("stride_c", C.c_int64),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("a_norm", C.c_int32), ("a_norm_eps", C.c_float),
        ("gn_part", C.c_void_p),
    ]


class TcGemmMxParams(C.Structure):
    _fields_ = [("g", TcGemmParams), ("a_scale", C.c_void_p), ("w_scale", C.c_void_p),
                ("lda_s", C.c_int32), ("ldw_s", C.c_int32)]


class TcAttnParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("batch", C.c_int32), ("heads", C.c_int32), ("lq", C.c_int32), ("lk", C.c_int32),
        ("q_sb", C.c_int64), ("k_sb", C.c_int64), ("v_sb", C.c_int64), ("o_sb", C.c_int64),
        ("q_ss", C.c_int32), ("k_ss", C.c_int32), ("v_ss", C.c_int32), ("o_ss", C.c_int32),
        ("kv_bdiv", C.c_int32), ("accumulate", C.c_int32), ("scale", C.c_float),
        ("k2", C.c_void_p), ("v2", C.c_void_p), ("lk2", C.c_int32), ("kv2_bdiv", C.c_int32),
        ("k2_sb", C.c_int64), ("v2_sb", C.c_int64), ("k2_ss", C.c_int32), ("v2_ss", C.c_int32),
    ]


class TcAttnQ8Params(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("batch", C.c_int32), ("heads", C.c_int32), ("lq", C.c_int32), ("lk", C.c_int32),
        ("q_sb", C.c_int64), ("k_sb", C.c_int64), ("v_sb", C.c_int64), ("o_sb", C.c_int64),
        ("q_ss", C.c_int32), ("k_ss", C.c_int32), ("v_ss", C.c_int32), ("o_ss", C.c_int32),
        ("scale", C.c_float),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcDdimParams(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("e_cond", C.c_void_p), ("e_uncond", C.c_void_p), ("noise", C.c_void_p),
        ("x_prev", C.c_void_p), ("pred_x0", C.c_void_p),
        ("b", C.c_int32), ("n", C.c_int64),
        ("cfg_scale", C.c_float), ("guidance_rescale", C.c_float),
        ("sqrt_ac", C.c_float), ("sqrt_1m_ac", C.c_float), ("sqrt_a_prev", C.c_float),
        ("dir_coef", C.c_float), ("sigma", C.c_float), ("x0_rescale", C.c_float),
        ("e_uncond_img", C.c_void_p), ("cfg_img", C.c_float),
    ]


class TcDdimMsParams(C.Structure):
    """tc_ddim_step_ms / tc_ddim_step_ms_eps: the step plus the multistep history term (additive within ABI 14)."""
    _fields_ = [("base", TcDdimParams), ("x0_hist", C.c_void_p), ("corr", C.c_float)]


class TcDdimBlendParams(C.Structure):
    """Pinned-frame blend / forward noising (tc_ddim_blend; additive within ABI 14)."""
    _fields_ = [
        ("x", C.c_void_p), ("x0", C.c_void_p), ("noise", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("n", C.c_int64),
        ("sqrt_ac", C.c_float), ("sqrt_1m_ac", C.c_float),
    ]


# name -> (restype, argtypes): every symbol include/tooncrafter_hip.h declares
class TcFfParams(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("out", C.c_void_p),
        ("m", C.c_int32), ("c", C.c_int32), ("hidden", C.c_int32), ("ldx", C.c_int32), ("ldo", C.c_int32), ("ln", C.c_int32),
        ("ln_eps", C.c_float),
    ]


class TcTbParams(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("wqkv", C.c_void_p), ("bqkv", C.c_void_p), ("wo", C.c_void_p), ("bo", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("hw", C.c_int32), ("c", C.c_int32), ("heads", C.c_int32),
        ("ldx", C.c_int32), ("ldo", C.c_int32), ("ln", C.c_int32),
        ("ln_eps", C.c_float), ("scale", C.c_float),
    ]


class TcTqaParams(C.Structure):
    """ABI 13: temporal qkv projection + attention as one launch (csrc/qkv_attn.hip; 17 .. 64 frames: csrc/qkv_attn_long.hip)."""
    _fields_ = [
        ("x", C.c_void_p), ("wqkv", C.c_void_p), ("bqkv", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("hw", C.c_int32), ("c", C.c_int32), ("heads", C.c_int32),
        ("ldx", C.c_int32), ("ldo", C.c_int32),
        ("scale", C.c_float),
    ]


class TcAttnTemporalRelParams(C.Structure):
    """Temporal attention with relative position / a causal mask (tc_attn_temporal_rel; additive within ABI 14)."""
    _fields_ = [
        ("qkv", C.c_void_p), ("out", C.c_void_p), ("rel_k", C.c_void_p), ("rel_v", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("hw", C.c_int32), ("heads", C.c_int32), ("max_rel", C.c_int32),
        ("causal", C.c_int32),
        ("scale", C.c_float),
    ]


class TcFramesU8Params(C.Structure):
    """uint8 HWC images -> fp32 clip frames (tc_frames_from_u8; additive within ABI 14).  `slots` is a HOST array."""
    _fields_ = [
        ("src", C.c_void_p), ("image_stride", C.c_int64), ("pitch", C.c_int32),
        ("n", C.c_int32), ("sh", C.c_int32), ("sw", C.c_int32),
        ("slots", C.POINTER(C.c_int32)), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("h_bounds", C.c_void_p), ("h_coefs", C.c_void_p), ("h_kmax", C.c_int32),
        ("v_bounds", C.c_void_p), ("v_coefs", C.c_void_p), ("v_kmax", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcClipPatchesParams(C.Structure):
    """fp32 frames -> the CLIP image tower's patch rows (tc_clip_patches; additive within ABI 14)."""
    _fields_ = [
        ("x", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("size", C.c_int32), ("patch", C.c_int32), ("ld", C.c_int32), ("antialias", C.c_int32),
        ("mean", C.c_float * 3), ("std", C.c_float * 3),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcFramesOutParams(C.Structure):
    """fp32 clips -> resized uint8 RGB / I420 / NV12 frames at named places (tc_frames_to_u8; additive within ABI 14)."""
    _fields_ = [
        ("x", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("f0", C.c_int32), ("nf", C.c_int32), ("oh", C.c_int32), ("ow", C.c_int32),
        ("format", C.c_int32), ("pitch", C.c_int32),
        ("frame_stride", C.c_int64), ("clip_stride", C.c_int64),
        ("h_bounds", C.c_void_p), ("h_coefs", C.c_void_p), ("h_kmax", C.c_int32),
        ("v_bounds", C.c_void_p), ("v_coefs", C.c_void_p), ("v_kmax", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcFramesYuvParams(C.Structure):
    """Planar 4:2:0 images -> fp32 clip frames (tc_frames_from_yuv; additive within ABI 14).  `slots` is a HOST array."""
    _fields_ = [
        ("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p),
        ("image_stride_y", C.c_int64), ("image_stride_c", C.c_int64),
        ("pitch_y", C.c_int32), ("pitch_c", C.c_int32), ("format", C.c_int32), ("siting", C.c_int32),
        ("m", C.c_int32 * 7),
        ("n", C.c_int32), ("sh", C.c_int32), ("sw", C.c_int32),
        ("slots", C.POINTER(C.c_int32)), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("h_bounds", C.c_void_p), ("h_coefs", C.c_void_p), ("h_kmax", C.c_int32),
        ("v_bounds", C.c_void_p), ("v_coefs", C.c_void_p), ("v_kmax", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcFramesYuvOutParams(C.Structure):
    """fp32 clips -> I420 / NV12 / P010 frames by a caller's RGB -> YCbCr matrix and chroma siting, at named places
    (tc_frames_to_yuv; additive within ABI 14): TcFramesOutParams' fields, then the siting and the matrix."""
    _fields_ = TcFramesOutParams._fields_ + [("siting", C.c_int32), ("m", C.c_int32 * 11)]


class TcColourStatsParams(C.Structure):
    """Nine double sums per named frame of fp32 clips (tc_colour_stats; additive within ABI 14)."""
    _fields_ = [
        ("x", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("f0", C.c_int32), ("nf", C.c_int32), ("fstep", C.c_int32),
        ("stats", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcColourMatchParams(C.Structure):
    """Frames matched in colour to two reference images per clip (tc_colour_match; additive within ABI 14)."""
    _fields_ = [
        ("x", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("src", C.c_void_p), ("ref", C.c_void_p),
        ("ref_pixels", C.c_int64),
        ("method", C.c_int32), ("strength", C.c_float),
        ("coefs", C.c_void_p),
    ]


class TcColourHistParams(C.Structure):
    """3 x 1024 int32 counts per named frame of fp32 clips (tc_colour_hist; additive within ABI 14)."""
    _fields_ = [
        ("x", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("f0", C.c_int32), ("nf", C.c_int32), ("fstep", C.c_int32),
        ("hist", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcColourTransferParams(C.Structure):
    """Frames carried per channel onto the histograms of two reference images per clip (tc_colour_transfer; additive within
    ABI 14)."""
    _fields_ = [
        ("x", C.c_void_p), ("base", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("src", C.c_void_p), ("ref", C.c_void_p),
        ("ref_pixels", C.c_int64),
        ("strength", C.c_float),
        ("table", C.c_void_p),
    ]


class TcColourMatchKnotsParams(C.Structure):
    """TcColourMatchParams towards nk reference images at host knot indices, with a gain limit (tc_colour_match_knots; additive
    within ABI 14)."""
    _fields_ = TcColourMatchParams._fields_ + [("nk", C.c_int32), ("knot", C.c_int32 * TC_TEMPORAL_MAX_FRAMES),
                                               ("max_gain", C.c_float)]


class TcColourTransferKnotsParams(C.Structure):
    """TcColourTransferParams towards nk reference images at host knot indices (tc_colour_transfer_knots; additive within
    ABI 14)."""
    _fields_ = TcColourTransferParams._fields_ + [("nk", C.c_int32), ("knot", C.c_int32 * TC_TEMPORAL_MAX_FRAMES)]


class TcFrameDeltaParams(C.Structure):
    """64-bin histograms of n RGB / I420 / NV12 / P010 images and, per pair (p, p + lag) and component, sad / changed / hist_l1
    (tc_frame_deltas; additive within ABI 14)."""
    _fields_ = [
        ("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p),
        ("image_stride_y", C.c_int64), ("image_stride_c", C.c_int64),
        ("pitch_y", C.c_int32), ("pitch_c", C.c_int32), ("format", C.c_int32),
        ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("lag", C.c_int32), ("tau", C.c_int32),
        ("hist", C.c_void_p), ("delta", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class TcStillMapParams(C.Structure):
    """Where the two keyframes of a clip agree: latent mask, pixel weight and cell distance (tc_still_map; additive within
    ABI 14).  `h`, `w` are in pixels."""
    _fields_ = [
        ("ends", C.c_void_p),
        ("b", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("tau", C.c_int32), ("grow", C.c_int32), ("feather", C.c_int32),
        ("mask", C.c_void_p), ("alpha", C.c_void_p), ("dist", C.c_void_p),
    ]


class TcStillCompositeParams(C.Structure):
    """Frames held to the keyframes by a pixel weight (tc_still_composite; additive within ABI 14)."""
    _fields_ = [
        ("video", C.c_void_p), ("ends", C.c_void_p), ("alpha", C.c_void_p), ("out", C.c_void_p),
        ("b", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("f0", C.c_int32), ("nf", C.c_int32),
    ]


TC_STILL_CELL = 8                                        # include/tooncrafter_hip.h: pixels per cell side of tc_still_map
TC_STILL_MAX_DIST = 32                                   # include/tooncrafter_hip.h: the largest grow + feather + 1
TC_DELTA_BINS = 64                                       # include/tooncrafter_hip.h: bins per component of tc_frame_deltas
TC_COLOUR_BINS = 1024                                   # include/tooncrafter_hip.h: bins per channel of tc_colour_hist
TC_COLOUR_STATS = 9                                      # include/tooncrafter_hip.h: doubles per frame of tc_colour_stats
TC_COLOUR_METHODS = {"mean_std": 0, "mkl": 1}            # TC_COLOUR_MEAN_STD / TC_COLOUR_MKL
TC_YUV_FORMATS = {"i420": 1, "nv12": 2, "p010": 3}       # include/tooncrafter_hip.h: the TC_PIXFMT_* tc_frames_from_yuv reads
TC_YUV_STANDARDS = {"bt601": 0, "bt709": 1}              # TC_YUV_BT*
TC_YUV_RANGES = {"limited": 0, "full": 1}                # TC_YUV_LIMITED / TC_YUV_FULL
TC_CHROMA_SITINGS = {"nearest": 0, "center": 1, "left": 2}                     # TC_CHROMA_*
TC_RESIZE_FILTERS = {"bilinear": 0, "bicubic": 1, "lanczos": 2, "box": 3}      # include/tooncrafter_hip.h: TC_RESIZE_*
TC_PIXFMTS = {"rgb24": 0, "i420": 1, "nv12": 2}                                # include/tooncrafter_hip.h: TC_PIXFMT_*


class TcRandnParams(C.Structure):
    """Per-clip Philox noise (tc_randn_clips; additive within ABI 14).  `seeds` is a HOST array of b uint64."""
    _fields_ = [
        ("out", C.c_void_p), ("seeds", C.POINTER(C.c_uint64)), ("b", C.c_int32), ("n", C.c_int64),
        ("stream", C.c_uint32), ("scale", C.c_float), ("raw", C.c_int32),
    ]


TC_FRAMES_U8_MAX = 16            # include/tooncrafter_hip.h: images per tc_frames_from_u8 call
TC_RANDN_CLIPS = 16              # include/tooncrafter_hip.h: clips per launch of tc_randn_clips
TC_PREFETCH_MAX = 4


class TcPrefetch(C.Structure):
    """ABI 12: read-only device buffers (a consumer's weights) that extra blocks of a norm launch stream into the
    Infinity Cache."""
    _fields_ = [("ptr", C.c_void_p * TC_PREFETCH_MAX), ("bytes", C.c_int64 * TC_PREFETCH_MAX), ("n", C.c_int32)]


SYMBOLS = {
    "tc_gemm_bf16": (C.c_int, [C.POINTER(TcGemmParams), C.c_void_p]),
    "tc_gemm_workspace": (C.c_int64, [C.POINTER(TcGemmParams)]),
    "tc_gemm_mxfp8": (C.c_int, [C.POINTER(TcGemmMxParams), C.c_void_p]),
    "tc_quant_mxfp8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                 C.c_void_p]),
    "tc_layernorm_mxfp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "tc_attn_d64": (C.c_int, [C.POINTER(TcAttnParams), C.c_void_p]),
    "tc_attn_q8_workspace": (C.c_int64, [C.POINTER(TcAttnQ8Params)]),
    "tc_attn_q8_quant_kv": (C.c_int, [C.POINTER(TcAttnQ8Params), C.c_void_p]),
    "tc_attn_d64_q8": (C.c_int, [C.POINTER(TcAttnQ8Params), C.c_void_p]),
    "tc_attn_temporal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_float, C.c_void_p]),
    "tc_attn_temporal_rel": (C.c_int, [C.POINTER(TcAttnTemporalRelParams), C.c_void_p]),
    "tc_groupnorm_workspace": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "tc_groupnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                               C.c_float, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                               C.c_void_p]),
    "tc_groupnorm_pf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_float, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(TcPrefetch), C.c_void_p]),
    "tc_layernorm_pf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                  C.POINTER(TcPrefetch), C.c_void_p]),
    "tc_softmax_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]),
    "tc_nchw_to_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "tc_rows_to_nchw": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]),
    "tc_concat_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_timestep_embedding": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tc_silu_f32_to_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_timestep_embedding_i64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tc_repeat_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "tc_time_mix3": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                               C.c_int32, C.c_void_p]),
    "tc_video_to_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "tc_ddim_workspace": (C.c_int64, [C.c_int32]),
    "tc_ddim_step": (C.c_int, [C.POINTER(TcDdimParams), C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_ddim_step_eps": (C.c_int, [C.POINTER(TcDdimParams), C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_ddim_step_ms": (C.c_int, [C.POINTER(TcDdimMsParams), C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_ddim_step_ms_eps": (C.c_int, [C.POINTER(TcDdimMsParams), C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_ddim_blend": (C.c_int, [C.POINTER(TcDdimBlendParams), C.c_void_p]),
    "tc_resize_tables": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64]),
    "tc_frames_from_u8_resized": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tc_frames_from_u8_workspace": (C.c_int64, [C.POINTER(TcFramesU8Params)]),
    "tc_frames_from_u8": (C.c_int, [C.POINTER(TcFramesU8Params), C.c_void_p]),
    "tc_clip_patches_workspace": (C.c_int64, [C.POINTER(TcClipPatchesParams)]),
    "tc_clip_patches": (C.c_int, [C.POINTER(TcClipPatchesParams), C.c_void_p]),
    "tc_resize_tables_filter": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64]),
    "tc_frames_to_u8_workspace": (C.c_int64, [C.POINTER(TcFramesOutParams)]),
    "tc_frames_to_u8": (C.c_int, [C.POINTER(TcFramesOutParams), C.c_void_p]),
    "tc_randn_clips": (C.c_int, [C.POINTER(TcRandnParams), C.c_void_p]),
    "tc_yuv_matrix": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "tc_frames_from_yuv_workspace": (C.c_int64, [C.POINTER(TcFramesYuvParams)]),
    "tc_frames_from_yuv": (C.c_int, [C.POINTER(TcFramesYuvParams), C.c_void_p]),
    "tc_yuv_out_matrix": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "tc_frames_to_yuv_workspace": (C.c_int64, [C.POINTER(TcFramesYuvOutParams)]),
    "tc_frames_to_yuv": (C.c_int, [C.POINTER(TcFramesYuvOutParams), C.c_void_p]),
    "tc_colour_stats_workspace": (C.c_int64, [C.POINTER(TcColourStatsParams)]),
    "tc_colour_stats": (C.c_int, [C.POINTER(TcColourStatsParams), C.c_void_p]),
    "tc_colour_match": (C.c_int, [C.POINTER(TcColourMatchParams), C.c_void_p]),
    "tc_colour_hist_workspace": (C.c_int64, [C.POINTER(TcColourHistParams)]),
    "tc_colour_hist": (C.c_int, [C.POINTER(TcColourHistParams), C.c_void_p]),
    "tc_colour_transfer": (C.c_int, [C.POINTER(TcColourTransferParams), C.c_void_p]),
    "tc_colour_match_knots": (C.c_int, [C.POINTER(TcColourMatchKnotsParams), C.c_void_p]),
    "tc_colour_transfer_knots": (C.c_int, [C.POINTER(TcColourTransferKnotsParams), C.c_void_p]),
    "tc_frame_deltas_workspace": (C.c_int64, [C.POINTER(TcFrameDeltaParams)]),
    "tc_frame_deltas": (C.c_int, [C.POINTER(TcFrameDeltaParams), C.c_void_p]),
    "tc_still_map": (C.c_int, [C.POINTER(TcStillMapParams), C.c_void_p]),
    "tc_still_composite": (C.c_int, [C.POINTER(TcStillCompositeParams), C.c_void_p]),
    "tc_gemm_ws_eligible":(C.c_int, [C.POINTER(TcGemmParams)]),
    "tc_gemm_gn_rows": (C.c_int, [C.POINTER(TcGemmParams)]),
    "tc_groupnorm_part": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "tc_ff_geglu_fused_eligible": (C.c_int, [C.POINTER(TcFfParams)]),
    "tc_ff_geglu_fused": (C.c_int, [C.POINTER(TcFfParams), C.c_void_p]),
    "tc_temporal_attn_fused_eligible": (C.c_int, [C.POINTER(TcTbParams)]),
    "tc_temporal_attn_fused": (C.c_int, [C.POINTER(TcTbParams), C.c_void_p]),
    "tc_temporal_qkv_attn_eligible": (C.c_int, [C.POINTER(TcTqaParams)]),
    "tc_temporal_qkv_attn": (C.c_int, [C.POINTER(TcTqaParams), C.c_void_p]),
    "tc_abi_version": (C.c_int, []),
    "tc_build_info": (C.c_char_p, []),
}

_lib = None


class TooncrafterHipError(RuntimeError):
    pass


class TooncrafterAbiError(TooncrafterHipError):
    """A library built against another ABI version was loaded: a stale build, never a reason to fall back."""


def load():
    """dlopen the in-tree library and type every entry point.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TooncrafterHipError(
            f"{LIB_PATH} not found: build it with `python -m tooncrafter_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    ver = lib.tc_abi_version()
    if ver != TC_ABI_VERSION:
        raise TooncrafterHipError(f"ABI mismatch: library {ver}, binding {TC_ABI_VERSION}")
    if os.environ.get("TC_DEBUG_SYNC"):
        lib = _TracedLib(lib)
    _lib = lib
    return lib


class _TracedLib:
    """TC_DEBUG_SYNC=1: print every entry-point call (arguments, GEMM/attention parameter blocks) to stderr
    BEFORE it runs and synchronise the device after it, so that a GPU memory fault -- which kills the
    process asynchronously -- is attributable to the last line printed."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in SYMBOLS or name in ("tc_abi_version", "tc_build_info", "tc_resize_tables", "tc_resize_tables_filter", "tc_frames_from_u8_resized", "tc_yuv_matrix", "tc_yuv_out_matrix") or name.endswith("_workspace"):
            return fn
        import sys

        import torch

        def show(a):
            s = getattr(a, "_obj", None)
            if isinstance(s, C.Structure):
                vals = []
                for f, _ in s._fields_:
                    v = getattr(s, f)
                    vals.append("%s=%s" % (f, hex(v) if isinstance(v, int) and v > 1 << 20 else v))
                return "{" + " ".join(vals) + "}"
            return hex(a) if isinstance(a, int) and a > 1 << 20 else repr(a)

        def traced(*args):
            sys.stderr.write("[tc] %s %s\n" % (name, " ".join(show(a) for a in args)))
            sys.stderr.flush()
            rc = fn(*args)
            torch.cuda.synchronize()
            return rc
        return traced


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc < 0:
        raise TooncrafterHipError(f"{what}: {ERRORS.get(rc, rc)}")
    raise TooncrafterHipError(f"{what}: hipError_t {rc}")
