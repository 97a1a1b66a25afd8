/*
 * tooncrafter_hip.h -- C ABI of the MI355X (gfx950) kernels behind the ToonCrafter
 * denoising hot path (DDIM sampler -> spatio-temporal UNet -> dual-reference
 * VideoDecoder).
 *
 * The reference (Doubiiu/ToonCrafter) is pure PyTorch: it has no FFI of its own.
 * What it binds instead are third-party kernels (ATen conv/GEMM/norm/softmax,
 * xformers.memory_efficient_attention).  Every entry point below replaces one of
 * those call sites; the reference file:line is given with each.
 *
 * Conventions (all entry points):
 *   - plain pointers to DEVICE memory, sizes as int/int64, no torch types;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it;
 *   - never allocates, never synchronises, hipGraph-capture safe;
 *   - returns 0 on success, a negative TC_E* code on a bad argument (nothing launched),
 *     or the positive hipError_t of a failed launch;
 *   - activations are bf16 "channels-last rows": a tensor (B,T,H,W,C) is a row-major
 *     matrix [B*T*H*W, C]; weights are bf16 [N, K] row-major (K contiguous).
 */
#ifndef TOONCRAFTER_HIP_H
#define TOONCRAFTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TC_ABI_VERSION 14

enum {
  TC_OK = 0,
  TC_EINVAL = -1,      /* null pointer / non-positive size */
  TC_EALIGN = -2,      /* pointer or leading dimension not 16-byte aligned */
  TC_ESHAPE = -3,      /* shape outside what the kernel supports */
  TC_EWORKSPACE = -4   /* workspace too small */
};

typedef uint16_t tc_bf16;   /* raw bfloat16 bits */

/* ---- activation applied in the GEMM epilogue ---- */
enum { TC_ACT_NONE = 0, TC_ACT_SILU = 1, TC_ACT_GELU = 2, TC_ACT_GEGLU = 3 };

/* ---- how GEMM rows of A are gathered (implicit-GEMM convolution) ---- */
enum {
  TC_GATHER_LINEAR = 0,   /* A[m, k] = a[m*lda + k]                                  (nn.Linear, 1x1 conv) */
  TC_GATHER_CONV3x3 = 1,  /* 3x3, pad 1, stride `stride`, optional nearest-x2 source  (nn.Conv2d)           */
  TC_GATHER_CONVT3 = 2    /* (3,1,1) over T, pad (1,0,0)                              (nn.Conv3d)           */
};

typedef struct TcGemmParams {
  /* operands */
  const tc_bf16* a;        /* activations, channels-last rows */
  const tc_bf16* w;        /* [N, K] bf16; K = taps*cin, tap-major then channel; for TC_ACT_GEGLU
                              every 32 rows are packed as 16 value rows then their 16 gate rows */
  void* c;                 /* [M, ldc] bf16 (or fp32 when out_f32) */
  const float* bias;       /* [N] fp32 or NULL (same packing as w rows) */
  const float* row_bias;   /* [ceil(M/row_div), N] fp32 or NULL: per-frame embedding add */
  const tc_bf16* residual; /* [M, ldr] bf16 or NULL, added last */
  /* sizes */
  int32_t m, n, k;         /* n, k as stored in w; with GEGLU the output has n/2 columns */
  int32_t lda, ldw, ldc, ldr; /* leading dimensions in elements (multiples of 8); ldw >= k */
  int32_t ldrb;            /* leading dimension of row_bias (>= n) */
  int32_t row_div;         /* rows sharing one row_bias row (H*W) */
  /* epilogue:  v = act(alpha*acc + bias + row_bias) * out_scale + residual */
  float alpha, out_scale;
  int32_t act;
  int32_t out_f32;
  /* gather geometry */
  int32_t gather;
  int32_t cin;             /* channels per tap (multiple of 64 when taps > 1) */
  int32_t frames;          /* B*T images */
  int32_t t_len;           /* T, frames per clip (CONVT3 bounds) */
  int32_t h_out, w_out;    /* output image size: m = (frame*h_out + y)*w_out + x */
  int32_t h_in, w_in;      /* source image size */
  int32_t stride;          /* 1 or 2 */
  int32_t upsample;        /* 1: source is nearest-upsampled x2 on the fly (Upsample + conv fused) */
  int32_t pad;             /* leading (top/left) zero padding of the 3x3 gather: 1 = symmetric pad 1;
                              0 = the VAE encoder's asymmetric (0,1,0,1) pad before its stride-2 conv */
  /* batching (blockIdx.z): element strides, 0 = shared */
  int32_t batch;
  int64_t stride_a, stride_w, stride_c;
  /* ABI 4 -- optional scratch for split-K: low-resolution layers (few output tiles, long K) are cut along K
   * over several blocks per tile, fp32 partial tiles go here and a second kernel sums them in a fixed order
   * and applies the epilogue (bit-reproducible).  NULL / too small = never split. */
  void* workspace;
  int64_t workspace_bytes;
  /* ABI 8 -- LayerNorm of the A rows as a prologue of the product (lvdm/modules/attention.py:225-227 in front of the
   * qkv / GEGLU projections, attention.py:242-246): a_norm = 1 normalises every row over its k columns,
   * (x - mean) * rsqrt(var + a_norm_eps) with fp32 statistics, before it is multiplied; the affine part is the
   * CALLER's job (w[n, :] *= gamma, bias += w @ beta: exact in real arithmetic).  Only problems tc_gemm_ws_eligible
   * accepts can carry it (whole rows of A must sit in one block); tc_gemm_bf16 returns TC_ESHAPE otherwise. */
  int32_t a_norm;
  float a_norm_eps;
  /* ABI 9 -- GroupNorm statistics from the producer (lvdm/basics.py:76-87 normalises what openaimodel3d.py:154,179,
   * 255-266 just wrote): not NULL = besides C the launch emits, for every block of tc_gemm_gn_rows() consecutive output
   * rows and every output column, the sum and the sum of squares of the bf16-ROUNDED outputs, fp32
   * [ceil(m / gn_rows)][2][n], summed in a fixed order (no atomics).  tc_groupnorm_part turns them into (mean, rstd) --
   * the consumer's own statistics pass over the tensor (one of GroupNorm's two reads) disappears.  Only for problems
   * whose tc_gemm_gn_rows() is non-zero; tc_gemm_bf16 returns TC_ESHAPE otherwise. */
  float* gn_part;
} TcGemmParams;

/* C = epilogue(gather(A) * W^T), bf16 MFMA, fp32 accumulate.
 * Replaces: nn.Linear (lvdm/modules/attention.py:53-57,75-76,269,290,336,362,418,438;
 * openaimodel3d.py:170,371-380), nn.Conv2d 3x3/1x1 (openaimodel3d.py:68-70,96,154,179,187,386,545;
 * autoencoder_dualref.py:52-68,419-462,921-927), nn.Conv3d (3,1,1) (openaimodel3d.py:255-266;
 * autoencoder_dualref.py:601-605,641-648), F.interpolate nearest x2 (openaimodel3d.py:98-106),
 * GEGLU (attention.py:420-422) and the residual/embedding adds around them. */
int tc_gemm_bf16(const TcGemmParams* p, void* stream);
/* bytes of TcGemmParams.workspace this problem would use (0: it is not a split-K candidate) */
int64_t tc_gemm_workspace(const TcGemmParams* p);
/* ABI 8 -- 1 if tc_gemm_bf16 would run this problem on the weight-stationary K = 320 kernel (csrc/gemm_ws.hip), the
 * only one that accepts a_norm = 1: the host asks BEFORE it decides to drop a LayerNorm launch. */
int tc_gemm_ws_eligible(const TcGemmParams* p);
/* ABI 9 -- row-block height of TcGemmParams.gn_part for this problem under the current routing (160: the 160x160-tile
 * kernel; 128: the 128x128-tile kernel without split-K), or 0 when the kernel that would run it cannot emit
 * statistics (the caller then leaves gn_part NULL and the consumer computes its own). */
int tc_gemm_gn_rows(const TcGemmParams* p);

/* ABI 7 -- MX block-scaled fp8 GEMM (BASELINE.json configs[4]: the CDNA4 fp8 MFMA GEMM path).
 * Operands are OCP MX "MXFP8": e4m3 elements with one E8M0 (power-of-two) scale per 32 consecutive K
 * elements of a row (OCP Microscaling Formats v1.0 section 5.1/6.3: shared exponent = floor(log2(amax)) - 8,
 * elements = RNE(x / 2^shared) saturated to +-448).  The reference has no fp8 path; the tensors this
 * replaces are the same nn.Linear / nn.Conv2d / nn.Conv3d operands as tc_gemm_bf16 above, and the parity
 * oracle is oracle/mx.py (exact restatement of the quantiser + fp32 matmul of the dequantised operands). */
typedef struct TcGemmMxParams {
  TcGemmParams g;        /* as for tc_gemm_bf16, except: a / w point to fp8 e4m3 BYTES, lda / ldw / stride_a /
                            stride_w are in elements (= bytes, multiples of 16), k and cin multiples of 32 (linear)
                            / 64 (taps); c, bias, row_bias, residual and the epilogue are unchanged (bf16 / fp32);
                            workspace is unused (no split-K), batch must be 1 */
  const uint8_t* a_scale; /* E8M0 [source rows, lda_s]: byte j of a row scales its K elements [32 j, 32 j + 32) */
  const uint8_t* w_scale; /* E8M0 [n, ldw_s] */
  int32_t lda_s, ldw_s;   /* leading dimensions of the scale matrices in bytes (multiples of 4; >= ceil(k / 128) * 4
                             for w and linear a, >= cin / 32 for a convolution source) */
} TcGemmMxParams;
int tc_gemm_mxfp8(const TcGemmMxParams* p, void* stream);
/* bf16 rows [rows, ld] (first k columns, k % 32 == 0) -> e4m3 bytes q[rows, ldq] + E8M0 scales s[rows, lds];
 * scale columns [k / 32, lds) are zero-filled so a K tail of the GEMM reads finite scales. */
int tc_quant_mxfp8(const tc_bf16* x, int64_t rows, int32_t k, int32_t ld, uint8_t* q, int32_t ldq,
                   uint8_t* s, int32_t lds, void* stream);
/* tc_layernorm followed by tc_quant_mxfp8 in one pass (the quantiser fused into its producer): nn.LayerNorm
 * (attention.py:225-227) whose only consumer is an MXFP8 GEMM (qkv / GEGLU projections).  Bit-identical to the two
 * separate calls.  c % 32 == 0; lds >= ceil(c / 128) * 4 as for tc_quant_mxfp8. */
int tc_layernorm_mxfp8(const tc_bf16* x, uint8_t* q, int32_t ldq, uint8_t* s, int32_t lds, const float* gamma,
                       const float* beta, int32_t rows, int32_t c, float eps, void* stream);

/* ABI 9 -- the feed-forward of a level-0 transformer block as ONE launch (lvdm/modules/attention.py:415-442 behind
 * norm3, attention.py:244-246):  out = x + w2 . GEGLU(w1 . LN(x) + b1) + b2.  The hidden tensor ([m, hidden] bf16: 210 MB
 * at the BASELINE shape) never reaches HBM.  c = 320 and hidden = 1280 only (tc_ff_geglu_fused_eligible).
 *   x    [m, ldx] bf16: the block's input rows -- LayerNorm input AND residual;
 *   w1   [2*hidden, c] bf16 in tc_gemm_bf16's GEGLU packing (every 32 rows = 16 value rows, then their 16 gate rows):
 *        the very tensor the TC_ACT_GEGLU projection takes; with ln != 0 the LayerNorm's gamma is folded in
 *        (w1[n, :] *= gamma) and b1 carries w1 . beta, as for TcGemmParams.a_norm;
 *   b1   [2*hidden] fp32, packed like w1's rows;   w2 [c, hidden] bf16;   b2 [c] fp32;   out [m, ldo] bf16;
 *   ln   != 0: rows are normalised, (x - mean) * rsqrt(var + ln_eps) with fp32 statistics, before the first product;
 *        0: x is taken as already normalised for the product (and still added as the residual). */
typedef struct TcFfParams {
  const tc_bf16* x; const tc_bf16* w1; const float* b1; const tc_bf16* w2; const float* b2; tc_bf16* out;
  int32_t m, c, hidden, ldx, ldo, ln;
  float ln_eps;
} TcFfParams;
int tc_ff_geglu_fused_eligible(const TcFfParams* p);
int tc_ff_geglu_fused(const TcFfParams* p, void* stream);

/* ABI 9 -- the temporal self-attention of a level-0 transformer block as ONE launch (lvdm/modules/attention.py:81-144 over
 * the T = 16 frames of a pixel, called from TemporalTransformer attention.py:365-412 behind norm1 / norm2, attention.py:
 * 225-246):  out = x + wo . Attn_frames(wqkv . LN(x) + bqkv) + bo.  The [rows, 960] qkv tensor and the [rows, 320]
 * attention output never reach HBM.  c = 320, heads = 5 (of 64), t = 16, hw % 8 == 0 only (tc_temporal_attn_fused_eligible).
 *   x     [b*t*hw, ldx] bf16, row = (batch * t + frame) * hw + pixel: LayerNorm input AND residual;
 *   wqkv  [3*c, c] bf16: rows [0, c) = to_q, [c, 2c) = to_k, [2c, 3c) = to_v (head h at h*64), the fused projection
 *         tc_gemm_bf16 takes in front of tc_attn_temporal; with ln != 0 the LayerNorm's gamma is folded in and bqkv
 *         carries wqkv . beta (zeros otherwise: the reference's projections have no bias);
 *   wo    [c, c] bf16, bo [c] fp32 (to_out);   out [b*t*hw, ldo] bf16;   scale = 64^-0.5;
 *   ln    != 0: rows are normalised ((x - mean) * rsqrt(var + ln_eps), fp32 statistics) before the projection. */
typedef struct TcTbParams {
  const tc_bf16* x; const tc_bf16* wqkv; const float* bqkv; const tc_bf16* wo; const float* bo; tc_bf16* out;
  int32_t b, t, hw, c, heads, ldx, ldo, ln;
  float ln_eps, scale;
} TcTbParams;
int tc_temporal_attn_fused_eligible(const TcTbParams* p);
int tc_temporal_attn_fused(const TcTbParams* p, void* stream);

/* ABI 13 -- the fused q / k / v projection of a temporal self-attention and the attention itself as ONE launch
 * (lvdm/modules/attention.py:81-144: to_q / to_k / to_v at :96-102, the per-head softmax(q k^T * scale) v over the T
 * frames of a pixel at :103-134 -- called with context = None from TemporalTransformer, attention.py:365-412):
 *     out[:, h*64 .. h*64+63] = Attn_frames(x . wqkv[q_h | k_h | v_h]^T + bqkv),     every head h
 * i.e. tc_gemm_bf16(x, wqkv) followed by tc_attn_temporal, without the [rows, 3c] tensor between them reaching HBM.
 * `out` is what to_out (a tc_gemm_bf16 with bias and residual) takes next.
 * Domain (tc_temporal_qkv_attn_eligible; anything else returns TC_ESHAPE and launches nothing): c = heads * 64; ldx, ldo >= c
 * and multiples of 8; a block's rows within 31 bits of its first; and
 *   t = 16                       hw % 8 == 0 (csrc/qkv_attn.hip): every level of the UNet (c = 320 ... 1280; since round 6
 *                                level 0 takes LayerNorm -> this -> to_out by default, tc_temporal_attn_fused only with
 *                                TC_TB_FUSED=1);
 *   17 <= t <= TC_TEMPORAL_MAX_FRAMES   hw % (128 / TT) == 0 with TT = 32 for t <= 32, else 64 (csrc/qkv_attn_long.hip).  The
 *                                frame count is padded to TT slots inside the kernel: a padded slot reads zeros (never
 *                                the next clip's rows, nor anything behind x), takes no part in any softmax, and is never
 *                                stored -- x and out hold exactly b*t*hw rows.
 *   t < 16 and t > TC_TEMPORAL_MAX_FRAMES are refused: tc_gemm_bf16 + tc_attn_temporal take them.
 * TC_QKV_ATTN (environment, read per call): 0 = never eligible; 1 (default) = 16 frames, plus the 17 .. 64-frame shapes
 * that measured ahead of the two launches: c = 320 or 640 with t >= 24 (t <= 32) or t >= 48 (t > 32), c = 1280
 * with t = 32 or t = 64; 2 = every shape above.
 *   x     [b*t*hw, ldx] bf16, row = (batch * t + frame) * hw + pixel: the projection's input (the LayerNorm's output);
 *   wqkv  [3*c, c] bf16: rows [0, c) = to_q, [c, 2c) = to_k, [2c, 3c) = to_v (head h at h*64) -- tc_gemm_bf16's operand;
 *   bqkv  [3*c] fp32 or NULL (the reference's projections have no bias);   out [b*t*hw, ldo] bf16;   scale = 64^-0.5.
 * `out` must not alias `x`: a block stores its rows while other blocks (the other heads of the same rows) still read x. */
typedef struct TcTqaParams {
  const tc_bf16* x; const tc_bf16* wqkv; const float* bqkv; tc_bf16* out;
  int32_t b, t, hw, c, heads, ldx, ldo;
  float scale;
} TcTqaParams;
int tc_temporal_qkv_attn_eligible(const TcTqaParams* p);
int tc_temporal_qkv_attn(const TcTqaParams* p, void* stream);

typedef struct TcAttnParams {
  const tc_bf16* q; const tc_bf16* k; const tc_bf16* v; tc_bf16* o;
  int32_t batch, heads, lq, lk;
  /* element (b, h, i, d) lives at ptr + b*sb + i*ss + h*64 + d  (head dim 64, contiguous) */
  int64_t q_sb, k_sb, v_sb, o_sb;
  int32_t q_ss, k_ss, v_ss, o_ss;
  int32_t kv_bdiv;     /* K/V batch index = b / kv_bdiv (shared reference / text keys) */
  int32_t accumulate;  /* 1: o += result (second softmax of the image cross-attention) */
  float scale;         /* d^-0.5 */
  /* ABI 6 -- optional SECOND key/value set with its own softmax, summed into the same output in one launch:
   * o = softmax(q k^T) v + softmax(q k2^T) v2 -- the text + image cross-attention of attention.py:153-207
   * (77 text keys shared by the frames of a clip, 16 image keys per frame).  k2 == NULL: single set. */
  const tc_bf16* k2; const tc_bf16* v2;
  int32_t lk2, kv2_bdiv;
  int64_t k2_sb, v2_sb;
  int32_t k2_ss, v2_ss;
} TcAttnParams;

/* softmax(q k^T * scale) v, head dim 64, flash-style (scores never leave the CU).
 * Replaces xformers.ops.memory_efficient_attention at lvdm/modules/attention.py:175,187 and
 * lvdm/models/autoencoder_dualref.py:316,326 (and the einsum fallback attention.py:103-134). */
int tc_attn_d64(const TcAttnParams* p, void* stream);

/* ABI 14 -- 8-bit spatial self-attention (BASELINE.json configs[4], the fp8 attention path; csrc/attention_q8.hip):
 * softmax(q k^T * scale) v with q k^T on int8 operands (one fp32 scale per row and head) and P v on MXFP8 operands (V^T and
 * the in-kernel P in e4m3 with one E8M0 scale per 32 keys).  Replaces the xformers self-attention of
 * lvdm/modules/attention.py:175 (CrossAttention.efficient_forward with context = None, called from the spatial
 * BasicTransformerBlock.attn1) where ops.HipOps.spatial_attn_q8_eligible routes it; formats in the source's header.
 * Two launches: tc_attn_q8_quant_kv quantises K and V into `workspace` (tc_attn_q8_workspace bytes, 16-byte aligned), then
 * tc_attn_d64_q8 reads q and that workspace and writes o.  Element (b, h, i, d) lives at ptr + b*sb + i*ss + h*64 + d, as in
 * TcAttnParams; the quantiser reads k / v, the attention q / o, both the workspace.  No key/value batch sharing, no second
 * key/value set, no accumulate: TcAttnParams covers those. */
typedef struct TcAttnQ8Params {
  const tc_bf16* q; const tc_bf16* k; const tc_bf16* v; tc_bf16* o;
  int32_t batch, heads, lq, lk;
  int64_t q_sb, k_sb, v_sb, o_sb;
  int32_t q_ss, k_ss, v_ss, o_ss;
  float scale;         /* d^-0.5; must be > 0 */
  void* workspace;
  int64_t workspace_bytes;
} TcAttnQ8Params;
int64_t tc_attn_q8_workspace(const TcAttnQ8Params* p);
int tc_attn_q8_quant_kv(const TcAttnQ8Params* p, void* stream);
int tc_attn_d64_q8(const TcAttnQ8Params* p, void* stream);

/* Temporal self-attention over 1 .. TC_TEMPORAL_MAX_FRAMES frames at every pixel (attention.py:81-144 via
 * TemporalTransformer, attention.py:365-412).  qkv: fused [rows, 3*C] projection with
 * row = (b*T + t)*HW + p; columns [0,C)=q, [C,2C)=k, [2C,3C)=v, head h at h*64.
 * out: [rows, C] bf16.  t <= 16: one wave per (pixel, head) on the VALU, fp32 softmax weights;
 * 16 < t <= 64 (long clips, --video_length above 16): csrc/attention_temporal_long.hip, MFMA with the frames padded
 * to 32 | 64, bf16 softmax weights as csrc/qkv_attn.hip; t > TC_TEMPORAL_MAX_FRAMES: TC_ESHAPE, nothing launched.
 * (The signature is unchanged from ABI 14 -- a caller built against it keeps working; the accepted t range grew.) */
#define TC_TEMPORAL_MAX_FRAMES 64
int tc_attn_temporal(const tc_bf16* qkv, tc_bf16* out, int32_t b, int32_t t, int32_t hw,
                     int32_t heads, float scale, void* stream);

/* The same attention with relative position and / or a causal mask (attention.py:20-39 RelativePosition, 103-124 the
 * two extra einsums and the mask in CrossAttention.forward, 343-345 / 376-390 the tril mask of TemporalTransformer:
 * use_relative_position / use_causal_attention of the UNet).  Per pixel and head, over the t frames:
 *     idx(i, j) = clamp(j - i, -max_rel, max_rel) + max_rel
 *     s[i, j]   = scale * (q_i . k_j + q_i . rel_k[idx(i, j)]),  -inf for j > i when causal
 *     o_i       = sum_j softmax_j(s[i, :])[j] * (v_j + rel_v[idx(i, j)])
 * qkv / out as tc_attn_temporal.  rel_k, rel_v: [2*max_rel + 1, 64] bf16 each, shared by every head, 16-byte aligned; both
 * NULL = mask only (max_rel is then ignored), exactly one NULL: TC_EINVAL.  1 <= t <= TC_TEMPORAL_MAX_FRAMES and, with
 * tables, 1 <= max_rel <= TC_TEMPORAL_MAX_FRAMES, else TC_ESHAPE: nothing launched, nothing written.  t may exceed
 * max_rel (distances clamp); the reference's causal mask is [max_rel, max_rel], so causal with t > max_rel has no
 * counterpart there and is the caller's to refuse.  One MFMA kernel for every t (csrc/attention_temporal_rel.hip), bf16
 * softmax weights and per-distance sums; with no tables and causal == 0 it is tc_attn_temporal's long-clip arithmetic.
 * No allocation, no synchronisation, safe under hipGraph capture.  Additive within ABI 14. */
typedef struct TcAttnTemporalRelParams {
  const tc_bf16* qkv;
  tc_bf16* out;
  const tc_bf16* rel_k;
  const tc_bf16* rel_v;
  int32_t b, t, hw, heads, max_rel, causal;
  float scale;
} TcAttnTemporalRelParams;
int tc_attn_temporal_rel(const TcAttnTemporalRelParams* p, void* stream);

/* GroupNorm(32 groups) over channels-last rows, fp32 statistics, optional fused SiLU.
 * x: [samples, rows, C]; statistics over (rows, C/32) per (sample, group): samples = B*T,
 * rows = H*W for the per-frame norms; samples = B, rows = T*H*W for the clip-wide ones.
 * Replaces GroupNormSpecific / nn.GroupNorm + nn.SiLU (lvdm/basics.py:76-87;
 * openaimodel3d.py:152-153,176-177,256-265; attention.py:265,331; autoencoder_dualref.py:29-32).
 * workspace: tc_groupnorm_workspace() bytes of fp32 partial sums. */
int64_t tc_groupnorm_workspace(int32_t samples, int32_t rows, int32_t c);
int tc_groupnorm(const tc_bf16* x, tc_bf16* y, const float* gamma, const float* beta,
                 int32_t samples, int32_t rows, int32_t c, float eps, int32_t silu,
                 void* workspace, int64_t workspace_bytes, void* stream);
/* ABI 9 -- the same with the statistics taken from a producer's partial sums (TcGemmParams.gn_part:
 * [samples * rows / part_rows][2][c] fp32; rows % part_rows == 0): a reduction over the partials (fp64, fixed order)
 * and ONE pass over x.  workspace: tc_groupnorm_workspace() bytes. */
int tc_groupnorm_part(const tc_bf16* x, tc_bf16* y, const float* gamma, const float* beta, const float* part,
                      int32_t part_rows, int32_t samples, int32_t rows, int32_t c, float eps, int32_t silu,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ABI 11 removed the three ABI-10 entry points tc_groupnorm_scale_shift / tc_conv_gn_eligible / tc_conv_gn_bf16 -- GroupNorm
 * applied inside the convolution that consumes it: parity-green on the GPU and 4 % SLOWER per clip than the two operators
 * (profiles/r05_fuse_clip_ab.txt).  A cooperative single-launch GroupNorm measured in the same round
 * (x read once, blocks meeting at an atomic counter) was correct and slower on every shape as well
 * (profiles/r05_gn_coop_bench.txt) and never entered the ABI; its source is kept as scripts/experiments/gn_coop.hip.txt. */

/* LayerNorm over the last axis of [rows, C] (attention.py:225-227), eps 1e-5, affine. */
int tc_layernorm(const tc_bf16* x, tc_bf16* y, const float* gamma, const float* beta,
                 int32_t rows, int32_t c, float eps, void* stream);

/* ABI 12 -- the same two norms, with a WEIGHT PREFETCH riding on the launch.  In the reference every norm is followed by the
 * layer that consumes it (openaimodel3d.py:152-154,176-179,255-266: GroupNorm -> SiLU -> convolution; attention.py:242-246:
 * LayerNorm -> attention / feed-forward projections), and inside a forward that layer's weights are always cold: 2.9 GB of
 * parameters cycle through the 256 MB Infinity Cache once per forward.  For the 1280-channel levels of the UNet that costs
 * the GEMM 7-29 % (profiles/r05_cold_operand_probe.txt); a read of the weights one launch ahead removes 93-100 % of it
 * (profiles/r05_prefetch_premise_probe.txt).  `prefetch` names up to TC_PREFETCH_MAX read-only device buffers (ptr 16-byte
 * aligned; whole 16-byte units of `bytes` are read, never a byte beyond); extra blocks of the norm's launch stream them
 * through a load and drop the values -- y is bit-identical to tc_groupnorm / tc_layernorm, nothing else is written.
 * prefetch == NULL or n == 0: exactly the plain entry point. */
#define TC_PREFETCH_MAX 4
typedef struct TcPrefetch {
  const void* ptr[TC_PREFETCH_MAX];
  int64_t bytes[TC_PREFETCH_MAX];
  int32_t n;
} TcPrefetch;
int tc_groupnorm_pf(const tc_bf16* x, tc_bf16* y, const float* gamma, const float* beta,
                    int32_t samples, int32_t rows, int32_t c, float eps, int32_t silu,
                    void* workspace, int64_t workspace_bytes, const TcPrefetch* prefetch, void* stream);
int tc_layernorm_pf(const tc_bf16* x, tc_bf16* y, const float* gamma, const float* beta,
                    int32_t rows, int32_t c, float eps, const TcPrefetch* prefetch, void* stream);

/* Row softmax fp32 [rows, n] -> bf16 [rows, ldo] for attention computed as GEMM + softmax + GEMM: the
 * single-head d=512 mid attention of the decoder (autoencoder_dualref.py:172-200) and the OpenCLIP towers
 * (head dim 80 / causal text attention, condition.py:215-231,340-372).  Columns [n, n_out) of p are written
 * as zeros (K padding of the following P.V GEMM).  causal_period > 0: row r attends columns
 * 0 .. (r mod causal_period) only -- the text tower's attn_mask -- masked columns get probability 0.  (ABI 5) */
int tc_softmax_rows(const float* s, tc_bf16* p, int32_t rows, int32_t n, int32_t n_out, int32_t lds, int32_t ldo,
                    int32_t causal_period, void* stream);

/* (B, C, T, H, W) fp32, optionally two tensors concatenated on C, -> channels-last bf16
 * [B*T*H*W, c_pad] zero padded, times `scale`.  The hybrid-conditioning concat of
 * ddpm3d.py:1260-1264 and the `b c t h w -> (b t) c h w` rearranges (openaimodel3d.py:566). */
int tc_nchw_to_rows(const float* x0, int32_t c0, const float* x1, int32_t c1, tc_bf16* out,
                    int32_t c_pad, int32_t b, int32_t t, int32_t hw, float scale, void* stream);
/* rows -> (B, C, T, H, W) fp32: the inverse rearrange (openaimodel3d.py:602). src may be bf16 or fp32. */
int tc_rows_to_nchw(const void* src, int32_t src_f32, int32_t ld, float* out, int32_t c,
                    int32_t b, int32_t t, int32_t hw, void* stream);
/* Channel concat of two rows tensors [rows, ca] | [rows, cb] -> [rows, ca+cb]: the UNet skip
 * connections (openaimodel3d.py:596). */
int tc_concat_rows(const tc_bf16* a, int32_t ca, const tc_bf16* b, int32_t cb, tc_bf16* out,
                   int64_t rows, void* stream);

/* Sinusoidal embedding [cos | sin] (utils_diffusion.py:19-23) -> bf16 [n, dim_pad], then optional SiLU elementwise helper. */
int tc_timestep_embedding(const float* t, tc_bf16* out, int32_t n, int32_t dim, int32_t ld, void* stream);
int tc_silu_f32_to_bf16(const float* x, tc_bf16* y, int64_t n, void* stream);
/* ABI 9 -- the same from the int64 timesteps the samplers hand over (ddim.py:166 `torch.full(..., dtype=torch.long)`,
 * openaimodel3d.py:567-575): the `.to(float32)` in front of the embedding is a launch of its own otherwise. */
int tc_timestep_embedding_i64(const int64_t* t, tc_bf16* out, int32_t n, int32_t dim, int32_t ld, void* stream);

/* ABI 9 -- dst[k * rows + r, :] = src[r, :] for k < n (rows of row_bytes bytes, a multiple of 16; both contiguous):
 * where batched guidance leaves the shared prefix (lvdm/common.py: CfgShare; the reference runs the n passes as n
 * separate UNet calls, ddim.py:226-233) the single-copy rows and embedding are repeated n-fold. */
int tc_repeat_rows(const void* src, void* dst, int64_t rows, int32_t row_bytes, int32_t n, void* stream);

/* AE3DConv tail (autoencoder_dualref.py:929-935): Conv3d 3->3 (3,1,1) over T on the fp32
 * [B*T*HW, ld] rows produced by the 128->3 conv, written as (B, 3, T, H, W) fp32. */
int tc_time_mix3(const float* rows, int32_t ld, const float* w, const float* bias, float* out,
                 int32_t b, int32_t t, int32_t hw, void* stream);

/* Output path, replaces scripts/evaluation/inference.py:148-153 on the device:
 * clamp(x, -1, 1) -> (x + 1) / 2 -> (* 255) -> uint8 (truncation) with the permute (c t h w) -> (t h w c),
 * for each of the b clips of x (b, 3, t, h, w) fp32; out is (b, t, h, w, 3) uint8.  Same fp32 operations in
 * the same order as the reference, so the bytes are identical; it makes the rank-0 gather 4x smaller. */
int tc_video_to_u8(const float* x, uint8_t* out, int32_t b, int32_t t, int32_t hw, void* stream);

typedef struct TcDdimParams {
  const float* x;        /* current latent (B, n) fp32 */
  const float* e_cond;   /* UNet output for the conditional pass (B, n) */
  const float* e_uncond; /* unconditional pass, or NULL */
  const float* noise;    /* N(0,1) draw or NULL (sigma == 0) */
  float* x_prev; float* pred_x0;
  int32_t b; int64_t n;  /* n = C*T*H*W */
  float cfg_scale, guidance_rescale;
  /* fp32 scalars in the reference's order of operations (ddim.py:251-277, ddpm3d.py:240-252) */
  float sqrt_ac, sqrt_1m_ac, sqrt_a_prev, dir_coef /* sqrt(1-a_prev-sigma^2) */, sigma, x0_rescale;
  /* ABI 3 -- three-way guidance of samplers/ddim_multiplecond.py:226-236: when e_uncond_img is not NULL the
   * combination is e_uncond + cfg_img*(e_uncond_img - e_uncond) + cfg_scale*(e_cond - e_uncond_img)
   * (e_uncond_img = UNet pass with the image condition kept and the text dropped) */
  const float* e_uncond_img;
  float cfg_img;
} TcDdimParams;

/* CFG combine + rescale_noise_cfg (unbiased std over each sample) + v->(eps,x0) + dynamic
 * rescale + x_prev, fused.  Replaces ddim.py:226-277 / ddim_multiplecond.py:226-288 and
 * utils_diffusion.py:147-158.  It is tc_ddim_step_ms below without a history, {*p, NULL, 0}: one launcher and one
 * kernel serve both, so no alignment is asked for (operands that are not 16-byte aligned take the scalar instance).
 * workspace: b * 64 * 4 doubles. */
int64_t tc_ddim_workspace(int32_t b);
int tc_ddim_step(const TcDdimParams* p, void* workspace, int64_t workspace_bytes, void* stream);

/* The same step for an eps-parameterised model (additive within ABI 14: one symbol, the struct and the workspace of
 * tc_ddim_step).  The model output after CFG and rescale_noise_cfg is e_t itself (samplers/ddim.py:231-234), so
 *   pred_x0 = (x - sqrt_1m_ac * e_t) / sqrt_ac                     (ddim.py:257-258, a true fp32 division)
 * and dynamic rescale, dir_coef * e_t, the noise term and x_prev follow as in tc_ddim_step (ddim.py:262-277).  The
 * callers pass sqrt_ac = sqrt(ddim_alphas[index]) and sqrt_1m_ac = ddim_sqrt_one_minus_alphas[index], the tables this
 * branch of the reference reads (ddim.py:251-254).  TC_EINVAL also for sqrt_ac == 0 (a zero-terminal-SNR step).  Like
 * tc_ddim_step it is the history-free case of its _ms form, tc_ddim_step_ms_eps. */
int tc_ddim_step_eps(const TcDdimParams* p, void* workspace, int64_t workspace_bytes, void* stream);

/* The same step with a second-order multistep correction (additive within ABI 14: one struct, two symbols; the workspace
 * and the statistics pass of tc_ddim_step).  Not in the reference, whose samplers know the first-order update only; it
 * extends the call sites of tc_ddim_step / tc_ddim_step_eps in samplers/ddim.py:226-277 and ddim_multiplecond.py:226-288
 * when the sampler is asked for solver_order = 2.  In exponential-integrator form this is DPM-Solver++(2M) (eta = 0) and
 * its SDE variant (eta = 1), written as the first-order update plus ONE term:
 *   x0u    = pred_x0 before x0_rescale   (v: sqrt_ac * x - sqrt_1m_ac * v;  eps: (x - sqrt_1m_ac * e_t) / sqrt_ac)
 *   x_prev = sqrt_a_prev * (x0u * x0_rescale) + dir_coef * e_t + corr * (x0u - x0_hist) + sigma * noise
 *   corr   = (sqrt_a_prev * x0_rescale - dir_coef * sqrt_ac / sqrt_1m_ac) * h / (2 * h_prev)
 * x0_hist is the pred_x0 the PREVIOUS step returned (already rescaled, so on the scale of this step's x0u), h and h_prev
 * this and the previous step's increments of log(sqrt(alpha) * scale / sqrt(1 - alpha)).  corr is one host scalar, computed
 * in double and rounded once; the callers pass 0 on the first step of a run, after a step with alpha = 0 (h_prev is not
 * finite) and on the final step.  The correction is added last before the noise term; every other operation is
 * tc_ddim_step's in its order, and pred_x0 is tc_ddim_step's.  x0_hist is read only when it is not NULL and corr != 0;
 * with x0_hist == NULL or corr == 0 both outputs are bit-identical to tc_ddim_step / tc_ddim_step_eps.
 * Any n >= 2; 16-byte vectors are used when every pointer and every sample's base allow it.
 * Aliasing: `base.pred_x0` may be EXACTLY `x0_hist` (the history updated in place; pred_x0 is then not NULL); any other
 * overlap of x_prev or pred_x0 with x0_hist returns TC_EINVAL.  Also TC_EINVAL: a corr that is not finite, whatever
 * tc_ddim_step / tc_ddim_step_eps refuse (sqrt_ac == 0 in the eps form included).  Nothing is launched on a refusal. */
typedef struct TcDdimMsParams {
  TcDdimParams base;     /* the step as tc_ddim_step takes it */
  const float* x0_hist;  /* the previous step's pred_x0 (B, n) fp32, or NULL: no history */
  float corr;            /* 0: first-order step */
} TcDdimMsParams;
int tc_ddim_step_ms(const TcDdimMsParams* p, void* workspace, int64_t workspace_bytes, void* stream);
int tc_ddim_step_ms_eps(const TcDdimMsParams* p, void* workspace, int64_t workspace_bytes, void* stream);

/* Pinned-frame blend and forward noising of the samplers, one elementwise launch (additive within ABI 14: one struct,
 * one symbol).  Replaces the mask / x0 blend at the top of a sampling step (ddim.py:173-180, ddim_multiplecond.py:177-184),
 * q_sample (ddpm3d.py:306-309) and the last line of stochastic_encode (ddim.py:316-317):
 *   orig = noise ? sqrt_ac * x0 + sqrt_1m_ac * noise : x0          (noise == NULL: clean_cond)
 *   out  = mask  ? orig * mask + (1 - mask) * x      : orig        (mask == NULL: q_sample / stochastic_encode)
 * in fp32 with every product, the subtraction and every sum rounded on its own (no FMA contraction), i.e. the bits of the
 * reference's separate torch ops.  Any n >= 1; pointers need only the 4-byte alignment of a float (16-byte vectors are
 * used when every pointer allows it).  No workspace, no synchronisation.
 * Aliasing: `out` may be EXACTLY `x` (the blend in place); any other overlap of `out` with x, x0, noise or mask --
 * partial overlap with x included -- returns TC_EINVAL.  Also TC_EINVAL: NULL x0 / out, b <= 0, n <= 0, mask without x. */
typedef struct TcDdimBlendParams {
  const float* x;      /* current latent (B, n) fp32; required when mask != NULL */
  const float* x0;     /* known latent (B, n) */
  const float* noise;  /* N(0,1) draw, or NULL: x0 is taken as it is (clean_cond) */
  const float* mask;   /* (B, n) weights, or NULL: out = noised x0 (q_sample / stochastic_encode) */
  float* out;          /* may be exactly x (in place) */
  int32_t b; int64_t n;
  float sqrt_ac, sqrt_1m_ac;
} TcDdimBlendParams;
int tc_ddim_blend(const TcDdimBlendParams* p, void* stream);

/* ---- Pixel front end: uint8 frames -> the model's and the CLIP image tower's inputs (additive within ABI 14: two
 * structs, five symbols).  The reference does both steps outside its model code, on PIL images and with kornia. ---- */

/* Coefficient tables of one axis of PIL's 8-bit BILINEAR resample (Pillow src/libImaging/Resample.c: precompute_coeffs
 * + normalize_coeffs_8bpc), HOST code, double precision, no device call.  For output index xx of an axis in_size -> out_size:
 *   scale = in / out, support = fs = max(scale, 1), kmax = ceil(support) * 2 + 1, center = (xx + 0.5) * scale,
 *   xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in),
 *   w[x] = max(0, 1 - |(x + xmin - center + 0.5) / fs|) for x < xmax - xmin, divided by their sum,
 *   coefs[xx * kmax + x] = int(w[x] * 2^22 + 0.5)  (0 from xmax - xmin on),  bounds[2 xx] = xmin, bounds[2 xx + 1] = xmax - xmin.
 * Returns kmax (> 0).  bounds == NULL and coefs == NULL is the sizing query: nothing is written; otherwise bounds holds
 * 2 * out_size and coefs coefs_len >= out_size * kmax int32 (TC_EWORKSPACE if fewer, TC_EINVAL for a size <= 0 or one
 * table without the other). */
int32_t tc_resize_tables(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs, int64_t coefs_len);

#define TC_FRAMES_U8_MAX 16   /* images per tc_frames_from_u8 call */

/* n uint8 HWC images -> fp32 frames of a (b, 3, t, H, W) clip tensor: the image transform of the reference's
 * load_data_prompts (scripts/evaluation/inference.py:64-69: Resize(min(size)), CenterCrop(size), ToTensor,
 * Normalize(0.5, 0.5) on PIL images), bit for bit:
 *   - resized size: the shorter source side becomes s = min(H, W), the other int(s * long / short); no resize when
 *     the shorter side is s already;
 *   - PIL's 8-bit BILINEAR resample with the tables of tc_resize_tables, horizontal pass (sw -> rw) into the uint8
 *     workspace, then vertical (sh -> rh).  PIL skips a pass whose size does not change; under the rule above both
 *     sides change or neither, so either both passes run or the source is cropped as it is (no tables needed).  A pixel
 *     is clip(((1 << 21) + sum coefs * src) >> 22, 0, 255).  Table entries are clamped to the image, so wrong tables
 *     give wrong pixels, never an access outside the source;
 *   - crop: left = round_half_even((rw - W) / 2), top likewise; outside the resized image the pixel is 0 (PIL's crop);
 *   - value: fp32 (v / 255 - 0.5) / 0.5, each operation rounded on its own (correctly rounded division).
 * Image i goes to frame slots[i] = batch * t + frame; frames no slot names are not written.  `slots` is a HOST array
 * (read before the launch); every other pointer is device memory.
 * workspace: tc_frames_from_u8_workspace bytes (n * sh * rw * 3 when the images are resized, else 0).
 * TC_EINVAL: NULL p / src / out / slots, n <= 0 or > TC_FRAMES_U8_MAX, a size <= 0, pitch < 3 * sw, image_stride < sh * pitch,
 * a slot outside [0, b * t), tables missing for a pass that runs; TC_EWORKSPACE: workspace too small.  Nothing is
 * launched or written on a refusal. */
typedef struct TcFramesU8Params {
  const uint8_t* src;        /* n images, HWC, 3 channels */
  int64_t image_stride;      /* bytes from one image to the next */
  int32_t pitch;             /* bytes from one row to the next, >= 3 * sw */
  int32_t n, sh, sw;
  const int32_t* slots;      /* HOST: n frame indices batch * t + frame */
  float* out;                /* (b, 3, t, H, W) fp32 */
  int32_t b, t, h, w;
  const int32_t* h_bounds; const int32_t* h_coefs; int32_t h_kmax;   /* tables sw -> rw (NULL when nothing is resized) */
  const int32_t* v_bounds; const int32_t* v_coefs; int32_t v_kmax;   /* tables sh -> rh */
  void* workspace; int64_t workspace_bytes;
} TcFramesU8Params;
/* The resized size (rh, rw) of an (sh, sw) source for an (h, w) target by the rule above; TC_EINVAL for a size <= 0. */
int tc_frames_from_u8_resized(int32_t sh, int32_t sw, int32_t h, int32_t w, int32_t* rh, int32_t* rw);
int64_t tc_frames_from_u8_workspace(const TcFramesU8Params* p);
int tc_frames_from_u8(const TcFramesU8Params* p, void* stream);

/* The CLIP image tower's preprocessing up to the A operand of its patch-embedding GEMM, replaces
 * lvdm/modules/encoders/condition.py:322-330 (kornia.geometry.resize(x, (S, S), 'bicubic', align_corners=True,
 * antialias=True), (x + 1) / 2, (x - mean) / std) and the unfold in front of open_clip's conv1:
 *   - antialias (only if h / S or w / S exceeds 1): separable Gaussian, per axis sigma = max((factor - 1) / 2, 0.001),
 *     kernel size int(max(4 sigma, 3)) made odd, reflect border; rows first, then columns;
 *   - bicubic (Keys, A = -0.75) at source coordinate dst * (in - 1) / (S - 1), tap indices clamped to the image;
 *   - (v + 1) / 2, then (v - mean[c]) / std[c];
 * all sums in double, rounded to bf16 once (the mean cancels the pixel value: near zero a bf16 ulp is below the rounding
 * error of an fp32 sum).  out: rows [b * g * g, ld], g = S / patch, row = (sample, patch row, patch
 * column), column = (c, py, px) as conv1.weight.reshape(width, -1); columns 3 * patch^2 .. ld - 1 are written as zero.
 * workspace: tc_clip_patches_workspace bytes (two double copies of x when the blur runs, else 0), 8-byte aligned.
 * TC_EINVAL: NULL p / x / out, a size <= 0, ld < 3 * patch^2; TC_ESHAPE: S % patch != 0, a reflect border that does
 * not fit (kernel size / 2 >= the image's extent), a kernel of more than TC_CLIP_BLUR_TAPS taps; TC_EWORKSPACE; TC_EALIGN. */
#define TC_CLIP_BLUR_TAPS 127
typedef struct TcClipPatchesParams {
  const float* x;            /* (b, 3, h, w) fp32 in [-1, 1], contiguous */
  tc_bf16* out;              /* [b * g * g, ld] */
  int32_t b, h, w;
  int32_t size, patch, ld;   /* S, the patch edge, the row length of out */
  int32_t antialias;         /* 0: never blur */
  float mean[3], std[3];
  void* workspace; int64_t workspace_bytes;
} TcClipPatchesParams;
int64_t tc_clip_patches_workspace(const TcClipPatchesParams* p);
int tc_clip_patches(const TcClipPatchesParams* p, void* stream);

/* ---- Pixel back end: the decoder's fp32 clips -> uint8 frames at a chosen size, in the pixel format an encoder takes,
 * written where they belong in a longer video (additive within ABI 14: one struct, three symbols).  The reference does
 * this step outside its own code, with torch on the host (scripts/evaluation/inference.py:146-155), PIL and torchvision.
 * tc_video_to_u8 above stays as it is: packed RGB at the model's size. ---- */

/* tc_resize_tables for PIL's other filters: the same contract (sizing query, the return value kmax, the refusals,
 * bounds[2 xx] = xmin, bounds[2 xx + 1] = xmax - xmin; TC_EINVAL also for an unknown filter), the rule Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc in double, for a filter F of support S:
 *   scale = in / out, fs = max(scale, 1), support = S * fs, kmax = ceil(support) * 2 + 1, center = (xx + 0.5) * scale,
 *   xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in),
 *   w[x] = F((x + xmin - center + 0.5) * (1 / fs))  -- a MULTIPLICATION by the reciprocal, as Pillow writes it --
 *   summed in tap order and divided by the sum when it is not zero,
 *   coefs[xx * kmax + x] = int(0.5 + w * 2^22) for w >= 0, int(-0.5 + w * 2^22) for w < 0; the cast truncates toward zero
 *   (bicubic and Lanczos have negative lobes: + 0.5 alone is wrong for them), 0 from xmax - xmin on.
 * The filters, as in Resample.c, each 0 outside the stated range:
 *   BILINEAR  S = 1    F = 1 - |x| on |x| < 1
 *   BICUBIC   S = 2    a = -0.5:  F = ((a + 2)|x| - (a + 3)) x^2 + 1 on |x| < 1,  (((|x| - 5)|x| + 8)|x| - 4) a on 1 <= |x| < 2
 *   LANCZOS   S = 3    F = sinc(x) sinc(x / 3) on -3 <= x < 3,  sinc(x) = sin(pi x) / (pi x),  sinc(0) = 1
 *   BOX       S = 0.5  F = 1 on -0.5 < x <= 0.5
 * At TC_RESIZE_BILINEAR the tables are tc_resize_tables' for every size pair 1 .. 128. */
enum { TC_RESIZE_BILINEAR = 0, TC_RESIZE_BICUBIC = 1, TC_RESIZE_LANCZOS = 2, TC_RESIZE_BOX = 3 };
int32_t tc_resize_tables_filter(int32_t filter, int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs,
                                int64_t coefs_len);

/* Frames f0 .. f0 + nf - 1 of every clip of x (b, 3, t, h, w) fp32 -> uint8 frames of (oh, ow) pixels, in this order:
 *   1. value: clamp(x, -1, 1), (v + 1) / 2, * 255, truncation to uint8 -- tc_video_to_u8's arithmetic, operation for
 *      operation (one __device__ function serves both);
 *   2. resample, only for an axis whose size changes: PIL's 8-bit two-pass resample of the uint8 RGB frame with tables of
 *      tc_resize_tables_filter, horizontal (w -> ow) first, then vertical (h -> oh), a pass skipped when its size is
 *      unchanged.  A pixel is clip(((1 << 21) + sum coefs * src) >> 22, 0, 255) in int32 with an arithmetic shift: with
 *      negative lobes the sum goes below zero, so shift and clip are signed.  For the four filters sum |w| < 1.6, so the
 *      sum stays inside int32.  Table entries are clamped to the image: wrong tables give wrong pixels, never an access
 *      outside a buffer;
 *   3. format, from the resized uint8 RGB:
 *        RGB24  HWC, 3 bytes per pixel, rows `pitch` apart;
 *        I420   Y plane of oh rows `pitch` apart, Cb at pitch * oh with oh / 2 rows pitch / 2 apart, Cr at
 *               pitch * oh + (pitch / 2) * (oh / 2);
 *        NV12   Y as for I420, then one plane of oh / 2 rows `pitch` apart with Cb, Cr interleaved.
 *      BT.601 limited range in integers; Rs, Gs, Bs are the sums over the 2 x 2 block:
 *        Y  = ( 16829 R  + 33039 G  +  6416 B  + (16 << 16)  + (1 << 15)) >> 16
 *        Cb = ( -9714 Rs - 19070 Gs + 28784 Bs + (128 << 18) + (1 << 17)) >> 18
 *        Cr = ( 28784 Rs - 24103 Gs -  4681 Bs + (128 << 18) + (1 << 17)) >> 18
 *      clipped to 0 .. 255; every shifted quantity is non-negative.  The chroma rows each sum to 0, the Y row to
 *      56284 ~ 219 / 255 * 2^16: black gives Y 16, white 235, pure red 81, pure blue 41; the 2 x 2 block {black, white,
 *      red, blue} gives Cb 147, Cr 151.  This is deliberately NOT the float32 numpy expression of mp4.rgb_to_yuv420, whose
 *      result depends on numpy's summation order for the 2 x 2 mean (that expression stays for RGB input): the two differ
 *      by at most 1 code value (over 40 random 64 x 96 frames and a 52^3 colour grid 0.05 % of the Y and 0.03 % of the
 *      chroma samples differ, none by more than 1);
 *   4. placement: frame f0 + j of clip i goes to out + i * clip_stride + j * frame_stride.  Bytes between rows (pitch
 *      padding), between frames and between clips are not written.  `loop` is nf = t - 1; a keyframe sequence is spliced
 *      in place by writing clips 1 .. K - 1 with f0 = 1 and clip_stride = (t - 1) * frame bytes into one video buffer.
 * A frame's bytes: pitch * oh (RGB24), pitch * oh + 2 * (pitch / 2) * (oh / 2) (I420), pitch * oh + pitch * (oh / 2) (NV12).
 * workspace: tc_frames_to_u8_workspace bytes -- the uint8 RGB frames at source size (b * nf * h * w * 3) plus, when
 * ow != w, the horizontal pass's intermediate (b * nf * h * ow * 3); 0 when nothing is resampled and the format is RGB24
 * (0 also for a request tc_frames_to_u8 refuses).  Every pointer is device memory.
 * TC_EINVAL: NULL p / x / out, a size <= 0, f0 / nf outside the clip, an unknown format, pitch below the row's bytes
 * (3 * ow for RGB24, ow for the Y plane), frame_stride below the frame's bytes, clip_stride < nf * frame_stride when b > 1,
 * tables missing for a pass that runs; TC_ESHAPE: I420 / NV12 with an odd oh or ow or, for I420, an odd pitch;
 * TC_EWORKSPACE: workspace too small.  Nothing is launched or written on a refusal. */
enum { TC_PIXFMT_RGB24 = 0, TC_PIXFMT_I420 = 1, TC_PIXFMT_NV12 = 2 };
typedef struct TcFramesOutParams {
  const float* x;              /* (b, 3, t, h, w) fp32: the decoder's output */
  uint8_t* out;
  int32_t b, t, h, w;
  int32_t f0, nf;              /* frames f0 .. f0+nf-1 of every clip are written, 0 <= f0, nf >= 1, f0+nf <= t */
  int32_t oh, ow;              /* output size; (oh, ow) == (h, w): no resample, no tables, and for RGB24 no workspace */
  int32_t format;              /* TC_PIXFMT_* */
  int32_t pitch;               /* bytes per row of the RGB image / of the Y plane */
  int64_t frame_stride, clip_stride;   /* bytes from one written frame / clip to the next in out */
  const int32_t* h_bounds; const int32_t* h_coefs; int32_t h_kmax;   /* w -> ow (NULL when ow == w) */
  const int32_t* v_bounds; const int32_t* v_coefs; int32_t v_kmax;   /* h -> oh (NULL when oh == h) */
  void* workspace; int64_t workspace_bytes;
} TcFramesOutParams;
int64_t tc_frames_to_u8_workspace(const TcFramesOutParams* p);
int tc_frames_to_u8(const TcFramesOutParams* p, void* stream);

/* ---- Per-clip Gaussian noise from a counter-based generator (additive within ABI 14: one struct, one symbol).  Replaces
 * the sampler's torch.randn draws from the process-wide device generator (reference ddim.py:157, 266 / common.py:31-34,
 * ddpm3d.py q_sample) when the caller names one seed per clip: element j of clip i is a pure function of
 * (seeds[i], stream, j).  It does not depend on b, on the clip's position in the batch, on the launch chunking, on the grid
 * or on the device; it is NOT torch's generator, so it does not reproduce a torch.manual_seed run. ----
 *   - generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): multipliers 0xD2511F53 and 0xCD9E8D57, key increments
 *     0x9E3779B9 and 0xBB67AE85, ten rounds;
 *   - indexing: for clip i and the 4-element group q = j >> 2, key = (lo32(seeds[i]), hi32(seeds[i])), counter =
 *     (q, 0, stream, 0); the four output words w0..w3 belong to elements 4q .. 4q + 3;
 *   - size limit: n > 2^34 returns TC_ESHAPE (q then fits counter word 0 and word 1 is the constant 0);
 *   - raw != 0: element 4q + m is the word w_m itself (the same bytes of `out` read as uint32);
 *   - otherwise Box-Muller on word pairs, with u(w) = (2 (w >> 9) + 1) 2^-24 (exact in fp32, in [2^-24, 1 - 2^-24], so
 *     ln u is finite) and v(w) = (w >> 9) 2^-23:  r(w) = sqrt(-2 ln u(w)),  z0 = r(w0) cos(2 pi v(w1)),
 *     z1 = r(w0) sin(2 pi v(w1)),  z2, z3 the same from (w2, w3); the accurate logf and sincospif(2 v), not the fast
 *     intrinsics; then one fp32 multiply by `scale` (1.0f leaves the value as it is);
 *   - launch shape: one thread produces one Philox block and one 16-byte store; a clip's tail (n % 4) and a row that does
 *     not start on a 16-byte boundary take scalar stores; the seeds travel as kernel arguments, TC_RANDN_CLIPS clips per
 *     launch and as many launches as b needs.  No device allocation, no copy, no synchronisation, no workspace.
 * `seeds` is a HOST array (read before the launches, like `slots` of tc_frames_from_u8); `out` is device memory.
 * TC_EINVAL: NULL p / out / seeds, b <= 0, n <= 0; TC_ESHAPE: n > 2^34.  Nothing is launched or written on a refusal. */
#define TC_RANDN_CLIPS 16   /* clips per launch of tc_randn_clips */
typedef struct TcRandnParams {
  float* out;             /* (b, n) fp32, or the same bytes as uint32 when raw != 0 */
  const uint64_t* seeds;  /* HOST array, b entries, one seed per clip */
  int32_t b; int64_t n;   /* n = elements per clip, any n >= 1 */
  uint32_t stream;        /* which draw of the clip this is (the samplers' numbering: lvdm/ddim.py) */
  float scale;            /* the sampler's temperature; one fp32 multiply */
  int32_t raw;            /* != 0: store the Philox words themselves (for tests and other hosts) */
} TcRandnParams;
int tc_randn_clips(const TcRandnParams* p, void* stream);

/* ---- Planar YUV keyframes: what a hardware decoder leaves in device memory -> the model's fp32 frames (additive within
 * ABI 14: one struct, three symbols, one pixel format).  tc_frames_from_u8 for 4:2:0 sources: NV12 surfaces of an 8-bit
 * stream, P010 / P016 surfaces of a 10-bit one, or the I420 / NV12 frames tc_frames_to_u8 writes. ---- */

/* The integer YCbCr -> RGB matrix of a standard, HOST code, double precision, no device call:
 *   m = {cy, crv, cgu, cgv, cbu, yoff, coff}.
 * (Kr, Kb) = (0.299, 0.114) for BT.601, (0.2126, 0.0722) for BT.709; Kg = 1 - Kr - Kb; q = 2^(bits - 8).
 *   limited range: Y gain 255 / (219 q), chroma gain s = 255 / (224 q), yoff = 16 q;
 *   full range:    Y gain = s = 255 / (2^bits - 1), yoff = 0;           coff = 128 q in both.
 * The five coefficients are floor(v * 65536 + 0.5) of the Y gain, 2 (1 - Kr) s, 2 Kb (1 - Kb) / Kg s, 2 Kr (1 - Kr) / Kg s,
 * 2 (1 - Kb) s -- e.g. BT.601 limited 8 bit: 76309, 104597, 25675, 53279, 132201, yoff 16, coff 128.
 * TC_EINVAL: an unknown standard or range, bits other than 8 or 10, NULL m. */
enum { TC_YUV_BT601 = 0, TC_YUV_BT709 = 1 };
enum { TC_YUV_LIMITED = 0, TC_YUV_FULL = 1 };
int tc_yuv_matrix(int32_t standard, int32_t range, int32_t bits, int32_t m[7]);

/* n planar 4:2:0 images -> fp32 frames of a (b, 3, t, H, W) clip tensor.  The result is DEFINED as tc_frames_from_u8 applied
 * to the packed RGB image (n, sh, sw, 3) that the per-pixel rule below gives: resize, crop and value steps and their bits
 * are that entry point's.  All arithmetic is int32, shifts are arithmetic, sums may be negative.
 *   - format: TC_PIXFMT_I420  y, c0 = Cb, c1 = Cr: three planes of 8-bit samples;
 *             TC_PIXFMT_NV12  y and c0 = one plane of interleaved Cb, Cr; c1 NULL;
 *             TC_PIXFMT_P010  NV12's layout in 16-bit little-endian words, sample = word >> 6 (the low six bits are
 *                             ignored): a decoder's P016 surface of a 10-bit stream; c1 NULL;
 *     luma rows are pitch_y bytes apart, chroma rows pitch_c; the chroma planes hold ch = (sh + 1) / 2 rows of
 *     cw = (sw + 1) / 2 samples (odd pictures are legal: decoders crop); image i starts image_stride_y / image_stride_c
 *     bytes after image i - 1, so with n = 1 the pointers describe any one surface, whatever its chroma offset;
 *   - chroma at luma pixel (y, x), j = y >> 1, i = x >> 1, every index clamped to the plane, at the source bit depth:
 *       TC_CHROMA_NEAREST  C[j][i];
 *       TC_CHROMA_CENTER   (the siting of a 2 x 2 mean: the inverse of tc_frames_to_u8)  i' = i - 1 for even x, i + 1 for
 *                          odd x, j' likewise from y:  (9 C[j][i] + 3 C[j][i'] + 3 C[j'][i] + C[j'][i'] + 8) >> 4;
 *       TC_CHROMA_LEFT     (H.264 / HEVC chroma_sample_loc_type 0: co-sited with even columns, centred between rows)
 *                          x even: (3 C[j][i] + C[j'][i] + 2) >> 2;
 *                          x odd, i+ = min(i + 1, cw - 1): (3 C[j][i] + 3 C[j][i+] + C[j'][i] + C[j'][i+] + 4) >> 3;
 *   - colour, with c = Y - yoff, d = Cb - coff, e = Cr - coff and the matrix m of the STRUCT (tc_yuv_matrix's or any other:
 *     the kernel has no built-in standard):
 *       R = clip((cy c + crv e + 32768) >> 16, 0, 255)
 *       G = clip((cy c - cgu d - cgv e + 32768) >> 16, 0, 255)
 *       B = clip((cy c + cbu d + 32768) >> 16, 0, 255)
 *     with 10-bit samples and tc_yuv_matrix's tables every sum stays below 2^27.
 * 10-bit code values map linearly to 8-bit RGB: no transfer function, no tone mapping.
 * `slots` is a HOST array; every other pointer is device memory.
 * workspace: tc_frames_from_yuv_workspace bytes = n * sh * sw * 3 (the RGB image) + tc_frames_from_u8_workspace of the same
 * sizes (0 for a request tc_frames_from_yuv refuses for its sizes).
 * TC_EINVAL: NULL p / y / c0 / out / slots, c1 missing for I420 or present otherwise, an unknown format or siting, n <= 0 or
 * > TC_FRAMES_U8_MAX, a size <= 0, pitch_y below the row's bytes (sw; 2 sw for P010), pitch_c below cw (I420), 2 cw (NV12),
 * 4 cw (P010), image_stride_y < sh * pitch_y, image_stride_c < ch * pitch_c, a slot outside [0, b * t), tables missing for a
 * pass that runs, cy <= 0; TC_EALIGN: a P010 pointer, pitch or image stride that is not 2-byte aligned; TC_EWORKSPACE:
 * workspace too small.  Nothing is launched or written on a refusal. */
enum { TC_PIXFMT_P010 = 3 };   /* an input format: tc_frames_to_u8 does not write it */
enum { TC_CHROMA_NEAREST = 0, TC_CHROMA_CENTER = 1, TC_CHROMA_LEFT = 2 };
typedef struct TcFramesYuvParams {
  const void* y;             /* n luma planes */
  const void* c0;            /* Cb (I420) or interleaved Cb, Cr (NV12, P010) */
  const void* c1;            /* Cr (I420), else NULL */
  int64_t image_stride_y, image_stride_c;   /* bytes from one image to the next */
  int32_t pitch_y, pitch_c;  /* bytes from one row to the next */
  int32_t format;            /* TC_PIXFMT_I420 / NV12 / P010 */
  int32_t siting;            /* TC_CHROMA_* */
  int32_t m[7];              /* cy, crv, cgu, cgv, cbu, yoff, coff */
  int32_t n, sh, sw;
  const int32_t* slots;      /* HOST: n frame indices batch * t + frame */
  float* out;                /* (b, 3, t, H, W) fp32 */
  int32_t b, t, h, w;
  const int32_t* h_bounds; const int32_t* h_coefs; int32_t h_kmax;   /* tables sw -> rw (NULL when nothing is resized) */
  const int32_t* v_bounds; const int32_t* v_coefs; int32_t v_kmax;   /* tables sh -> rh */
  void* workspace; int64_t workspace_bytes;
} TcFramesYuvParams;
int64_t tc_frames_from_yuv_workspace(const TcFramesYuvParams* p);
int tc_frames_from_yuv(const TcFramesYuvParams* p, void* stream);

/* ---- Planar frames out in a named colour: the decoder's fp32 clips -> I420 / NV12 frames of any standard and range with
 * centre or left chroma siting, or 10-bit P010 (additive within ABI 14: one struct, three symbols).  tc_frames_to_u8 above
 * stays as it is (8-bit BT.601 limited range, centre siting); tc_frames_to_yuv contains it: with tc_yuv_out_matrix's
 * BT.601 limited 8-bit row and TC_CHROMA_CENTER it writes the same bytes. ---- */

/* The integer RGB -> YCbCr matrix of a standard, the forward counterpart of tc_yuv_matrix: HOST code, double precision, no
 * device call.   m = {yr, yg, yb, ur, ug, ub, vr, vg, vb, yoff, coff}.
 * bits 8: the RGB samples are 8-bit; bits 10: they are the 16-bit intermediate of tc_frames_to_yuv's P010 path.  With
 * bits_in = 8 | 16:  F = 8 + bits_in (16 | 24), inmax = 2^bits_in - 1, q = 2^(bits - 8), (Kr, Kb) as for tc_yuv_matrix.
 *   limited range: gy = 219 q / inmax, gc = 224 q / inmax, yoff = 16 q;
 *   full range:    gy = gc = (2^bits - 1) / inmax, yoff = 0;                 coff = 128 q in both.
 * With r(v) = floor(v * 2^F + 0.5):
 *   yr = r(Kr gy), yb = r(Kb gy), yg = r(gy) - yr - yb                      (white lands exactly on r(gy));
 *   ub = vr = r(gc / 2), ur = r(-Kr / (2 (1 - Kb)) gc), ug = -(ub + ur),
 *   vb = r(-Kb / (2 (1 - Kr)) gc), vg = -(vr + vb)                          (each chroma row sums to 0: grey is neutral).
 * E.g. BT.601 limited 8 bit: 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, yoff 16, coff 128 -- the
 * constants of tc_frames_to_u8; BT.709 limited 10 bit: 47678, 160389, 16192, -26280, -88410, 114690, 114690, -104174,
 * -10516, yoff 64, coff 512 (red gives Y, Cb, Cr = 250, 409, 960; white Y 940; black Y 64).
 * TC_EINVAL: an unknown standard or range, bits other than 8 or 10, NULL m. */
int tc_yuv_out_matrix(int32_t standard, int32_t range, int32_t bits, int32_t m[11]);

/* Frames f0 .. f0 + nf - 1 of every clip of x (b, 3, t, h, w) fp32 -> planar 4:2:0 frames of (oh, ow) pixels by the matrix
 * m of the STRUCT (tc_yuv_out_matrix's or any other: the kernel has no built-in standard), in this order:
 *   I420 / NV12 (8 bit):
 *   1. value and 2. resample: steps 1 and 2 of tc_frames_to_u8, on uint8 RGB in int32 (the same device functions);
 *   P010 (10 bit) -- the path never passes through 8 bits:
 *   1. value: c = clamp(x, -1, 1), h = (c + 1) / 2, s = h * 65535.0f, q = (uint16_t)floorf(s + 0.5f), every fp32 operation
 *      rounded on its own (nothing contracted);
 *   2. resample of the uint16 RGB with the SAME tables (tc_resize_tables_filter, 2^22 coefficients), summed in int64:
 *      clip(((1 << 21) + sum coefs * src) >> 22, 0, 65535), passes and their order as for tc_frames_to_u8;
 *   3. colour, with F = 16 (8 bit) or 24 (P010), max = 255 or 1023, in int32 (8 bit) or int64 (P010):
 *        Y = clip((yr R + yg G + yb B + (yoff << F) + (1 << (F - 1))) >> F, 0, max)       for every pixel,
 *        C = clip((cr Rs + cg Gs + cb Bs + (coff << (F + s)) + (1 << (F + s - 1))) >> (F + s), 0, max)
 *      for every chroma sample (bx, by), with the row (ur, ug, ub) for Cb and (vr, vg, vb) for Cr:
 *        TC_CHROMA_CENTER  Rs, Gs, Bs = the sums over the 2 x 2 block, s = 2 (the siting of tc_frames_to_u8);
 *        TC_CHROMA_LEFT    (H.264 / HEVC chroma_sample_loc_type 0) the sample is co-sited with column x0 = 2 bx and centred
 *                          between rows 2 by and 2 by + 1: Rs, Gs, Bs = the sum over both rows of P[x0 - 1] + 2 P[x0] +
 *                          P[x0 + 1], x0 - 1 clamped to 0 (x0 + 1 exists: ow is even), s = 3.
 *      All shifts are arithmetic, sums may be negative, the clip is two-sided (full-range blue reaches 256 before it).  With
 *      tc_yuv_out_matrix's rows no 8-bit sum exceeds 2^27 (full-range blue reaches exactly that); a caller's own matrix
 *      must keep them inside int32.
 *   4. format: I420 and NV12 as tc_frames_to_u8 lays them out; P010 is NV12's layout in 16-bit little-endian words, the
 *      stored word = code << 6 (the low six bits are zero): `pitch` is in bytes and >= 2 ow;
 *   5. placement, f0 / nf, frame_stride, clip_stride (bytes): exactly tc_frames_to_u8's.
 * A frame's bytes: I420 / NV12 as there; P010 pitch * oh + pitch * (oh / 2).
 * workspace: tc_frames_to_yuv_workspace bytes -- 8 bit: b * nf * h * w * 3 plus, when ow != w, b * nf * h * ow * 3; P010: two
 * bytes per sample, b * nf * h * w * 6 plus b * nf * h * ow * 6 (0 for a request tc_frames_to_yuv refuses for anything but
 * its workspace).  Every pointer is device memory.
 * TC_EINVAL: what tc_frames_to_u8 refuses with it (pitch below ow bytes, 2 ow for P010), a format other than I420 / NV12 /
 * P010 (RGB24 too), a siting other than CENTER / LEFT (NEAREST is not a way to produce chroma), yr, yg, yb not all
 * positive; TC_ESHAPE: an odd oh or ow or, for I420, an odd pitch; TC_EALIGN: P010 with an odd out, pitch, frame_stride,
 * clip_stride or workspace; TC_EWORKSPACE: workspace too small.  Nothing is launched or written on a refusal. */
typedef struct TcFramesYuvOutParams {
  const float* x;              /* (b, 3, t, h, w) fp32: the decoder's output */
  void* out;
  int32_t b, t, h, w;
  int32_t f0, nf;              /* frames f0 .. f0+nf-1 of every clip are written, 0 <= f0, nf >= 1, f0+nf <= t */
  int32_t oh, ow;              /* output size, both even; (oh, ow) == (h, w): no resample, no tables */
  int32_t format;              /* TC_PIXFMT_I420 / NV12 / P010 */
  int32_t pitch;               /* bytes per row of the Y plane */
  int64_t frame_stride, clip_stride;   /* bytes from one written frame / clip to the next in out */
  const int32_t* h_bounds; const int32_t* h_coefs; int32_t h_kmax;   /* w -> ow (NULL when ow == w) */
  const int32_t* v_bounds; const int32_t* v_coefs; int32_t v_kmax;   /* h -> oh (NULL when oh == h) */
  void* workspace; int64_t workspace_bytes;
  int32_t siting;              /* TC_CHROMA_CENTER / TC_CHROMA_LEFT */
  int32_t m[11];               /* yr, yg, yb, ur, ug, ub, vr, vg, vb, yoff, coff */
} TcFramesYuvOutParams;
int64_t tc_frames_to_yuv_workspace(const TcFramesYuvOutParams* p);
int tc_frames_to_yuv(const TcFramesYuvOutParams* p, void* stream);

/* ---- Colour match: decoded frames to their keyframes, on the device (additive within ABI 14: three structs, four symbols).
 * The decoder's frames drift in colour and contrast away from the keyframes they interpolate; this is the linear colour
 * transfer that workflows around the model run on the host (mean / std transfer, or the Monge-Kantorovich linear map), as
 * one reduction, one 3 x 3 solve per frame and one affine pass, without a synchronisation.  THE RULE, stated once (its
 * float64 restatement for the tests: tests/colour_match_ref.py):
 *
 * All statistics are taken of c = clamp(x, -1, 1): what the output path shows (tc_video_to_u8 clamps to it).
 *
 * Frame statistics: TC_COLOUR_STATS = 9 doubles per frame over its n = h * w pixels, in this order:
 *   sum r, sum g, sum b, sum rr, sum rg, sum rb, sum gg, sum gb, sum bb.
 * Products are formed in double (exact: both factors are fp32); sums are in double in an order fixed by h * w alone: the
 * frame is cut into P = min(64, ceil(h * w / 2048)) parts of 256 threads, thread j of part p adds pixels 4 q .. 4 q + 3 for
 * q = p * 256 + j, then q + 256 P, ..., in that order; the 64 lanes of a wave are added by an xor tree (32, 16, .. 1), the four
 * waves in index order, and the P per-part sums (in the workspace) in index order.  No atomics.  A frame's nine numbers
 * therefore do not depend on b, on the batch slot, on the alignment of x or on which other frames are requested.
 * From the sums: m = S1 / n, C = S2 / n - m m^T (symmetric 3 x 3).
 *
 * Knots.  A clip of t frames has nk reference images, 1 <= nk <= TC_TEMPORAL_MAX_FRAMES, at strictly increasing frame indices
 * k_0 < ... < k_{nk-1}, all in [0, t) and the same for every clip of the batch, each with statistics (tc_colour_match_knots)
 * or a histogram (tc_colour_transfer_knots) over ref_pixels pixels.  The indices are HOST values inside the params struct
 * (int32_t nk; int32_t knot[TC_TEMPORAL_MAX_FRAMES]); the launcher copies them into the kernel arguments: no device read, no
 * synchronisation, safe to capture.  tc_colour_match and tc_colour_transfer are the knots {0, t - 1} ({0} when t = 1, with
 * the first reference image) and no gain limit: the same launcher, the same bits as ever.
 *
 * Course of frame f (csrc/colour_course.h states it once for both kernels).  f <= k_0: the target is knot 0 itself;
 * f >= k_{nk-1}: the last knot itself; otherwise j is the last knot with k_j <= f and
 *   w = (double)(f - k_j) / (double)(k_{j+1} - k_j);
 * a frame on a knot takes that knot itself.  For the linear methods m_t = (1 - w) m_j + w m_{j+1} and C_t likewise (a
 * convex combination of covariances is a covariance); for the histogram transfer T = q_j + w (q_{j+1} - q_j), below.
 *
 * Regularisation: eps = 2^-16 in value^2 units (about half an 8-bit code value squared), added to every diagonal that is
 * inverted or rooted, on the source and on the target side.
 *
 * Map of frame f, with (m_s, C_s) the frame's own statistics; every step in double:
 *   TC_COLOUR_MEAN_STD  A = diag(sqrt((C_t[k][k] + eps) / (C_s[k][k] + eps)));
 *   TC_COLOUR_MKL       S = C_s + eps I, T = C_t + eps I,  A = S^(-1/2) (S^(1/2) T S^(1/2))^(1/2) S^(-1/2), the symmetric
 *                       roots from an eigendecomposition of the 3 x 3 matrix: cyclic Jacobi, pairs (0,1), (0,2), (1,2), a
 *                       fixed eight sweeps; eigenvalues of S are clamped below at eps / 2, those of the middle matrix at 0,
 *                       and the middle matrix is symmetrised, (M + M^T) / 2, before it is decomposed;
 *   gain limit          max_gain g (tc_colour_match_knots): 0 = none; otherwise finite and >= 1, applied to A in double before o
 *                       and before the strength, so the means are still matched.  MEAN_STD: every diagonal entry is clamped
 *                       to [1 / g, g], 1 / g formed once.  MKL: A is symmetrised, (A + A^T) / 2, decomposed by the same cyclic
 *                       Jacobi (same pairs, eight sweeps), its eigenvalues are clamped to [1 / g, g] and A = V diag V^T is
 *                       rebuilt -- whenever g > 0, whether or not an eigenvalue was outside: one path, a continuous map.
 *   o = m_t - A m_s;   with strength s in [0, 1]:  A' = I + s (A - I),  o' = s o.
 * Each of the twelve numbers is rounded to fp32 once and written to coefs[frame][12]: A' row-major, then o'.
 *
 * Apply, in fp32, per pixel and output channel k, with r, g, b the CLAMPED inputs:
 *   y_k = ((o'_k + A'_k0 r) + A'_k1 g) + A'_k2 b,
 * every product and every sum rounded on its own (nothing contracted into an FMA), so that separate float32 operations on
 * any host give the same bits.  y is NOT clamped: the back end clamps.  Exact consequences: strength 0 returns clamp(x);
 * MEAN_STD of a frame against its own statistics returns clamp(x); MEAN_STD with g = 1 gives A' = I exactly and
 * o' = fp32(s (m_t - m_s)), the mean shift alone.  Without a limit a frame that is flat where its references are not gets a gain
 * of about sqrt(var_ref / eps), tens to hundreds: that is what max_gain is for.
 *
 * Not offered: a colour space other than the model's RGB values. */
#define TC_COLOUR_STATS 9
typedef struct TcColourStatsParams {
  const float* x;            /* (b, 3, t, h, w) fp32 */
  int32_t b, t, h, w;
  int32_t f0, nf, fstep;     /* frames f0, f0 + fstep, ... (nf of them) of every clip; nf = 1: fstep is ignored */
  double* stats;             /* [b * nf][TC_COLOUR_STATS], 8-byte aligned */
  void* workspace; int64_t workspace_bytes;
} TcColourStatsParams;
/* Statistics of the named frames: two launches (per-part sums, then their sum in index order).  h * w need not be a
 * multiple of anything: 16-byte loads where every plane base allows them, 4-byte loads otherwise, the same order either way.
 * workspace: b * nf * P * 9 doubles (0 for a request that is refused for anything but its workspace).
 * TC_EINVAL: NULL p / x / stats, a size <= 0, nf <= 0, f0 outside [0, t), fstep < 1 with nf > 1, a frame past t - 1;
 * TC_EALIGN: stats or workspace not 8-byte aligned; TC_EWORKSPACE: workspace NULL or too small; TC_ESHAPE: more than 2^31 - 1
 * parts in all.  Nothing is launched or written on a refusal. */
int64_t tc_colour_stats_workspace(const TcColourStatsParams* p);
int tc_colour_stats(const TcColourStatsParams* p, void* stream);

enum { TC_COLOUR_MEAN_STD = 0, TC_COLOUR_MKL = 1 };
typedef struct TcColourMatchParams {
  const float* x; float* out;   /* (b, 3, t, h, w); out may be EXACTLY x, any other overlap is TC_EINVAL */
  int32_t b, t, h, w;
  const double* src;            /* [b * t][9]: the statistics of x with f0 = 0, nf = t, fstep = 1 */
  const double* ref;            /* [b * 2][9]: statistics of the two reference images of every clip */
  int64_t ref_pixels;           /* pixels per reference image (need not be h * w) */
  int32_t method; float strength;
  float* coefs;                 /* [b * t][12] fp32, written by the call (required) */
} TcColourMatchParams;
/* The match: two launches (the coefficients, one thread per frame in double; then the apply pass).  No allocation, no
 * synchronisation, no host read of device memory.
 * TC_EINVAL: NULL p / x / out / src / ref / coefs, a size <= 0, an unknown method, a strength outside [0, 1] or not finite,
 * ref_pixels <= 0, out overlapping x other than out == x; TC_EALIGN: src or ref not 8-byte aligned; TC_ESHAPE: more than
 * 2^31 - 1 blocks in all.  Nothing is launched or written on a refusal. */
int tc_colour_match(const TcColourMatchParams* p, void* stream);

typedef struct TcColourMatchKnotsParams {
  const float* x; float* out;   /* as in TcColourMatchParams, field for field, down to coefs */
  int32_t b, t, h, w;
  const double* src;            /* [b * t][9] */
  const double* ref;            /* [b * nk][9]: statistics of the nk reference images of every clip, in knot order */
  int64_t ref_pixels;
  int32_t method; float strength;
  float* coefs;                 /* [b * t][12] fp32, written by the call (required) */
  int32_t nk;                   /* 1 .. TC_TEMPORAL_MAX_FRAMES */
  int32_t knot[TC_TEMPORAL_MAX_FRAMES];   /* the first nk: strictly increasing frame indices in [0, t); host values */
  float max_gain;               /* 0: no limit; otherwise finite and >= 1 */
} TcColourMatchKnotsParams;
/* tc_colour_match towards nk reference images at the knots, with an optional gain limit (the rule above): the same two
 * launches; only the coefficient kernel knows the course.  Refuses what tc_colour_match refuses, with the same codes, and
 * TC_EINVAL: nk outside [1, TC_TEMPORAL_MAX_FRAMES], knots not strictly increasing or outside [0, t), max_gain negative, in
 * (0, 1) or not finite.  Nothing is launched or written on a refusal. */
int tc_colour_match_knots(const TcColourMatchKnotsParams* p, void* stream);

/* ---- Histogram colour transfer (additive within ABI 14: three structs, four symbols).  What a decoder does to toon frames is
 * a bent tone curve per channel (blacks lift, highlights compress), which no 3 x 3 matrix repairs: this is the per-channel
 * monotone transfer that carries a frame's histogram onto its keyframes'.  THE RULE, stated once (restated with numpy integers
 * and float64 for the tests: tests/colour_hist_ref.py):
 *
 * Bins.  TC_COLOUR_BINS = 1024: four per 8-bit code, one per 10-bit code.  c = clamp(x, -1, 1) = fminf(fmaxf(x, -1), 1), the
 * clamp of tc_colour_stats (a NaN becomes -1);  bin(c) = min(1023, (int) floorf((c + 1.0f) * 512.0f)), the fp32 add rounded,
 * the multiply exact.  So -1 and everything below fall into bin 0, +-0 into bin 512, 1, everything above it and the largest
 * float below 1 into bin 1023, 1/512 - 1 into bin 1 and its fp32 predecessor into bin 0.
 *
 * Histogram of a frame: 3 x 1024 int32 counts, channel r, then g, then b.  Counts are exact integers: no order of summation
 * is part of the result, and the result does not depend on what hist or the workspace held before the call.
 *
 * Transfer of frame f of t, per channel.  s[i]: the frame's counts, n = h * w;  a[i], b[i]: the counts of the reference
 * images at knots j and j + 1 of the frame's course (the knots and the course: tc_colour_match above; tc_colour_transfer is
 * the knots {0, t - 1}, the clip's first and last reference image), m = ref_pixels each.
 *   midpoint rank   P_i = 2 S_i - s_i with S_i = sum_{j <= i} s_j: an integer in [0, 2n].  Only bins with s_i > 0 get an
 *                   entry (there P_i > 0); every other entry of the table is +0.0f.
 *   quantile        for r in {a, b}:  A_j = sum_{i < j} r_i (A_0 = 0, A_1024 = m);  j the smallest index in [1, 1024] with
 *                   A_j 2n >= P_i m, compared in integers (both sides < 2^53 by the size limit below); then A_{j-1} 2n < P_i m
 *                   and r_{j-1} > 0, and in bin units
 *                     q_r = (double)(j - 1) + (double)(P_i m - A_{j-1} 2n) / (double)(r_{j-1} 2n):
 *                   both integers exact in double, one division, one addition.
 *   course          T = q_a + w (q_b - q_a) with the w of the course;  a frame on a knot, before the first or after the last
 *                   takes that knot's q itself (with knots {0, t - 1}: w = (double) f / (double)(t - 1), frame t - 1 takes
 *                   q_b itself, and t = 1 takes q_a).  This interpolates quantile functions (the one-dimensional transport
 *                   geodesic), the counterpart of the linear course of (m, C) in tc_colour_match.
 *   entry           D[f][k][i] = (float)((T - ((double) i + 0.5)) / 512.0): the displacement of bin i in value units, rounded
 *                   to fp32 once.  Every double operation is rounded on its own; nothing is contracted.
 *
 * Apply, in fp32, nothing contracted, per pixel and channel:  v = c + D[bin(c)],  y = beta + s (v - beta)  with s the
 * strength and beta = c, or beta = clamp(base) when a base clip is given.  y is NOT clamped: it can leave [-1, 1] by less than
 * a bin, and the back end clamps.  Each bin is translated rigidly: detail inside a bin survives, there is no banding.
 *
 * Exact consequences (checked on the numpy statement and on the device):
 *   strength 0      returns clamp(x), or clamp(base), exactly;
 *   self-match      a frame whose two references have its own histogram (also at a multiple of its pixel count) gets an
 *                   all-zero table and comes back as clamp(x), at every frame index and every strength;
 *   whole-bin shift a frame whose values all lie on the grid (2k + 1)/2048 - 1 and whose reference is the frame shifted by a
 *                   whole number of bins, nothing clipped on either side, gets exactly that shift in every occupied bin
 *                   and comes back equal to the reference bit for bit (64 bins: D = 0.125);
 *   monotone        T is non-decreasing over the occupied bins.
 *
 * Size limit: h * w <= 2^26 and ref_pixels <= 2^26, otherwise TC_ESHAPE: what keeps P_i m and A_j 2n exact in int64 and double.
 *
 * Not offered: a colour space other than the model's RGB values; and a flat frame cannot be spread by any histogram match:
 * all its pixels share a bin and move together (a tone curve has no matrix, so there is no gain limit here). */
#define TC_COLOUR_BINS 1024
typedef struct TcColourHistParams {
  const float* x;            /* (b, 3, t, h, w) fp32 */
  int32_t b, t, h, w;
  int32_t f0, nf, fstep;     /* frames f0, f0 + fstep, ... (nf of them) of every clip, as in TcColourStatsParams */
  int32_t* hist;             /* [b * nf][3][TC_COLOUR_BINS], 4-byte aligned */
  void* workspace; int64_t workspace_bytes;
} TcColourHistParams;
/* Histograms of the named frames: two launches (per-part histograms built with LDS integer atomics, a private one per wave;
 * then their sum).  No memset and no global atomic.  16-byte loads where every plane base allows them, 4-byte loads
 * otherwise; the counts are the same.  workspace: b * nf * 3 * P * 1024 int32 with P = min(16, ceil(h * w / 1024)) (0 for a
 * request that is refused for anything but its workspace).
 * TC_EINVAL: NULL p / x / hist, a size <= 0, nf <= 0, f0 outside [0, t), fstep < 1 with nf > 1, a frame past t - 1;
 * TC_EALIGN: hist or workspace not 4-byte aligned; TC_EWORKSPACE: workspace NULL or too small; TC_ESHAPE: h * w > 2^26 or
 * more than 2^31 - 1 blocks in all.  Nothing is launched or written on a refusal. */
int64_t tc_colour_hist_workspace(const TcColourHistParams* p);
int tc_colour_hist(const TcColourHistParams* p, void* stream);

typedef struct TcColourTransferParams {
  const float* x;               /* (b, 3, t, h, w) */
  const float* base;            /* NULL, or a clip of the shape of x: what strength blends against */
  float* out;                   /* may be EXACTLY x; any other overlap with x, and any overlap with base, is TC_EINVAL */
  int32_t b, t, h, w;
  const int32_t* src;           /* [b * t][3][1024]: the histograms of all frames of x (f0 = 0, nf = t, fstep = 1) */
  const int32_t* ref;           /* [b * 2][3][1024]: histograms of the two reference images of every clip */
  int64_t ref_pixels;           /* pixels per reference image (need not be h * w) */
  float strength;
  float* table;                 /* [b * t][3][1024] fp32, written by the call (required) */
} TcColourTransferParams;
/* The transfer: two launches (the tables, one block per frame and channel in integers and double; then the apply pass).  No
 * allocation, no synchronisation, no host read of device memory: safe to capture in a hipGraph.  The call trusts its
 * histograms as tc_colour_match trusts src: src must hold the counts of x and sum to h * w per channel, ref must sum to
 * ref_pixels; with other counts the tables mean nothing (no access leaves the buffers).
 * TC_EINVAL: NULL p / x / out / src / ref / table, a size <= 0, a strength outside [0, 1] or not finite, ref_pixels <= 0,
 * out overlapping x other than out == x, out overlapping base; TC_EALIGN: src, ref or table not 4-byte aligned; TC_ESHAPE:
 * h * w or ref_pixels > 2^26, more than 2^31 - 1 blocks in all.  Nothing is launched or written on a refusal. */
int tc_colour_transfer(const TcColourTransferParams* p, void* stream);

typedef struct TcColourTransferKnotsParams {
  const float* x;               /* as in TcColourTransferParams, field for field, down to table */
  const float* base;
  float* out;
  int32_t b, t, h, w;
  const int32_t* src;           /* [b * t][3][1024] */
  const int32_t* ref;           /* [b * nk][3][1024]: histograms of the nk reference images of every clip, in knot order */
  int64_t ref_pixels;
  float strength;
  float* table;                 /* [b * t][3][1024] fp32, written by the call (required) */
  int32_t nk;                   /* 1 .. TC_TEMPORAL_MAX_FRAMES */
  int32_t knot[TC_TEMPORAL_MAX_FRAMES];   /* the first nk: strictly increasing frame indices in [0, t); host values */
} TcColourTransferKnotsParams;
/* tc_colour_transfer towards nk reference images at the knots: the same two launches; only the table kernel knows the
 * course.  Refuses what tc_colour_transfer refuses, with the same codes, and TC_EINVAL: nk outside
 * [1, TC_TEMPORAL_MAX_FRAMES], knots not strictly increasing or outside [0, t).  Nothing is launched or written on a refusal. */
int tc_colour_transfer_knots(const TcColourTransferKnotsParams* p, void* stream);

/* ---- Frame deltas: how much consecutive keyframes differ, measured on the surfaces a decoder leaves (additive within ABI 14:
 * one struct, two symbols).  What a timeline needs to know where NOT to interpolate -- a scene cut, a held drawing -- without
 * pulling the surfaces to the host.  THE RULE, stated once (restated with numpy integers for the tests:
 * tests/frame_delta_ref.py):
 *
 * Images.  n images of h x w pixels in one of four layouts.  Pointers, pitches, image strides and the chroma size
 * ch = (h + 1) / 2, cw = (w + 1) / 2 mean what they mean in TcFramesYuvParams (I420: y, c0 = Cb, c1 = Cr; NV12 / P010: y and
 * c0 = interleaved Cb, Cr, c1 NULL).  TC_PIXFMT_RGB24: y is the packed (n, h, w, 3) image, pitch_y >= 3 w, c0 = c1 = NULL and
 * pitch_c / image_stride_c are not read.
 *
 * Components.  Planar formats: 0 = Y (S_0 = h w samples), 1 = Cb, 2 = Cr (S_1 = S_2 = ch cw samples).  RGB24: R, G, B
 * (S_c = h w each).
 *
 * The 8-bit value of a sample is the byte itself; for P010 it is word >> 8 (the upper byte of the little-endian word), so a
 * P010 surface holding v << 8, whatever its low eight bits, gives exactly the NV12 numbers of v.  (tc_frames_from_yuv reads
 * ten bits, word >> 6; a measure of difference needs no more than eight.)
 *
 * hist[i][c][k], k < TC_DELTA_BINS = 64: the number of samples of component c of image i with v >> 2 == k.  Exact int32.
 *
 * delta[p][c], for the pair (image p, image p + lag), 0 <= p < n - lag, over the samples a of image p and b of image p + lag
 * at the same place, is three int64:
 *   [0] sad      sum of |a - b|;
 *   [1] changed  the number of samples with |a - b| > tau;
 *   [2] hist_l1  sum over k of |hist[p][c][k] - hist[p + lag][c][k]|.
 *
 * All results are exact integers: no order of summation is part of the result, the width of the loads is not, and nothing
 * depends on what hist, delta or the workspace held before the call.
 *
 * Exact consequences (checked on the numpy statement and on the device): equal images give sad = changed = hist_l1 = 0; an
 * image of 0 against an image of 255 gives sad = 255 S_c, changed = S_c (tau < 255), hist_l1 = 2 S_c; sum_k hist = S_c.
 *
 * Two launches: per-part counts (a histogram per wave in LDS, integer LDS atomics; |a - b| four bytes at a time), then the sum
 * of the parts in int64 and hist_l1.  A part is at most 3 * 2^18 samples, so its int32 counters cannot overflow (255 * 3 * 2^18
 * < 2^31).  No memset, no global atomic, no allocation, no synchronisation, no host read of device memory: safe to capture in
 * a hipGraph.  16-byte loads where every plane base, pitch and image stride is 16-byte aligned, byte loads otherwise and at
 * the end of a row; the numbers are the same.  Every sample is read at most twice: once as a, once as b.
 * workspace: tc_frame_deltas_workspace bytes = n * P * 3 * 66 int32, P the parts of one image (0 for a request that is refused
 * for anything but its workspace).  n <= lag is legal: histograms only, delta is not touched and may be NULL.
 * TC_EINVAL: NULL p / y / hist, NULL delta with n > lag, c0 / c1 not as the format says, an unknown format, n <= 0, lag < 1,
 * tau outside [0, 255], a size <= 0, a pitch below the row's bytes (3 w; w; 2 w for P010; chroma cw, 2 cw, 4 cw for I420,
 * NV12, P010), image_stride_y < h * pitch_y, image_stride_c < ch * pitch_c; TC_EALIGN: a P010 pointer, pitch or image stride
 * that is not 2-byte aligned, hist not 4-byte aligned, delta (n > lag) or the workspace not 8-byte aligned; TC_ESHAPE:
 * h * w > 2^26 or more than 2^31 - 1 blocks in all; TC_EWORKSPACE: workspace NULL or too small.  Nothing is launched or
 * written on a refusal.
 *
 * Not offered: a judgement.  These are counts; what makes a cut or a hold of them is the caller's rule (clip.ShotRule, whose
 * default thresholds nobody has measured on real footage).  A dissolve or a fade is a gradual change and no cut by any count
 * of one pair. */
#define TC_DELTA_BINS 64
typedef struct TcFrameDeltaParams {
  const void* y;               /* n luma planes, or n packed RGB images */
  const void* c0;              /* Cb (I420) or interleaved Cb, Cr (NV12, P010); NULL for RGB24 */
  const void* c1;              /* Cr (I420), else NULL */
  int64_t image_stride_y, image_stride_c;   /* bytes from one image to the next */
  int32_t pitch_y, pitch_c;    /* bytes from one row to the next */
  int32_t format;              /* TC_PIXFMT_RGB24 / I420 / NV12 / P010 */
  int32_t n, h, w, lag, tau;
  int32_t* hist;               /* [n][3][TC_DELTA_BINS], written by the call */
  int64_t* delta;              /* [n - lag][3][3]: sad, changed, hist_l1; written by the call */
  void* workspace; int64_t workspace_bytes;
} TcFrameDeltaParams;
int64_t tc_frame_deltas_workspace(const TcFrameDeltaParams* p);
int tc_frame_deltas(const TcFrameDeltaParams* p, void* stream);

/* ---- Still regions: where the two keyframes of a clip agree, and the decoded clip held to the keyframes there (additive
 * within ABI 14: two structs, two symbols; csrc/still.hip).  A segment is mostly a character over a background that is the
 * same in both keyframes; tc_still_map says where, as a latent mask for the sampler's mask / x0 blend (tc_ddim_blend) and as
 * a pixel weight for tc_still_composite.  THE RULE, stated once (restated in numpy for the tests: tests/still_ref.py):
 *
 * Input.  ends (b, 3, 2, H, W) fp32: per clip and channel the first and the last keyframe a and b, values nominally in
 * [-1, 1] (clip.Conditions.ends_px).  H and W are multiples of TC_STILL_CELL = 8, the first stage's factor; h = H / 8,
 * w = W / 8 cells.  tau in 0 .. 255 (8-bit code values), grow >= 0 and feather >= 1 in cells,
 * D = grow + feather + 1 <= TC_STILL_MAX_DIST = 32.
 *
 * Threshold.  thr = float32(tau) / float32(127.5): one code value is 2 / 255 of [-1, 1].
 * Moved pixel.  A pixel has moved if for any channel !(fabsf(clamp(a) - clamp(b)) <= thr), where
 * clamp(v) = v < -1 ? -1 : v > 1 ? 1 : v and the subtraction is rounded on its own.  This clamp keeps a NaN (the colour path's
 * fminf / fmaxf form would turn it into -1), and the comparison is written so that a NaN fails it: a NaN counts as moved.
 * Values beyond [-1, 1] on the same side clamp to equal.
 * Moved cell.  An 8 x 8 cell has moved if any of its pixels has.
 * Distance.  d(cell) = min(D, the Chebyshev distance in cells to the nearest moved cell of the same clip).  Outside the
 * image nothing has moved; a clip with no moved cell has d = D everywhere, a moved cell has d = 0.
 * Latent mask.  mask (b, 1, 1, h, w) fp32 = 1.0 where d > grow, else 0.0: the moving area grown by `grow` cells is sampled,
 * the rest can be pinned.
 * Cell weight.  a(cell) = clamp(d - grow - 1, 0, feather), an integer: the ring of held cells next to the grown moving area
 * has 0, cells at least `feather` further in have `feather`.
 * Pixel weight.  alpha (b, H, W) fp32 is the bilinear upsampling of a(cell) with cell centres at 8 i + 3.5 and replicated
 * edges: pixel 8 i + r takes cells (i - 1, i) with weights ((7 - 2 r) / 16, (2 r + 9) / 16) for r < 4 and cells (i, i + 1)
 * with ((23 - 2 r) / 16, (2 r - 7) / 16) for r >= 4, a cell index outside the map replaced by the nearest inside -- odd
 * sixteenths per axis, so N = sum of (wy * wx * a) over the four cells is an exact integer in units of 1 / 256, and
 * alpha = float32(N) / float32(256 * feather) with one correctly rounded division.  alpha == 1.0 exactly where all four cells
 * have full weight, == 0.0 exactly where all four have none.
 * dist (b, h, w) uint8 = d, returned so that callers and tests can see the map.
 *
 * Three launches ordered by the stream (per-cell flags, kept in `dist`; the distance of one clip's cell map in LDS as a
 * separable min filter; alpha).  No workspace, no memset, no global atomic, no allocation, no synchronisation, no host read
 * of device memory: safe to capture in a hipGraph.  Nothing depends on what mask, alpha or dist held before the call.
 * TC_EINVAL: NULL p / ends / mask / alpha / dist, b, H or W <= 0, tau outside [0, 255], grow < 0, feather < 1,
 * D > TC_STILL_MAX_DIST; TC_ESHAPE: H or W not a multiple of 8, more than 16384 cells per clip, b > 65535; TC_EALIGN: ends or
 * alpha not 16-byte aligned, mask not 4-byte aligned.  Nothing is launched or written on a refusal.
 *
 * Not offered: motion compensation (a panned background has moved), and a judgement -- tau, grow and feather are the
 * caller's (clip.StillRegions, whose defaults nobody has measured on real footage). */
#define TC_STILL_CELL 8
#define TC_STILL_MAX_DIST 32
typedef struct TcStillMapParams {
  const float* ends;           /* (b, 3, 2, H, W) fp32 */
  int32_t b, h, w;             /* clips; H and W in PIXELS */
  int32_t tau, grow, feather;
  float* mask;                 /* (b, 1, 1, H / 8, W / 8) fp32, written by the call */
  float* alpha;                /* (b, H, W) fp32, written by the call */
  uint8_t* dist;               /* (b, H / 8, W / 8) uint8, written by the call */
} TcStillMapParams;
int tc_still_map(const TcStillMapParams* p, void* stream);

/* The decoded clip held to its keyframes where alpha says so.  video (b, 3, t, H, W) fp32, ends (b, 3, 2, H, W) fp32 = (e0, e1),
 * alpha (b, H, W) fp32 in [0, 1] (tc_still_map's), frames f0 .. f0 + nf - 1.  For frame j the entry point computes one float
 * on the host, s = float32(j) / float32(t - 1), and per pixel and channel, with v the video's value:
 *   key = e0 + s * (e1 - e0)
 *   out = v                        where alpha == 0, bit for bit (key is not part of the result: a NaN in the keyframes there
 *                                  does not spread)
 *   out = key                      where alpha == 1
 *   out = v + alpha * (key - v)    elsewhere
 * every operation rounded on its own (no FMA contraction).  Frame 0 gives key = e0 + 0 * (e1 - e0); frame t - 1 gives
 * e0 + (e1 - e0), which is e1 up to one rounding.  `out` has the layout of `video`; frames outside the range are not written.
 * One launch, no workspace, no synchronisation, capture safe.
 * Aliasing: `out` may be EXACTLY `video` (in place; pixels whose alpha is 0 are then not touched at all); any other overlap
 * of `out` with video, ends or alpha returns TC_EINVAL.  Also TC_EINVAL: a NULL pointer, b, t, H or W <= 0, a frame range
 * outside [0, t); TC_ESHAPE: H or W not a multiple of 8, t < 2 or t > TC_TEMPORAL_MAX_FRAMES, b > 65535; TC_EALIGN: a pointer
 * that is not 16-byte aligned.  Nothing is launched or written on a refusal. */
typedef struct TcStillCompositeParams {
  const float* video;          /* (b, 3, t, H, W) fp32 */
  const float* ends;           /* (b, 3, 2, H, W) fp32 */
  const float* alpha;          /* (b, H, W) fp32 */
  float* out;                  /* (b, 3, t, H, W) fp32; may be exactly video */
  int32_t b, t, h, w;          /* H and W in pixels */
  int32_t f0, nf;              /* frames f0 .. f0 + nf - 1 */
} TcStillCompositeParams;
int tc_still_composite(const TcStillCompositeParams* p, void* stream);

/* introspection */
int tc_abi_version(void);
const char* tc_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* TOONCRAFTER_HIP_H */
