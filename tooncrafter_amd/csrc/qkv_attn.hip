// Temporal self-attention behind its qkv projection as ONE launch, gfx950 (ABI 13):
//
//     out[:, h*64 .. h*64+64] = Attn_frames( x . Wqkv[q_h | k_h | v_h]^T + bqkv )          x: [B*16*HW, C] bf16
//
// (reference lvdm/modules/attention.py:81-144 CrossAttention over the T = 16 frames of a pixel -- to_q / to_k / to_v,
// 16 x 16 softmax per head, heads re-concatenated in front of to_out -- called from TemporalTransformer,
// attention.py:365-412, behind norm1 / norm2 of BasicTransformerBlock, attention.py:225-246.)  At UNet levels 1 and 2
// (C = 640 / 1280) the two launches this replaces are tc_gemm_bf16 (20480 x 1920 x 640, 5120 x 3840 x 1280) and
// tc_attn_temporal: the projection's epilogue is bound by its 79 / 39 MB of stores (chip-wide store ceiling ~3 TB/s,
// DESIGN 5.7) and the attention kernel reads those bytes straight back for 0.01 TFLOP of arithmetic.  Here the qkv
// tensor never exists: a third of the bytes are written, one launch instead of two.  (Level 0 has the larger fusion,
// csrc/tb_fused.hip, which also swallows the LayerNorm and the output projection: its rows are 320 wide and fit a wave's
// registers; at 640 / 1280 columns they do not, and the projection weights -- 2.4 / 9.8 MB per block tile -- would be
// re-streamed per 128 rows at the L2 -> LDS line.  DESIGN 5.9 prices that; this kernel is the part of it that pays.)
//
//  * a block owns 8 consecutive pixels x 16 frames = 128 GATHERED rows (tile row = pixel * 16 + frame; a pixel's frames are
//    HW rows apart in memory) and ONE head: a 128 x 192 output tile [q_h | k_h | v_h] over K = C, on the 4-wave skeleton
//    of csrc/gemm.hip -- tiles global -> LDS by buffer_load ... lds (XOR swizzle on the source side), two K-steps in
//    flight (gemm_common.h tc_kloop_pipe), waves 2 x 2, each 64 x 96 = 4 x 6 v_mfma_f32_16x16x32_bf16 sub-tiles (qkv_attn_tile.h);
//  * epilogue: + bias, bf16 (the roundings of the projection's own output), q and k row-major, v TRANSPOSED into the stage
//    memory; then every wave runs the attention of two pixels on 16x16x32 MFMAs (attn_frames16.h tc_attn_frames16, shared with tb_fused.hip; S^T = K Q^T:
//    a lane owns one query, softmax in-lane + two cross-row swaps, P re-laid as the A operand by permlane swaps, O = P V),
//    writes O as bf16 over its pixels' q rows and stores those rows itself: 128 contiguous bytes per row, no block barrier
//    after the attention;
//  * blocks are dealt so that the heads of one row tile run back to back on one XCD (its L2 serves the A re-reads).
//
// LDS: 2 stages x (128 + 192) rows x 128 B = 80 KiB (two blocks per CU); the epilogue's q | k | v^T (16 + 16 + 17 KiB)
// live in the stage memory.  Roundings: q / k / v, the softmax weights and the attention output in bf16, sums in fp32 --
// tc_gemm_bf16 + tc_attn_temporal differ in ONE place (tc_attn_temporal keeps its softmax weights in fp32), as
// tb_fused.hip does.
#include "qkv_attn_tile.h"     // the tile's geometry, the LDS places of q / k / v^T, QaArgs, the projection (shared with qkv_attn_long.hip)
#include "attn_frames16.h"

#include <stdlib.h>

namespace {

template <int MF>      // the projection's MFMA shape (qkv_attn_tile.h)
__global__ __launch_bounds__(QA_THREADS, 2) void qkv_attn_kernel(const QaArgs p) {
  __shared__ __attribute__((aligned(1024))) char smem[QA_LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);

  // block -> (row tile, head): XCD x (= blockIdx & 7) walks the row tiles x, x + 8, ..., all heads of a tile back to back
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int tile = (slot / p.heads) * 8 + xcd;
  const int h = slot - (slot / p.heads) * p.heads;
  if (tile >= p.tiles) return;
  const int bb = tile / p.tiles_per_b;
  const int p0 = (tile - bb * p.tiles_per_b) * 8;
  // tile row lr = pixel * 16 + frame -> memory row row0 + frame * hw + pixel
  const int64_t row0 = (int64_t)bb * QA_T * p.hw + p0;

  // ---- projection (qkv_attn_tile.h): q | k | v^T of the tile's 128 rows in the stage memory.  The A descriptor ends
  // with the last column of frame 15 of the tile's last pixel.
  const tc_rsrc_t a_rsrc = make_rsrc(p.x + row0 * p.ldx, (((int64_t)(QA_T - 1) * p.hw + 7) * p.ldx + p.c) * 2);
  qa_project<MF>(smem, a_rsrc, p.w, p.bias, p.c, h, [&](int lr, int chunk) {
    return (uint32_t)((((int64_t)(lr & 15) * p.hw + (lr >> 4)) * p.ldx) * 2 + chunk * 16);
  });

  // ---- attention: wave w takes pixels 2 w and 2 w + 1 (tile rows pr .. pr + 16 = the pixel's 16 frames); O lands as bf16
  // over the pixel's q rows (dead: this wave alone read them)
#pragma unroll
  for (int pp = 0; pp < 2; ++pp)
    tc_attn_frames16(smem + QA_Q_OFF, smem + QA_K_OFF, smem + QA_VT_OFF, QA_VT_LD, wave_u * 32 + pp * 16, lane, p.scale_log2e);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's 32 output rows are in LDS (written by this wave only)

  // ---- store: the wave's 32 rows x 64 columns, 8 lanes per row (128 contiguous bytes), 8 rows per pass
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int lr = wave_u * 32 + ps * 8 + (lane >> 3);
    const int ch = lane & 7;
    const u32x4 v = *reinterpret_cast<const u32x4*>(smem + QA_Q_OFF + lr * 128 + ((ch ^ ((lr >> 1) & 7)) << 4));
    const int64_t m = row0 + (int64_t)(lr & 15) * p.hw + (lr >> 4);
    *reinterpret_cast<u32x4*>(p.out + m * p.ldo + h * 64 + ch * 8) = v;
  }
}

// TC_QKV_ATTN, read per call: 0 never | 1 (default) 16 frames wherever eligible, 17 .. 64 frames where the measured rule of
// qkv_attn_long.hip admits the shape | 2 every shape either kernel can take
int qa_mode() {
  const char* e = getenv("TC_QKV_ATTN");
  return e ? atoi(e) : 1;
}

}  // namespace

extern "C" int tc_temporal_qkv_attn_eligible(const TcTqaParams* p) {
  if (!p || qa_mode() == 0) return 0;
  if (p->t > QA_T) return qkv_attn_long_eligible(p, qa_mode());
  return p->t == QA_T && qa_shape_ok(p, QA_T, 8);
}

extern "C" int tc_temporal_qkv_attn(const TcTqaParams* p, void* stream) {
  if (!p || !p->x || !p->wqkv || !p->out) return TC_EINVAL;
  if (!tc_temporal_qkv_attn_eligible(p)) return TC_ESHAPE;
  if (!tc_aligned16(p->x) || !tc_aligned16(p->wqkv) || !tc_aligned16(p->out)) return TC_EALIGN;
  if (p->t > QA_T) return qkv_attn_long_launch(p, reinterpret_cast<hipStream_t>(stream));
  QaArgs a;
  const unsigned grid = qa_fill(a, p, 8);
  if (tc_qkv_mfma() == 16) hipLaunchKernelGGL(qkv_attn_kernel<16>, dim3(grid), dim3(QA_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(qkv_attn_kernel<32>, dim3(grid), dim3(QA_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
