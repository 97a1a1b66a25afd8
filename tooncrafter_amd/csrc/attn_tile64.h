// The 128-query x 64-key tile of the spatial attention kernels, head dim 64: the register-level parts that attn_d64_kernel,
// attn_d64_dma_kernel<DUAL> (attention.hip) and attn_d64_q8_kernel (attention_q8.hip) share.  How K and V reach LDS and
// which MFMAs form S^T and O^T stay in those files.  The sibling of attn_frames16.h / attn_frames_long.h.
//
// THE LAYOUT, stated here once.  A block is 4 waves x 32 queries; S^T = K Q^T is the "swapped" product, so a lane
// (l31 = lane & 31, half = lane >> 5) owns ONE query, q = 32 wave + l31, and a softmax row reduction is in-lane plus one
// lane ^ 32 exchange.  A 64-key tile is two 32-key blocks of 16 accumulator registers each:
//     register r of key block kbk  =  key 32 kbk + (r & 3) + 8 (r >> 2) + 4 half           (the 32x32 MFMA's C layout).
// The probabilities go straight back in as the B operand of O^T += V^T P^T, registers 8 s .. 8 s + 7 of a block being
// k-step s of a 32x32x16 MFMA.  The k order inside such a step is then permuted,
//     k-slot (half, j) of step s of block kbk  =  key 32 kbk + 16 s + 8 (j >> 2) + 4 half + (j & 3),
// for BOTH operands: the V^T fragments are read in that same order (keys +0..3 and +8..11 of the lane's slab), so P never
// touches LDS.  O comes out in the same C layout, over dims instead of keys:
//     oacc[d][4 g + i]  =  O[q][32 d + 8 g + 4 half + i],        four consecutive dims = one 8-byte store.
#pragma once
#include "common.h"

namespace {

// Q fragments, the B operand of S^T = K Q^T: lane holds Q[q][16 kk + 8 half + j].  qb: row 0 of this (batch, head).
// A tail row (q_row >= lq) loads the last row instead: it computes garbage that is never stored.
__device__ __forceinline__ void tc_tile64_load_q(bf16x8 (&qf)[4], const bf16_t* qb, int q_row, int lq, int q_ss, int half) {
  const int q_ld = q_row < lq ? q_row : lq - 1;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qb + (int64_t)q_ld * q_ss + kk * 16 + half * 8);
}

// The ragged last tile: scores of keys >= lk become `masked` (-1e30f where exp2 of it is all that follows, -INFINITY where
// a block exponent is taken from the scores).  S: f32x16 or float[16].
template <class S>
__device__ __forceinline__ void tc_tile64_mask(S (&s)[2], int key0, int lk, int half, float masked) {
  if (key0 + 64 <= lk) return;
#pragma unroll
  for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = key0 + kbk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      s[kbk][r] = key < lk ? s[kbk][r] : masked;
    }
}

// The running maximum moves to m_new (>= m_run) and l, O are rescaled -- skipped whenever no row of the wave raised its
// maximum (exact: alpha would be 1).
__device__ __forceinline__ void tc_tile64_raise_max(float m_new, float& m_run, float& l_run, f32x16 (&oacc)[2]) {
  if (!__all(m_new == m_run)) {
    const float alpha = fast_exp2(m_run - m_new);
    l_run *= alpha;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
    m_run = m_new;
  }
}

// One tile of the bf16 online softmax, base 2 (c = scale * log2 e > 0, so the max commutes with it and the scale is one fma
// per score): st, the raw scores, becomes P = exp2(st c - m_run); the row sum goes into l_run.  Kept lean: the softmax,
// not the MFMAs, bounds these kernels.
__device__ __forceinline__ void tc_tile64_softmax(f32x16 (&st)[2], float c, float& m_run, float& l_run, f32x16 (&oacc)[2]) {
  float mx = st[0][0];
#pragma unroll
  for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[kbk][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  tc_tile64_raise_max(fmaxf(m_run, mx * c), m_run, l_run, oacc);
  float rs = 0.f;
#pragma unroll
  for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = fast_exp2(fmaf(st[kbk][r], c, -m_run));   // masked keys: exp2(-huge) = 0
      st[kbk][r] = pv;
      rs += pv;
    }
  rs += __shfl_xor(rs, 32, 64);
  l_run += rs;
}

// k-step s of a key block's probabilities as the bf16 B operand of O^T += V^T P^T
__device__ __forceinline__ bf16x8 tc_tile64_pack_p(const f32x16& st, int s) {
  bf16x8 pf;
#pragma unroll
  for (int j = 0; j < 8; ++j) pf[j] = (bf16_t)st[8 * s + j];
  return pf;
}

// O = oacc / l_run [+ o1, the first key/value stream's normalised result (DUAL)] [+ what orow holds (accumulate)], rounded
// to bf16 once; orow: this query's output row at its head.
template <bool DUAL>
__device__ __forceinline__ void tc_tile64_store(const f32x16 (&oacc)[2], const f32x16 (&o1)[2], float l_run, bf16_t* orow,
                                                int half, bool accumulate) {
  const float inv = 1.0f / l_run;
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float x0 = oacc[d][4 * g + 0] * inv, x1 = oacc[d][4 * g + 1] * inv;
      float x2 = oacc[d][4 * g + 2] * inv, x3 = oacc[d][4 * g + 3] * inv;
      if (DUAL) { x0 += o1[d][4 * g + 0]; x1 += o1[d][4 * g + 1]; x2 += o1[d][4 * g + 2]; x3 += o1[d][4 * g + 3]; }
      u32x2* dst = reinterpret_cast<u32x2*>(orow + d * 32 + 8 * g + 4 * half);
      if (accumulate) {
        const u32x2 old = *dst;
        x0 += __uint_as_float(old[0] << 16);
        x1 += __uint_as_float(old[0] & 0xffff0000u);
        x2 += __uint_as_float(old[1] << 16);
        x3 += __uint_as_float(old[1] & 0xffff0000u);
      }
      const u32x2 out = {pack2(x0, x1), pack2(x2, x3)};
      *dst = out;
    }
}
__device__ __forceinline__ void tc_tile64_store(const f32x16 (&oacc)[2], float l_run, bf16_t* orow, int half, bool accumulate) {
  tc_tile64_store<false>(oacc, /*o1, never read without DUAL:*/ oacc, l_run, orow, half, accumulate);
}

// host: a [batch][row][head * 64] operand -- 16-byte pointer, row and batch strides in whole 16-byte units
inline bool tc_tile64_aligned(const void* p, int64_t ss, int64_t sb) { return tc_aligned16(p) && !(ss & 7) && !(sb & 7); }

}  // namespace
