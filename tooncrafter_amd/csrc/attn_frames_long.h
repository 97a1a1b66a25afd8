// Softmax and P.V of self-attention over 17 .. 64 frames of ONE pixel and one 64-wide head, 32 queries of one wave, on
// v_mfma_f32_32x32x16_bf16 -- the core shared by attention_temporal_long.hip and attention_temporal_rel.hip (K / Q fragments
// from global memory, O to global memory: attn_temporal_wave.h) and qkv_attn_long.hip (K / Q from LDS, O over the q rows in
// LDS).  The sibling of attn_frames16.h.
#pragma once
#include "common.h"

namespace {

// max / sum of a lane and lane ^ 32.  (A permlane32_swap(x, x) would be one VALU op, but hipcc, with the flags of
// attention_temporal_long.hip, folded its two results into one -- the listing took x + x -- so the cross-half step is a
// plain shuffle; it runs twice per 32 queries.)
__device__ __forceinline__ float tc_half_max(float x) { return fmaxf(x, __shfl_xor(x, 32, 64)); }
__device__ __forceinline__ float tc_half_sum(float x) { return x + __shfl_xor(x, 32, 64); }

// Accumulator register r of lane half `half` -> key within its 32-key block (the S^T / O^T layout attn_tile64.h states):
// one set of 16 serves every block
__device__ __forceinline__ int tc_frames_key(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// st: the raw S^T = K Q^T accumulators of the NKB = TT / 32 key blocks (frames padded to TT = 32 | 64 slots), in the layout
// that attn_tile64.h states: a lane (l31 = lane & 31, half = lane >> 5) owns ONE query, a register is a key of its block.
// Keys >= t are set to -inf; max and sum are in-lane plus one exchange between the lane halves; P^T is rounded to bf16 in
// registers (st is overwritten) and fed straight in as the B operand of O^T = V^T P^T, whose k order is permuted as stated
// there; the V^T fragments are read from LDS in that same order.
// vt: V^T of the pixel in LDS, [64 dims][keys] bf16 with rows of `vt_ld` bytes, pointing at the pixel's key 0; keys
// t .. TT - 1 must hold finite values (their P is 0: 0 * garbage could still be NaN).
// oacc comes out in that header's O layout: how O leaves is the caller's.  Returns 1 / sum of the lane's query: st holds
// exp2(..) on return, and (bf16_t)(st * that) is the weight V was multiplied by.
template <int NKB>
__device__ __forceinline__ float tc_attn_frames_long(f32x16 (&st)[NKB], f32x16 (&oacc)[2], int t, float scale_log2e,
                                                    const char* vt, int vt_ld, int l31, int half) {
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[kb][r] = tc_frames_key(r, half) < t - kb * 32 ? st[kb][r] : -INFINITY;
      mx = fmaxf(mx, st[kb][r]);
    }
  mx = tc_half_max(mx);                            // key 0 is always valid: mx is finite
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f((st[kb][r] - mx) * scale_log2e);   // masked: exp2(-inf) = 0
      st[kb][r] = e;
      sum += e;
    }
  sum = tc_half_sum(sum);
  const float inv = __builtin_amdgcn_rcpf(sum);

  // compiler-only fence, no instruction: the V^T reads stay behind the softmax.  They depend on nothing above and would
  // otherwise be lifted to the top of the caller's query block, where they hold registers across the S^T MFMAs
  asm volatile("" ::: "memory");
  // O^T[dim][query] = sum_key V^T[dim][key] P^T[key][query]: k-step s of key block kb = registers 8 s .. 8 s + 7 of P^T,
  // V^T (lane: dim db*32 + l31) in the permuted key order above
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (bf16_t)(st[kb][8 * s + j] * inv);
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const char* vrow = vt + (db * 32 + l31) * vt_ld + (kb * 32 + 16 * s + 4 * half) * 2;
        const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow);        // keys +0..3
        const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + 16);   // keys +8..11
        const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), pf, oacc[db], 0, 0, 0);
      }
    }
  return inv;
}

}  // namespace
