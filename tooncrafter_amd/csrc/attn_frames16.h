// Self-attention over the 16 frames of ONE pixel and one 64-wide head, by one wave, on v_mfma_f32_16x16x32_bf16 --
// the core shared by qkv_attn.hip (two pixels per wave) and tb_fused.hip (one pixel per wave).
#pragma once
#include "common.h"

// q, k: row-major [tile rows][64] bf16 in LDS, 128-byte rows, 16-byte chunks XOR-swizzled by (row >> 1) & 7; vt: v
// TRANSPOSED, [64 dims][tile rows] bf16 with rows of `vt_ld` bytes.  The pixel's frames are tile rows pr .. pr + 15.
// S^T = K Q^T (a lane owns one query: softmax in-lane + two cross-row swaps), P re-laid as the A operand by permlane
// swaps, O = P V; O goes as bf16 over the pixel's q rows (this wave alone read them).  The caller waits (lgkmcnt /
// barrier) before anybody reads them.  `lane` is the caller's lane id (tb_fused.hip passes an opaque copy).
__device__ __forceinline__ void tc_attn_frames16(char* q, const char* k, const char* vt, int vt_ld, int pr, int lane,
                                                 float scale_log2e) {
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  const int l15 = lane & 15, g4 = lane >> 4;
  const int row = pr + l15;
  const int sw = (row >> 1) & 7;
  const char* qrow = q + row * 128;
  const char* krow = k + row * 128;
  f32x4_t st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {                  // S^T[key][query] = sum_d K[key][d] Q[query][d]
    const int c = ((ks * 4 + g4) ^ sw) << 4;
    const bf16x8 ka = *reinterpret_cast<const bf16x8*>(krow + c);
    const bf16x8 qb = *reinterpret_cast<const bf16x8*>(qrow + c);
    st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qb, st, 0, 0, 0);
  }
  // lane: query l15, keys 4 g4 + r.  Softmax over the 16 keys: in-lane over r, across g4 by two swaps
  float mx = fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3]));
  mx = tc_max_rows(mx);
  float e[4], sum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) { e[r] = fast_exp2((st[r] - mx) * scale_log2e); sum += e[r]; }
  sum = tc_sum_rows(sum);
  const float inv = __builtin_amdgcn_rcpf(sum);
  const uint32_t pk0 = pack2(e[0] * inv, e[1] * inv), pk1 = pack2(e[2] * inv, e[3] * inv);
  // P as the A operand of P.V (rows = queries, k = keys 8 g' .. +7, keys 16..31 of the 32-deep slice are zero):
  // lane (query, g' = 0) <- keys 0..3 (own) | 4..7 (lane + 16); (query, 1) <- 8..11 (lane + 16) | 12..15 (lane + 32)
  // (rows of 16 lanes r0..r3 = g4: swap16(x) gives row 0 (x.r0, x.r1); swap32(x)'s second value brings rows 2, 3 down
  // to rows 0, 1, and swap16 of THAT gives row 1 (x.r2, x.r3))
  uint32_t a0, b0, a1, b1, lo, hi, c0, d0, c1, d1;
  tc_swap16(pk0, a0, b0);
  tc_swap16(pk1, a1, b1);
  tc_swap32(pk0, lo, hi);
  tc_swap16(hi, c0, d0);
  tc_swap32(pk1, lo, hi);
  tc_swap16(hi, c1, d1);
  const bool r0 = g4 == 0, r1 = g4 == 1;
  u32x4 pw;
  pw[0] = r0 ? a0 : (r1 ? c0 : 0u);
  pw[1] = r0 ? a1 : (r1 ? c1 : 0u);
  pw[2] = r0 ? b0 : (r1 ? d0 : 0u);
  pw[3] = r0 ? b1 : (r1 ? d1 : 0u);
  const bf16x8 pa = __builtin_bit_cast(bf16x8, pw);
  // O[query][d] = sum_key P[query][key] V[key][d]: B operand from v^T (lane: dim db*16 + l15, keys 8 g' .. +7 of the
  // pixel; g' >= 2 meets the zero half of P: it re-reads the valid half, never uninitialised bytes)
  const char* vrow = vt + l15 * vt_ld + (pr + 8 * (g4 & 1)) * 2;
  f32x4_t od[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const bf16x8 vb = *reinterpret_cast<const bf16x8*>(vrow + db * 16 * vt_ld);
    od[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
  // lane: dim db*16 + l15, queries 4 g4 + r -> bf16 over the pixel's q rows
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = pr + 4 * g4 + r;
      const int d = db * 16 + l15;
      char* dst = q + orow * 128 + (((d >> 3) ^ ((orow >> 1) & 7)) << 4) + (d & 7) * 2;
      *reinterpret_cast<bf16_t*>(dst) = (bf16_t)od[db][r];
    }
}
