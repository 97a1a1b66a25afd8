// The MXFP8 block quantiser (OCP e4m3 values, one E8M0 scale per 32 elements), pinned bit for bit to oracle/mx.py.  Used by
// quant_mx_kernel (gemm_mx.hip), the MX branch of layernorm_kernel (norm.hip) and the V^T pass of attn_q8_quant_kv_kernel
// (attention_q8.hip).  How a site finds its block's amax is layout and stays with it: one thread, four lanes, a lane pair.
#pragma once
#include "common.h"

namespace {

// amax: the block's max |x| as bf16 bits (x & 0x7fff: integer order == magnitude order).  Shared exponent =
// floor(log2 amax) - 8 (e4m3's emax), clamped to E8M0's [-127, 127], as the biased scale byte.
__device__ __forceinline__ int mx_scale_byte(uint32_t amax) {
  const int e = (int)(amax >> 7) - 8;                    // bf16 exponent field of amax, less emax
  return e < 0 ? 0 : (e > 254 ? 254 : e);
}

// 1 / scale = 2^(127 - byte), built from bits: exact
__device__ __forceinline__ float mx_inv_scale(int byte) { return __uint_as_float((uint32_t)(254 - byte) << 23); }

// four fp32 -> one word of four e4m3 bytes, round to nearest even (v_cvt_pk_fp8_f32); |f| <= 448 is the caller's
__device__ __forceinline__ uint32_t mx_pack4(float f0, float f1, float f2, float f3) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, w, true);
  return (uint32_t)w;
}

// ... of four block elements: scaled, saturated to +-448 (e4m3's largest finite value), packed
__device__ __forceinline__ uint32_t mx_quant4(float f0, float f1, float f2, float f3, float inv) {
  return mx_pack4(fminf(fmaxf(f0 * inv, -448.f), 448.f), fminf(fmaxf(f1 * inv, -448.f), 448.f),
                  fminf(fmaxf(f2 * inv, -448.f), 448.f), fminf(fmaxf(f3 * inv, -448.f), 448.f));
}

}  // namespace
