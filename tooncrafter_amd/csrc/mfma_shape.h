// The bf16 MFMA shape a K loop is written on, as a per-call A/B switch (16 = v_mfma_f32_16x16x32_bf16, 32 =
// v_mfma_f32_32x32x16_bf16): same wave tile, same LDS image, same fragment bytes, same launch -- so it is no routing switch
// (gemm_route.cpp knows nothing of it; tile, grid and instance name do not depend on it).  Read the way fused_l0.h's
// l0_env_int reads its switches; anything but 16 or 32 means the default.
//   TC_GEMM_MFMA: gemm.hip gemm_kernel AND gemm8.hip gemm8_kernel.  One reader for both files: tests/test_gpu_gemm8.py
//                 demands bit-identical results of the two, so they always sit on the same shape.
//   TC_QKV_MFMA:  qkv_attn_tile.h qa_project as qkv_attn.hip calls it: the projection of tc_temporal_qkv_attn at 16 frames.
//                 (qkv_attn_long.hip, 17 .. 64 frames, takes the template's default, 32x32x16: no run has measured it.)
#pragma once
#include <stdlib.h>

constexpr int TC_GEMM_MFMA_DEFAULT = 16;      // measured: profiles/mfma_shape_forward_ab.txt, mfma_shape_kernel_ab.txt
constexpr int TC_QKV_MFMA_DEFAULT = 16;       // measured with TC_GEMM_MFMA at 16: profiles/mfma_shape_forward_ab.txt

inline int tc_mfma_shape(const char* name, int dflt) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return v == 16 || v == 32 ? v : dflt;
}
inline int tc_gemm_mfma() { return tc_mfma_shape("TC_GEMM_MFMA", TC_GEMM_MFMA_DEFAULT); }
inline int tc_qkv_mfma() { return tc_mfma_shape("TC_QKV_MFMA", TC_QKV_MFMA_DEFAULT); }
