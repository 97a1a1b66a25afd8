// The 128 x 192 [q_h | k_h | v_h] tile of the one-launch qkv projection + temporal attention (qkv_attn.hip: 16 frames,
// qkv_attn_long.hip: 17 .. 64 frames): its geometry, the places of q / k / v^T in the dead stage memory, the kernel
// arguments.  Constants and a plain struct only: nothing here emits code.
#pragma once
#include "gemm_common.h"

namespace {

constexpr int QA_BM = 128, QA_BN = 192, QA_THREADS = 256, QA_T = 16;
constexpr int QA_A_BYTES = QA_BM * TC_BK * 2;                 // 16 KiB
constexpr int QA_STAGE = (QA_BM + QA_BN) * TC_BK * 2;         // 40 KiB
constexpr int QA_LDS = 2 * QA_STAGE;                          // 80 KiB
constexpr int QA_Q_OFF = 0;                                   // [128 rows][64] bf16, 16-byte chunks XOR-swizzled by (row >> 1) & 7
constexpr int QA_K_OFF = 128 * 128;
constexpr int QA_VT_OFF = 2 * 128 * 128;                      // [64 dims][128 rows + 8] bf16: 272-byte rows
constexpr int QA_VT_LD = 272;
static_assert(QA_VT_OFF + 64 * QA_VT_LD <= QA_LDS, "epilogue buffers live in the stage memory");
constexpr int QA_RA = QA_BM / 32, QA_RB = QA_BN / 32;         // loader rows per thread: 4 + 6 requests per K-step

struct QaArgs {
  const bf16_t* x; const bf16_t* w; const float* bias; bf16_t* out;
  int hw, c, heads, ldx, ldo;
  float scale_log2e;
  int tiles, tiles_per_b;
};

}  // namespace
