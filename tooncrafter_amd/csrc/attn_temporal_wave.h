// One wave of temporal self-attention over 17 .. 64 frames with its operands in global memory: the steps a wave of
// attention_temporal_long.hip and of attention_temporal_rel.hip takes around the shared softmax / P.V core
// (attn_frames_long.h) that are stated once -- which problem the wave owns, V^T into LDS and how O leaves.  Frames are
// padded to TT = 32 | 64 slots.  A padded slot reads frame t - 1 (a valid address), is never used as data and never stored.
// Every row address is formed in 64 bits by the caller's frame pointer: at T = 64 the level-0 qkv of one guided clip is
// 0.63 GB, a batch of four crosses 2^31 bytes.
// The K fragment load and the Q + S^T block are NOT here: both kernels keep them written out.  With the Q + S^T block as
// a function hipcc scheduled attn_temporal_long_kernel<64> differently and it measured 2 - 3 % slower on the MI355X; the
// K load as a function moves that kernel's code too (7380 -> 7400 bytes) and has not been timed on its own.
// Change one file's copy, change the other's.
#pragma once
#include "gemm_common.h"
#include "attn_frames_long.h"

namespace {

constexpr int tl_vt_ld(int tt) { return tt * 2 + 8; }          // bytes per V^T row in LDS: 72 | 136 ([TT keys + 4 pad] bf16)

// Which (clip, pixel, head) a wave owns: `waves` waves per block, one problem each, over nb * hw * heads with the head
// fastest.  A tail wave (active false) computes the last problem again, a valid one, and stores nothing.  Frame f of the
// problem is row row0 + f * hw of qkv and of out; the products that follow are the caller's, in 64 bits.
struct TlWave {
  bool active;
  int hd;                                          // head
  int64_t row0;
};
__device__ __forceinline__ TlWave tl_wave_map(int waves, int wave, int nb, int t_len, int hw, int heads) {
  const int64_t seq = (int64_t)blockIdx.x * waves + wave;
  const int64_t total = (int64_t)nb * hw * heads;
  const bool active = seq < total;
  const int64_t sq = active ? seq : total - 1;
  const int hd = (int)(sq % heads);
  const int64_t bp = sq / heads;
  const int px = (int)(bp % hw);
  const int bb = (int)(bp / hw);
  return {active, hd, (int64_t)bb * t_len * hw + px};
}

// V^T of the wave's pixel / head into its LDS slice vts: [dim][key] with rows of tl_vt_ld(TT) bytes, keys >= t zero (their
// P is 0: 0 * garbage could still be NaN).  16-byte chunk idx -> key = idx % TT, 8-dim chunk idx / TT: lane-consecutive
// keys per dim row.  All loads are issued before the first LDS write.  frame_ptr(f): the q row of frame f, this head.
template <int TT, typename FP>
__device__ __forceinline__ void tl_stage_vt(const FP& frame_ptr, int C, int lane, int t_len, char* vts) {
  constexpr int VT_LD = tl_vt_ld(TT);
  uint16_t* vt = reinterpret_cast<uint16_t*>(vts);
  constexpr int PER_LANE = TT * 8 / 64;            // 4 | 8 chunks of 16 bytes
  u32x4 vreg[PER_LANE];
#pragma unroll
  for (int it = 0; it < PER_LANE; ++it) {
    const int idx = lane + it * 64;
    const int key = idx % TT, dch = idx / TT;
    const int kc = key < t_len ? key : t_len - 1;
    vreg[it] = *reinterpret_cast<const u32x4*>(frame_ptr(kc) + 2 * C + dch * 8);
  }
#pragma unroll
  for (int it = 0; it < PER_LANE; ++it) {
    const int idx = lane + it * 64;
    const int key = idx % TT, dch = idx / TT;
    const u32x4 v4 = key < t_len ? vreg[it] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      vt[(dch * 8 + 2 * e) * (VT_LD / 2) + key] = (uint16_t)(v4[e] & 0xffffu);
      vt[(dch * 8 + 2 * e + 1) * (VT_LD / 2) + key] = (uint16_t)(v4[e] >> 16);
    }
  }
}

// O of the lane's query to orow = its 64 columns of `out` when `store` (an active wave, a query < t): oacc[db][4 g + i] =
// O[q][db*32 + 8 g + 4 half + i].  For each group pair (g, g + 1) one permlane32_swap per dword leaves lanes 0-31 with dims
// 8 g .. 8 g + 7 and lanes 32-63 with 8 g + 8 .. 8 g + 15: 16-byte stores.  The swaps run on every lane; only the store is
// predicated.
__device__ __forceinline__ void tl_store(bf16_t* orow, int half, bool store, const f32x16 (&oacc)[2]) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      uint32_t a0 = pack2(oacc[db][4 * g + 0], oacc[db][4 * g + 1]);
      uint32_t a1 = pack2(oacc[db][4 * g + 2], oacc[db][4 * g + 3]);
      uint32_t b0 = pack2(oacc[db][4 * g + 4], oacc[db][4 * g + 5]);
      uint32_t b1 = pack2(oacc[db][4 * g + 6], oacc[db][4 * g + 7]);
      const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      a0 = r0[0]; b0 = r0[1];
      a1 = r1[0]; b1 = r1[1];
      if (store) *reinterpret_cast<u32x4*>(orow + db * 32 + 8 * g + 8 * half) = u32x4{a0, a1, b0, b1};
    }
}

}  // namespace
