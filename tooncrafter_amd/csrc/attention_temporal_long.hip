// Temporal self-attention over 17 .. 64 frames, gfx950 (the long-clip route of tc_attn_temporal):
//
//     out[(bb*t + f)*hw + p, h*64 .. h*64+64] = softmax_f'( q[f] . k[f'] * scale ) v[f']        over the t frames of pixel p
//
// (reference lvdm/modules/attention.py:81-144 CrossAttention called from TemporalTransformer, attention.py:365-412, at a
// --video_length above 16.)  attn_temporal_kernel (csrc/attention.hip) keeps a pixel's K and V in a fixed [16][64] LDS slot
// and one query per 4 lanes on the VALU; at 64 frames its work is 16x that and its layout does not grow.  Here:
//
//  * one wave per (clip, pixel, head); the frame count is padded to TT = 32 | 64 (template parameter);
//  * S^T = K Q^T on v_mfma_f32_32x32x16_bf16 straight from global memory (a lane's K and Q fragments are 16 contiguous
//    bytes of one qkv row): 4 k-steps over d = 64, TT / 32 key blocks per 32-query block.  A lane then owns ONE query and
//    its keys lie along its 16 accumulator registers and the two lane halves -- keys >= t are set to -inf, the softmax
//    max / sum are in-lane plus one exchange between the lane halves;
//  * P^T is rounded to bf16 in registers and fed straight in as the B operand of O^T = V^T P^T, the V^T fragments read
//    from LDS in the accumulator's permuted key order (attn_frames_long.h tc_attn_frames_long, shared with
//    qkv_attn_long.hip, states the permutation);
//  * O^T has dims on registers and the query on the lane: one permlane32_swap per dword pair turns two 8-byte halves
//    into one 16-byte row store; padded query rows (>= t) are never stored.
//
// LDS: V^T of the wave's pixel / head only, [64 dims][TT keys + 4 pad] bf16 (4.5 | 8.5 KiB per wave).  Roundings as
// csrc/qkv_attn.hip: bf16 q / k / v, bf16 softmax weights, fp32 sums, bf16 output (attn_temporal_kernel keeps its
// softmax weights in fp32).  Every row address is formed in 64 bits: at T = 64 the level-0 qkv of one guided clip is
// 0.63 GB, a batch of four crosses 2^31 bytes.
#include "gemm_common.h"
#include "attn_frames_long.h"

namespace {

template <int TT>
__global__ __launch_bounds__(256) void attn_temporal_long_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                int nb, int t_len, int hw, int heads, float scale_log2e) {
  static_assert(TT == 32 || TT == 64, "frames padded to 32 or 64");
  constexpr int NKB = TT / 32;                     // 32-key blocks (and 32-query blocks)
  constexpr int VT_LD = TT * 2 + 8;                // bytes per V^T row: 72 | 136
  __shared__ __attribute__((aligned(16))) char smem[4 * 64 * VT_LD];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int64_t seq = (int64_t)blockIdx.x * 4 + wave;         // over nb * hw * heads, head fastest
  const int64_t total = (int64_t)nb * hw * heads;
  const bool active = seq < total;
  const int64_t sq = active ? seq : total - 1;                // tail waves compute a valid problem and store nothing
  const int hd = (int)(sq % heads);
  const int64_t bp = sq / heads;
  const int px = (int)(bp % hw);
  const int bb = (int)(bp / hw);
  const int C = heads * 64;
  const int64_t ld = 3 * (int64_t)C;
  const int64_t row0 = (int64_t)bb * t_len * hw + px;         // frame f -> row row0 + f * hw
  const bf16_t* base = qkv + hd * 64;
  auto frame_ptr = [&](int f) { return base + (row0 + (int64_t)f * hw) * ld; };

  // ---- V^T of this pixel / head into the wave's LDS slice: [dim][key], keys >= t zero (their P is 0: 0 * garbage
  // could still be NaN).  Chunk idx -> key = idx % TT, 8-dim chunk idx / TT; lane-consecutive keys per dim row.
  char* vts = smem + wave * 64 * VT_LD;
  {
    uint16_t* vt = reinterpret_cast<uint16_t*>(vts);
    constexpr int PER_LANE = TT * 8 / 64;          // 4 | 8 chunks of 16 bytes
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

  // ---- K fragments (A operand of S^T = K Q^T): lane holds K[key kb*32 + l31][16 kk + 8 half + j]; padded keys read
  // the last frame's row (a valid address) and are masked below
  bf16x8 kf[NKB][4];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int key = kb * 32 + l31;
    const bf16_t* kp = frame_ptr(key < t_len ? key : t_len - 1) + C + half * 8;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) kf[kb][kk] = *reinterpret_cast<const bf16x8*>(kp + kk * 16);
  }
  __syncthreads();                                 // V^T complete (each wave reads only its own slice)

#pragma unroll
  for (int qb = 0; qb < NKB; ++qb) {
    if (qb * 32 >= t_len) break;                   // wave-uniform: no valid query in this block
    const int q = qb * 32 + l31;
    const bf16_t* qp = frame_ptr(q < t_len ? q : t_len - 1) + half * 8;
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qp + kk * 16);

    // S^T[key][query]: lane = query q, registers = keys (the layout of attn_tile64.h)
    f32x16 st[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[kb][r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][kk], qf[kk], st[kb], 0, 0, 0);
    }
    // masked softmax, P^T in bf16, O^T = V^T P^T (attn_frames_long.h)
    f32x16 oacc[2];
    tc_attn_frames_long<NKB>(st, oacc, t_len, scale_log2e, vts, VT_LD, l31, half);

    // ---- store: oacc[db][4 g + i] = O[q][db*32 + 8 g + 4 half + i].  For each group pair (g, g + 1) one permlane32_swap
    // per dword leaves lanes 0-31 with dims 8 g .. 8 g + 7 and lanes 32-63 with 8 g + 8 .. 8 g + 15: 16-byte stores.
    // The swaps run on every lane; only the store is predicated.
    bf16_t* orow = out + (row0 + (int64_t)q * hw) * C + hd * 64;
    const bool store = active && q < t_len;
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
}

}  // namespace

// t in 17 .. TC_TEMPORAL_MAX_FRAMES; the caller (tc_attn_temporal, csrc/attention.hip) has checked the pointers and t
int attn_temporal_long_launch(const bf16_t* qkv, bf16_t* out, int32_t b, int32_t t, int32_t hw, int32_t heads, float scale,
                          hipStream_t stream) {
  const int64_t total = (int64_t)b * hw * heads;
  const int64_t nblk = (total + 3) / 4;
  if (nblk > 0x7fffffffLL) return TC_ESHAPE;
  const float c = scale * 1.44269504088896340736f;
  if (t <= 32)
    hipLaunchKernelGGL(attn_temporal_long_kernel<32>, dim3((unsigned)nblk), dim3(256), 0, stream, qkv, out, b, t, hw, heads, c);
  else
    hipLaunchKernelGGL(attn_temporal_long_kernel<64>, dim3((unsigned)nblk), dim3(256), 0, stream, qkv, out, b, t, hw, heads, c);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
