// Temporal self-attention over 17 .. 64 frames, gfx950 (the long-clip route of tc_attn_temporal):
//
//     out[(bb*t + f)*hw + p, h*64 .. h*64+64] = softmax_f'( q[f] . k[f'] * scale ) v[f']        over the t frames of pixel p
//
// (reference lvdm/modules/attention.py:81-144 CrossAttention called from TemporalTransformer, attention.py:365-412, at a
// --video_length above 16.)  attn_temporal_kernel (csrc/attention.hip) keeps a pixel's K and V in a fixed [16][64] LDS slot
// and one query per 4 lanes on the VALU; at 64 frames its work is 16x that and its layout does not grow.  Here:
//
//  * one wave per (clip, pixel, head), four to a block; the frame count is padded to TT = 32 | 64 (template parameter);
//  * S^T = K Q^T on v_mfma_f32_32x32x16_bf16 straight from global memory (a lane's K and Q fragments are 16 contiguous
//    bytes of one qkv row): 4 k-steps over d = 64, TT / 32 key blocks per 32-query block.  A lane then owns ONE query and
//    its keys lie along its 16 accumulator registers and the two lane halves -- keys >= t are set to -inf, the softmax
//    max / sum are in-lane plus one exchange between the lane halves;
//  * P^T is rounded to bf16 in registers and fed straight in as the B operand of O^T = V^T P^T, the V^T fragments read
//    from LDS in the accumulator's permuted key order (attn_frames_long.h tc_attn_frames_long, shared with
//    qkv_attn_long.hip, states the permutation);
//  * O^T has dims on registers and the query on the lane: 16-byte row stores; padded query rows (>= t) are never stored.
//
// The wave map, V^T into LDS and the store are attn_temporal_wave.h, shared with attention_temporal_rel.hip, which states
// their layouts, the padded-slot rule and why row addresses are 64-bit; the K load and the Q + score block are the same
// text in both files (that header says why).  LDS: V^T of the wave's pixel / head only, [64 dims][TT keys + 4 pad]
// bf16 (4.5 | 8.5 KiB per wave).  Roundings as csrc/qkv_attn.hip: bf16 q / k / v, bf16 softmax weights, fp32 sums, bf16
// output (attn_temporal_kernel keeps its softmax weights in fp32).
#include "attn_temporal_wave.h"

namespace {

template <int TT>
__global__ __launch_bounds__(256) void attn_temporal_long_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                int nb, int t_len, int hw, int heads, float scale_log2e) {
  static_assert(TT == 32 || TT == 64, "frames padded to 32 or 64");
  constexpr int NKB = TT / 32;                     // 32-key blocks (and 32-query blocks)
  constexpr int VT_LD = tl_vt_ld(TT);
  __shared__ __attribute__((aligned(16))) char smem[4 * 64 * VT_LD];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const TlWave w = tl_wave_map(4, wave, nb, t_len, hw, heads);
  const bool active = w.active;
  const int hd = w.hd;
  const int C = heads * 64;
  const int64_t ld = 3 * (int64_t)C;
  const int64_t row0 = w.row0;                                // frame f -> row row0 + f * hw
  const bf16_t* base = qkv + hd * 64;
  auto frame_ptr = [&](int f) { return base + (row0 + (int64_t)f * hw) * ld; };

  char* vts = smem + wave * 64 * VT_LD;
  tl_stage_vt<TT>(frame_ptr, C, lane, t_len, vts);

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
    bf16_t* orow = out + (row0 + (int64_t)q * hw) * C + hd * 64;
    tl_store(orow, half, active && q < t_len, oacc);   // padded query rows (>= t) are never stored
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
