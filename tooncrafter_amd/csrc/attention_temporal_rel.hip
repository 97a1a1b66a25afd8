// Temporal self-attention with relative position and / or a causal mask over 1 .. 64 frames, gfx950 (tc_attn_temporal_rel):
//
//     idx(i, j) = clamp(j - i, -L, L) + L                                   L = max_rel (the module's temporal_length)
//     s[i, j]   = scale * ( q_i . k_j  +  q_i . Rk[idx(i, j)] ),            -inf for j > i when causal
//     o_i       = sum_j softmax_j(s[i, :])[j] * ( v_j + Rv[idx(i, j)] )     over the t frames of one pixel and head
//
// (reference lvdm/modules/attention.py:20-39 RelativePosition, 103-124 the two extra einsums and the mask of
// CrossAttention.forward, 343-345 and 376-390 the tril mask of TemporalTransformer: use_relative_position /
// use_causal_attention of the UNet.)  Rk and Rv are [2 L + 1, 64] bf16 tables shared by every head.
//
// The kernel is attention_temporal_long.hip with three additions.  The wave map, V^T into LDS and the store
// (attn_temporal_wave.h) and the softmax and P.V (attn_frames_long.h tc_attn_frames_long) are the same functions in both, the
// K load and the Q + score block the same text (that header says why), so with no tables and no mask it computes that kernel's bits:
//
//  * both relative terms depend on j - i only, and of the 2 L + 1 distances a clip of t frames uses the
//    NC = 2 Lc + 1 with Lc = min(L, t - 1): the kernel works on that compact range c = clamp(j - i, -Lc, Lc) + Lc, at most
//    127 values = NRB = TT / 16 blocks of 32.  No [t, t, 64] tensor exists anywhere;
//  * QR^T[c][i] = Rk[c] . q_i on the score MFMA (A = table rows straight from global memory, like the K fragments; B = the
//    Q fragments already in registers), fp32.  A score lane owns one query with its keys along the registers, so the
//    shift c -> j = c + i - Lc differs per lane: the lane that holds QR[i][c] writes it to slot j of row i of the wave's
//    fp32 bounce buffer in LDS (the two clamped ends c = 0 and c = 2 Lc go to two extra slots), and the lane that holds
//    s[i][j] adds what it finds there -- before the scale, before the mask;
//  * the causal mask is -inf on keys j > i, set on the raw scores in front of the shared core, which masks the padded
//    keys the same way (key 0 is never masked: no row is empty);
//  * after the softmax the bf16 weights go the other way through the same buffer: PB[i][c] = sum of p[i][j] over the j
//    of distance c (one j per c inside the range, the clamped ends are fp32 sums rounded to bf16), read back as the B
//    operand of O^T += Rv^T PB^T into the fp32 accumulator, Rv^T (compact, zero beyond NC) held in LDS once per block.
//
// One wave per (clip, pixel, head), frames padded to TT = 32 | 64.  LDS per block: V^T slices as in the long kernel, plus,
// with tables, Rv^T [64][NRB * 32 + 4] bf16 and one bounce buffer [32][TT + 3] fp32 per wave -- 44 KiB at TT = 32 (4 waves),
// 50 KiB at TT = 64 (2 waves per block: four would not fit the 64 KiB of a static allocation).  Nothing here was tuned.
// Roundings: bf16 q / k / v / tables, fp32 scores and QR, bf16 softmax weights and bucket sums, fp32 sums, bf16 output.
// A padded frame slot is never read as data and never stored; every row address is formed in 64 bits (attn_temporal_wave.h).
#include "attn_temporal_wave.h"

namespace {

template <int TT, int WAVES, bool REL>
__global__ __launch_bounds__(WAVES * 64) void attn_temporal_rel_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                      const bf16_t* __restrict__ rel_k,
                                                                      const bf16_t* __restrict__ rel_v, int nb, int t_len, int hw,
                                                                      int heads, int max_rel, int causal, float scale_log2e) {
  static_assert(TT == 32 || TT == 64, "frames padded to 32 or 64");
  constexpr int NKB = TT / 32;                     // 32-key blocks (and 32-query blocks)
  constexpr int NRB = 2 * NKB;                     // 32-distance blocks: 2 Lc + 1 <= 2 TT - 1
  constexpr int VT_LD = tl_vt_ld(TT);
  constexpr int RV_LD = NRB * 64 + 8;              // bytes per Rv^T row and per PB row: 136 | 264
  constexpr int BQ_LD = TT + 3;                    // floats per QR row: TT key slots + the two clamped ends, odd stride
  constexpr int BOUNCE = 32 * BQ_LD * 4;           // bytes per wave: 4480 | 8576 (the PB rows, 32 * RV_LD, fit inside)
  static_assert(32 * RV_LD <= BOUNCE && BOUNCE % 16 == 0, "PB rows alias the QR rows");
  constexpr int VT_BYTES = WAVES * 64 * VT_LD;
  constexpr int RV_BYTES = REL ? 64 * RV_LD : 0;
  __shared__ __attribute__((aligned(16))) char smem[VT_BYTES + RV_BYTES + (REL ? WAVES * BOUNCE : 0)];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const TlWave w = tl_wave_map(WAVES, wave, nb, t_len, hw, heads);
  const bool active = w.active;
  const int hd = w.hd;
  const int C = heads * 64;
  const int64_t ld = 3 * (int64_t)C;
  const int64_t row0 = w.row0;                                // frame f -> row row0 + f * hw
  const bf16_t* base = qkv + hd * 64;
  auto frame_ptr = [&](int f) { return base + (row0 + (int64_t)f * hw) * ld; };
  const int lc = max_rel < t_len - 1 ? max_rel : t_len - 1;   // distances in use: -lc .. lc -> c = 0 .. 2 lc

  char* vts = smem + wave * 64 * VT_LD;
  tl_stage_vt<TT>(frame_ptr, C, lane, t_len, vts);
  // ---- Rv^T over the compact distance range, once per block: [dim][c] = Rv[c - lc + max_rel][dim], c > 2 lc zero (their
  // bucket sums are zero as well: 0 * garbage could still be NaN)
  char* rvt = smem + VT_BYTES;
  char* bounce = smem + VT_BYTES + RV_BYTES + wave * BOUNCE;
  if constexpr (REL) {
    uint16_t* rt = reinterpret_cast<uint16_t*>(rvt);
    constexpr int NCP = NRB * 32;
    for (int idx = threadIdx.x; idx < NCP * 8; idx += WAVES * 64) {
      const int c = idx % NCP, dch = idx / NCP;
      const bool valid = c <= 2 * lc;
      const u32x4 ld4 = *reinterpret_cast<const u32x4*>(rel_v + (int64_t)((valid ? c : 0) - lc + max_rel) * 64 + dch * 8);
      const u32x4 v4 = valid ? ld4 : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        rt[(dch * 8 + 2 * e) * (RV_LD / 2) + c] = (uint16_t)(v4[e] & 0xffffu);
        rt[(dch * 8 + 2 * e + 1) * (RV_LD / 2) + c] = (uint16_t)(v4[e] >> 16);
      }
    }
  }

  // ---- K fragments (A operand of S^T = K Q^T), as attention_temporal_long.hip
  bf16x8 kf[NKB][4];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int key = kb * 32 + l31;
    const bf16_t* kp = frame_ptr(key < t_len ? key : t_len - 1) + C + half * 8;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) kf[kb][kk] = *reinterpret_cast<const bf16x8*>(kp + kk * 16);
  }
  __syncthreads();                                 // V^T and Rv^T complete

#pragma unroll
  for (int qb = 0; qb < NKB; ++qb) {
    if (qb * 32 >= t_len) break;                   // block-uniform: no valid query in this block
    const int q = qb * 32 + l31;
    const int qc = q < t_len ? q : t_len - 1;      // a padded query lane repeats the last frame and stores nothing
    const bf16_t* qp = frame_ptr(qc) + half * 8;
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

    if constexpr (REL) {
      // ---- QR^T[c][query] = Rk_c Q^T, same layout: lane = query, registers = c of block rb.  Shift through LDS: row =
      // query, slot j = c + q - lc for the inner distances, slots TT / TT + 1 for the clamped ends c = 0 / c = 2 lc
      float* bq = reinterpret_cast<float*>(bounce) + l31 * BQ_LD;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        if (rb * 32 > 2 * lc) break;               // block-uniform: no distance of this block is in use
        const int crow = rb * 32 + l31;
        const bf16_t* rp = rel_k + (int64_t)((crow < 2 * lc ? crow : 2 * lc) - lc + max_rel) * 64 + half * 8;
        f32x16 qr;
#pragma unroll
        for (int r = 0; r < 16; ++r) qr[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          qr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(rp + kk * 16), qf[kk], qr, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = rb * 32 + tc_frames_key(r, half);
          const int j = c + qc - lc;
          if (c == 0) bq[TT] = qr[r];
          if (c == 2 * lc && lc > 0) bq[TT + 1] = qr[r];
          if (c > 0 && c < 2 * lc && j >= 0 && j < t_len) bq[j] = qr[r];
        }
      }
      __syncthreads();                             // a row is written by both lane halves
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb * 32 + tc_frames_key(r, half);
          const int d = key - qc;                  // keys >= t read a slot nobody wrote: the mask below replaces the sum
          st[kb][r] += bq[d <= -lc ? TT : d >= lc ? TT + 1 : key];
        }
    }
    if (causal) {
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb * 32 + tc_frames_key(r, half);
          st[kb][r] = key > qc ? -INFINITY : st[kb][r];
        }
    }
    // masked softmax, P^T in bf16, O^T = V^T P^T (attn_frames_long.h); st comes back as exp2(..), not yet normalised
    f32x16 oacc[2];
    const float inv = tc_attn_frames_long<NKB>(st, oacc, t_len, scale_log2e, vts, VT_LD, l31, half);

    if constexpr (REL) {
      // ---- PB[query][c] through the wave's buffer
      char* pbrow = bounce + l31 * RV_LD;
      uint16_t* pb = reinterpret_cast<uint16_t*>(pbrow);
      __syncthreads();                             // the QR rows have been read
#pragma unroll
      for (int i = 0; i < NRB * 4; ++i) *reinterpret_cast<u32x2*>(pbrow + half * (NRB * 32) + i * 8) = u32x2{0u, 0u};
      __syncthreads();
      float lo = 0.f, hi = 0.f;                    // the clamped ends: several keys share c = 0 and c = 2 lc
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb * 32 + tc_frames_key(r, half);
          const int d = key - qc;
          const bf16_t pw = (bf16_t)(st[kb][r] * inv);             // the weight the core multiplied V by; 0 on masked keys
          if (d <= -lc) lo += (float)pw;
          else if (d >= lc) hi += (float)pw;
          else pb[d + lc] = __builtin_bit_cast(uint16_t, pw);      // one key per inner distance
        }
      lo = tc_half_sum(lo);
      hi = tc_half_sum(hi);
      if (half == 0) pb[0] = __builtin_bit_cast(uint16_t, (bf16_t)lo);
      else if (lc > 0) pb[2 * lc] = __builtin_bit_cast(uint16_t, (bf16_t)hi);
      __syncthreads();
      // O^T[dim][query] += sum_c Rv^T[dim][c] PB^T[c][query]: the operand order of the core's P.V, c in place of the key
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        if (rb * 32 > 2 * lc) break;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int cb = (rb * 32 + 16 * s + 4 * half) * 2;
          const u32x2 plo = *reinterpret_cast<const u32x2*>(pbrow + cb);
          const u32x2 phi = *reinterpret_cast<const u32x2*>(pbrow + cb + 16);
          const u32x4 pp = {plo[0], plo[1], phi[0], phi[1]};
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const char* vrow = rvt + (db * 32 + l31) * RV_LD + cb;
            const u32x2 vlo = *reinterpret_cast<const u32x2*>(vrow);
            const u32x2 vhi = *reinterpret_cast<const u32x2*>(vrow + 16);
            const u32x4 vv = {vlo[0], vlo[1], vhi[0], vhi[1]};
            oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), __builtin_bit_cast(bf16x8, pp),
                                                               oacc[db], 0, 0, 0);
          }
        }
      }
      __syncthreads();                             // the PB rows have been read: the next query block writes QR over them
    }

    bf16_t* orow = out + (row0 + (int64_t)qc * hw) * C + hd * 64;
    tl_store(orow, half, active && q < t_len, oacc);   // padded query rows (>= t) are never stored
  }
}

template <int TT, int WAVES, bool REL>
void launch(const TcAttnTemporalRelParams* p, int64_t total, hipStream_t stream) {
  const int64_t nblk = (total + WAVES - 1) / WAVES;
  hipLaunchKernelGGL((attn_temporal_rel_kernel<TT, WAVES, REL>), dim3((unsigned)nblk), dim3(WAVES * 64), 0, stream,
                     reinterpret_cast<const bf16_t*>(p->qkv), reinterpret_cast<bf16_t*>(p->out),
                     reinterpret_cast<const bf16_t*>(p->rel_k), reinterpret_cast<const bf16_t*>(p->rel_v), p->b, p->t, p->hw,
                     p->heads, p->max_rel, p->causal != 0, p->scale * 1.44269504088896340736f);
}

}  // namespace

extern "C" int tc_attn_temporal_rel(const TcAttnTemporalRelParams* p, void* stream) {
  if (!p || !p->qkv || !p->out || p->b <= 0 || p->t <= 0 || p->hw <= 0 || p->heads <= 0 || !(p->scale > 0.f)) return TC_EINVAL;
  if ((p->rel_k == nullptr) != (p->rel_v == nullptr)) return TC_EINVAL;
  const bool rel = p->rel_k != nullptr;
  if (p->t > TC_TEMPORAL_MAX_FRAMES) return TC_ESHAPE;
  if (rel && (p->max_rel < 1 || p->max_rel > TC_TEMPORAL_MAX_FRAMES)) return TC_ESHAPE;
  if (!tc_aligned16(p->qkv) || !tc_aligned16(p->out) || !tc_aligned16(p->rel_k) || !tc_aligned16(p->rel_v)) return TC_EALIGN;
  const int64_t total = (int64_t)p->b * p->hw * p->heads;
  if ((total + 1) / 2 > 0x7fffffffLL) return TC_ESHAPE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (p->t <= 32) {
    if (rel) launch<32, 4, true>(p, total, s);
    else launch<32, 4, false>(p, total, s);
  } else {
    if (rel) launch<64, 2, true>(p, total, s);
    else launch<64, 4, false>(p, total, s);
  }
  TC_LAUNCH_CHECK();
  return TC_OK;
}
