// 8-bit spatial self-attention, head dim 64, gfx950 (BASELINE.json configs[4]: the fp8 attention path).
//
//   o = softmax(q k^T * scale) v      with  q k^T on int8 operands   and   P v on MXFP8 operands
//
// Formats (restated on the CPU in tests/q8_attn_ref.py; the quantisers are pinned to it bit for bit):
//   * K, Q: int8, one fp32 scale per (row, head):  amax = max |x| over the 64 dims,  inv = 127 / amax,
//     x_q = clamp(rint(x * inv), -127, 127),  s = amax / 127  (amax == 0: inv = 0, s = 1; both correctly rounded fp32).
//   * V^T: OCP e4m3 with one E8M0 scale per 32 consecutive keys of one (batch, head, d) column -- oracle.mx.quantize_mxfp8
//     of V^T, keys past lk zero.
//   * P: e4m3 in the kernel, per query over the same 32-key blocks, exponent from the scores before any exp2:
//         e_blk = max(floor(blockmax(s') - m) - 8, -127),   P_q = cvt_e4m3(min(exp2(s' - (m + e_blk)), 448)),
//     with s' = score * scale * log2(e) and m the running maximum after this tile (masked keys: s' = -inf, P = 0; an
//     all-masked block gets e = -127, a finite scale).
//   * The row sum l is the sum of the fp32 P BEFORE the e4m3 rounding, l = sum_blk 2^e_blk * sum exp2(s' - (m + e_blk)):
//     it costs one add per score like the bf16 kernel's (the sum of the dequantised P would add one fp8 -> fp32 convert
//     per score), and round-to-nearest-even leaves the P rounding errors zero-mean, so the two sums differ by O(ulp / sqrt n).
//
// tc_attn_q8_quant_kv: one launch over (key tile, head, batch) that quantises K and V into a workspace of 9 KiB records,
// one per (batch, head, 64-key tile), laid out in the lane order the attention kernel's MFMAs read (so every fragment
// read is one lane-linear ds_read_b128 and the record travels global -> LDS as nine plain 1-KiB DMA pieces):
//   [0, 4096)     K fragments f = 2 kbk + kk: lane L holds K_q[key 32 kbk + (L&31)][d 32 kk + 16 (L>>5) + j], j < 16
//   [4096, 8192)  V fragments f = 2 d0 + blk: lane L holds V_q[key 32 blk + (j&3) + 8 (j>>2) + 4 (L>>5)][d 32 d0 + (L&31)]
//   [8192, 8448)  fp32 K scales of the 64 keys
//   [8448, 8576)  E8M0 V scales, byte 2 d + blk
// Each K/V tile is read by lq / 128 query blocks: quantising once is cheaper than in every block.
//
// attn_d64_q8_kernel: the structure of attn_d64_dma_kernel<false> (attention.hip) -- 128 queries per block, 4 waves,
// double-buffered 64-key tiles staged by DMA, swapped S^T = K Q^T so each lane owns one query column, P kept in
// registers as the next MFMA's operand; the lane / register / key layout, the mask, the rescale and the output pass are
// those of csrc/attn_tile64.h:
//   * S^T on v_mfma_i32_32x32x32_i8: two instructions per 32x32 score tile (bf16 needs four).  A (K) and B (Q) carry the
//     same d in the same byte of the same lane half, so the product needs no other knowledge of the k order.  The int32
//     result has the shape-determined C layout of the header.
//     Score = float(acc) * s_k[key] * s_q: the key scale is per register (one multiply), the query scale is folded with
//     scale * log2(e) into the per-lane multiplier of the exp2 argument.
//   * O^T += V^T P^T on v_mfma_scale_f32_32x32x64_f8f6f4 with K = 64 keys = one tile.  Measured layout of that
//     instruction (gemm_mx.hip): bytes 0..15 of lane (l31, h) lie in K block 0, bytes 16..31 in K block 1, and the lane's
//     scale byte is block h's.  Score tile kbk = 0 (registers 0..15) fills bytes 0..15 and kbk = 1 bytes 16..31, so block
//     kbk is keys 32 kbk .. 32 kbk + 31 -- the V^T fragments are stored in that same key order.  The block max needs one
//     lane^32 exchange per block.
//   * P is packed by mx_pack4 (csrc/mx_quant.h: round to nearest even).
#include "attn_tile64.h"
#include "gemm_common.h"
#include "mx_quant.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int KT = 64;                 // keys per tile
constexpr int REC = 9216;              // bytes per (batch, head, tile) record: 9 DMA pieces of 1 KiB
constexpr int REC_V = 4096;            // V fragments
constexpr int REC_KS = 8192;           // fp32 K scales
constexpr int REC_VS = 8448;           // E8M0 V scales
constexpr int VT_PITCH = 72;           // bf16 per row of the pre-pass's staged V tile (64 + 8 pad)

// int8 quantisation of n values by a row amax (the formula of the header)
__device__ __forceinline__ float q8_inv(float amax) { return amax > 0.f ? 127.f / amax : 0.f; }
__device__ __forceinline__ float q8_scale(float amax) { return amax > 0.f ? amax / 127.f : 1.f; }
__device__ __forceinline__ uint32_t q8_pack4(const float* x, float inv) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float r = fminf(fmaxf(rintf(x[i] * inv), -127.f), 127.f);
    w |= ((uint32_t)(int)r & 0xffu) << (8 * i);
  }
  return w;
}

// ---- pre-pass: one block per (tile, head, batch)
__global__ __launch_bounds__(256) void attn_q8_quant_kv_kernel(const TcAttnQ8Params p, const int n_tiles) {
  __shared__ __attribute__((aligned(16))) uint16_t vt[KT * VT_PITCH];
  const int tid = threadIdx.x, t = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int key0 = t * KT;
  const bf16_t* kb = reinterpret_cast<const bf16_t*>(p.k) + (int64_t)b * p.k_sb + h * 64;
  const bf16_t* vb = reinterpret_cast<const bf16_t*>(p.v) + (int64_t)b * p.v_sb + h * 64;
  char* rec = reinterpret_cast<char*>(p.workspace) + (((int64_t)b * p.heads + h) * n_tiles + t) * REC;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // V tile -> LDS [key][d] (coalesced 16-byte loads; keys past lk are zero)
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + it * 256;
    const int key = idx >> 3, ch = idx & 7;
    const bool ok = key0 + key < p.lk;
    const u32x4 v = ok ? *reinterpret_cast<const u32x4*>(vb + (int64_t)(key0 + key) * p.v_ss + ch * 8) : zero4;
    *reinterpret_cast<u32x4*>(vt + key * VT_PITCH + ch * 8) = v;
  }

  // K: four threads per key, 16 dims each = one 16-byte fragment chunk
  {
    const int key = tid >> 2, c = tid & 3;
    const bool ok = key0 + key < p.lk;
    u32x4 raw[2] = {zero4, zero4};
    if (ok) {
      const u32x4* src = reinterpret_cast<const u32x4*>(kb + (int64_t)(key0 + key) * p.k_ss + c * 16);
      raw[0] = src[0];
      raw[1] = src[1];
    }
    float x[16];
    unpack8(raw[0], x);
    unpack8(raw[1], x + 8);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(x[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const float inv = q8_inv(amax);
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = q8_pack4(x + 4 * i, inv);
    const int kbk = key >> 5, kk = c >> 1, hh = c & 1;
    *reinterpret_cast<u32x4*>(rec + ((kbk * 2 + kk) * 64 + hh * 32 + (key & 31)) * 16) = out;
    if (c == 0) reinterpret_cast<float*>(rec + REC_KS)[key] = ok ? q8_scale(amax) : 0.f;
  }
  __syncthreads();

  // V^T: thread (d, blk, half) quantises the 16 keys 32 blk + (j&3) + 8 (j>>2) + 4 half of column d; the partner
  // half (lane ^ 1) holds the other 16 keys of the block
  {
    const int hh = tid & 1, d = (tid >> 1) & 63, blk = tid >> 7;
    uint32_t bits[16];
    uint32_t amax = 0;                                     // |x| as bf16 bits: integer order == magnitude order
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int key = 32 * blk + (j & 3) + 8 * (j >> 2) + 4 * hh;
      bits[j] = vt[key * VT_PITCH + d];
      amax = max(amax, bits[j] & 0x7fffu);
    }
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
    const int byte = mx_scale_byte(amax);
    const float inv = mx_inv_scale(byte);
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      out[i] = mx_quant4(bf16_bits_to_f32(bits[4 * i]), bf16_bits_to_f32(bits[4 * i + 1]), bf16_bits_to_f32(bits[4 * i + 2]),
                         bf16_bits_to_f32(bits[4 * i + 3]), inv);
    const int d0 = d >> 5;
    *reinterpret_cast<u32x4*>(rec + REC_V + ((d0 * 2 + blk) * 64 + hh * 32 + (d & 31)) * 16) = out;
    if (hh == 0) reinterpret_cast<uint8_t*>(rec + REC_VS)[d * 2 + blk] = (uint8_t)byte;
  }
  // bytes [8576, 9216) of the record are padding the DMA reads and nothing uses
}

// ---- attention over the quantised records
__global__ __launch_bounds__(256) void attn_d64_q8_kernel(const TcAttnQ8Params p, const int n_tiles) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * REC];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int l31 = lane & 31, half = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const bf16_t* qb = reinterpret_cast<const bf16_t*>(p.q) + (int64_t)b * p.q_sb + h * 64;
  bf16_t* ob = reinterpret_cast<bf16_t*>(p.o) + (int64_t)b * p.o_sb + h * 64;
  const char* recs = reinterpret_cast<const char*>(p.workspace) + ((int64_t)b * p.heads + h) * n_tiles * REC;

  // ---- Q: int8 B operand of S^T = K Q^T, lane (q, half) holds d 32 kk + 16 half + j; row scale over the lane pair
  const int q_row = blockIdx.x * 128 + wave * 32 + l31;
  const int q_ld = q_row < p.lq ? q_row : p.lq - 1;   // clamp: tail rows compute garbage, never stored
  float qx[2][16];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const u32x4* src = reinterpret_cast<const u32x4*>(qb + (int64_t)q_ld * p.q_ss + kk * 32 + half * 16);
    unpack8(src[0], qx[kk]);
    unpack8(src[1], qx[kk] + 8);
  }
  float qmax = 0.f;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int i = 0; i < 16; ++i) qmax = fmaxf(qmax, fabsf(qx[kk][i]));
  qmax = fmaxf(qmax, __shfl_xor(qmax, 32, 64));
  i32x4 qf[2];
  {
    const float inv = q8_inv(qmax);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) qf[kk][i] = (int)q8_pack4(qx[kk] + 4 * i, inv);
  }
  const float cq = p.scale * 1.4426950408889634f * q8_scale(qmax);   // softmax in base 2, query scale folded in

  float m_run = -1e30f, l_run = 0.f;
  f32x16 oacc[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;

  // a record is nine 1-KiB pieces: wave w issues pieces w and w + 4, wave 0 also piece 8
  const tc_rsrc_t rsrc = make_rsrc(recs, (int64_t)n_tiles * REC);
  auto dma_tile = [&](int kt, int stage) {
    char* dst = smem + stage * REC + wave_u * 1024;
    const uint32_t soff = (uint32_t)kt * (uint32_t)REC;
    glds16(rsrc, dst, (uint32_t)(wave_u * 1024 + lane * 16), soff);
    glds16(rsrc, dst + 4096, (uint32_t)((wave_u + 4) * 1024 + lane * 16), soff);
    if (wave_u == 0) glds16(rsrc, dst + 8192, (uint32_t)(8 * 1024 + lane * 16), soff);
  };

  const i32x16 izero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  dma_tile(0, 0);
  for (int kt = 0; kt < n_tiles; ++kt) {
    const int key0 = kt * KT;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < n_tiles) dma_tile(kt + 1, (kt + 1) & 1);
    const char* rec = smem + (kt & 1) * REC;

    // ---- S^T = K Q^T, int32
    i32x16 sacc[2];
#pragma unroll
    for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const i32x4 kf = *reinterpret_cast<const i32x4*>(rec + ((kbk * 2 + kk) * 64 + lane) * 16);
        sacc[kbk] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf, qf[kk], kk == 0 ? izero : sacc[kbk], 0, 0, 0);
      }
    // scores with the key scales of the registers' keys
    const float* ks = reinterpret_cast<const float*>(rec + REC_KS);
    float s[2][16];
#pragma unroll
    for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 sk = *reinterpret_cast<const f32x4*>(ks + 32 * kbk + 8 * g + 4 * half);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[kbk][4 * g + i] = (float)sacc[kbk][4 * g + i] * sk[i];
      }
    tc_tile64_mask(s, key0, p.lk, half, -INFINITY);
    float bmx[2];
#pragma unroll
    for (int kbk = 0; kbk < 2; ++kbk) {
      float mx = s[kbk][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[kbk][r]);
      bmx[kbk] = fmaxf(mx, __shfl_xor(mx, 32, 64));
    }
    tc_tile64_raise_max(fmaxf(m_run, fmaxf(bmx[0], bmx[1]) * cq), m_run, l_run, oacc);   // cq > 0: max commutes with the scale
    // P in e4m3 with one E8M0 exponent per query and 32-key block; l from the fp32 values
    i32x8 pf;
    float rs = 0.f;
    int ebyte[2];
#pragma unroll
    for (int kbk = 0; kbk < 2; ++kbk) {
      const float bm = bmx[kbk] * cq;                    // its own statement: no fma contraction against m_run, so the
      const float e = fmaxf(floorf(bm - m_run) - 8.f, -127.f);   // block holding the row max gets exactly floor(0) - 8
      ebyte[kbk] = (int)e + 127;
      const float mb = m_run + e;
      float pv[16], rsb = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pv[r] = fast_exp2(fmaf(s[kbk][r], cq, -mb));      // masked keys: exp2(-inf) = 0
        rsb += pv[r];
        pv[r] = fminf(pv[r], 448.f);
      }
      rs += ldexpf(rsb, (int)e);
#pragma unroll
      for (int w = 0; w < 4; ++w) pf[4 * kbk + w] = (int)mx_pack4(pv[4 * w], pv[4 * w + 1], pv[4 * w + 2], pv[4 * w + 3]);
    }
    rs += __shfl_xor(rs, 32, 64);
    l_run += rs;
    const int psc = half ? ebyte[1] : ebyte[0];          // this lane's scale byte: block `half` of its query

    // ---- O^T += V^T P^T, 64 keys in one instruction per 32 dims
    const uint8_t* vs = reinterpret_cast<const uint8_t*>(rec + REC_VS);
#pragma unroll
    for (int d0 = 0; d0 < 2; ++d0) {
      const i32x4 lo = *reinterpret_cast<const i32x4*>(rec + REC_V + ((d0 * 2 + 0) * 64 + lane) * 16);
      const i32x4 hi = *reinterpret_cast<const i32x4*>(rec + REC_V + ((d0 * 2 + 1) * 64 + lane) * 16);
      const i32x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      const int vsc = vs[(d0 * 32 + l31) * 2 + half];
      oacc[d0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, oacc[d0], 0, 0, 0, vsc, 0, psc);
    }
  }

  if (q_row < p.lq) tc_tile64_store(oacc, l_run, ob + (int64_t)q_row * p.o_ss, half, false);
}

int q8_check(const TcAttnQ8Params* pp, bool need_q) {
  if (!pp) return TC_EINVAL;
  const TcAttnQ8Params& p = *pp;
  if (p.batch <= 0 || p.heads <= 0 || p.lq <= 0 || p.lk <= 0 || !p.workspace) return TC_EINVAL;
  if (!(p.scale > 0.f) || !(p.scale < INFINITY)) return TC_EINVAL;
  if (need_q) {
    if (!p.q || !p.o) return TC_EINVAL;
    if (!tc_tile64_aligned(p.q, p.q_ss, p.q_sb) || !tc_tile64_aligned(p.o, p.o_ss, p.o_sb)) return TC_EALIGN;
  } else {
    if (!p.k || !p.v) return TC_EINVAL;
    if (!tc_tile64_aligned(p.k, p.k_ss, p.k_sb) || !tc_tile64_aligned(p.v, p.v_ss, p.v_sb)) return TC_EALIGN;
  }
  if (!tc_aligned16(p.workspace)) return TC_EALIGN;
  if (p.heads > 65535 || p.batch > 65535) return TC_ESHAPE;
  const int64_t n_tiles = (p.lk + KT - 1) / KT;
  if (n_tiles * REC >= 0x7ffffff0LL) return TC_ESHAPE;        // one (batch, head)'s records under one buffer descriptor
  if (p.workspace_bytes < tc_attn_q8_workspace(pp)) return TC_EWORKSPACE;
  return TC_OK;
}

}  // namespace

extern "C" int64_t tc_attn_q8_workspace(const TcAttnQ8Params* p) {
  if (!p || p->batch <= 0 || p->heads <= 0 || p->lk <= 0) return 0;
  return (int64_t)p->batch * p->heads * ((p->lk + KT - 1) / KT) * REC;
}

extern "C" int tc_attn_q8_quant_kv(const TcAttnQ8Params* p, void* stream) {
  const int rc = q8_check(p, false);
  if (rc != TC_OK) return rc;
  const int n_tiles = (p->lk + KT - 1) / KT;
  hipLaunchKernelGGL(attn_q8_quant_kv_kernel, dim3(n_tiles, p->heads, p->batch), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), *p, n_tiles);
  TC_LAUNCH_CHECK();
  return TC_OK;
}

extern "C" int tc_attn_d64_q8(const TcAttnQ8Params* p, void* stream) {
  const int rc = q8_check(p, true);
  if (rc != TC_OK) return rc;
  const int n_tiles = (p->lk + KT - 1) / KT;
  hipLaunchKernelGGL(attn_d64_q8_kernel, dim3((p->lq + 127) / 128, p->heads, p->batch), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), *p, n_tiles);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
