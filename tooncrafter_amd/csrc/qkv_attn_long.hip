// Temporal self-attention behind its qkv projection as ONE launch for clips of 17 .. 64 frames, gfx950 (the long-clip
// route of tc_temporal_qkv_attn; the 16-frame kernel is csrc/qkv_attn.hip, whose header states the fusion):
//
//     out[:, h*64 .. h*64+64] = Attn_frames( x . Wqkv[q_h | k_h | v_h]^T + bqkv )          x: [B*t*HW, C] bf16, 17 <= t <= 64
//
// (reference lvdm/modules/attention.py:81-144 CrossAttention over the t frames of a pixel, called from TemporalTransformer,
// attention.py:365-412, at a --video_length above 16.)  The two launches this replaces are tc_gemm_bf16, which writes the
// [B*t*HW, 3C] qkv tensor, and tc_attn_temporal (csrc/attention_temporal_long.hip), which reads it straight back.
//
// The projection is qkv_attn_kernel's (qkv_attn_tile.h qa_project: the 128 x 192 [q_h | k_h | v_h] tile over K = C, which
// leaves q and k row-major swizzled and v transposed in the dead stage memory).  Two things differ:
//
//  * ROW MAP.  The frame count is padded to TT = 32 | 64 slots (template parameter; t <= 32 takes 32).  A block owns
//    PX = 128 / TT consecutive pixels x TT slots: tile row lr = pixel * TT + slot -> memory row row0 + slot * hw + pixel.
//    PADDED SLOTS (slot >= t) READ ZEROS, they are not clamped to frame t - 1: the loader gives such a row the offset
//    TC_OOB, which no descriptor covers, so nothing is fetched for it -- not the next clip's rows, not what follows the
//    tensor.  That is the mechanism.  The A descriptor is a second guard only: it ends ((t-1) * hw + PX-1) * ldx + c
//    elements past the tile's first row, the last element a real slot of this tile can name.  (hw % PX == 0, which the
//    host requires, is the pixel map's condition -- every pixel p0 + px of a tile exists -- not the descriptor's.)
//    A padded slot's q / k / v are then the bias: finite.  Padded keys are set to -inf in front of the max; padded query
//    rows are computed and never stored.
//  * ATTENTION on v_mfma_f32_32x32x16_bf16, as attention_temporal_long.hip does it, with its operands from LDS:
//    S^T = K Q^T (4 k-steps over d = 64; a lane owns ONE query, its keys lie along the 16 accumulator registers and the two
//    lane halves), then the masked softmax and O^T = V^T P^T of attn_frames_long.h tc_attn_frames_long, which states the
//    permuted key order V^T is read in.  TT = 32: wave w takes pixel w.  TT = 64: wave w takes pixel w >> 1, queries
//    32 (w & 1) ..., both key blocks.  Either way the wave's queries are tile rows 32 w .. 32 w + 31: O lands there as
//    bf16 (no other wave reads those q rows), and after one s_waitcnt lgkmcnt(0) the wave stores them itself, 128
//    contiguous bytes per row, rows with slot < t only.  No block barrier after the attention.
//
// Roundings: those of the two launches at these lengths -- bf16 q / k / v, bf16 softmax weights, fp32 sums, bf16 output.
// Row addresses are formed in 64 bits; per-lane offsets are relative to the tile's first row and 31-bit (host-checked).
#include "qkv_attn_tile.h"
#include "attn_frames_long.h"

namespace {

struct QalArgs : QaArgs { int t; };

template <int TT>
__global__ __launch_bounds__(QA_THREADS, 2) void qkv_attn_long_kernel(const QalArgs p) {
  static_assert(TT == 32 || TT == 64, "frames padded to 32 or 64 slots");
  constexpr int PX = QA_BM / TT;                   // pixels per tile: 4 | 2
  constexpr int NKB = TT / 32;                     // 32-key blocks of a pixel
  __shared__ __attribute__((aligned(1024))) char smem[QA_LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fhalf = lane >> 5;

  // block -> (row tile, head): XCD x (= blockIdx & 7) walks the row tiles x, x + 8, ..., all heads of a tile back to back
  const int xcd = blockIdx.x & 7, bslot = blockIdx.x >> 3;
  const int tile = (bslot / p.heads) * 8 + xcd;
  const int h = bslot - (bslot / p.heads) * p.heads;
  if (tile >= p.tiles) return;
  const int bb = tile / p.tiles_per_b;
  const int p0 = (tile - bb * p.tiles_per_b) * PX;
  // tile row lr = pixel * TT + slot -> memory row row0 + slot * hw + pixel (slot < t)
  const int64_t row0 = (int64_t)bb * p.t * p.hw + p0;

  // ---- projection (qkv_attn_tile.h): q | k | v^T of the tile's 128 rows in the stage memory.  The descriptor of A ends
  // with the last column of frame t - 1 of the tile's last pixel; padded slots are out of range.
  const tc_rsrc_t a_rsrc = make_rsrc(p.x + row0 * p.ldx, (((int64_t)(p.t - 1) * p.hw + PX - 1) * p.ldx + p.c) * 2);
  qa_project(smem, a_rsrc, p.w, p.bias, p.c, h, [&](int lr, int chunk) {
    const int fs = lr & (TT - 1), px = lr / TT;
    return fs < p.t ? (uint32_t)((((int64_t)fs * p.hw + px) * p.ldx) * 2 + chunk * 16) : TC_OOB;
  });

  // ---- attention: the wave's 32 queries are tile rows qbase .. qbase + 31 of the pixel whose TT slots start at pbase
  const int qbase = wave_u * 32;
  const int pbase = qbase & ~(TT - 1);
  const int qslot0 = qbase - pbase;                // 0, or 32 for the odd waves at TT = 64 (t > 32: never all padding)
  {
    // S^T[key][query]: A = K (lane: key kb*32 + frow, dims 16 kk + 8 fhalf ..), B = Q (lane: query frow, same dims)
    f32x16 st[NKB];
    {
      bf16x8 qf[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        qf[kk] = *reinterpret_cast<const bf16x8*>(smem + QA_Q_OFF + lds_off(qbase + frow, 2 * kk + fhalf));
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[kb][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(smem + QA_K_OFF + lds_off(pbase + kb * 32 + frow, 2 * kk + fhalf));
          st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], st[kb], 0, 0, 0);
        }
      }
    }
    // masked softmax, P^T in bf16, O^T = V^T P^T with V^T from the pixel's keys in LDS (attn_frames_long.h)
    f32x16 oacc[2];
    tc_attn_frames_long<NKB>(st, oacc, p.t, p.scale_log2e, smem + QA_VT_OFF + pbase * 2, QA_VT_LD, frow, fhalf);

    // O as bf16 over the query's own q row: oacc[db][4 g + i] = O[query][db*32 + 8 g + 4 fhalf + i] -> the fhalf half of
    // 16-byte chunk db*4 + g
    const int row = qbase + frow;
    char* orow = smem + QA_Q_OFF + row * 128 + 8 * fhalf;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint32_t lo = pack2(oacc[db][4 * g], oacc[db][4 * g + 1]);
        const uint32_t hi = pack2(oacc[db][4 * g + 2], oacc[db][4 * g + 3]);
        *reinterpret_cast<uint2*>(orow + (((db * 4 + g) ^ ((row >> 1) & 7)) << 4)) = uint2{lo, hi};
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's 32 output rows are in LDS (written by this wave only)

  // ---- store: the wave's 32 rows x 64 columns, 8 lanes per row (128 contiguous bytes), 8 rows per pass; real frames only
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int lr = qbase + ps * 8 + (lane >> 3);
    const int ch = lane & 7;
    const int fs = qslot0 + ps * 8 + (lane >> 3);
    const u32x4 v = *reinterpret_cast<const u32x4*>(smem + QA_Q_OFF + lr * 128 + ((ch ^ ((lr >> 1) & 7)) << 4));
    const int64_t m = row0 + (int64_t)fs * p.hw + (pbase / TT);
    if (fs < p.t) *reinterpret_cast<u32x4*>(p.out + m * p.ldo + h * 64 + ch * 8) = v;
  }
}

// What TC_QKV_ATTN = 1 (the default) admits of this kernel: the (TT, C) cells, with a lower bound on t, in which the per-call
// table of scripts/long_clip_bench.py --qkv-attn had the slower of two one-launch timings ahead of the faster of two
// tc_gemm_bf16 + tc_attn_temporal timings by more than the spread of the repeats (profiles/r09_qkv_attn_long_bench.txt,
// DESIGN 5.11; measured at t = 24, 32, 48, 64, B = 2, the four level geometries):
//   C = 320, 640:  ahead at all four lengths (+9.6 ... +51.5 %)    -> t >= 24 (TT = 32), t >= 48 (TT = 64)
//   C = 1280:      ahead at t = 32, 64 (+15 ... +23 %), behind or level at t = 24, 48 (-4.9 ... +0.5 %: the padding to
//                  TT slots costs the projection 33 % more rows there)   -> t = 32 and t = 64 only
// Below the lowest measured t of a cell the padding only grows, and between a losing and a winning t nothing was timed:
// neither is admitted, nor is a width that was not measured.  The lengths BETWEEN TWO WINNING t of a cell (t = 25 ... 31
// and 49 ... 63 at C = 320 / 640) are admitted and were NOT timed: the one launch costs what its TT slots cost whatever t is
// (the table: t = 24 as t = 32, t = 48 as t = 64), the two launches cost more the larger t is, so a length between two
// winning ones is ahead by at least the lower one's margin -- an argument from monotonicity, not a measurement.
// TC_QKV_ATTN=2 takes them all.
bool qal_default_admits(int t, int c) {
  const int tt = t <= 32 ? 32 : 64;
  if (c == 320 || c == 640) return t >= tt - tt / 4;
  if (c == 1280) return t == tt;
  return false;
}

}  // namespace

// 17 <= t <= TC_TEMPORAL_MAX_FRAMES; mode = TC_QKV_ATTN (1: the measured rule above, 2: every shape the kernel can take).
// The caller (csrc/qkv_attn.hip) has checked p and mode != 0.
int qkv_attn_long_eligible(const TcTqaParams* p, int mode) {
  if (p->t <= QA_T || p->t > TC_TEMPORAL_MAX_FRAMES) return 0;
  if (!qa_shape_ok(p, p->t, QA_BM / (p->t <= 32 ? 32 : 64))) return 0;
  if (mode < 2 && !qal_default_admits(p->t, p->c)) return 0;
  return 1;
}

// the caller has checked the pointers, their alignment and qkv_attn_long_eligible
int qkv_attn_long_launch(const TcTqaParams* p, hipStream_t stream) {
  const int tt = p->t <= 32 ? 32 : 64;
  QalArgs a;
  const unsigned grid = qa_fill(a, p, QA_BM / tt);
  a.t = p->t;
  if (tt == 32) hipLaunchKernelGGL(qkv_attn_long_kernel<32>, dim3(grid), dim3(QA_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(qkv_attn_long_kernel<64>, dim3(grid), dim3(QA_THREADS), 0, stream, a);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
