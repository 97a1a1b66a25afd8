// Temporal self-attention behind its qkv projection as ONE launch for clips of 17 .. 64 frames, gfx950 (the long-clip
// route of tc_temporal_qkv_attn; the 16-frame kernel is csrc/qkv_attn.hip, whose header states the fusion):
//
//     out[:, h*64 .. h*64+64] = Attn_frames( x . Wqkv[q_h | k_h | v_h]^T + bqkv )          x: [B*t*HW, C] bf16, 17 <= t <= 64
//
// (reference lvdm/modules/attention.py:81-144 CrossAttention over the t frames of a pixel, called from TemporalTransformer,
// attention.py:365-412, at a --video_length above 16.)  The two launches this replaces are tc_gemm_bf16, which writes the
// [B*t*HW, 3C] qkv tensor, and tc_attn_temporal (csrc/attention_temporal_long.hip), which reads it straight back.
//
// The projection is qkv_attn_kernel's, restated here because that kernel is frozen: a 128 x 192 [q_h | k_h | v_h] tile over
// K = C on the 4-wave skeleton (glds16 with the swizzle on the source side, tc_kloop_pipe with two K-steps in flight, waves
// 2 x 2 with 2 x 3 v_mfma_f32_32x32x16_bf16 sub-tiles, 2 stages x 40 KiB of LDS, two blocks per CU), and an epilogue that
// leaves q and k row-major swizzled and v transposed in the dead stage memory at qkv_attn_tile.h's offsets.  A change to
// that projection is made in both files until the two share one template.  Two things differ:
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
//    lane halves; max and sum in-lane plus one __shfl_xor of the halves); P^T rounded to bf16 is the B operand of
//    O^T = V^T P^T, V^T read in the accumulator's permuted key order (k-slot (half, j) of step s = key 16 s + 8 (j >> 2)
//    + 4 half + (j & 3)).  TT = 32: wave w takes pixel w.  TT = 64: wave w takes pixel w >> 1, queries 32 (w & 1) ...,
//    both key blocks.  Either way the wave's queries are tile rows 32 w .. 32 w + 31: O lands there as bf16 (no other
//    wave reads those q rows), and after one s_waitcnt lgkmcnt(0) the wave stores them itself, 128 contiguous bytes per
//    row, rows with slot < t only.  No block barrier after the attention.
//
// Roundings: those of the two launches at these lengths -- bf16 q / k / v, bf16 softmax weights, fp32 sums, bf16 output.
// Row addresses are formed in 64 bits; per-lane offsets are relative to the tile's first row and 31-bit (host-checked).
#include "qkv_attn_tile.h"

namespace {

struct QalArgs : QaArgs { int t; };

__device__ __forceinline__ float qal_half_max(float x) { return fmaxf(x, __shfl_xor(x, 32, 64)); }
__device__ __forceinline__ float qal_half_sum(float x) { return x + __shfl_xor(x, 32, 64); }

template <int TT>
__global__ __launch_bounds__(QA_THREADS, 2) void qkv_attn_long_kernel(const QalArgs p) {
  static_assert(TT == 32 || TT == 64, "frames padded to 32 or 64 slots");
  constexpr int PX = QA_BM / TT;                   // pixels per tile: 4 | 2
  constexpr int NKB = TT / 32;                     // 32-key blocks of a pixel
  __shared__ __attribute__((aligned(1024))) char smem[QA_LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_u >> 1, wn = wave_u & 1;
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

  // ---- loader geometry: thread -> (row lrow + 32 i, 16-byte chunk) of both tiles; the swizzle is on the SOURCE chunk.
  // The descriptor of A ends with the last column of frame t - 1 of the tile's last pixel; padded slots are out of range.
  const int lrow = tid >> 3;
  const int chunk = (tid & 7) ^ ((lrow >> 1) & 7);
  const tc_rsrc_t a_rsrc = make_rsrc(p.x + row0 * p.ldx, (((int64_t)(p.t - 1) * p.hw + PX - 1) * p.ldx + p.c) * 2);
  const tc_rsrc_t w_rsrc = make_rsrc(p.w, (int64_t)3 * p.c * p.c * 2);
  uint32_t a_voff[QA_RA], b_voff[QA_RB];
#pragma unroll
  for (int i = 0; i < QA_RA; ++i) {
    const int lr = lrow + 32 * i;
    const int fs = lr & (TT - 1), px = lr / TT;
    a_voff[i] = fs < p.t ? (uint32_t)((((int64_t)fs * p.hw + px) * p.ldx) * 2 + chunk * 16) : TC_OOB;
  }
#pragma unroll
  for (int i = 0; i < QA_RB; ++i) {
    // stage rows 0..63 <- to_q rows of head h, 64..127 <- to_k, 128..191 <- to_v (Wqkv = [q | k | v] blocks of C rows)
    const int r = lrow + 32 * i;
    b_voff[i] = (uint32_t)(((int64_t)((i >> 1) * p.c + h * 64 + (r & 63)) * p.c) * 2 + chunk * 16);
  }
  auto load_tile = [&](int kb, int stage) {
    const uint32_t soff = (uint32_t)kb * (TC_BK * 2);
    char* sa = smem + stage * QA_STAGE + wave_u * 1024;
    char* sb = sa + QA_A_BYTES;
#pragma unroll
    for (int i = 0; i < QA_RB; ++i) glds16(w_rsrc, sb + i * 4096, b_voff[i], soff);
#pragma unroll
    for (int i = 0; i < QA_RA; ++i) glds16(a_rsrc, sa + i * 4096, a_voff[i], soff);
  };

  // bias of this lane's column in each of the wave's three 32-column blocks (nullptr: the reference's projections have none)
  float bcol[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int jb = wn * 3 + j;                       // 32-column block of the 192: 0, 1 = q | 2, 3 = k | 4, 5 = v
    bcol[j] = p.bias ? p.bias[(jb >> 1) * p.c + h * 64 + (jb & 1) * 32 + frow] : 0.f;
  }

  f32x16 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto compute = [&](int stage) {
    const char* sa = smem + stage * QA_STAGE;
    const char* sb = sa + QA_A_BYTES;
    bf16x8 af[2][2], bf[2][3];
    auto frags = [&](int kk, bf16x8 (&a)[2], bf16x8 (&b)[3]) {
      const int c = kk * 2 + fhalf;
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const bf16x8*>(sa + lds_off(wm * 64 + i * 32 + frow, c));
#pragma unroll
      for (int j = 0; j < 3; ++j) b[j] = *reinterpret_cast<const bf16x8*>(sb + lds_off(wn * 96 + j * 32 + frow, c));
    };
    auto mfmas = [&](bf16x8 (&a)[2], bf16x8 (&b)[3]) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    };
    frags(0, af[0], bf[0]);
    frags(1, af[1], bf[1]);
    __builtin_amdgcn_sched_barrier(0);
    mfmas(af[0], bf[0]);
    __builtin_amdgcn_sched_barrier(0);
    frags(2, af[0], bf[0]);
    __builtin_amdgcn_sched_barrier(0);
    mfmas(af[1], bf[1]);
    __builtin_amdgcn_sched_barrier(0);
    frags(3, af[1], bf[1]);
    __builtin_amdgcn_sched_barrier(0);
    mfmas(af[0], bf[0]);
    mfmas(af[1], bf[1]);
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- K loop: two K-steps in flight (gemm_common.h tc_kloop_pipe); its last barrier frees the stage memory for the epilogue
  tc_kloop_pipe<QA_RA + QA_RB>(0, p.c / TC_BK, load_tile, compute);

  // ---- write-out of the projection: + bias, bf16.  Accumulator register r of a lane = row cr = (r & 3) + 8 (r >> 2)
  // + 4 fhalf of the 32-row block, column frow.  q / k: row-major [128][64], chunks swizzled by (row >> 1) & 7;
  // v: transposed [64 dims][128 rows], four consecutive rows of a lane as one 8-byte store.
  auto write_rm = [&](char* buf, const f32x16& a, int i, int colblk, float bias) {
    const int col = colblk * 32 + frow;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
      *reinterpret_cast<bf16_t*>(buf + row * 128 + (((col >> 3) ^ ((row >> 1) & 7)) << 4) + (col & 7) * 2) = (bf16_t)(a[r] + bias);
    }
  };
  auto write_vt = [&](const f32x16& a, int i, int colblk, float bias) {
    char* v0 = smem + QA_VT_OFF + (colblk * 32 + frow) * QA_VT_LD + (wm * 64 + i * 32 + 4 * fhalf) * 2;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                  // rows 8 g + 4 fhalf + (0..3) of the block
      const uint32_t lo = pack2(a[4 * g] + bias, a[4 * g + 1] + bias);
      const uint32_t hi = pack2(a[4 * g + 2] + bias, a[4 * g + 3] + bias);
      *reinterpret_cast<uint2*>(v0 + g * 16) = uint2{lo, hi};
    }
  };
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (wn == 0) {                                  // column blocks 0, 1 = q | 2 = k columns 0..31
      write_rm(smem + QA_Q_OFF, acc[i][0], i, 0, bcol[0]);
      write_rm(smem + QA_Q_OFF, acc[i][1], i, 1, bcol[1]);
      write_rm(smem + QA_K_OFF, acc[i][2], i, 0, bcol[2]);
    } else {                                        // 3 = k columns 32..63 | 4, 5 = v
      write_rm(smem + QA_K_OFF, acc[i][0], i, 1, bcol[0]);
      write_vt(acc[i][1], i, 0, bcol[1]);
      write_vt(acc[i][2], i, 1, bcol[2]);
    }
  }
  __syncthreads();

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
    // lane = query; register r of key block kb = key kb*32 + (r & 3) + 8 (r >> 2) + 4 fhalf; padded keys -> -inf
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fhalf;
        st[kb][r] = key < p.t ? st[kb][r] : -INFINITY;
        mx = fmaxf(mx, st[kb][r]);
      }
    mx = qal_half_max(mx);                         // key 0 is always valid: mx is finite
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f((st[kb][r] - mx) * p.scale_log2e);   // masked: exp2(-inf) = 0
        st[kb][r] = e;
        sum += e;
      }
    sum = qal_half_sum(sum);
    const float inv = __builtin_amdgcn_rcpf(sum);

    // O^T[dim][query] = sum_key V^T[dim][key] P^T[key][query]: P^T in bf16 as the B operand (k-step s of key block kb =
    // registers 8 s .. 8 s + 7), V^T (lane: dim db*32 + frow) read in the same permuted key order
    f32x16 oacc[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (bf16_t)(st[kb][8 * s + j] * inv);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const char* vrow = smem + QA_VT_OFF + (db * 32 + frow) * QA_VT_LD + (pbase + kb * 32 + 16 * s + 4 * fhalf) * 2;
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow);        // keys +0..3
          const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + 16);   // keys +8..11
          const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
          oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), pf, oacc[db], 0, 0, 0);
        }
      }

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
  if (p->t <= QA_T || p->t > TC_TEMPORAL_MAX_FRAMES || p->b <= 0 || p->hw <= 0) return 0;
  const int px = QA_BM / (p->t <= 32 ? 32 : 64);
  if (p->hw % px) return 0;
  if (p->heads <= 0 || p->c != p->heads * 64) return 0;
  if (p->ldx < p->c || p->ldo < p->c || (p->ldx & 7) || (p->ldo & 7)) return 0;
  // per-lane offsets are relative to the tile's first row and span t frames: 31-bit
  if (((int64_t)p->t * p->hw + px) * p->ldx * 2 >= 0x7fffff00LL) return 0;
  if ((int64_t)3 * p->c * p->c * 2 >= 0x7fffff00LL) return 0;
  const int64_t blocks = (int64_t)p->heads * 8 * (((int64_t)p->b * (p->hw / px) + 7) / 8);
  if (blocks > 0x7fffffffLL) return 0;
  if (mode < 2 && !qal_default_admits(p->t, p->c)) return 0;
  return 1;
}

// the caller has checked the pointers, their alignment and qkv_attn_long_eligible
int qkv_attn_long_launch(const TcTqaParams* p, hipStream_t stream) {
  const int tt = p->t <= 32 ? 32 : 64;
  QalArgs a;
  a.x = reinterpret_cast<const bf16_t*>(p->x); a.w = reinterpret_cast<const bf16_t*>(p->wqkv); a.bias = p->bqkv;
  a.out = reinterpret_cast<bf16_t*>(p->out);
  a.hw = p->hw; a.c = p->c; a.heads = p->heads; a.ldx = p->ldx; a.ldo = p->ldo;
  a.scale_log2e = p->scale * 1.44269504088896340736f;
  a.tiles_per_b = p->hw / (QA_BM / tt);
  a.tiles = p->b * a.tiles_per_b;
  a.t = p->t;
  const unsigned grid = (unsigned)(p->heads * 8 * ((a.tiles + 7) / 8));
  if (tt == 32) hipLaunchKernelGGL(qkv_attn_long_kernel<32>, dim3(grid), dim3(QA_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(qkv_attn_long_kernel<64>, dim3(grid), dim3(QA_THREADS), 0, stream, a);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
