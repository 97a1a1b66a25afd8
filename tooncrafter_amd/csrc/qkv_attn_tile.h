// The 128 x 192 [q_h | k_h | v_h] tile of the one-launch qkv projection + temporal attention (qkv_attn.hip: 16 frames,
// qkv_attn_long.hip: 17 .. 64 frames): its geometry, the places of q / k / v^T in the dead stage memory, the kernel
// arguments, the projection itself (qa_project: the two kernels differ in the row map they hand it) and the host's
// shape rule and argument fill.
#pragma once
#include "fused_l0.h"      // L0Scatter: the swizzled [128][64] layout of q / k is the level-0 fused kernels'
#include "mfma_shape.h"    // TC_QKV_MFMA

// the long-clip route of tc_temporal_qkv_attn (csrc/qkv_attn_long.hip): 17 .. TC_TEMPORAL_MAX_FRAMES frames, its own pixel
// count per tile, and what TC_QKV_ATTN = 1 admits of it
int qkv_attn_long_eligible(const TcTqaParams* p, int mode);
int qkv_attn_long_launch(const TcTqaParams* p, hipStream_t stream);

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

// The shape rule of either kernel: `frames` frames of `px` pixels to a tile (16 and 8 | t and 128 / TT).  The caller has
// checked the frame count itself.
inline bool qa_shape_ok(const TcTqaParams* p, int frames, int px) {
  if (p->b <= 0 || p->hw <= 0 || p->hw % px) return false;
  if (p->heads <= 0 || p->c != p->heads * 64) return false;
  if (p->ldx < p->c || p->ldo < p->c || (p->ldx & 7) || (p->ldo & 7)) return false;
  // per-lane offsets are relative to the tile's first row and span all frames: 31-bit
  if (((int64_t)frames * p->hw + px) * p->ldx * 2 >= 0x7fffff00LL) return false;
  if ((int64_t)3 * p->c * p->c * 2 >= 0x7fffff00LL) return false;
  const int64_t blocks = (int64_t)p->heads * 8 * (((int64_t)p->b * (p->hw / px) + 7) / 8);
  return blocks <= 0x7fffffffLL;
}

// kernel arguments of a launch with `px` pixels per tile; the grid is heads * 8 * ceil(tiles / 8) blocks
inline unsigned qa_fill(QaArgs& a, const TcTqaParams* p, int px) {
  a.x = reinterpret_cast<const bf16_t*>(p->x); a.w = reinterpret_cast<const bf16_t*>(p->wqkv); a.bias = p->bqkv;
  a.out = reinterpret_cast<bf16_t*>(p->out);
  a.hw = p->hw; a.c = p->c; a.heads = p->heads; a.ldx = p->ldx; a.ldo = p->ldo;
  a.scale_log2e = p->scale * 1.44269504088896340736f;
  a.tiles_per_b = p->hw / px;
  a.tiles = p->b * a.tiles_per_b;
  return (unsigned)(p->heads * 8 * ((a.tiles + 7) / 8));
}

// The projection of one block: smem <- q (QA_Q_OFF) | k (QA_K_OFF) | v^T (QA_VT_OFF) of head h for the tile's 128 rows,
// + bias, in bf16 (the roundings of the projection's own output), visible to the whole block on return.  On the 4-wave
// skeleton of csrc/gemm.hip: tiles global -> LDS by buffer_load ... lds, two K-steps in flight, waves 2 x 2, each
// 64 x 96 = 4 x 6 v_mfma_f32_16x16x32_bf16 sub-tiles (the shape that ships at 16 frames; 2 x 3 v_mfma_f32_32x32x16_bf16 behind
// TC_QKV_MFMA=32 and in qkv_attn_long.hip).  `a_rsrc` covers the tile's rows of x from its first row on;
// `a_off(tile row, 16-byte chunk)` is a row's 32-bit byte offset in it, or TC_OOB for a row that reads zeros.
// MF = 16 (what qkv_attn.hip asks for unless TC_QKV_MFMA=32, mfma_shape.h; qkv_attn_long.hip stays on 32, unmeasured there): the wave tile as 4 x 6 v_mfma_f32_16x16x32_bf16 tiles over two 32-deep
// K-slices per K-step -- the same 20 ds_read_b128 per K-step on the same image (row lane & 15, chunk 4 ks + (lane >> 4)),
// and the scatter of q / k / v^T restated for the 16 x 16 D (column lane & 15, rows 4 (lane >> 4) + r).  Measured against
// MF = 32 with bit-identical outputs: the launch 2.3-2.6 % shorter at levels 1 / 2 on a 5-7 % higher engine clock (2.6 %
// longer at level 3: 0.7 us), the guided forward +1.1-1.2 % (profiles/mfma_shape_kernel_ab.txt, mfma_shape_forward_ab.txt).
template <int MF = 32, class RowMap>
__device__ __forceinline__ void qa_project(char* smem, const tc_rsrc_t a_rsrc, const bf16_t* w, const float* bias, int c, int h,
                                           RowMap a_off) {
  // the lane's coordinates are formed HERE from threadIdx, not passed in: handed over as plain ints they lose their
  // ranges, and the LDS addresses of the K loop stop folding into instruction offsets (+190 instructions per kernel)
  const int tid = threadIdx.x;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_u >> 1, wn = wave_u & 1;
  const int frow = tid & 31, fhalf = (tid & 63) >> 5;
  const int frow16 = tid & 15, fq = (tid & 63) >> 4;

  // ---- loader geometry: thread -> (row lrow + 32 i, 16-byte chunk) of both tiles; the swizzle is on the SOURCE chunk
  const int lrow = tid >> 3;
  const int chunk = (tid & 7) ^ ((lrow >> 1) & 7);
  const tc_rsrc_t w_rsrc = make_rsrc(w, (int64_t)3 * c * c * 2);
  uint32_t a_voff[QA_RA], b_voff[QA_RB];
#pragma unroll
  for (int i = 0; i < QA_RA; ++i) a_voff[i] = a_off(lrow + 32 * i, chunk);
#pragma unroll
  for (int i = 0; i < QA_RB; ++i) {
    // stage rows 0..63 <- to_q rows of head h, 64..127 <- to_k, 128..191 <- to_v (Wqkv = [q | k | v] blocks of C rows)
    const int r = lrow + 32 * i;
    b_voff[i] = (uint32_t)(((int64_t)((i >> 1) * c + h * 64 + (r & 63)) * c) * 2 + chunk * 16);
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

  // bias of this lane's column in each of the wave's three 32-column blocks (the projections of the reference have none:
  // bias == nullptr; a LayerNorm folded into Wqkv brings one)
  float bcol[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int jb = wn * 3 + j;                       // 32-column block of the 192: 0, 1 = q | 2, 3 = k | 4, 5 = v
    bcol[j] = bias ? bias[(jb >> 1) * c + h * 64 + (jb & 1) * 32 + frow] : 0.f;
  }

  float bcol16[6];                                 // MF == 16: the same for the wave's six 16-column blocks wn * 6 + j of the twelve
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int jb = wn * 6 + j;                     // 0..3 = q | 4..7 = k | 8..11 = v
    bcol16[j] = (MF == 16 && bias) ? bias[(jb >> 2) * c + h * 64 + (jb & 3) * 16 + frow16] : 0.f;
  }

  f32x16 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  f32x4 acc16[4][6];                               // MF == 16 (the other shape's set is never touched and costs nothing)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int stage) {
    const char* sa = smem + stage * QA_STAGE;
    const char* sb = sa + QA_A_BYTES;
    if constexpr (MF == 16) {
      bf16x8 a16[2][4], b16[2][6];                  // both 32-deep slices are read before the first MFMA
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int ck = ks * 4 + fq;
#pragma unroll
        for (int i = 0; i < 4; ++i) a16[ks][i] = *reinterpret_cast<const bf16x8*>(sa + lds_off(wm * 64 + i * 16 + frow16, ck));
#pragma unroll
        for (int j = 0; j < 6; ++j) b16[ks][j] = *reinterpret_cast<const bf16x8*>(sb + lds_off(wn * 96 + j * 16 + frow16, ck));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j)
            acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a16[ks][i], b16[ks][j], acc16[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      return;
    }
    bf16x8 af[2][2], bf[2][3];
    auto frags = [&](int kk, bf16x8 (&a)[2], bf16x8 (&b)[3]) {
      const int ck = kk * 2 + fhalf;
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const bf16x8*>(sa + lds_off(wm * 64 + i * 32 + frow, ck));
#pragma unroll
      for (int j = 0; j < 3; ++j) b[j] = *reinterpret_cast<const bf16x8*>(sb + lds_off(wn * 96 + j * 32 + frow, ck));
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
  tc_kloop_pipe<QA_RA + QA_RB>(0, c / TC_BK, load_tile, compute);

  if constexpr (MF == 16) {
    // ---- write-out from the 16 x 16 D layout: the lane holds column frow16 of its 16-column block, rows 4 fq + (0..3).
    // The wave's six blocks are blocks wn * 6 + j of the twelve: 0..3 = q | 4..7 = k | 8..11 = v.  q / k: the place of
    // (row, col) in the swizzled row-major [128][64] buffer (fused_l0.h, L0Scatter's formula);  v^T: the lane's four rows
    // are consecutive -> one 8-byte store
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int jb = wn * 6 + j;                    // wave-uniform
      const int col = (jb & 3) * 16 + frow16;
      const float b = bcol16[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row0 = wm * 64 + i * 16 + 4 * fq;
        if (jb < 8) {
          char* buf = smem + (jb < 4 ? QA_Q_OFF : QA_K_OFF);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = row0 + r;
            *reinterpret_cast<bf16_t*>(buf + row * 128 + (((col >> 3) ^ ((row >> 1) & 7)) << 4) + (col & 7) * 2) = (bf16_t)(acc16[i][j][r] + b);
          }
        } else {
          const uint32_t lo = pack2(acc16[i][j][0] + b, acc16[i][j][1] + b);
          const uint32_t hi = pack2(acc16[i][j][2] + b, acc16[i][j][3] + b);
          *reinterpret_cast<uint2*>(smem + QA_VT_OFF + col * QA_VT_LD + row0 * 2) = uint2{lo, hi};
        }
      }
    }
    __syncthreads();
    return;
  }

  // ---- write-out of the projection: + bias, bf16.  q / k: row-major [128][64], chunks swizzled by (row >> 1) & 7 -- the
  // scatter of a 32 x 32 accumulator block stated in fused_l0.h (L0Scatter);  v: transposed [64 dims][128 rows], four
  // consecutive rows of a lane (accumulator registers 4 g .. 4 g + 3 = rows 8 g + 4 fhalf + (0..3)) as one 8-byte store.
  auto write_rm = [&](char* buf, const f32x16& a, int i, int colblk, float b) {
    const L0Scatter sc(buf + (wm * 64 + i * 32) * 128, colblk * 32 + frow, fhalf);
#pragma unroll
    for (int r = 0; r < 16; ++r) *sc.at(r) = (bf16_t)(a[r] + b);
  };
  auto write_vt = [&](const f32x16& a, int i, int colblk, float b) {
    char* v0 = smem + QA_VT_OFF + (colblk * 32 + frow) * QA_VT_LD + (wm * 64 + i * 32 + 4 * fhalf) * 2;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                  // rows 8 g + 4 fhalf + (0..3) of the block
      const uint32_t lo = pack2(a[4 * g] + b, a[4 * g + 1] + b);
      const uint32_t hi = pack2(a[4 * g + 2] + b, a[4 * g + 3] + b);
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
}

}  // namespace
