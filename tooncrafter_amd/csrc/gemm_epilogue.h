// The epilogue arithmetic of the GEMM kernels, stated once: bias / row bias / activation / GEGLU / residual on 16-byte row
// vectors.  Two groups: first the pieces the per-wave epilogues share (the GEGLU pair, the row-vector finisher, the
// accumulator -> slab passes: gemm_wide.hip, gemm16.hip, conv_halo.hip, gemm8.hip, ff_fused.hip, tb_fused.hip), then the
// epilogues over the whole fp32 tile staged in LDS of the 4-wave kernels (gemm.hip, gemm_mx.hip), which use the pair too.
#pragma once
#include "gemm_common.h"

// ---- GEGLU on a pair of columns: x <- v . gelu(g), v = x alpha + bv, g = gt alpha + bg, times out_scale; pairs because
// the arithmetic is packed fp32 (common.h gelu_erf_f2).  PLAIN: alpha = out_scale = 1, the multiplies are not emitted.
// The TC_ABLATE & 8 hook (scripts/ablate_gemm.sh: no erf) sits here and so in every caller's PLAIN path; only gemm.hip is
// ever compiled with TC_ABLATE, the other callers (gemm_wide.hip, gemm8.hip, gemm_mx.hip) never see the macro.
template <bool PLAIN>
__device__ __forceinline__ void epi_geglu_pair(const TcGemmParams& p, float* x, const float* gt, const float* bv, const float* bg) {
#if defined(TC_ABLATE) && (TC_ABLATE & 8)      // scripts/ablate_gemm.sh: the GEGLU epilogue without its erf
  if (PLAIN) { x[0] = (x[0] + bv[0]) * (gt[0] + bg[0]); x[1] = (x[1] + bv[1]) * (gt[1] + bg[1]); }
#else
  if (PLAIN) {
    const tc_f32x2 v = {x[0] + bv[0], x[1] + bv[1]};
    const tc_f32x2 h = v * gelu_erf_f2(tc_f32x2{gt[0] + bg[0], gt[1] + bg[1]});
    x[0] = h[0]; x[1] = h[1];
  }
#endif
  else {
    const tc_f32x2 v = {x[0] * p.alpha + bv[0], x[1] * p.alpha + bv[1]};
    const tc_f32x2 h = v * gelu_erf_f2(tc_f32x2{gt[0] * p.alpha + bg[0], gt[1] * p.alpha + bg[1]}) * p.out_scale;
    x[0] = h[0]; x[1] = h[1];
  }
}

// ---- Row-vector finisher: 8 consecutive columns n0.. of output row m, raw accumulators in x:
//     out = act(alpha x + (bias + row_bias[m / row_div])) out_scale + residual,   stored as bf16 or fp32.
// Every operand is fetched here; c_base / res_base are the batch item's.  stored(packed) is called with the bf16 vector
// that went to memory (the GroupNorm statistics of gemm16.hip sum the ROUNDED values); nothing is called for fp32 output.
// ORDER OF ADDITIONS.  There are two in this library and both are part of their kernels' bits:
//   x alpha + (bias + row_bias)   -- this finisher: gemm_wide.hip (non-GEGLU), gemm16.hip, conv_halo.hip;
//   (x alpha + bias) + row_bias   -- the staged-tile path below (epilogue_fast / epilogue_tail: gemm.hip, gemm_mx.hip),
//                                    splitk_reduce_kernel (gemm.hip) and gemm8.hip, which keep their own prefetch structure.
template <class Stored>
__device__ __forceinline__ void epi_finish_row8(const TcGemmParams& p, char* c_base, const bf16_t* res_base, int m, int n0,
                                                float (&x)[8], Stored&& stored) {
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (p.bias) {
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + n0);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + n0 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { bv[e] = b0[e]; bv[4 + e] = b1[e]; }
  }
  if (p.row_bias) {
    const float* rp = p.row_bias + (int64_t)(m / p.row_div) * p.ldrb + n0;
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(rp);
    const f32x4 r1 = *reinterpret_cast<const f32x4*>(rp + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { bv[e] += r0[e]; bv[4 + e] += r1[e]; }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = apply_act(x[e] * p.alpha + bv[e], p.act) * p.out_scale;
  if (res_base) {
    float rf[8];
    unpack8(*reinterpret_cast<const u32x4*>(res_base + (int64_t)m * p.ldr + n0), rf);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += rf[e];
  }
  if (p.out_f32) {
    float* op = reinterpret_cast<float*>(c_base) + (int64_t)m * p.ldc + n0;
    *reinterpret_cast<f32x4*>(op) = f32x4{x[0], x[1], x[2], x[3]};
    *reinterpret_cast<f32x4*>(op + 4) = f32x4{x[4], x[5], x[6], x[7]};
  } else {
    const u32x4 packed = pack8(x);
    *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(c_base) + (int64_t)m * p.ldc + n0) = packed;
    stored(packed);
  }
}
__device__ __forceinline__ void epi_finish_row8(const TcGemmParams& p, char* c_base, const bf16_t* res_base, int m, int n0,
                                                float (&x)[8]) {
  epi_finish_row8(p, c_base, res_base, m, n0, x, [](const u32x4&) {});
}

// ---- 16-row slab pass of the 16x16 MFMA layout (gemm16.hip, conv_halo.hip): one tile row of a wave -- NT accumulator
// tiles `acc`, C/D layout col = lane & 15, row = 4 (lane >> 4) + reg -- goes to the wave's private fp32 slab [16][16 NT];
// the same wave reads it back (LDS operations of one wave complete in order) as 16 x 2 NT vectors of 8 columns walked
// over 64 lanes, vector v = lane + 64 q = (slab row v / VPR, column group v % VPR), and finishes each (epi_finish_row8).
// frow = lane & 15, fq = lane >> 4: the kernel's own values (its fragment addressing uses them; formed afresh here they
// fold into other address arithmetic and the spill loses its paired LDS writes).
// row_of(slab row) -> output row;  col_w0: first output column of the wave;  stored(q, packed): see the finisher.
template <int NT, class RowOf, class Stored>
__device__ __forceinline__ void epi_slab_pass16(const TcGemmParams& p, float* slab, const f32x4 (&acc)[NT], int lane, int frow,
                                                int fq, int col_w0, char* c_base, const bf16_t* res_base, RowOf&& row_of,
                                                Stored&& stored) {
  constexpr int WT = 16 * NT, VPR = WT / 8;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) slab[(fq * 4 + r) * WT + j * 16 + frow] = acc[j][r];
#pragma unroll
  for (int q = 0; q < (16 * VPR + 63) / 64; ++q) {
    const int v = lane + 64 * q;
    const int lr = v / VPR, vc = v - lr * VPR;
    const int m = row_of(lr);
    const int n0 = col_w0 + vc * 8;
    if (v < 16 * VPR && m < p.m && n0 < p.n) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(slab + lr * WT + vc * 8);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(slab + lr * WT + vc * 8 + 4);
      float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      epi_finish_row8(p, c_base, res_base, m, n0, x, [&](const u32x4& packed) { stored(q, packed); });
    }
  }
}

// ---- half-accumulator spill of the 32x32 MFMA layout (gemm_wide.hip, gemm8.hip, ff_fused.hip, tb_fused.hip): registers
// r = 8 HALF .. 8 HALF + 7 of NJ accumulator blocks side by side hold local rows (r & 3) + 4 fhalf + 8 ((r >> 2) & 1),
// column frow of their block -> a 16-row fp32 slab with rows of LD floats.  HALF is a template argument so that the
// accumulator indices stay static (a run-time index would send the whole accumulator file to scratch).
template <int HALF, int NJ, int LD>
__device__ __forceinline__ void epi_spill32_half(float* slab, const f32x16* acc, int frow, int fhalf) {
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = 8 * HALF + q;
      const int lr = (r & 3) + 4 * fhalf + 8 * ((r >> 2) & 1);
      slab[lr * LD + j * 32 + frow] = acc[j][r];
    }
}

// ---- output pass of the level-0 fused kernels (fused_l0.h l0_epilogue: ff_fused.hip, tb_fused.hip): 16 rows x (32 NJ <= 64) columns of a wave's
// output accumulators through its private slab [16][64]; out = (acc + bias) + residual, the residual being the block's own
// input rows x, as bf16.  n0w: first output column of the pass;  bias: the output bias (LDS);  row_of(slab row, m) ->
// whether the row exists, and its row m of x / out (a flag beside the row, not a negative row: tb_fused.hip's rows always
// exist, its constant `true` folds away, and a sentinel would cost that kernel a compare and a branch per row).
template <int HALF, int NJ, class RowOf>
__device__ __forceinline__ void epi_fused_out_pass(float* slab, const f32x16* acc, int lane, int n0w, const float* bias,
                                                   const bf16_t* x, int ldx, bf16_t* out, int ldo, RowOf&& row_of) {
  epi_spill32_half<HALF, NJ, 64>(slab, acc, lane & 31, lane >> 5);
  const int vc = lane & 7, lr0 = lane >> 3;
  const int n0 = n0w + vc * 8;
  if (vc * 8 < NJ * 32) {
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
      const int lr = lr0 + 8 * qq;
      int64_t m;
      const bool ok = row_of(lr, m);
      const f32x4 lo = *reinterpret_cast<const f32x4*>(slab + lr * 64 + vc * 8);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(slab + lr * 64 + vc * 8 + 4);
      if (ok) {
        float xv[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        float rf[8];
        unpack8(*reinterpret_cast<const u32x4*>(x + m * ldx + n0), rf);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = (xv[e] + bias[n0 + e]) + rf[e];
        *reinterpret_cast<u32x4*>(out + m * ldo + n0) = pack8(xv);
      }
    }
  }
}

// ======== the 4-wave kernels' epilogue over the whole fp32 tile staged in LDS (gemm.hip, gemm_mx.hip) ========
// The operands of the epilogue that come from global memory -- bias vectors and the residual rows -- are requested EARLY
// (EpiPrefetch): the bias before the K loop, the residual in front of the last K-step, so their latency runs under the
// MFMAs instead of standing between the K loop and the stores.  With K as short as 320-640 a tile's life is a dependent
// chain (first loads -> K-steps -> LDS transpose -> bias/residual loads -> stores) that two resident blocks per CU only
// half hide; every exposed memory round trip taken out of it is a few per cent of those launches.
template <bool GEGLU, int BM, int BN>
struct EpiGeo {
  static constexpr int GROUPS = GEGLU ? BN / 16 : BN / 8;   // 8-column groups per output row of this tile
  static constexpr int ITERS = BM * GROUPS / 256;
  static constexpr int ROWS_PER_IT = 256 / GROUPS;
};

// GroupNorm statistics of the tile (ABI 9, TcGemmParams.gn_part): per thread the sum and the sum of squares of the
// bf16-ROUNDED outputs of its 8 columns over its rows of the tile; gemm.hip folds them over the tile's rows
struct EpiStats {
  float s[8], q[8];
};

struct EpiPrefetch {
  float bv[8], bg[8];       // bias of this thread's 8 output columns (GEGLU: values | gates)
  u32x4 rres[8];            // residual vectors of its rows (non-GEGLU tiles of at most 128 x 128 / 256 threads)
  bool have_res;
};

// GEGLU weights are packed per 32 rows as [16 values | 16 gates]: output column j of the tile lives at packed column
// 32*(j/16) + j%16, its gate 16 columns further
template <bool GEGLU>
__device__ __forceinline__ int epi_packed_col(int g) { return GEGLU ? 32 * ((g * 8) / 16) + (g * 8) % 16 : g * 8; }

template <bool GEGLU, int BM, int BN>
__device__ __forceinline__ void epi_load_bias(const TcGemmParams& p, int tid, int tile_n, EpiPrefetch& e) {
  using G = EpiGeo<GEGLU, BM, BN>;
  const int g = tid % G::GROUPS;
  const int n_out = GEGLU ? p.n / 2 : p.n;
  const int n0 = (GEGLU ? tile_n * (BN / 2) : tile_n * BN) + g * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) { e.bv[i] = 0.f; e.bg[i] = 0.f; }
  e.have_res = false;
  if (n0 >= n_out || !p.bias) return;
  const int pc = epi_packed_col<GEGLU>(g);
  const float* bp = p.bias + (GEGLU ? tile_n * BN + pc : n0);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { e.bv[i] = b0[i]; e.bv[4 + i] = b1[i]; }
  if (GEGLU) {
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(bp + 16), g1 = *reinterpret_cast<const f32x4*>(bp + 20);
#pragma unroll
    for (int i = 0; i < 4; ++i) { e.bg[i] = g0[i]; e.bg[4 + i] = g1[i]; }
  }
}

// residual rows of a non-GEGLU tile (GEGLU launches carry none)
template <int BM, int BN>
__device__ __forceinline__ void epi_load_residual(const TcGemmParams& p, int tid, int tile_m, int tile_n, int64_t bz,
                                                  EpiPrefetch& e) {
  using G = EpiGeo<false, BM, BN>;
  static_assert(G::ITERS <= 8, "EpiPrefetch::rres holds 8 vectors");
  e.have_res = true;
  const int g = tid % G::GROUPS, row0 = tid / G::GROUPS;
  const int n0 = tile_n * BN + g * 8;
  const bf16_t* res_base = reinterpret_cast<const bf16_t*>(p.residual) + bz * p.stride_c;
#pragma unroll
  for (int it = 0; it < G::ITERS; ++it) {
    const int m = tile_m * BM + row0 + it * G::ROWS_PER_IT;
    const int mc = m < p.m ? m : p.m - 1;
    e.rres[it] = u32x4{0u, 0u, 0u, 0u};
    if (n0 < p.n) e.rres[it] = *reinterpret_cast<const u32x4*>(res_base + (int64_t)mc * p.ldr + n0);
  }
}

// ---- epilogue over the fp32 tile staged in LDS ----------------------------------------
// Fast path: every 8-column vector of the tile is fully inside N and 16-byte addressable.
// PLAIN = the common "acc + bias (+ residual)" case (alpha = out_scale = 1, no activation, no row bias):
// with K as short as 320 the epilogue is a third of a block's instructions, so it gets its own
// straight-line instance without the per-element multiplies and activation selects.
// `pre`: bias already loaded by epi_load_bias; residual loaded by epi_load_residual if pre.have_res.
template <bool GEGLU, int BM, int BN, bool PLAIN, bool STATS = false>
__device__ __forceinline__ void epilogue_fast(const TcGemmParams& p, const float* cs, int tid, int tile_m, int tile_n,
                                              int64_t bz, EpiPrefetch& pre, EpiStats* st = nullptr) {
  using G = EpiGeo<GEGLU, BM, BN>;
  constexpr int GROUPS = G::GROUPS, ITERS = G::ITERS, ROWS_PER_IT = G::ROWS_PER_IT;
  const int g = tid % GROUPS;
  const int row0 = tid / GROUPS;
  const int n_out = GEGLU ? p.n / 2 : p.n;
  const int n0 = (GEGLU ? tile_n * (BN / 2) : tile_n * BN) + g * 8;
  if (n0 >= n_out) return;
  const int pc = epi_packed_col<GEGLU>(g);
  const float (&bv)[8] = pre.bv;
  const float (&bg)[8] = pre.bg;
  const bool with_res = !GEGLU && p.residual != nullptr;
  char* c_base = reinterpret_cast<char*>(p.c) + bz * p.stride_c * (p.out_f32 ? 4 : 2);
  if (!GEGLU) {
    if (with_res && !pre.have_res) epi_load_residual<BM, BN>(p, tid, tile_m, tile_n, bz, pre);
  }
  // row-bias loads first
  f32x4 rb0[ITERS], rb1[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int m = tile_m * BM + row0 + it * ROWS_PER_IT;
    const int mc = m < p.m ? m : p.m - 1;
    rb0[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    rb1[it] = rb0[it];
    if (!GEGLU && !PLAIN && p.row_bias) {
      const float* rp = p.row_bias + (int64_t)(mc / p.row_div) * p.ldrb + n0;
      rb0[it] = *reinterpret_cast<const f32x4*>(rp);
      rb1[it] = *reinterpret_cast<const f32x4*>(rp + 4);
    }
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int row = row0 + it * ROWS_PER_IT;
    const int m = tile_m * BM + row;
    float x[8];
    {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(cs + row * BN + pc);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(cs + row * BN + pc + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { x[e] = lo[e]; x[4 + e] = hi[e]; }
    }
    if (GEGLU) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(cs + row * BN + pc + 16);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(cs + row * BN + pc + 20);
      float gt[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { gt[e] = lo[e]; gt[4 + e] = hi[e]; }
#pragma unroll
      for (int e = 0; e < 8; e += 2) epi_geglu_pair<PLAIN>(p, x + e, gt + e, bv + e, bg + e);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (PLAIN) {
          x[e] += bv[e];
        } else {
          const float rbv = e < 4 ? rb0[it][e] : rb1[it][e - 4];
          x[e] = apply_act(x[e] * p.alpha + bv[e] + rbv, p.act) * p.out_scale;
        }
      }
    }
    if (with_res) {
      float rf[8];
      unpack8(pre.rres[it < 8 ? it : 0], rf);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] += rf[e];
    }
#if defined(TC_ABLATE) && (TC_ABLATE & 16)     // ... without its global stores
    if (x[0] == 1.2345e30f) {
#else
    if (m < p.m) {
#endif
      if (p.out_f32) {
        float* op = reinterpret_cast<float*>(c_base) + (int64_t)m * p.ldc + n0;
        *reinterpret_cast<f32x4*>(op) = f32x4{x[0], x[1], x[2], x[3]};
        *reinterpret_cast<f32x4*>(op + 4) = f32x4{x[4], x[5], x[6], x[7]};
      } else {
        const u32x4 packed = pack8(x);
        *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(c_base) + (int64_t)m * p.ldc + n0) = packed;
        if (STATS) {
          float fr[8];
          unpack8(packed, fr);                     // what GroupNorm will read back: the rounded values
#pragma unroll
          for (int e = 0; e < 8; ++e) { st->s[e] += fr[e]; st->q[e] += fr[e] * fr[e]; }
        }
      }
    }
  }
}

// the same with every operand fetched inside the epilogue (callers without an early-prefetch point)
template <bool GEGLU, int BM, int BN, bool PLAIN>
__device__ __forceinline__ void epilogue_fast(const TcGemmParams& p, const float* cs, int tid, int tile_m, int tile_n,
                                              int64_t bz) {
  EpiPrefetch pre;
  epi_load_bias<GEGLU, BM, BN>(p, tid, tile_n, pre);
  epilogue_fast<GEGLU, BM, BN, PLAIN>(p, cs, tid, tile_m, tile_n, bz, pre);
}

// Slow path: N not a multiple of 8 (the 4-channel UNet output, the 3-channel decoder output).
template <int BM, int BN>
__device__ __forceinline__ void epilogue_tail(const TcGemmParams& p, const float* cs, int tid, int tile_m, int tile_n,
                                              int64_t bz) {
  const bf16_t* res_base = p.residual ? reinterpret_cast<const bf16_t*>(p.residual) + bz * p.stride_c : nullptr;
  char* c_base = reinterpret_cast<char*>(p.c) + bz * p.stride_c * (p.out_f32 ? 4 : 2);
  for (int v = tid; v < BM * BN; v += 256) {
    const int row = v / BN, col = v - row * BN;
    const int m = tile_m * BM + row, n = tile_n * BN + col;
    if (m >= p.m || n >= p.n) continue;
    float val = cs[row * BN + col] * p.alpha;
    if (p.bias) val += p.bias[n];
    if (p.row_bias) val += p.row_bias[(int64_t)(m / p.row_div) * p.ldrb + n];
    val = apply_act(val, p.act) * p.out_scale;
    if (res_base) val += (float)res_base[(int64_t)m * p.ldr + n];
    if (p.out_f32) reinterpret_cast<float*>(c_base)[(int64_t)m * p.ldc + n] = val;
    else reinterpret_cast<bf16_t*>(c_base)[(int64_t)m * p.ldc + n] = (bf16_t)val;
  }
}
