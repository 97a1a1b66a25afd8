// The skeleton the two level-0 fused kernels share (ff_fused.hip, tb_fused.hip; their headers describe it): 8 waves on
// 128 rows x C = 320, the rows' LayerNorm in registers, a FIRST product of the resident rows against streamed [128 x 64 k]
// weight K-tiles (a 32 x 64 block per wave in acc_v | acc_g), a SECOND product of a [128 x 64] bf16 chunk in LDS against a
// [320 x 64] weight slice into 32 x 160 output accumulators per wave.  Each kernel keeps its LDS map, its weight-stream
// schedule with the hand-counted vmcnt tables, and what it does between the two products.
//
// Both kernels live at the register limit (80 A-fragment + 80 output + 32 accumulator + 32 B-fragment registers under
// the 256 of an 8-wave block): nothing here keeps an address across the chunk / head loop -- the callers hand over the
// lane id and the addresses as they form them at the place of use -- and nothing here issues or waits for an LDS-DMA
// request: the order of requests and counted waits is the callers' text.
#pragma once
#include "gemm_persist.h"
#include "gemm_epilogue.h"

#include <stdlib.h>

namespace {

constexpr int L0_C = 320, L0_BM = 128, L0_THREADS = 512;
constexpr int L0_KT = L0_C / TC_BK;               // 5 K-steps of 64 in a first product
constexpr int L0_NSLICE = L0_C / 16;              // 20 K-slices of 16: one MFMA each, a 16-byte A fragment per lane
constexpr int L0_NPARK = 3;                       // the last K-slices of the normalised rows live in LDS, not in registers
constexpr int L0_NRES = L0_NSLICE - L0_NPARK;
constexpr int L0_W_STAGE = 128 * 128;             // 16 KiB: a weight K-tile, 128 rows x 64 k
constexpr int L0_W2_BYTES = 320 * 128;            // 40 KiB: the second product's weight slice, 320 rows x 64 k
constexpr int L0_BUF_BYTES = 128 * 128;           // 16 KiB: a [128 rows][64] bf16 chunk buffer (A operand of the second product)
constexpr int L0_PARK_SLOT = 4096;                // a parked K-slice: [wm][lane] x 16 B
constexpr int L0_PARK_BYTES = L0_NPARK * L0_PARK_SLOT;

// ---- the 32x32x16 MFMA fragment layout.  Operands: a lane holds row (lane & 31), k = 8 (lane >> 5) .. + 8 of K-slice kk,
// i.e. 16-byte chunk 2 kk + (lane >> 5) of a 64-k row.  LDS rows are 128 bytes with the chunk XOR-swizzled by
// (row >> 1) & 7 (the weight stream applies it to the SOURCE chunk of its request).  Accumulator: register r of a lane is
// row cr = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the 32, column lane & 31.
__device__ __forceinline__ int l0_coff(int kk, int frow, int fhalf) { return ((kk * 2 + fhalf) ^ ((frow >> 1) & 7)) << 4; }

// the lane id taken afresh (and opaquely): an address hoisted out of the chunk / head loop is a register the loop does not
// have, i.e. a scratch reload, i.e. a compiler "s_waitcnt vmcnt(0)" inside the counted stream
__device__ __forceinline__ int l0_lane_now() {
  int gl = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  asm volatile("" : "+v"(gl));
  return gl;
}

// two bias vectors into LDS once, bl = [a (na) | b (nb)]: no global load may sit inside the chunk / head loop (hipcc would
// wait vmcnt(0) for it and drain the stream); in LDS before the first barrier
__device__ __forceinline__ void l0_stage_biases(float* bl, const float* a, int na, const float* b, int nb, int tid) {
  for (int i = tid; i < na; i += L0_THREADS) bl[i] = a[i];
  for (int i = tid; i < nb; i += L0_THREADS) bl[na + i] = b[i];
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// ---- weight stream, lane map: a request moves a 64-row piece, thread -> (row tid >> 3, 16-byte chunk tid & 7); the XOR
// swizzle is on the SOURCE chunk.  voff: the per-lane byte offset for source row `src_row` of a matrix with `ld` elements
// per row;  dst: the wave's 1 KiB of the piece (+ the piece's place in the kernel's LDS map)
__device__ __forceinline__ int l0_stream_row(int tid) { return tid >> 3; }
__device__ __forceinline__ uint32_t l0_stream_voff(int src_row, int ld, int tid) {
  const int sch = (tid & 7) ^ (((tid >> 3) >> 1) & 7);
  return (uint32_t)(src_row * ld * 2 + sch * 16);
}
__device__ __forceinline__ uint32_t l0_stream_dst(uint32_t lds0, int wave_u) { return lds0 + wave_u * 1024; }

// barrier of the timed builds: block 0's waves 0 (group 0) and 4 (group 1) store the shader clock after every barrier
// while the caller's window `tr_on` is open -> trace[wave >> 2][n].  TRACE = false: the plain barrier
template <bool TRACE>
__device__ __forceinline__ void l0_bar(unsigned long long* trace, int wave_u, int lane, bool tr_on, int& tr_n) {
  g8_barrier();
  if constexpr (TRACE) {
    if (tr_on && tr_n < 64) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      if (lane == 0) trace[(wave_u >> 2) * 64 + tr_n] = t;
      ++tr_n;
    }
  }
}
// the stagger, per tile: group 1 runs one barrier interval behind group 0 through the chunks / heads, and is let catch up
// before the epilogue (every wave has then executed the same number of barriers), so that the two groups' epilogues and
// row loads -- long, barrier-free -- run side by side
__device__ __forceinline__ void l0_stagger(int grp) { if (grp == 1) g8_barrier(); }
__device__ __forceinline__ void l0_realign(int grp) { if (grp == 0) g8_barrier(); }

// ---- row prologue: the lane's half of its row (20 x 16 B from xrow + 8 fhalf; load = false substitutes ones: a timing
// ablation) -> two-pass LayerNorm without affine (ln != 0; a row's 320 values sit in two lanes: one lane swap) -> K-slices
// 0 .. L0_NRES-1 as A fragments in xa, the last L0_NPARK parked at park + slot * L0_PARK_SLOT (both N-waves of a row
// group write the same bytes)
__device__ __forceinline__ void l0_rows_prologue(const bf16_t* xrow, int fhalf, bool load, int ln, float eps, bf16x8 (&xa)[L0_NRES],
                                                 char* park) {
  u32x4 raw[L0_NSLICE];
  const bf16_t* xr = xrow + 8 * fhalf;
#pragma unroll
  for (int s = 0; s < L0_NSLICE; ++s)
    raw[s] = load ? *reinterpret_cast<const u32x4*>(xr + 16 * s) : u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
  if (ln) {
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < L0_NSLICE; ++s) {
      float f[8];
      unpack8(raw[s], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += f[e];
    }
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / L0_C);
    float sq = 0.f;
#pragma unroll
    for (int s = 0; s < L0_NSLICE; ++s) {
      float f[8];
      unpack8(raw[s], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = f[e] - mean; sq += d * d; }
    }
    sq += __shfl_xor(sq, 32, 64);
    const float rstd = rsqrtf(sq * (1.0f / L0_C) + eps);
    // the deviations of the variance pass must not be kept for the normalise pass (160 live values: the kernels have no
    // such registers, they would go to scratch): the mean is handed to that pass opaquely, so f - mean is formed again
    float mean_n = mean;
    asm volatile("" : "+v"(mean_n));
#pragma unroll
    for (int s = 0; s < L0_NSLICE; ++s) {
      float f[8];
      unpack8(raw[s], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = (f[e] - mean_n) * rstd;
      raw[s] = pack8(f);
    }
  }
#pragma unroll
  for (int s = 0; s < L0_NSLICE; ++s) {
    if (s < L0_NRES) xa[s] = __builtin_bit_cast(bf16x8, raw[s]);
    else *reinterpret_cast<u32x4*>(park + (s - L0_NRES) * L0_PARK_SLOT) = raw[s];
  }
  // without LayerNorm nothing has consumed the row loads yet: a load still "pending" at the chunk loop's header makes
  // the compiler wait vmcnt(0) at its first use INSIDE the loop, every chunk -- so they are consumed here, once
#pragma unroll
  for (int s = 0; s < L0_NRES; ++s) asm volatile("" ::"v"(xa[s]));
}

// ---- first product.  B fragments of one K-step: st = the wave's row of the stage (+ its lane's row), two 32-row blocks
// 4096 bytes apart (value | gate, q | k columns 0..31 | 32..63)
__device__ __forceinline__ void l0_read_bw(const char* st, int frow, int fhalf, bf16x8 (&bw)[2][4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) bw[j][kk] = *reinterpret_cast<const bf16x8*>(st + j * 4096 + l0_coff(kk, frow, fhalf));
}
// K-slice KK of K-step S: two MFMAs; the A fragment is resident (xa) or parked -- the parked slices are read here, in the
// MFMA segment of the last K-step, into registers its first MFMAs have just released.  NOMFMA: a timing ablation
template <int S, int KK, bool NOMFMA = false>
__device__ __forceinline__ void l0_mm(const bf16x8 (&xa)[L0_NRES], const char* park, const bf16x8 (&bw)[2][4], f32x16& acc_v,
                                      f32x16& acc_g) {
  constexpr int ks = 4 * S + KK;
  if constexpr (NOMFMA) {
    asm volatile("" : "+v"(acc_v), "+v"(acc_g) : "v"(bw[0][KK]), "v"(bw[1][KK]));
  } else {
    bf16x8 a;
    if constexpr (ks < L0_NRES) a = xa[ks];
    else a = *reinterpret_cast<const bf16x8*>(park + (ks - L0_NRES) * L0_PARK_SLOT);
    acc_v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bw[0][KK], acc_v, 0, 0, 0);
    acc_g = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bw[1][KK], acc_g, 0, 0, 0);
  }
  if constexpr (S == 4) __builtin_amdgcn_sched_barrier(0);
}
template <int S, bool NOMFMA = false>
__device__ __forceinline__ void l0_mm4(const bf16x8 (&xa)[L0_NRES], const char* park, const bf16x8 (&bw)[2][4], f32x16& acc_v,
                                       f32x16& acc_g) {
  l0_mm<S, 0, NOMFMA>(xa, park, bw, acc_v, acc_g);
  l0_mm<S, 1, NOMFMA>(xa, park, bw, acc_v, acc_g);
  l0_mm<S, 2, NOMFMA>(xa, park, bw, acc_v, acc_g);
  l0_mm<S, 3, NOMFMA>(xa, park, bw, acc_v, acc_g);
}

// ---- the swizzled scatter of a 32 x 32 accumulator block into a row-major [128][64] bf16 buffer, 16-byte chunks
// XOR-swizzled by (row >> 1) & 7.  The place of (row, col):
//     row * 128 + (((col >> 3) ^ ((row >> 1) & 7)) << 4) + (col & 7) * 2
// With row = row0 + cr + 4 fhalf (row0 a multiple of 32) and cr = (r & 3) + 8 (r >> 2): (row >> 1) & 7 = kr | 2 fhalf with
// kr = (cr >> 1) & 7 in {0, 1, 4, 5}: four lane-dependent bases serve all registers, everything else is an immediate.
// Column col + 32 is chunk ^ 4, i.e. kr ^ 4: the base two places on.
struct L0Scatter {
  char* b[4];
  // rows = the buffer at the block's first row (buf + row0 * 128);  col = the lane's column of the 64;  fh = lane >> 5
  __device__ __forceinline__ L0Scatter(char* rows, int col, int fh) {
    char* const hrow = rows + 4 * fh * 128 + (col & 7) * 2;
    const int a2 = (col >> 3) ^ (2 * fh);
    b[0] = hrow + (a2 << 4); b[1] = hrow + ((a2 ^ 1) << 4); b[2] = hrow + ((a2 ^ 4) << 4); b[3] = hrow + ((a2 ^ 5) << 4);
  }
  static __device__ __forceinline__ int base_of(int r) {
    const int kr = (((r & 3) + 8 * (r >> 2)) >> 1) & 7;          // 0, 1, 4 or 5; the same for r and r + 1 when r is even
    return (kr & 1) + (kr >> 2) * 2;
  }
  // where accumulator register r goes (register r + 1, r even: the next row, + 128);  at32: the same row, column col + 32
  __device__ __forceinline__ bf16_t* at(int r) const { return reinterpret_cast<bf16_t*>(b[base_of(r)] + ((r & 3) + 8 * (r >> 2)) * 128); }
  __device__ __forceinline__ bf16_t* at32(int r) const { return reinterpret_cast<bf16_t*>(b[base_of(r) ^ 2] + ((r & 3) + 8 * (r >> 2)) * 128); }
};

// ---- second product: [32 x 64] chunk (A, from LDS: ha = the chunk buffer at the lane's row) x weight slice [160 x 64]
// (B, from LDS: wb = the slice at the lane's row of the wave's 160) -> out_acc, 20 MFMAs; the B set just consumed is
// refilled two column blocks ahead.  One barrier between the first reads and the MFMAs, one behind them.
template <bool NOMFMA = false, class Bar>
__device__ __forceinline__ void l0_second_product(const char* hb, const char* wb, int frow, int fhalf, f32x16 (&out_acc)[5], Bar&& bar) {
  bf16x8 ha[4], b2[2][4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) ha[kk] = *reinterpret_cast<const bf16x8*>(hb + l0_coff(kk, frow, fhalf));
  l0_read_bw(wb, frow, fhalf, b2);
  bar();
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int j = 0; j < 5; ++j) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      if constexpr (NOMFMA) asm volatile("" : "+v"(out_acc[j]) : "v"(ha[kk]), "v"(b2[j & 1][kk]));
      else out_acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha[kk], b2[j & 1][kk], out_acc[j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (j + 2 < 5) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) b2[j & 1][kk] = *reinterpret_cast<const bf16x8*>(wb + (j + 2) * 4096 + l0_coff(kk, frow, fhalf));
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_s_setprio(0);
  bar();
}

// ---- epilogue: out = (acc + bias) + residual (the raw rows of x), bf16.  Per wave six passes of (16 rows x 64 | 32
// columns) through its private 4 KiB slab (gemm_epilogue.h epi_fused_out_pass).  row_of(tile row, m) -> whether the row
// exists, and its row m of x / out
template <class RowOf>
__device__ __forceinline__ void l0_epilogue(float* slab, const f32x16* out_acc, int lane, int wm, int wn, const float* bias,
                                            const bf16_t* x, int ldx, bf16_t* out, int ldo, RowOf&& row_of) {
  auto pass = [&](auto J0_, auto NJ_, auto HALF_) {
    constexpr int j0 = decltype(J0_)::value, nj = decltype(NJ_)::value, half = decltype(HALF_)::value;
    epi_fused_out_pass<half, nj>(slab, out_acc + j0, lane, wn * 160 + j0 * 32, bias, x, ldx, out, ldo,
                                 [&](int lr, int64_t& m) { return row_of(wm * 32 + half * 16 + lr, m); });
  };
  pass(ic<0>{}, ic<2>{}, ic<0>{});
  pass(ic<0>{}, ic<2>{}, ic<1>{});
  pass(ic<2>{}, ic<2>{}, ic<0>{});
  pass(ic<2>{}, ic<2>{}, ic<1>{});
  pass(ic<4>{}, ic<1>{}, ic<0>{});
  pass(ic<4>{}, ic<1>{}, ic<1>{});
}

// ======== host side ========
inline int l0_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
// the persistent grid: every block the same number of tiles -- 640 tiles on 256 CUs are three rounds either way, and 214
// blocks of three leave the weight stream (L2 -> LDS, shared by all) less contended than 256 blocks of two or three.
// `grid_env` (TC_FF_GRID / TC_TB_GRID) > 0 replaces the CU count as the most blocks a launch may have
inline int l0_grid(int tiles, const char* grid_env) {
  const int v = l0_env_int(grid_env, 0);
  const int gmax = v > 0 ? v : tc_cu_count();
  const int rounds = (tiles + gmax - 1) / gmax;
  return (tiles + rounds - 1) / rounds;
}
// where the interval trace of a timing build goes: a device address in `trace_env`
inline unsigned long long* l0_trace_ptr(const char* trace_env) {
  const char* e = getenv(trace_env);
  return e ? reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0)) : nullptr;
}
// row pitches of x and out: at least a row, rows start on 16 bytes;  `rows` rows at pitch `ld` within the offset bound
inline bool l0_rows_ok(int ldx, int ldo, int64_t rows, int ld) {
  return ldx >= L0_C && ldo >= L0_C && !(ldx & 7) && !(ldo & 7) && rows * ld * 2 < 0x7fffffffLL * 64;
}
// what both entry points check, in their order: a null pointer, the kernel's own shape rule (its *_eligible), alignment
inline int l0_check_call(const void* x, const void* wa, const float* ba, const void* wb, const float* bb, const void* out, int eligible) {
  if (!x || !wa || !ba || !wb || !bb || !out) return TC_EINVAL;
  if (!eligible) return TC_ESHAPE;
  if (!tc_aligned16(x) || !tc_aligned16(wa) || !tc_aligned16(wb) || !tc_aligned16(out)) return TC_EALIGN;
  return TC_OK;
}

}  // namespace
