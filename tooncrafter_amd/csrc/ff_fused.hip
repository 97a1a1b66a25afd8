// Fused feed-forward of a level-0 transformer block, gfx950:
//
//     out = x + W2 . GEGLU(W1 . LayerNorm(x) + b1) + b2            x: [M, 320] bf16, hidden 1280
//
// (reference lvdm/modules/attention.py:415-442 FeedForward / GEGLU behind norm3, attention.py:244-246).  As three launches
// -- LayerNorm, the GEGLU projection (81920 x 2560 x 320) and ff2 (81920 x 320 x 1280) -- the block writes its 210 MB
// hidden tensor to HBM and reads it back: 240 + 111 (+ 20) us, both GEMMs far from the matrix roof because they are bound by
// those bytes and by the GEGLU epilogue (profiles/r03_ablate_gemm.txt, r04_gemm8_ablation.txt).  Here the hidden tensor
// never exists:
//
//  * a block owns 128 rows; wave (wm, wn) of its 8 waves owns rows wm*32..+32.  The rows' LayerNorm runs in REGISTERS on
//    the MFMA A-operand layout (a row's 320 values sit in two lanes: one lane swap) and the normalised rows stay there as
//    the A fragments of the first product for the whole tile (80 VGPRs) -- x is read once, nothing of it goes through LDS;
//  * the hidden dimension is walked in 20 chunks of 64.  Per chunk: ff1 = 5 K-steps against a [128 packed rows x 64]
//    W1 tile (wave: its 32 rows x 64 packed columns = one value block + one gate block, 8 MFMAs per K-step; the stage
//    holds, per 64 rows, [32 values | 32 gates], so a value and its gate meet in the same lane and register); GEGLU on the
//    accumulators; the 32 x 32 hidden values of the wave go to LDS as bf16 in A-operand layout; ff2 = the tile's
//    [128 x 64] hidden chunk against W2's [320 x 64] slice into the wave's 32 x 160 output accumulators (80 VGPRs,
//    20 MFMAs), which live across all 20 chunks;
//  * the weights (2.4 MB, L2-resident) stream through LDS by LDS-DMA from inline asm: W1 K-tiles through a ring of four
//    16 KiB stages (requested two steps ahead), W2's 40 KiB slice once per chunk (five pieces spread over the chunk's
//    steps).  The stream does not depend on the tile, so it simply runs on across the tiles of a persistent block;
//  * the two wave GROUPS (wm >> 1: one wave per SIMD each) run one barrier interval apart, as in gemm8.hip: while one
//    group issues its MFMAs the other reads its fragments / requests tiles / evaluates GEGLU.
//
// LDS: W1 ring 64 KiB | W2 slice 40 KiB | hidden chunk 2 x 16 KiB (also the epilogue slabs) | biases 12 KiB = 148 KiB.
// Order of the fp32 sums: ff1 over K in ascending 16-slices, ff2 over the hidden index in ascending 16-slices -- the
// order of the tiled kernels, so the result equals LayerNorm -> tc_gemm_bf16(GEGLU) -> tc_gemm_bf16(+residual) up to the
// LayerNorm's own rounding.  What this kernel shares with tb_fused.hip is stated in csrc/fused_l0.h; here: the LDS map,
// the weight-stream schedule with its counted waits, and the GEGLU between the two products.
#include "fused_l0.h"

namespace {

constexpr int FF_C = L0_C, FF_H = 1280, FF_BM = L0_BM, FF_THREADS = L0_THREADS;
constexpr int FF_CH = 64;                       // hidden columns per chunk = 128 packed W1 rows
constexpr int FF_NCH = FF_H / FF_CH;            // 20 chunks
constexpr int FF_KT = L0_KT;                    // 5 K-steps of ff1 per chunk
constexpr int FF_W1_STAGE = L0_W_STAGE;         // 16 KiB: 128 packed rows x 64 k
constexpr int FF_W1_OFF = 0;                    // ring of 4
constexpr int FF_W2_OFF = 4 * FF_W1_STAGE;      // 40 KiB: 320 rows x 64 k
constexpr int FF_H_OFF = FF_W2_OFF + L0_W2_BYTES;   // 2 x 16 KiB: 128 rows x 64 hidden
constexpr int FF_H_BYTES = L0_BUF_BYTES;
constexpr int FF_B_OFF = FF_H_OFF + 2 * FF_H_BYTES; // b1 (2560 fp32) | b2 (320 fp32)
constexpr int FF_P_OFF = FF_B_OFF + (2 * FF_H + FF_C) * 4;   // the parked A fragments
constexpr int FF_LDS = FF_P_OFF + L0_PARK_BYTES;
static_assert(FF_LDS <= 160 * 1024, "LDS");

struct FfArgs {
  const bf16_t* x; const bf16_t* w1; const float* b1; const bf16_t* w2; const float* b2; bf16_t* out;
  int m, ldx, ldo, ln;
  float eps;
  int tiles;
  unsigned long long* trace;     // TC_FF_TRACE (ABL bit 16 build): s_memtime after every barrier of block 0's waves 0 and 4
};

// LA: W1 K-tiles requested ahead (2 or 3 of the ring's 4 stages; 4 = three ahead with the requests issued in the MFMA segment,
// between the MFMAs, instead of in the read segment: 274-280 us against 265-268, profiles/r04_ff_fused_bench.txt -- kept as a switch).  ABL: timing ablations (TC_FF_ABLATE; wrong results) --
// 1 no GELU arithmetic, 2 no weight requests, 4 no ff1 MFMAs, 8 no ff2 MFMAs.
template <int LA, int ABL, int GI>
__global__ __launch_bounds__(FF_THREADS, 2) void ff_fused_kernel(const FfArgs p) {
  __shared__ __attribute__((aligned(1024))) char smem[FF_LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_u >> 1, wn = wave_u & 1;
  const int grp = wave_u >> 2;                   // = wm >> 1: waves w and w + 4 share a SIMD, one of each group
  const int frow = lane & 31, fhalf = lane >> 5;

  const g8_srd_t w1_srd = g8_make_srd(p.w1, (int64_t)2 * FF_H * FF_C * 2);
  const g8_srd_t w2_srd = g8_make_srd(p.w2, (int64_t)FF_C * FF_H * 2);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  l0_stage_biases(reinterpret_cast<float*>(smem + FF_B_OFF), p.b1, 2 * FF_H, p.b2, FF_C, tid);

  // ---- weight stream (lane map: fused_l0.h)
  const int lrow = l0_stream_row(tid);
  // W1 arrives in the GEMM's GEGLU packing (lvdm/common.py pack_geglu: every 32 rows = 16 value rows | their 16 gate rows);
  // the stage wants, per 64 rows, [32 values | 32 gates], so that a value and its gate meet in one lane of the two 32 x 32
  // accumulator blocks -- a permutation of the SOURCE row, free in the request's address
  const int w1_src = ((lrow & 31) >> 4) * 32 + (lrow >> 5) * 16 + (lrow & 15);
  const uint32_t v1 = l0_stream_voff(w1_src, FF_C, tid);              // W1: + soffset (packed row block, K-step, pass)
  const uint32_t v2 = l0_stream_voff(lrow, FF_H, tid);                // W2: + soffset (hidden chunk, pass)
  const uint32_t dma_dst = l0_stream_dst(lds0, wave_u);
  auto dma_w1 = [&](int q) {                                          // W1 K-tile q of the cyclic stream -> ring stage q & 3
    if constexpr (ABL & 2) return;
    const int qq = q % (FF_NCH * FF_KT);
    const int c = qq / FF_KT, kt = qq - c * FF_KT;
    const uint32_t so = (uint32_t)((c * 128 * FF_C + kt * TC_BK) * 2);
    const uint32_t dst = dma_dst + FF_W1_OFF + (q & 3) * FF_W1_STAGE;
    g8_dma16(w1_srd, dst, v1, so);
    g8_dma16(w1_srd, dst + 8192, v1, so + 64 * FF_C * 2);
  };
  auto dma_w1_half = [&](int q, int half) {                           // one of the K-tile's two pieces (LA == 4)
    if constexpr (ABL & 2) return;
    const int qq = q % (FF_NCH * FF_KT);
    const int c = qq / FF_KT, kt = qq - c * FF_KT;
    const uint32_t so = (uint32_t)((c * 128 * FF_C + kt * TC_BK) * 2) + (uint32_t)half * (64 * FF_C * 2);
    g8_dma16(w1_srd, dma_dst + FF_W1_OFF + (q & 3) * FF_W1_STAGE + half * 8192, v1, so);
  };
  auto dma_w2 = [&](int c, int piece) {                               // rows 64 piece .. +64 of W2's slice for hidden chunk c
    if constexpr (ABL & 2) return;
    const int cc = c % FF_NCH;
    const uint32_t so = (uint32_t)((piece * 64 * FF_H + cc * FF_CH) * 2);
    g8_dma16(w2_srd, dma_dst + FF_W2_OFF + piece * 8192, v2, so);
  };

  // ---- fragment addressing (layout: fused_l0.h), computed where it is used, from the lane id: the kernel lives at the
  // register limit -- 80 A-fragment + 80 output + 32 ff1 accumulator + 32 B-fragment registers -- and every address kept
  // across the chunk loop is a spill into scratch, i.e. a vector-memory load inside the counted LDS-DMA stream
  auto w1_row = [&]() { return (wn * 64 + frow) * 128; };          // + j * 4096 (value / gate block)
  auto h_row = [&]() { return (wm * 32 + frow) * 128; };
  auto w2_row = [&]() { return (wn * 160 + frow) * 128; };         // + j * 4096

  // the tile's normalised rows, A fragments of ff1: K-slices 0 .. L0_NRES-1 in registers, the last L0_NPARK in LDS
  bf16x8 xa[L0_NRES];
  char* const park = smem + FF_P_OFF + wm * 1024 + lane * 16;
  f32x16 out_acc[5];
  f32x16 acc_v, acc_g;

  // ABL bit 16: per-interval timing.  Block 0, waves 0 (group 0) and 4 (group 1), second tile, first three chunks: the
  // shader clock after every barrier -> trace[wave >> 2][n]
  int tr_n = 0;
  bool tr_on = false;
  auto bar = [&]() { l0_bar<(ABL & 16) != 0>(p.trace, wave_u, lane, tr_on, tr_n); };
  int q = 0;                                          // W1 K-tile stream position consumed next (cyclic)
  int cw2 = 0;                                        // hidden chunk whose W2 slice is requested next (cyclic): the one
                                                      // the CURRENT chunk's ff2 reads -- requested during its ff1 steps
  // prologue of the stream: W1(0), W1(1)
  dma_w1(0);
  dma_w1(1);
  if constexpr (LA >= 3) dma_w1(2);
  tc_wait_vmcnt<0>();
  g8_barrier();

  const float* bl = reinterpret_cast<const float*>(smem + FF_B_OFF);

  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    // ---- the wave's 32 rows: raw -> LayerNorm -> A fragments
    const int row = tile * FF_BM + wm * 32 + frow;
    const bool rok = row < p.m;
    l0_rows_prologue(p.x + (int64_t)(rok ? row : p.m - 1) * p.ldx, fhalf, true, p.ln, p.eps, xa, park);   // rows past M: a valid row, never stored
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) out_acc[j][r] = 0.f;

    l0_stagger(grp);
    for (int c = 0; c < FF_NCH; ++c) {
      if constexpr (ABL & 16) tr_on = blockIdx.x == 0 && (wave_u & 3) == 0 && tile == (int)(blockIdx.x + gridDim.x) && c < 3;
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc_v[r] = 0.f; acc_g[r] = 0.f; }
      // ---- ff1: five K-steps; step s reads W1 K-tile q (ring stage q & 3) and requests K-tile q + 2
      auto ff1_step = [&](auto S_) {
        constexpr int s = decltype(S_)::value;
        const char* st = smem + FF_W1_OFF + (q & 3) * FF_W1_STAGE + w1_row();
        bf16x8 bw[2][4];
        l0_read_bw(st, frow, fhalf, bw);
        if constexpr (LA != 4) {
          dma_w1(q + LA);
          if (s == 1) { dma_w2(cw2, 0); dma_w2(cw2, 1); }
          if (s >= 2) { dma_w2(cw2, s); }
        }
        // the K-tile the NEXT step reads has landed (this wave's pieces; the barrier makes it everybody's): the counts are
        // the requests issued after it -- see the table above the steps
        if constexpr (LA == 2) {
          if (s == 0) tc_wait_vmcnt<2>();
          else if (s == 2) tc_wait_vmcnt<5>();
          else tc_wait_vmcnt<4>();
        } else if constexpr (LA == 3) {
          if (s == 0) tc_wait_vmcnt<2>();
          else if (s == 1) tc_wait_vmcnt<6>();
          else if (s == 3) tc_wait_vmcnt<8>();
          else tc_wait_vmcnt<7>();
        } else {
          // requests in the MFMA segments: M_s issues W1(q + 3) (two pieces), then piece s of this chunk's W2 slice.  The
          // tile the next step reads was requested two MFMA segments ago, first there; behind it: that segment's W2 piece
          // and the last segment's three requests (across the chunk seam everything was drained at the end of G)
          if (s == 0) tc_wait_vmcnt<0>();
          else if (s == 1) tc_wait_vmcnt<3>();
          else tc_wait_vmcnt<4>();
        }
        bar();
        __builtin_amdgcn_s_setprio(1);
        auto mm = [&](auto KK_) { l0_mm<s, decltype(KK_)::value, (ABL & 4) != 0>(xa, park, bw, acc_v, acc_g); };
        if constexpr (LA == 4) {
          mm(ic<0>{});
          __builtin_amdgcn_sched_barrier(0);
          dma_w1_half(q + 3, 0);
          __builtin_amdgcn_sched_barrier(0);
          mm(ic<1>{});
          __builtin_amdgcn_sched_barrier(0);
          dma_w1_half(q + 3, 1);
          __builtin_amdgcn_sched_barrier(0);
          mm(ic<2>{});
          __builtin_amdgcn_sched_barrier(0);
          dma_w2(cw2, s);
          __builtin_amdgcn_sched_barrier(0);
          mm(ic<3>{});
        } else {
          l0_mm4<s, (ABL & 4) != 0>(xa, park, bw, acc_v, acc_g);
        }
        __builtin_amdgcn_s_setprio(0);
        bar();
        ++q;
      };
      // Requests in program order, per chunk (W1 = two pieces per thread, a W2 piece = one; the W2 slice requested is THIS
      // chunk's -- its buffer is single, and the other group reads the previous slice until the end of this group's R0,
      // hence nothing for it in R0):
      //     R0: W1(q+2) | R1: W1, p0, p1 | R2: W1, p2 | R3: W1, p3 | R4: W1, p4 | G: none, then vmcnt(0)
      // The drain at the end of G (behind ~600 cycles of GEGLU arithmetic: what is in flight was requested at least an
      // MFMA segment earlier) retires the whole W2 slice and the two K-tiles requested ahead.  The wait at the end of R_s
      // retires W1 K-tile q+1; what may stay in flight is what was requested after it:
      //     s = 0: W1 = 2 | s = 1: W1, p0, p1 = 4 | s = 2: p0, p1, W1, p2 = 5 | s = 3: p2, W1, p3 = 4 | s = 4: p3, W1, p4 = 4
      ff1_step(ic<0>{});
      ff1_step(ic<1>{});
      ff1_step(ic<2>{});
      ff1_step(ic<3>{});
      ff1_step(ic<4>{});
      // ---- G: GEGLU on the accumulators -> the wave's 32 x 32 hidden values, bf16, into the chunk buffer (A layout of ff2)
      {
        const int gl = l0_lane_now();                               // afresh: nothing hoisted out of the chunk loop
        const int frow = gl & 31, fhalf = gl >> 5;
        const int pr = c * 128 + wn * 64 + (frow >> 4) * 32 + (frow & 15);   // pack_geglu row of this lane's value; gate 16 on
        const float bv = bl[pr], bg = bl[pr + 16];
        // the wave's block is columns wn * 32 .. + 32 of the chunk buffer (fused_l0.h L0Scatter)
        const L0Scatter sc(smem + FF_H_OFF + (c & 1) * FF_H_BYTES + wm * 32 * 128, wn * 32 + frow, fhalf);
#pragma unroll
        for (int r = 0; r < 16; r += 2) {                             // register pairs (rows cr, cr + 1): packed fp32 arithmetic
          const tc_f32x2 v = {acc_v[r] + bv, acc_v[r + 1] + bv};
          const tc_f32x2 g = {acc_g[r] + bg, acc_g[r + 1] + bg};
          const tc_f32x2 h = (ABL & 1) ? v * g : v * gelu_erf_f2(g);
          bf16_t* const dst = sc.at(r);
          dst[0] = (bf16_t)h[0];
          dst[64] = (bf16_t)h[1];                                     // the next row: + 128 bytes
          if ((r + 2) % GI == 0) __builtin_amdgcn_sched_barrier(0);   // GI values in flight: the chain of a GELU is ~20 dependent instructions
        }
        ++cw2;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the hidden values are in LDS, the W2 slice has landed
        bar();
      }
      // ---- X: the other group's G -- its threads' pieces of the W2 slice are only known to have landed after ITS drain --
      // an empty interval for this group (the hidden rows a group reads are written by that group alone)
      bar();
      // ---- ff2: [32 x 64] hidden (A, from LDS) x W2 slice [160 x 64] (B, from LDS) -> out_acc, 20 MFMAs
      {
        const char* hb = smem + FF_H_OFF + (c & 1) * FF_H_BYTES + h_row();
        const char* wb = smem + FF_W2_OFF + w2_row();
        l0_second_product<(ABL & 8) != 0>(hb, wb, frow, fhalf, out_acc, bar);
      }
    }

    l0_realign(grp);
    // ---- epilogue: + b2 + residual (the raw rows), bf16.  Per wave six passes of (16 rows x 64 columns) through a
    // private 4 KiB slab carved from the hidden-chunk buffers: wave (wm, wn) takes buffer wn, rows wm*32..+32 -- rows only
    // its own group reads, and this group's last read of them is behind it
    {
      float* slab = reinterpret_cast<float*>(smem + FF_H_OFF + wn * FF_H_BYTES + wm * 32 * 128);
      l0_epilogue(slab, out_acc, lane, wm, wn, bl + 2 * FF_H, p.x, p.ldx, p.out, p.ldo,
                  [&](int tr, int64_t& m) { m = tile * FF_BM + tr; return m < p.m; });
    }
  }
  tc_wait_vmcnt<0>();                               // the stream ran ahead: nothing may land in LDS after the block is gone
}

int ff_mode() {        // TC_FF_FUSED = 0 never | 1 (default) whenever the shape is the level-0 block's; read per call
  return l0_env_int("TC_FF_FUSED", 1);
}

}  // namespace

extern "C" int tc_ff_geglu_fused_eligible(const TcFfParams* p) {
  if (!p || ff_mode() == 0) return 0;
  if (p->c != FF_C || p->hidden != FF_H || p->m <= 0) return 0;
  return l0_rows_ok(p->ldx, p->ldo, p->m, p->ldx);
}

extern "C" int tc_ff_geglu_fused(const TcFfParams* p, void* stream) {
  if (!p) return TC_EINVAL;
  if (const int rc = l0_check_call(p->x, p->w1, p->b1, p->w2, p->b2, p->out, tc_ff_geglu_fused_eligible(p))) return rc;
  FfArgs a;
  a.x = reinterpret_cast<const bf16_t*>(p->x); a.w1 = reinterpret_cast<const bf16_t*>(p->w1); a.b1 = p->b1;
  a.w2 = reinterpret_cast<const bf16_t*>(p->w2); a.b2 = p->b2; a.out = reinterpret_cast<bf16_t*>(p->out);
  a.m = p->m; a.ldx = p->ldx; a.ldo = p->ldo; a.ln = p->ln ? 1 : 0; a.eps = p->ln_eps;
  a.tiles = (p->m + FF_BM - 1) / FF_BM;
#ifdef TC_TIMING_BUILDS      /* interval trace / timing ablations: WRONG results by construction, never in the product library */
  a.trace = l0_trace_ptr("TC_FF_TRACE");
#else
  a.trace = nullptr;
#endif
  const int grid = l0_grid(a.tiles, "TC_FF_GRID");
#ifdef TC_TIMING_BUILDS
  const int abl = l0_env_int("TC_FF_ABLATE", 0);
#endif
  const int gi = l0_env_int("TC_FF_GILP", 8), la = l0_env_int("TC_FF_LOOKAHEAD", 3);
  const dim3 g((unsigned)grid), b(FF_THREADS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define FF_LAUNCH(LA_, ABL_) hipLaunchKernelGGL((ff_fused_kernel<LA_, ABL_, 2>), g, b, 0, st, a)
#ifdef TC_TIMING_BUILDS
  if (abl == 1) FF_LAUNCH(3, 1);
  else if (abl == 2) FF_LAUNCH(3, 2);
  else if (abl == 3) FF_LAUNCH(3, 3);
  else if (abl == 12) FF_LAUNCH(3, 12);
  else if (abl == 15) FF_LAUNCH(3, 15);
  else if (abl == 16 && a.trace) FF_LAUNCH(3, 16);
  else
#endif
  if (gi == 2) FF_LAUNCH(3, 0);
  else if (la == 2) FF_LAUNCH(2, 0);
  else if (la == 4) hipLaunchKernelGGL((ff_fused_kernel<4, 0, 8>), g, b, 0, st, a);
  else hipLaunchKernelGGL((ff_fused_kernel<3, 0, 8>), g, b, 0, st, a);       // the product kernel
#undef FF_LAUNCH
  TC_LAUNCH_CHECK();
  return TC_OK;
}
