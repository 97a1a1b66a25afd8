// Fused temporal self-attention of a level-0 transformer block, gfx950:
//
//     out = x + Wo . Attn_frames( Wqkv . LayerNorm(x) + bqkv ) + bo        x: [B*16*HW, 320] bf16, 5 heads of 64
//
// (reference lvdm/modules/attention.py:81-144 CrossAttention over the T = 16 frames of a pixel, called from
// TemporalTransformer, attention.py:365-412, behind norm1 / norm2 of BasicTransformerBlock, attention.py:225-246).  As four
// launches -- LayerNorm(-prologue) qkv projection (81920 x 960 x 320), tc_attn_temporal, output projection + residual --
// the block writes a 157 MB qkv tensor and a 52 MB attention output to HBM and reads both back for 0.018 TFLOP of
// attention arithmetic.  Here neither exists:
//
//  * a block owns 8 consecutive pixels x 16 frames = 128 GATHERED rows (tile row = pixel * 16 + frame; a pixel's frames are
//    HW rows apart in memory, each row 640 contiguous bytes); wave (wm, wn) of its 8 waves owns rows wm*32..+32 = two pixels.
//    The rows' LayerNorm runs in registers on the MFMA A-operand layout and stays there for the whole tile;
//  * the five heads are walked one after the other.  Per head two "stages" of five K-steps against [128 rows x 64 k] tiles
//    of Wqkv: stage A = the head's 64 q rows | its 64 k rows (waves wn = 0 produce q, wn = 1 produce k, 8 MFMAs per K-step),
//    stage B = its 64 v rows (waves wn = 0 only).  q and k go to LDS row-major, v TRANSPOSED ([64 dims][128 rows], the B
//    operand of P.V); then every wave runs the attention of ONE pixel (wave (wm, wn): pixel 2 wm + wn) on 16x16x32 MFMAs:
//    S^T = K Q^T (a lane owns one query: softmax reductions in-lane + two cross-row swaps), P re-laid as the A operand by
//    permlane swaps, O = P V, written as bf16 in A layout over the head's q rows (attn_frames16.h tc_attn_frames16); then
//    20 MFMAs of the output projection against Wo's [320 x 64] slice into the wave's 32 x 160 output accumulators, which
//    live across the heads;
//  * weights (819 KB, L2-resident) stream by LDS-DMA from inline asm: Wqkv K-tiles through a ring of three 16 KiB stages
//    (requested two steps ahead; the stream runs on across heads and tiles), Wo's slice once per head in five pieces;
//    every wait is a hand-counted vmcnt;
//  * the two wave groups (wm >> 1: one wave per SIMD each) run one barrier interval apart, as in gemm8.hip.
//
// What this kernel shares with ff_fused.hip is stated once, in csrc/fused_l0.h; this file keeps the LDS map, the weight-stream
// schedule with its counted waits, the v^T write-out and the attention between the two products.
// LDS: W ring 48 KiB | Wo slice 40 | q (then the head's output) 16 | k 16 | v^T 17 | biases 5 | parked A fragments 12 = 154 KiB.
// Roundings: LayerNorm output, q / k / v, the softmax weights and the attention output in bf16, sums in fp32 -- the
// roundings of the four launches (tc_attn_temporal keeps its softmax weights in fp32: the one difference).
#include "fused_l0.h"
#include "attn_frames16.h"

namespace {

constexpr int TB_C = L0_C, TB_HEADS = 5, TB_T = 16, TB_THREADS = L0_THREADS;
constexpr int TB_KT = L0_KT;                      // 5 K-steps per stage
constexpr int TB_W_STAGE = L0_W_STAGE;            // 16 KiB: 128 rows x 64 k
constexpr int TB_NRING = 3;
constexpr int TB_W_OFF = 0;
constexpr int TB_WO_OFF = TB_NRING * TB_W_STAGE;  // 40 KiB: 320 rows x 64 k
constexpr int TB_Q_OFF = TB_WO_OFF + L0_W2_BYTES; // [128 rows][64] bf16, swizzled (fused_l0.h)
constexpr int TB_K_OFF = TB_Q_OFF + L0_BUF_BYTES;
constexpr int TB_VT_OFF = TB_K_OFF + L0_BUF_BYTES;   // [64 dims][128 rows + 8] bf16: 272-byte rows (conflict-free 16-lane reads)
constexpr int TB_VT_LD = 272;
constexpr int TB_B_OFF = TB_VT_OFF + 64 * TB_VT_LD;          // bqkv (960 fp32) | bo (320 fp32)
constexpr int TB_P_OFF = TB_B_OFF + (3 * TB_C + TB_C) * 4;   // the parked A fragments
constexpr int TB_LDS = TB_P_OFF + L0_PARK_BYTES;
static_assert(TB_LDS <= 160 * 1024, "LDS");
static_assert(TB_VT_OFF + 64 * TB_VT_LD - TB_K_OFF >= 8 * 4096, "epilogue slabs live in the k / v^T buffers");

struct TbArgs {
  const bf16_t* x; const bf16_t* wqkv; const float* bqkv; const bf16_t* wo; const float* bo; bf16_t* out;
  int hw, ldx, ldo, ln;
  float eps, scale_log2e;
  int tiles, tiles_per_b;
  int abl;          // timing ablations (TC_TB_ABLATE; wrong results): 1 no head loop (row loads, LayerNorm, epilogue only), 2 no row loads, 4 no epilogue, 8 interval trace (TC_TB_TRACE)
  unsigned long long* trace;   // TC_TB_TRACE (with TC_TB_ABLATE bit 8): s_memtime after every barrier of block 0's waves 0 and 4
  int stagger;      // TC_TB_STAGGER: block i starts (i & 3) * stagger * ~3.4 us late (de-phases the blocks' memory phases)
};

template <bool TRACE>
__global__ __launch_bounds__(TB_THREADS, 2) void tb_fused_kernel(const TbArgs p) {
  __shared__ __attribute__((aligned(1024))) char smem[TB_LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave_u >> 1, wn = wave_u & 1;
  const int grp = wave_u >> 2;                   // = wm >> 1: waves w and w + 4 share a SIMD, one of each group
  const int frow = lane & 31, fhalf = lane >> 5;

  const g8_srd_t w_srd = g8_make_srd(p.wqkv, (int64_t)3 * TB_C * TB_C * 2);
  const g8_srd_t wo_srd = g8_make_srd(p.wo, (int64_t)TB_C * TB_C * 2);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  l0_stage_biases(reinterpret_cast<float*>(smem + TB_B_OFF), p.bqkv, 3 * TB_C, p.bo, TB_C, tid);

  // ---- weight stream (lane map: fused_l0.h).  Wqkv and Wo both have 320-element rows, so one per-lane offset serves both
  const uint32_t voff = l0_stream_voff(l0_stream_row(tid), TB_C, tid);
  const uint32_t dma_dst = l0_stream_dst(lds0, wave_u);
  // K-tile q of the cyclic stream (50 per tile: head h = q / 10, stage (q % 10) / 5, K-step q % 5) -> ring stage q % 3.
  // Stage A: rows 0..63 <- the head's q rows (h*64 ..), rows 64..127 <- its k rows (320 + h*64 ..): two pieces per thread;
  // stage B: rows 0..63 <- its v rows (640 + h*64 ..): one piece
  auto dma_w = [&](int q) {
    const int qq = q % (TB_HEADS * 2 * TB_KT);
    const int h = qq / (2 * TB_KT), r = qq - h * 2 * TB_KT;
    const int kt = r < TB_KT ? r : r - TB_KT;
    const uint32_t dst = dma_dst + TB_W_OFF + (q % TB_NRING) * TB_W_STAGE;
    if (r < TB_KT) {
      const uint32_t so = (uint32_t)((h * 64 * TB_C + kt * TC_BK) * 2);
      g8_dma16(w_srd, dst, voff, so);
      g8_dma16(w_srd, dst + 8192, voff, so + TB_C * TB_C * 2);
    } else {
      const uint32_t so = (uint32_t)(((2 * TB_C + h * 64) * TB_C + kt * TC_BK) * 2);
      g8_dma16(w_srd, dst, voff, so);
    }
  };
  auto dma_wo = [&](int h, int piece) {             // rows 64 piece .. +64 of Wo's slice for head h (columns h*64 .. +64)
    const uint32_t so = (uint32_t)((piece * 64 * TB_C + h * 64) * 2);
    g8_dma16(wo_srd, dma_dst + TB_WO_OFF + piece * 8192, voff, so);
  };

  bf16x8 xa[L0_NRES];                               // the tile's normalised rows: K-slices 0 .. L0_NRES-1 (the rest parked in LDS)
  char* const park = smem + TB_P_OFF + wm * 1024 + lane * 16;
  f32x16 out_acc[5];
  f32x16 acc_v, acc_g;                              // the stage's 32 x 64 block of the wave: columns 0..31 | 32..63

  // TRACE build (abl bit 8): per-interval timing.  Block 0, waves 0 (group 0) and 4 (group 1), second tile, first two heads: the shader clock
  // after every barrier -> trace[wave >> 2][n] (a store per barrier: the timed build is not the product kernel's schedule to the
  // cycle, its waits are the same)
  int tr_n = 0;
  bool tr_on = false;
  auto bar = [&]() { l0_bar<TRACE>(p.trace, wave_u, lane, tr_on, tr_n); };
  for (int i = (blockIdx.x & 3) * p.stagger; i > 0; --i) __builtin_amdgcn_s_sleep(127);
  int q = 0;                                        // K-tile stream position consumed next
  dma_w(0);
  dma_w(1);
  tc_wait_vmcnt<0>();
  g8_barrier();

  const float* bl = reinterpret_cast<const float*>(smem + TB_B_OFF);

  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int bb = tile / p.tiles_per_b;
    const int p0 = (tile - bb * p.tiles_per_b) * 8;
    // tile row lr = pixel * 16 + frame -> memory row (bb * 16 + frame) * hw + p0 + pixel
    auto grow = [&](int lr) { return (int64_t)(bb * TB_T + (lr & 15)) * p.hw + p0 + (lr >> 4); };
    l0_rows_prologue(p.x + grow(wm * 32 + frow) * p.ldx, fhalf, !(p.abl & 2), p.ln, p.eps, xa, park);
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) out_acc[j][r] = 0.f;

    l0_stagger(grp);
    for (int h = (p.abl & 1) ? TB_HEADS : 0; h < TB_HEADS; ++h) {
      if constexpr (TRACE) tr_on = blockIdx.x == 0 && (wave_u & 3) == 0 && tile == (int)(blockIdx.x + gridDim.x) && h < 2;
      // ---- one K-step of a stage: fragments of W K-tile q (ring stage q % 3), K-tile q + 2 and this step's share of Wo's
      // slice requested, 8 MFMAs.  Requests per head in program order (pieces per thread):
      //   A0: W 2 | A1: W 2 | A2: W 2 | A3: W 1 | A4: W 1 | B0: W 1 | B1: W 1, p0, p1 | B2: W 1, p2 | B3: W 2, p3 | B4: W 2, p4
      // (the tile requested at step pos is pos + 2: a stage-A tile has two pieces, a stage-B tile one); everything is
      // drained at the end of the v write-out.  The wait at the end of a step's read segment retires K-tile q + 1 (requested
      // one step earlier, first in that step's requests); what may stay in flight is what was requested after it:
      //   A0 2 | A1 2 | A2 2 | A3 1 | A4 1 | B0 1 | B1 3 | B2 4 | B3 4 | B4 4
      auto step = [&](auto STAGE_, auto S_) {
        constexpr int stage = decltype(STAGE_)::value, s = decltype(S_)::value;
        const bool act = stage == 0 || wn == 0;       // stage B: the k-side waves have no columns
        const char* st = smem + TB_W_OFF + (q % TB_NRING) * TB_W_STAGE + (wn * 64 + frow) * 128;
        bf16x8 bw[2][4];
        if (act) l0_read_bw(st, frow, fhalf, bw);
        dma_w(q + 2);
        if (stage == 1 && s == 1) { dma_wo(h, 0); dma_wo(h, 1); }
        if (stage == 1 && s >= 2) dma_wo(h, s);
        constexpr int pos = stage * 5 + s;
        constexpr int keep = pos <= 2 ? 2 : (pos <= 5 ? 1 : (pos == 6 ? 3 : 4));
        tc_wait_vmcnt<keep>();
        bar();
        __builtin_amdgcn_s_setprio(1);
        if (act) l0_mm4<s>(xa, park, bw, acc_v, acc_g);
        __builtin_amdgcn_s_setprio(0);
        bar();
        ++q;
      };
      // ---- write-out of a stage's block: + bias, bf16 (the lane id afresh: nothing hoisted out of the head loop).  q / k:
      // row-major [128][64], swizzled: columns frow | 32 + frow of the wave's rows (fused_l0.h L0Scatter); v: transposed,
      // [64 dims][128 rows], four consecutive rows of a lane as one 8-byte store
      auto write_qk = [&]() {
        const int gl = l0_lane_now();
        const int fr = gl & 31, fh = gl >> 5;
        const float b0 = bl[wn * TB_C + h * 64 + fr], b1 = bl[wn * TB_C + h * 64 + 32 + fr];
        const L0Scatter sc(smem + (wn ? TB_K_OFF : TB_Q_OFF) + wm * 32 * 128, fr, fh);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          *sc.at(r) = (bf16_t)(acc_v[r] + b0);
          *sc.at32(r) = (bf16_t)(acc_g[r] + b1);
        }
      };
      auto write_vt = [&]() {
        if (wn != 0) return;
        const int gl = l0_lane_now();
        const int fr = gl & 31, fh = gl >> 5;
        const float b0 = bl[2 * TB_C + h * 64 + fr], b1 = bl[2 * TB_C + h * 64 + 32 + fr];
        char* const v0 = smem + TB_VT_OFF + fr * TB_VT_LD + (wm * 32 + 4 * fh) * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {                  // rows 8 i + 4 fhalf + (0..3) of the wave's 32
          uint32_t lo[2], hi[2];
          lo[0] = pack2(acc_v[4 * i] + b0, acc_v[4 * i + 1] + b0);
          lo[1] = pack2(acc_v[4 * i + 2] + b0, acc_v[4 * i + 3] + b0);
          hi[0] = pack2(acc_g[4 * i] + b1, acc_g[4 * i + 1] + b1);
          hi[1] = pack2(acc_g[4 * i + 2] + b1, acc_g[4 * i + 3] + b1);
          *reinterpret_cast<uint2*>(v0 + i * 16) = uint2{lo[0], lo[1]};
          *reinterpret_cast<uint2*>(v0 + 32 * TB_VT_LD + i * 16) = uint2{hi[0], hi[1]};
        }
      };

#pragma unroll
      for (int r = 0; r < 16; ++r) { acc_v[r] = 0.f; acc_g[r] = 0.f; }
      step(ic<0>{}, ic<0>{});
      step(ic<0>{}, ic<1>{});
      step(ic<0>{}, ic<2>{});
      step(ic<0>{}, ic<3>{});
      step(ic<0>{}, ic<4>{});
      write_qk();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      bar();
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc_v[r] = 0.f; acc_g[r] = 0.f; }
      step(ic<1>{}, ic<0>{});
      step(ic<1>{}, ic<1>{});
      step(ic<1>{}, ic<2>{});
      step(ic<1>{}, ic<3>{});
      step(ic<1>{}, ic<4>{});
      write_vt();
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // q, k, v of the head are in LDS; this thread's Wo pieces landed
      bar();

      // ---- attention of ONE pixel per wave (rows pr .. pr + 16 of the tile = its 16 frames), 16x16x32 MFMAs.
      // (The other group's Wo pieces are only known to have landed after ITS drain, one interval behind this one: this
      // interval separates that drain from the output projection's reads.)
      {
        // attn_frames16.h: S^T = K Q^T, softmax, O = P V, the head's output over its q rows in the A layout of the projection
        tc_attn_frames16(smem + TB_Q_OFF, smem + TB_K_OFF, smem + TB_VT_OFF, TB_VT_LD, wm * 32 + wn * 16, l0_lane_now(), p.scale_log2e);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bar();
      }

      // ---- output projection: [32 x 64] head output (A, from LDS) x Wo slice [160 x 64] (B, from LDS) -> out_acc, 20 MFMAs
      {
        const char* hb = smem + TB_Q_OFF + (wm * 32 + frow) * 128;
        const char* wb = smem + TB_WO_OFF + (wn * 160 + frow) * 128;
        l0_second_product(hb, wb, frow, fhalf, out_acc, bar);
      }
    }

    l0_realign(grp);
    // ---- epilogue: + bo + residual (the raw rows), bf16, through a private 4 KiB slab per wave carved from the k / v^T
    // buffers (dead: the last head's attention is behind every wave)
    {
      float* slab = reinterpret_cast<float*>(smem + TB_K_OFF + wave_u * 4096);
      if (!(p.abl & 4))
        l0_epilogue(slab, out_acc, lane, wm, wn, bl + 3 * TB_C, p.x, p.ldx, p.out, p.ldo,
                    [&](int tr, int64_t& m) { m = grow(tr); return true; });
    }
  }
  tc_wait_vmcnt<0>();                               // the stream ran ahead: nothing may land in LDS after the block is gone
}

// TC_TB_FUSED = 1 whenever the shape is the level-0 block's | 0 never (the DEFAULT since round 6); read per call.
// Rounds 4-5 shipped this kernel as the level-0 route: 1.39x the four launches it replaced (LayerNorm, qkv projection,
// tc_attn_temporal, output projection).  Round 6's csrc/qkv_attn.hip made a better THREE-launch chain of those -- LayerNorm,
// projection + attentions in one launch (72 us at this width where the two launches took 145), the weight-stationary
// output projection -- and in the same-process A/B of the guided forward that chain is ahead of this kernel on both leases
// tried: +0.57 % and +0.38 % (profiles/r06_l0_chain_vs_tb_fused_forward_ab*.txt).  This kernel is LDS-bandwidth-bound
// (header); the chain's launches are HBM-bound and each runs near its own roof.  Kept, tested, one switch away.
int tb_mode() {
  return l0_env_int("TC_TB_FUSED", 0);
}

}  // namespace

extern "C" int tc_temporal_attn_fused_eligible(const TcTbParams* p) {
  if (!p || tb_mode() == 0) return 0;
  if (p->c != TB_C || p->heads != TB_HEADS || p->t != TB_T || p->b <= 0 || p->hw <= 0 || (p->hw & 7)) return 0;
  return l0_rows_ok(p->ldx, p->ldo, (int64_t)p->b * p->t * p->hw, p->ldx > p->ldo ? p->ldx : p->ldo);
}

extern "C" int tc_temporal_attn_fused(const TcTbParams* p, void* stream) {
  if (!p) return TC_EINVAL;
  if (const int rc = l0_check_call(p->x, p->wqkv, p->bqkv, p->wo, p->bo, p->out, tc_temporal_attn_fused_eligible(p))) return rc;
  TbArgs a;
  a.x = reinterpret_cast<const bf16_t*>(p->x); a.wqkv = reinterpret_cast<const bf16_t*>(p->wqkv); a.bqkv = p->bqkv;
  a.wo = reinterpret_cast<const bf16_t*>(p->wo); a.bo = p->bo; a.out = reinterpret_cast<bf16_t*>(p->out);
  a.hw = p->hw; a.ldx = p->ldx; a.ldo = p->ldo; a.ln = p->ln ? 1 : 0; a.eps = p->ln_eps;
  a.scale_log2e = p->scale * 1.44269504088896340736f;
  a.tiles_per_b = p->hw / 8;
  a.tiles = p->b * a.tiles_per_b;
#ifdef TC_TIMING_BUILDS      /* timing ablations / interval trace: WRONG results by construction, never in the product library */
  a.abl = l0_env_int("TC_TB_ABLATE", 0);
  a.trace = l0_trace_ptr("TC_TB_TRACE");
  if (!a.trace) a.abl &= ~8;
#else
  a.abl = 0;
  a.trace = nullptr;
#endif
  a.stagger = l0_env_int("TC_TB_STAGGER", 0);
  const int grid = l0_grid(a.tiles, "TC_TB_GRID");
#ifdef TC_TIMING_BUILDS
  if (a.abl & 8) hipLaunchKernelGGL(tb_fused_kernel<true>, dim3((unsigned)grid), dim3(TB_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  else
#endif
  hipLaunchKernelGGL(tb_fused_kernel<false>, dim3((unsigned)grid), dim3(TB_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
