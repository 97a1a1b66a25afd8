// Tap-reuse convolutions on 160x160 tiles, gfx950: the 3x3 (stride 1, pad 1) and the temporal (3,1,1) convolutions of the
// UNet with the A operand of ALL taps read from ONE halo patch in LDS.  Written in round 4 without GPU access (index
// arithmetic checked on the CPU: tests/test_conv_halo_cpu.py, tests/conv_halo_host_check.cpp); first executed in round 5, where
// all of its GPU tests passed on the first run (profiles/r05_pytest_conv_halo_first_gpu_run.log).  MEASURED
// (profiles/r05_conv_halo_bench.txt, r05_halo3x3_clip_ab.txt, r05_fuse_clip_ab.txt; same process / same lease, interleaved):
//   3x3, level 0 / 1 (1024 / 512 patches):  1.03-1.07x the 160-tile implicit GEMM (tall patches 1.06-1.10x)
//   3x3, level 2 (256 patches, K split inside the block):  1.15-1.27x
//   temporal (3,1,1):  0.98x / 0.98x / 0.93x / 0.50x at levels 0 / 1 / 2 / 3 -- three taps re-use too little
//   a clip with the 3x3 convolutions here: 8.29 / 8.30 vs 8.20 / 8.21 frames/s (+1.1 %)
// so the ROUTING is: 3x3 convolutions of UNet levels 0-2 by default; the temporal geometry only on request
// (TC_CONV_HALO_T3=1) and in the strict test mode.  Round 4 PREDICTED 1.3x from an additive model of the request traffic
// (docs/LAB_NOTEBOOK.md 5.5 (11)); the A bytes fell 6.7x as designed and the time fell 5 %: the 160-tile K loop was not waiting for
// those bytes.  The GroupNorm prologue this kernel carried (ABI 10, tc_conv_gn_bf16: normalise the halo in registers)
// was parity-green and LOST 4 % of a clip (7.80 / 7.81 vs 8.15 / 8.18 frames/s: +8 % convolution time for -0.7 ms of
// GroupNorm, whose statistics pass + finalize stay): removed in ABI 11.
//
// Why.  The implicit-GEMM kernels (gemm16.hip) request the A tile once per K-step = once per (tap, 64 channels): every
// input pixel goes L2 -> LDS nine times per output-column tile (three times for the temporal taps).  The timing builds
// of round 4 (profiles/r04_g16_ablate.txt) say what that costs on the level-0 3x3 convolution: 145 us with all
// requests, 104 without A's, 91 without any -- and the chip's L2->LDS path delivers 12.6-18 TB/s inside a GEMM against
// the 31 TB/s a 160x160x64 step needs at the MFMA roof (docs/LAB_NOTEBOOK.md 5.5).  Here a block owns a 2-D PATCH of the output:
//   3x3     : 10 image rows x 16 pixels of one frame        -> halo 12 x 18 = 216 pixels
//   temporal: 10 consecutive pixels x the clip's 16 frames  -> halo 10 x 18 = 180 (frames -1 and 16 are the zero padding)
// = 160 GEMM rows either way, tile row = 16 y + x, so one 16-row MFMA block is one image row (one pixel's frames).  Per
// 64-channel chunk the halo patch is brought in ONCE (216 x 128 B instead of 9 x 160 x 128 B: 6.7x fewer A bytes; 2.7x
// for the temporal taps) and the K loop runs chunk-major: for each chunk, for each tap, 50 MFMAs per wave against the
// W tile of (tap, chunk) -- the same packed weights, visited in another order (k0 = tap * cin + 64 chunk).
//   * A fragments of tap (ty, tx): halo pixel hp = (y + ty) * 18 + (x + tx), i.e. the 16 lanes of an MFMA row block read
//     16 CONSECUTIVE halo pixels from an arbitrary base.  The 16-byte segment index is XOR-swizzled by (hp & 7): every
//     ds_read_b128 lane group then touches 16 distinct bank slots for every base (gemm16's (row >> 1) & 7 is conflict-free
//     for 16-aligned bases only; both checked by brute force in the CPU test).
//   * The halo goes through REGISTERS (7 buffer_load_dwordx4 per thread and chunk, requested at the start of the chunk's
//     last tap, written with ds_write_b128 behind that step's barrier): a DMA fill would have to wait until the last
//     fragment of the old chunk is read and would expose its whole latency once per chunk; a second halo buffer would
//     cost the second resident block (LDS: 28 KiB halo + 2 x 20 KiB W stages = 68 KiB, two blocks per CU).
//   * W tiles: LDS-DMA from inline asm into two stages, one K-step ahead (gemm_persist.h g8_dma16), vmcnt(0) + barrier
//     per step -- the plain loop; the interleaved loops of gemm16 can follow once this one is measured.
//   * Epilogue: gemm16's (gemm_epilogue.h epi_slab_pass16: per-wave fp32 slab, 16-byte row vectors, bias / row bias /
//     activation / residual), with the tile row -> output row map of the patch.
// Summation order over K differs from the implicit GEMM's (chunk-major instead of tap-major): results agree to fp32
// rounding of the accumulators, not bit for bit.
#include "gemm_persist.h"
#include "gemm_epilogue.h"

#include "conv_halo_index.h"

namespace {

// every address formula of the kernel lives in conv_halo_index.h (namespace chx), shared with the host-side check
constexpr int CH_BN = chx::BN, CH_WT = chx::WT, CH_NT = chx::NT;
constexpr int CH_HX = chx::HX;                             // halo patch width (16 + 2) for both geometries
constexpr int CH_W_STAGE = chx::W_STAGE;                   // 20 KiB
constexpr int CH_NV = chx::NV;                             // halo vectors per thread and chunk: ceil(216 * 8 / 256) = ceil(396 * 8 / 512)
static_assert(chx::GATHER_3x3 == TC_GATHER_CONV3x3 && chx::GATHER_T3 == TC_GATHER_CONVT3 && chx::BK == TC_BK && chx::OOB == TC_OOB && chx::BN == TC_T16, "conv_halo_index.h");
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// WM = waves along M: 2 = the 160-row patch (PY = 10 patch rows, 4 waves, two blocks per CU); 4 = a TALL 320-row patch
// (PY = 20, 8 waves, one block per CU; TC_CONV_HALO_TALL): the halo makes A rows nearly free -- 22 x 18 halo pixels per
// chunk and NINE K-steps -- so the W tile is what a K-step pays for, and a tall block requests it once for twice the rows:
// 25.6 KiB per 320 x 160 x 64 step, 9.8 TB/s chip-wide at the MFMA roof (the 160-row patch: 18; the implicit GEMM: 31).
template <int GATHER, int WM>
using ChGeo = chx::Shape<GATHER, WM>;                      // TAPS, PY, HY, NPIX, THREADS, A_BYTES, RSTEP, RB, PIECE

// KS = 2 (TC_CONV_HALO_KSPLIT, WM = 2 only): the K loop split over TWO 4-wave groups inside one 8-wave block -- for the
// launches whose patches do not fill the chip (level 2: 256 tiles on 256 CUs = one 4-wave block per CU, one MFMA wave per
// SIMD, which reaches 45 % of the matrix pipe where two reach 70 %: docs/LAB_NOTEBOOK.md 5.5).  Group g owns the channel chunks
// [g nch / 2, (g + 1) nch / 2) with its OWN halo buffer and W stages (2 x 68 KiB of LDS), both groups run the same loop in
// lockstep (the barriers are the block's), and at the end group 1 hands its accumulators to group 0 through LDS (fixed
// order: acc0 + acc1), which runs the epilogue.  Unlike the split over blocks (TC_GEMM_SPLITK) no fp32 partial tile
// reaches memory and no second kernel runs.
constexpr int CH_RED_OFF = 32 * 1024;                      // the hand-over area starts behind group 0's epilogue slabs
constexpr int CH_RED_BYTES = 4 * CH_NT * CH_NT * 4 * 64 * 4;       // 4 waves x 25 MFMA tiles x 4 registers x 64 lanes x fp32 = 100 KiB

template <int GATHER, int WM, int KS>
__global__ __launch_bounds__(128 * WM * KS, (WM == 2 && KS == 1) ? 2 : 1) void conv_halo_kernel(const TcGemmParams p, const int order) {
  using G = ChGeo<GATHER, WM>;
  static_assert(KS == 1 || WM == 2, "the K split runs two 4-wave groups");
  constexpr int CH_A_BYTES = G::A_BYTES;
  constexpr int PY = G::PY;
  constexpr int GROUP_BYTES = CH_A_BYTES + 2 * CH_W_STAGE;
  constexpr int SMEM_BYTES = KS == 1 ? GROUP_BYTES : (KS * GROUP_BYTES > CH_RED_OFF + CH_RED_BYTES ? KS * GROUP_BYTES : CH_RED_OFF + CH_RED_BYTES);
  __shared__ __attribute__((aligned(1024))) char smem[SMEM_BYTES];

  const int lane = threadIdx.x & 63;
  const int grp = KS == 1 ? 0 : (int)threadIdx.x / G::THREADS;            // wave-uniform: a group is four whole waves
  const int grp_u = __builtin_amdgcn_readfirstlane(grp);
  const int tid = threadIdx.x - grp * G::THREADS;                         // thread within its group
  const int wave = tid >> 6;                                              // wave within its group
  const int wm = wave >> 1, wn = wave & 1;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  char* const sA = smem + grp_u * GROUP_BYTES;
  char* const sW = sA + CH_A_BYTES;

  // ---- block -> patch
  const int hw = p.h_out * p.w_out;
  const int tiles_n = p.n / CH_BN;
  const int tiles_m = chx::tiles_m<GATHER, WM>(p.frames, p.h_out, p.w_out);
  int tile_m, tile_n;
  tc_tile_of_block(blockIdx.x, tiles_m, tiles_n, order, tile_m, tile_n);
  if (tile_m >= tiles_m) return;
  const chx::Patch pt = chx::patch_of<GATHER, WM>(tile_m, p.h_out, p.w_out);
  const int img = pt.img;
  const int64_t m00 = pt.m00, row_lo = pt.row_lo;            // first output row; lowest source row (the SRD of A starts there)
  const int ys = pt.ys, xs = pt.xs;                          // output row of patch position (y, x): m00 + y ys + x xs

  const int64_t bz = blockIdx.z;
  const tc_rsrc_t a_rsrc = tc_a_rsrc(p, bz, row_lo);
  const g8_srd_t w_srd = g8_make_srd(reinterpret_cast<const bf16_t*>(p.w) + bz * p.stride_w, tc_w_extent(p));
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem + (uint32_t)(grp_u * GROUP_BYTES);

  // ---- halo vectors of this thread: v = tid + THREADS i -> halo pixel v >> 3, 16-byte segment v & 7 (8 lanes = one pixel's
  // 128 bytes: coalesced source lines, conflict-free ds_write_b128 groups)
  uint32_t hv_off[CH_NV];
  int hv_lds[CH_NV];                                       // -1: no such pixel
#pragma unroll
  for (int i = 0; i < CH_NV; ++i) {
    const chx::HaloVec hvv = chx::halo_vec<GATHER, WM>(pt, tid, i, p.h_in, p.w_in, p.lda);     // (h_in = h_out, w_in = w_out: host)
    hv_off[i] = hvv.off;
    hv_lds[i] = hvv.lds;
  }
  u32x4 hv[CH_NV];
  auto load_halo = [&](int chunk_idx) {
    const uint32_t soff = (uint32_t)chunk_idx * (TC_BK * 2);
#pragma unroll
    for (int i = 0; i < CH_NV; ++i) hv[i] = buf_load16(a_rsrc, hv_off[i], soff);
  };
  auto store_halo = [&]() {
#pragma unroll
    for (int i = 0; i < CH_NV; ++i)
      if (hv_lds[i] >= 0) *reinterpret_cast<u32x4*>(sA + hv_lds[i]) = hv[i];
  };

  // ---- W tile requests: thread -> (row lrow + RSTEP i, 16-byte chunk), the swizzle on the SOURCE chunk (gemm16.hip).
  // The tall block's third pass covers rows 128..191 of a 160-row tile: waves 4..7 have no rows there and request nothing
  // (every wait of this loop is vmcnt(0): the waves need not issue equal numbers of requests)
  constexpr int RSTEP = G::RSTEP, RB = G::RB, PIECE = G::PIECE;      // 32 | 64 rows per pass, 5 | 3 passes
  const int lrow = chx::w_lrow(tid);
  const int wchunk = chx::w_chunk(tid);
  uint32_t b_voff[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const int nl = lrow + RSTEP * i;
    const int n = tile_n * CH_BN + nl;
    b_voff[i] = (nl < CH_BN && n < p.n) ? (uint32_t)((int64_t)n * p.ldw * 2 + wchunk * 16) : TC_OOB;
  }
  auto request_w = [&](int k0, int stage) {
    const uint32_t dst = lds0 + (uint32_t)(CH_A_BYTES + stage * CH_W_STAGE + wave_u * 1024);
    const uint32_t soff = (uint32_t)k0 * 2u;
#pragma unroll
    for (int i = 0; i < RB; ++i)
      if (chx::w_pass_live<WM>(i, wave_u)) g8_dma16(w_srd, dst + i * PIECE, b_voff[i], soff);
  };

  f32x4_t acc[CH_NT][CH_NT];
#pragma unroll
  for (int i = 0; i < CH_NT; ++i)
#pragma unroll
    for (int j = 0; j < CH_NT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // v_mfma_f32_16x16x32_bf16 operands: lane holds row (lane & 15) of a 16-row block, k = 8 (lane >> 4) .. +7 of the slice
  const int frow = lane & 15;
  const int fq = lane >> 4;
  int hp0[CH_NT], b_off[CH_NT];
#pragma unroll
  for (int i = 0; i < CH_NT; ++i) {
    hp0[i] = chx::frag_a_hp0(wm, i, frow);                 // halo pixel of (y = 5 wm + i, x = frow) for tap (0, 0)
    b_off[i] = chx::frag_b_off(wn, i, frow);
  }

  auto compute = [&](int stage, int shift) {
    const char* sb = sW + stage * CH_W_STAGE;
    int a_addr[CH_NT];
#pragma unroll
    for (int i = 0; i < CH_NT; ++i) a_addr[i] = chx::frag_a_addr(hp0[i], shift, fq);      // K-slice 0; slice 1 = this ^ 64
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[CH_NT], bf[CH_NT];
      const int cb = chx::frag_b_chunk(wn, frow, fq, ks);
#pragma unroll
      for (int i = 0; i < CH_NT; ++i) af[i] = *reinterpret_cast<const bf16x8*>(sA + (a_addr[i] ^ (ks << 6)));
#pragma unroll
      for (int j = 0; j < CH_NT; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(sb + b_off[j] + cb);
#pragma unroll
      for (int i = 0; i < CH_NT; ++i)
#pragma unroll
        for (int j = 0; j < CH_NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  // ---- K loop, chunk-major: step kb = (chunk c, tap t); W(kb + 1) is requested while step kb computes
  const int nch = (p.cin / TC_BK) / KS;                    // chunks of this group (KS = 2: cin / 64 is even -- host)
  const int c0 = grp_u * nch;                              // its first chunk
  const int nk = G::TAPS * nch;
  request_w(chx::w_k0(0, c0, p.cin), 0);
  load_halo(c0);
  store_halo();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int c = 0, tap = 0, ty = 0, tx = 0;                      // tap = 3 ty + tx (3x3) | tx (temporal)
  for (int kb = 0; kb < nk; ++kb) {
    const int st = kb & 1;
    int ntap = tap + 1, nc = c, nty = ty, ntx = tx + 1;
    if (ntx == 3) { ntx = 0; nty = ty + 1; }
    if (ntap == G::TAPS) { ntap = 0; nc = c + 1; nty = 0; ntx = 0; }
    const bool more = kb + 1 < nk;
    const bool refill = more && ntap == 0;                 // block-uniform: the next step opens a new channel chunk
    if (more) request_w(chx::w_k0(ntap, c0 + nc, p.cin), st ^ 1);
    if (refill) load_halo(c0 + nc);
    compute(st, chx::tap_shift(GATHER, ty, tx));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // own pieces of W(kb + 1) (and the halo vectors) have landed
    __syncthreads();                                       // every wave's fragment reads of this step are done
    if (refill) {
      store_halo();
      __syncthreads();
    }
    tap = ntap; c = nc; ty = nty; tx = ntx;
  }

  if (KS == 2) {
    // group 1 -> group 0: [wave][tile][register][lane] fp32, a lane's values 256 bytes apart (conflict-free both ways)
    float* red = reinterpret_cast<float*>(smem + CH_RED_OFF) + wave * (CH_NT * CH_NT * 4 * 64) + lane;
    if (grp_u == 1) {
#pragma unroll
      for (int i = 0; i < CH_NT; ++i)
#pragma unroll
        for (int j = 0; j < CH_NT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) red[((i * CH_NT + j) * 4 + r) * 64] = acc[i][j][r];
    }
    __syncthreads();
    if (grp_u == 1) return;
#pragma unroll
    for (int i = 0; i < CH_NT; ++i)
#pragma unroll
      for (int j = 0; j < CH_NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += red[((i * CH_NT + j) * 4 + r) * 64];
  }

  // ---- epilogue: per wave, five passes of one 16-row MFMA block through a private fp32 slab [16][80] (epi_slab_pass16),
  // tile row 16 y + x -> output row m00 + y ys + x xs
  float* slab = reinterpret_cast<float*>(smem) + wave * (16 * CH_WT);
  const bf16_t* res_base = p.residual ? reinterpret_cast<const bf16_t*>(p.residual) + bz * p.stride_c : nullptr;
  char* c_base = reinterpret_cast<char*>(p.c) + bz * p.stride_c * (p.out_f32 ? 4 : 2);
  const int col_w0 = tile_n * CH_BN + wn * CH_WT;
  auto epi_pass = [&](auto I_) {
    constexpr int i = decltype(I_)::value;
    epi_slab_pass16<CH_NT>(p, slab, acc[i], lane, frow, fq, col_w0, c_base, res_base,
                           [&](int lr) { return (int)chx::out_row(pt, wm, i, lr); }, [](int, const u32x4&) {});
  };
  epi_pass(ic<0>{});
  epi_pass(ic<1>{});
  epi_pass(ic<2>{});
  epi_pass(ic<3>{});
  epi_pass(ic<4>{});
}

}  // namespace

void tc_conv_halo_launch(const TcGemmParams& p, const TcGemmRoute& r, hipStream_t s) {
  const dim3 grid(r.grid[0], r.grid[1], r.grid[2]), block(r.block);
  const auto go = [&](auto g) {
    constexpr int G = decltype(g)::value;
    if (r.wm == 4) hipLaunchKernelGGL((conv_halo_kernel<G, 4, 1>), grid, block, 0, s, p, r.order);
    else if (r.ks == 2) hipLaunchKernelGGL((conv_halo_kernel<G, 2, 2>), grid, block, 0, s, p, r.order);
    else hipLaunchKernelGGL((conv_halo_kernel<G, 2, 1>), grid, block, 0, s, p, r.order);
  };
  if (p.gather == TC_GATHER_CONV3x3) go(std::integral_constant<int, TC_GATHER_CONV3x3>{});      // two gathers only: no linear form
  else go(std::integral_constant<int, TC_GATHER_CONVT3>{});
}
