// The routing of tc_gemm_bf16: one switch table, one function that decides.  See gemm_route.h.
#include "gemm_route.h"

#include <stdlib.h>
#include <string.h>

namespace {

// name | default (the text an unset switch is read as; nullptr: unset has a meaning of its own) | selects among the
// implicit-GEMM kernels (the halo route then keeps out of its way) | how the text is read (i: atoi, 0: on unless it starts
// with 0, 1: off unless it starts with 1, else see tc_gemm_switches) | field | meaning.  All are read per call (tests and A/B
// scripts flip them inside one process); of TC_GEMM_ORDER / TC_GEMM_ORDER_MIB the VALUES of the first call are kept.
typedef TcGemmSwitches S;
const struct Sw { const char* name; const char* dflt; bool implicit_gemm; char kind; int S::*field; } kSwitches[] = {
    {"TC_GEMM_TILE", nullptr, false, 't', &S::tile},          // wide | 22 | 21 | 12 | 11 (b = 22, s = 11): force one tile family (tuning / A-B runs)
    {"TC_GEMM_TILE16", "1", true, 'i', &S::tile16},           // 0 never | 1 heuristic | 2 whenever the shape allows
    {"TC_GEMM8", "1", true, 'i', &S::gemm8},                  // 0 never | 1 heuristic | 2 whenever the shape allows
    {"TC_GEMM_PIPE", "1", true, 'p', &S::pipe},               // 0: one K-step in flight | 1: two on the 4-wave tiles | 2: also on the 256-row / 160 tiles
    {"TC_GEMM_SPLITK", nullptr, true, 'k', &S::splitk},       // unset (-1): heuristic | 0 never | n: force n slices (tuning)
    {"TC_GEMM_WS", "1", true, 'i', &S::ws},                   // 0 never | 1 heuristic | 2 whenever the shape allows | 3 = 2 + vmcnt(0) waits | 4 = 2 + deeper store window | 5 = 1 + deeper store window
    {"TC_G16_ILV", nullptr, true, 'l', &S::ilv},              // unset: loop 2 for convolutions, plain for linear | 0 never | 1 | 2: that loop wherever it can run
    {"TC_G16_TALL", "0", true, 'i', &S::g16_tall},            // 0 never | 1 convolutions whose tall tiles fill the CUs | 2 whenever the shape allows
    {"TC_GEMM_WIDE", "1", true, '0', &S::wide},               // 0: never the 256-row tile
    {"TC_GEMM_ORDER", "8", true, 'i', &S::order},             // chunk width of the tile walk in N-tiles (0: always the plain walk)
    {"TC_GEMM_NMAJOR", "1", true, 'i', &S::nmajor},           // 0 never | 1 heuristic | 2 always the W-stationary walk
    {"TC_GEMM_ORDER_MIB", "4", false, 'm', nullptr},          // weight size from which the chunked walk is used (4 = one XCD's L2)
    {"TC_GEMM_EPI_LATE", "0", false, '1', &S::epi_late},      // 1: epilogue operands requested inside the epilogue (A/B runs)
    {"TC_G8_GRID", "0", false, 'i', &S::g8_grid},             // n > 0: at most n blocks of the 8-wave kernel instead of one per CU
    {"TC_G8_STAGGER", "0", false, 'i', &S::g8_stagger},       // handed to the 8-wave kernel
    {"TC_CONV_HALO", "1", false, 'i', &S::halo},              // 0 never | 1 the measured routing | 2 strict (tests): whenever the shape allows, else FAIL
    {"TC_CONV_HALO_3X3", "1", false, '0', &S::halo_3x3},      // 0: mode 1 keeps the 3x3 convolutions on the implicit GEMM (A/B runs)
    {"TC_CONV_HALO_T3", "0", false, '1', &S::halo_t3},        // 1: mode 1 takes the temporal convolutions too
    {"TC_CONV_HALO_TALL", "0", false, 'i', &S::halo_tall},    // 0: 160-row patches | 1: 320-row patches where they fill the 256 CUs | 2: wherever they tile
    {"TC_CONV_HALO_KSPLIT", "1", false, 'i', &S::halo_ksplit},   // 0 never | 1: launches of at most 256 blocks (one per CU) | 2: whenever cin / 64 is even
    {"TC_GN_PART", "1", false, '0', &S::gn_part},             // 0: never emit GroupNorm statistics (A/B switch)
};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

void take(TcGemmRoute* r, int family, int64_t gx, int gy, int gz, int block) {          // the family and its launch geometry
  r->family = family, r->block = (unsigned)block;
  r->grid[0] = (unsigned)gx, r->grid[1] = (unsigned)gy, r->grid[2] = (unsigned)gz;
}

}  // namespace

TcGemmSwitches tc_gemm_switches() {
  TcGemmSwitches s{};
  for (const Sw& sw : kSwitches) {
    const char* e = getenv(sw.name);
    const char* v = e ? e : sw.dflt;
    // a switch that selects among the IMPLICIT-GEMM kernels names the kernel under test / under measurement -- but only when
    // it actually FORCES something, i.e. carries a value other than its default (an A/B script that exports
    // `TC_GEMM8=1` for one arm had every 3x3 convolution moved to another kernel in BOTH arms, silently)
    if (sw.implicit_gemm && !s.forcing_name && e && e[0] && !(sw.dflt && strcmp(e, sw.dflt) == 0)) s.forcing_name = sw.name, s.forcing_value = e;
    if (sw.kind == 'i') s.*sw.field = atoi(v);
    else if (sw.kind == '0') s.*sw.field = v[0] != '0';
    else if (sw.kind == '1') s.*sw.field = v[0] == '1';
    else if (sw.kind == 'p') s.pipe = v[0] == '0' ? 0 : v[0] == '2' ? 2 : 1;
    else if (sw.kind == 'k') s.splitk = e ? atoi(e) : -1;
    else if (sw.kind == 'l') s.ilv_set = e != nullptr, s.ilv = e ? atoi(e) : 0;
    else if (sw.kind == 'm') s.order_bytes = (int64_t)(atof(v) * (1 << 20));
    else if (e) {
      const int t = e[0] == 'w' ? 1 : e[0] == 'b' ? 22 : e[0] == 's' ? 11 : atoi(e);
      s.tile = (t == 22 || t == 21 || t == 12 || t == 11 || e[0] == 'w') ? t : 0, s.tile_set = e[0] != 0;
    }
  }
  static const TcGemmSwitches first = s;
  s.order = first.order, s.order_bytes = first.order_bytes;
  return s;
}

// Block -> tile walk (gemm_common.h tc_tile_of_block): the chunked walk when the weight matrix outgrows one XCD's L2 and
// there are enough N-tiles to chunk
int tc_gemm_tile_order(const TcGemmParams& p, int tiles_n, const TcGemmSwitches& sw) {
  return (sw.order > 0 && tiles_n >= 2 * sw.order && (int64_t)p.n * p.ldw * 2 > sw.order_bytes) ? sw.order : 0;
}

int tc_gemm_validate(const TcGemmParams& p) {
  if (!p.a || !p.w || !p.c || p.m <= 0 || p.n <= 0 || p.k <= 0) return TC_EINVAL;
  if (!aligned16(p.a) || !aligned16(p.w) || !aligned16(p.c)) return TC_EALIGN;
  if (p.residual && !aligned16(p.residual)) return TC_EALIGN;
  if ((p.k & 7) || (p.lda & 7) || (p.ldw & 7)) return TC_EALIGN;
  if (p.ldw < p.k) return TC_ESHAPE;
  const bool geglu = p.act == TC_ACT_GEGLU;
  const int n_out = geglu ? p.n / 2 : p.n;
  if ((n_out & 7) == 0) {
    if (p.out_f32 ? (p.ldc & 3) : (p.ldc & 7)) return TC_EALIGN;
    if (p.residual && (p.ldr & 7)) return TC_EALIGN;
    if (p.bias && !aligned16(p.bias)) return TC_EALIGN;
    if (p.row_bias && (!aligned16(p.row_bias) || (p.ldrb & 3))) return TC_EALIGN;
  }
  if (p.ldc < n_out || (p.residual && p.ldr < n_out)) return TC_ESHAPE;
  if (geglu && ((p.n % 128) != 0 || p.row_bias || p.residual)) return TC_ESHAPE;
  if (p.row_bias && (p.row_div <= 0 || p.ldrb < p.n)) return TC_EINVAL;
  if (p.act < TC_ACT_NONE || p.act > TC_ACT_GEGLU) return TC_EINVAL;
  if (p.gather == TC_GATHER_LINEAR) {
    if (p.lda < p.k) return TC_ESHAPE;
  } else if (p.gather == TC_GATHER_CONV3x3 || p.gather == TC_GATHER_CONVT3) {
    const int taps = p.gather == TC_GATHER_CONV3x3 ? 9 : 3;
    if (p.cin <= 0 || (p.cin % 64) != 0 || p.k != taps * p.cin || p.lda < p.cin) return TC_ESHAPE;
    if (p.frames <= 0 || p.h_out <= 0 || p.w_out <= 0) return TC_ESHAPE;
    if ((int64_t)p.frames * p.h_out * p.w_out != p.m) return TC_ESHAPE;
    if (p.gather == TC_GATHER_CONV3x3) {
      if (p.h_in <= 0 || p.w_in <= 0 || (p.stride != 1 && p.stride != 2)) return TC_ESHAPE;
      if (p.upsample && p.stride != 1) return TC_ESHAPE;
      const int hvv = p.upsample ? 2 * p.h_in : p.h_in, wvv = p.upsample ? 2 * p.w_in : p.w_in;
      if (p.pad != 0 && p.pad != 1) return TC_ESHAPE;
      // pad = 1: symmetric padding 1; pad = 0: one trailing row/column of zeros only (0,1,0,1)
      const int extra = p.pad == 1 ? 2 : 1;
      if ((hvv + extra - 3) / p.stride + 1 != p.h_out || (wvv + extra - 3) / p.stride + 1 != p.w_out) return TC_ESHAPE;
    } else {
      if (p.t_len <= 0 || (p.frames % p.t_len) != 0) return TC_ESHAPE;
    }
  } else {
    return TC_EINVAL;
  }
  // Every byte offset a tile load can form must fit the 31-bit range the out-of-range marker relies on.  For A that is the
  // span of ONE block's source rows from its tc_tile_row_lo (tiles of at most 256 output rows), not the tensor.
  int64_t span_rows = 256;
  if (p.gather == TC_GATHER_CONVT3) span_rows += 2 * (int64_t)p.h_out * p.w_out;
  else if (p.gather == TC_GATHER_CONV3x3)
    span_rows = ((int64_t)256 / (p.w_out > 0 ? p.w_out : 1) + 2) * p.stride * p.w_in + 4 * (int64_t)p.w_in + 8;
  const int64_t a_bytes = (span_rows + 1) * p.lda * 2, w_bytes = (int64_t)p.n * p.ldw * 2;
  return (a_bytes < 0x7fffff00LL && w_bytes < 0x7fffff00LL) ? TC_OK : TC_ESHAPE;
}

// ---- weight-stationary kernel (gemm_ws.hip).  One definition for the route and for the host layer that decides whether a
// LayerNorm may be folded into its consumer (tc_gemm_ws_eligible).
static bool tc_gemm_ws_takes(const TcGemmParams& p, const TcGemmSwitches& sw, int batch) {
  // TC_GEMM_TILE forces a tile family: the route then never comes here, so the host must not be told that a
  // LayerNorm may be folded into this launch (the two rules disagreed under forced-tile sweeps)
  if (sw.tile_set) return false;
  if (sw.ws == 0 || batch != 1 || p.gather != TC_GATHER_LINEAR || p.k != TC_WS_K || p.lda < TC_WS_K) return false;
  if (p.row_bias || p.alpha != 1.f || p.out_scale != 1.f || p.out_f32) return false;
  const bool geglu = p.act == TC_ACT_GEGLU;
  if (!geglu && p.act != TC_ACT_NONE) return false;
  if (p.n % (geglu ? 256 : 320) != 0) return false;
  if (p.residual && geglu) return false;
  // Heuristic (profiles/r03_ws_bench_hipblaslt_yardstick.txt, B = 2 shapes): the N = 320 projections are HBM-bound and gain
  // 1.15x (plain / + residual) to 1.53x (LayerNorm prologue instead of a LayerNorm launch); with more than one N-slab the
  // single wave per SIMD serialises LayerNorm, MFMAs and epilogue and the kernel LOSES to the tiled one (qkv 0.89x,
  // 0.67x with the prologue; GEGLU 0.61x / 0.50x), and at M = 40960 it only ties -- so: one slab, plain, M >= 64K rows.
  if ((sw.ws == 1 || sw.ws == 5) && (p.m < 65536 || geglu || p.n != 320)) return false;
  if ((int64_t)p.m * p.lda * 2 >= 0x7fffff00LL) return false;       // this kernel addresses A from the tensor base
  if ((int64_t)p.m * p.ldc * 2 >= 0x7fffff00LL || (p.residual && (int64_t)p.m * p.ldr * 2 >= 0x7fffff00LL)) return false;
  return true;
}

static void route_ws(const TcGemmParams& p, const TcGemmSwitches& sw, TcGemmRoute* r) {
  r->geglu = p.act == TC_ACT_GEGLU, r->res = p.residual != nullptr, r->ln = p.a_norm != 0;
  const int slabs = p.n / (r->geglu ? 256 : 320);
  const int ntiles = (p.m + TC_WS_ROWS - 1) / TC_WS_ROWS;
  int nchunks = 256 / slabs < 1 ? 1 : 256 / slabs;              // one block per CU
  r->nchunks = nchunks = nchunks > ntiles ? ntiles : nchunks;
  // wait mode: the heuristic (1) runs with the deeper store window (+1-6 %, profiles/r03_ws_bench_hipblaslt_yardstick.txt);
  // 2 = counted waits that also retire the stores of two tiles ago, 3 = vmcnt(0) everywhere (parity tests)
  r->safe = sw.ws == 3 ? 1 : (sw.ws == 2 ? 0 : 2);
  take(r, TC_FAM_WS, slabs * 8 * ((nchunks + 7) / 8), 1, 1, 256);
}

// ---- halo-patch convolutions (conv_halo.hip).  1 = taken, 0 = not taken, -1 = TC_CONV_HALO=2 ("strict", the parity tests)
// and a convolution was NOT taken: the call fails, so a test that passes under mode 2 has provably run this kernel and not
// a fallback.  Mode 1 (the default) is the measured routing: the 3x3 convolutions (1.03-1.27x), not the temporal ones
// (0.5-0.99x) unless TC_CONV_HALO_T3=1; TC_CONV_HALO_3X3=0 keeps the 3x3 ones on the implicit GEMM as well (A/B runs).
static int route_halo(const TcGemmParams& p, const TcGemmSwitches& sw, int batch, TcGemmRoute* r) {
  if (sw.halo == 0) return 0;
  if (p.gather != TC_GATHER_CONV3x3 && p.gather != TC_GATHER_CONVT3) return 0;
  if (sw.halo == 1) {
    if (sw.forcing_name) return r->halo_yielded = true, 0;        // keep out of the way of the kernel under measurement
    if (p.gather == TC_GATHER_CONV3x3 ? !sw.halo_3x3 : !sw.halo_t3) return 0;
  }
  const int declined = sw.halo == 2 ? -1 : 0;
  if (p.act == TC_ACT_GEGLU || p.a_norm || (p.n % TC_T16) != 0 || (p.cin % TC_BK) != 0 ||
      p.k != (p.gather == TC_GATHER_CONV3x3 ? 9 : 3) * p.cin) return declined;
  const int hw = p.h_out * p.w_out;
  int64_t tiles_m, tiles_tall = 0;                                       // 160-row patches; 320-row patches (0: do not tile)
  if (p.gather == TC_GATHER_CONV3x3) {
    if (p.stride != 1 || p.upsample || p.pad != 1 || p.h_in != p.h_out || p.w_in != p.w_out) return declined;
    if ((p.h_out % 10) != 0 || (p.w_out % 16) != 0) return declined;
    tiles_m = (int64_t)p.frames * (p.h_out / 10) * (p.w_out / 16);
    if ((p.h_out % 20) == 0) tiles_tall = tiles_m / 2;
  } else {
    if (p.t_len != 16 || (p.frames % 16) != 0 || (hw % 10) != 0) return declined;
    tiles_m = (int64_t)(p.frames / 16) * (hw / 10);
    if ((hw % 20) == 0) tiles_tall = tiles_m / 2;
    if ((int64_t)17 * hw * p.lda * 2 >= 0x7fffff00LL) return declined;   // a patch spans the clip's 16 frames: 31-bit offsets
  }
  if (tiles_m * 160 != p.m) return declined;
  const int tiles_n = p.n / TC_T16;
  const bool use_tall = tiles_tall > 0 && (sw.halo_tall == 2 || (sw.halo_tall == 1 && tiles_tall * tiles_n * batch >= 256));
  const int64_t tm = use_tall ? tiles_tall : tiles_m;
  const int64_t nblk = (int64_t)tiles_n * 8 * ((tm + 7) / 8);
  if (nblk > 0x7fffffffLL || batch > 65535) return declined;
  const int nchunks = p.cin / TC_BK;
  const bool ksplit = !use_tall && (nchunks % 2) == 0 && nchunks >= 4 &&
                      (sw.halo_ksplit == 2 || (sw.halo_ksplit == 1 && tiles_m * tiles_n * batch <= 256));
  take(r, TC_FAM_HALO, nblk, 1, batch, (use_tall || ksplit) ? 512 : 256);
  r->wm = use_tall ? 4 : 2, r->ks = ksplit ? 2 : 1;
  r->order = tc_gemm_tile_order(p, tiles_n, sw);
  return 1;
}

// ---- 8-wave 256x256 kernel (gemm8.hip)
static bool route_gemm8(const TcGemmParams& p, const TcGemmSwitches& sw, int batch, int cus, TcGemmRoute* r) {
  if (sw.gemm8 == 0) return false;
  const bool geglu = p.act == TC_ACT_GEGLU;
  const int n_out = geglu ? p.n / 2 : p.n;
  if ((n_out & 7) != 0 || (geglu && (p.n & 31) != 0)) return false;   // vector epilogue only; GEGLU packs per 32
  if (p.k <= TC_BK) return false;                                     // the K-tile stream needs two K-tiles per tile
  // the epilogue is the common case only (plain or GEGLU, bf16 out): every option it carried was code the wave streams
  // through once per tile
  if ((p.act != TC_ACT_NONE && !geglu) || p.alpha != 1.f || p.out_scale != 1.f || p.out_f32) return false;
  if (p.gather == TC_GATHER_CONV3x3 && (p.stride != 1 || p.upsample || p.pad != 1)) return false;   // plain 3x3 only
  if (p.gather != TC_GATHER_LINEAR && (p.k / TC_BK >= 1024 || p.cin > 4096)) return false;          // tap = multiply-high
  const int tiles_n = (p.n + TC_BIG - 1) / TC_BIG;
  const int tiles_m = (p.m + TC_BIG - 1) / TC_BIG;
  if (sw.gemm8 == 1) {
    // Measured (profiles/r04_gemm8_bench.txt, interleaved against the default routing): the kernel is ahead where ONE
    // round of 256x256 tiles fills the chip and K is long -- the level-1 ff2 (20480 x 640 x 2560: 240 tiles,
    // 1.11-1.21x), square problems from 4096 (1.00-1.07x), the decoder's 512-channel convolutions (1.03x) -- and
    // behind wherever the tile grid quantises badly on 256 CUs (every UNet width is 320 k, every row count 5 * 2^n:
    // N = 320 pads to 512, 320 / 160 / 100 tiles run 1.25 / 0.63 / 0.39 rounds) or K is short (K <= 1280: the epilogue
    // of a 256 x 256 tile -- 128 KiB of stores, for GEGLU as many VALU cycles as the tile's MFMAs -- is not overlapped
    // with matrix work when a CU holds a single block).  The heuristic takes the first class only.
    const int64_t tiles = (int64_t)tiles_n * tiles_m * batch;
    const double n_eff = (double)p.n / ((double)tiles_n * TC_BIG);
    // (one round: linear layers only -- the convolutions of that size are on the 160x160-tile kernel, which the 8-wave
    // kernel does NOT beat: level-1 3x3 640 -> 640 0.85x, 1920 -> 640 0.80x)
    const bool one_round = tiles >= 224 && tiles <= 256 && p.gather == TC_GATHER_LINEAR;
    const bool many = tiles >= 1024 && p.n % TC_BIG == 0 && p.n >= 512 && p.k >= 4096;   // (256 -> 256 convolutions: 0.89-0.92x)
    // GEGLU projections of levels 0 and 1 (81920 x 2560 x 320, 20480 x 5120 x 640: 3200 / 1600 tiles): once the GELU of
    // the epilogue lost its division sequence (common.h gelu_erf_f) the kernel is ahead there too -- 1.09-1.13x and
    // 1.06-1.09x (profiles/r04_gelu_ab.txt); level 2 (5120 x 10240 x 1280) stays behind (0.95x)
    const bool gated = geglu && p.gather == TC_GATHER_LINEAR && tiles >= 1536 && p.k <= 640 && p.n % TC_BIG == 0;
    if (!gated && (geglu || p.k < 2048 || n_eff < 0.8 || !(one_round || many))) return false;
  }
  const int64_t total = (int64_t)tiles_n * tiles_m;
  if (total > 0x7fffffffLL) return false;
  const int gmax = (sw.g8_grid > 0 ? sw.g8_grid : cus) & ~7;
  take(r, TC_FAM_GEMM8, (int)(total < gmax ? total : gmax), 1, batch, 512);    // a multiple of 8 unless it covers every tile in one round
  r->total_tiles = (int)total, r->stagger = sw.g8_stagger;
  return true;
}

// ---- 160x160 tiles (gemm16.hip)
static bool route_tile16(const TcGemmParams& p, const TcGemmSwitches& sw, int batch, TcGemmRoute* r) {
  if (sw.tile16 == 0 || p.act == TC_ACT_GEGLU || (p.n % TC_T16) != 0) return false;
  const int tiles_n = p.n / TC_T16;
  const int tiles_m = (p.m + TC_T16 - 1) / TC_T16;
  const int64_t tiles = (int64_t)tiles_n * tiles_m * batch;
  if (sw.tile16 == 1) {
    // worth it where the 160-grid quantises better than the 128-grid onto the 512 resident block slots:
    // efficiency = useful work / (whole rounds of 512 blocks x padded tile area)
    const int64_t t128 = (int64_t)((p.n + 127) / 128) * ((p.m + 127) / 128) * batch;
    const double eff16 = (double)tiles / (double)((tiles + 511) / 512 * 512) * ((double)p.m / ((double)tiles_m * TC_T16));
    const double eff128 = (double)t128 / (double)((t128 + 511) / 512 * 512) *
                          ((double)p.n / (double)((p.n + 127) / 128 * 128)) *
                          ((double)p.m / (double)((p.m + 127) / 128 * 128));
    // measured (profiles/r02_tile16_ab.txt, r02_tile16_cold_sustained.txt): 3x3 / temporal convolutions gain
    // 1.12-1.32x (cache-hot, cache-cold and sustained alike), K >= 1280 linear layers 1.0-1.18x, short-K projections
    // (K <= 640: five-pass epilogue per 160x160 tile against 5-10 K-steps) LOSE 8-18 %.  The heuristic takes the
    // convolutions only: the linear layers' gain is within the run-to-run spread of a whole clip.
    if (tiles < 512 || eff16 < eff128 + 0.04 || p.k < 960 || p.gather == TC_GATHER_LINEAR) return false;
  }
  const int64_t nblk = (int64_t)tiles_n * 8 * ((tiles_m + 7) / 8);
  if (nblk > 0x7fffffffLL) return false;
  take(r, TC_FAM_TILE16, nblk, 1, batch, 256);
  r->wm = 2;
  r->order = tc_gemm_tile_order(p, tiles_n, sw);
  const bool stats = p.gn_part != nullptr;
  // TC_G16_ILV: requests between the MFMAs (see the kernel header).  Unset = loop 2 for the convolutions, the plain loop
  // for linear problems (measured, profiles/r04_g16_tall_ilv_bench.txt: 3x3 / temporal convolutions 1.01-1.03x on the
  // 160-row tile, linear 0.98-1.02x; inside the UNet 8.29 / 8.30 against 8.27 / 8.28 frames/s, alternating on one lease:
  // profiles/r04_clip_ab_g16.txt); 0 = never; 1 | 2 = that loop wherever it can run.
  const bool ilv_ok = (p.gather == TC_GATHER_LINEAR || ((p.cin % TC_BK) == 0 && p.cin <= 4096)) && p.k < 1024 * TC_BK &&
                      (p.gather != TC_GATHER_CONV3x3 || (p.stride == 1 && !p.upsample && p.pad == 1));
  const int ilv = sw.ilv_set ? sw.ilv : (p.gather != TC_GATHER_LINEAR ? 2 : 0);
  // TC_G16_TALL: the 320 x 160 tile on eight waves (WM = 4), one block per CU.  0 (default) = never; 1 = convolutions whose
  // tall tiles fill whole rounds of the 256 CUs as well as the 160-row tiles fill their 512 slots (levels 0 / 1 of the
  // UNet); 2 = whenever the shape allows.  OFF although it wins kernel by kernel (with loop 2: level 0 1.035-1.06x, level
  // 1 1.09x; level 2 has 128 tall tiles: 0.8x; linear problems 0.94-1.05x): inside the UNet, alternating on one lease, it
  // LOSES 0.8 % of a clip (8.22 vs 8.27-8.29 frames/s, and 7.32 vs 7.38 together with loop 2:
  // profiles/r04_clip_ab_g16.txt) -- one 8-wave block per CU has nothing to fill its ramp and tail with.
  if (sw.g16_tall >= 1 && !stats && (ilv == 0 || ilv_ok) && (sw.g16_tall == 2 || p.gather != TC_GATHER_LINEAR)) {
    const int tm4 = (p.m + 2 * TC_T16 - 1) / (2 * TC_T16);
    const int64_t t4 = (int64_t)tiles_n * tm4 * batch;
    const double e4 = (double)t4 / (double)((t4 + 255) / 256 * 256) * ((double)p.m / ((double)tm4 * 2 * TC_T16));
    const double e2 = (double)tiles / (double)((tiles + 511) / 512 * 512) * ((double)p.m / ((double)tiles_m * TC_T16));
    if (sw.g16_tall == 2 || (t4 >= 256 && e4 >= e2 - 0.02)) {
      take(r, TC_FAM_TILE16, (int64_t)tiles_n * 8 * ((tm4 + 7) / 8), 1, batch, 512);
      r->wm = 4, r->ilv = (ilv == 1 || ilv == 2) ? ilv : 0;
      return true;
    }
  }
  if ((ilv == 1 || ilv == 2) && !stats && ilv_ok) {
    r->ilv = ilv;
    return true;
  }
  r->stats = stats;
  // TC_GEMM_PIPE = 2 only: on this tile the deeper prefetch measured 0.97-1.02x (profiles/r03_pipe_bench.txt) -- two
  // blocks of 80 KiB per CU already overlap each other's load latency -- so the default keeps the plain loop
  r->pipe = !stats && sw.pipe == 2;
  return true;
}

// ---- 256-row tiles (gemm_wide.hip)
static bool route_wide(const TcGemmParams& p, const TcGemmSwitches& sw, int batch, bool force, TcGemmRoute* r) {
  if (!sw.wide) return false;
  const bool geglu = p.act == TC_ACT_GEGLU;
  const int n_out = geglu ? p.n / 2 : p.n;
  if ((n_out & 7) != 0 || (p.n & 31) != 0) return false;       // vector epilogue only; GEGLU packs per 32
  int tnw;
  if (p.n % 320 == 0) tnw = 5;
  else if (p.n >= 256) tnw = 4;
  else if (p.n >= 128) tnw = 2;
  else return false;
  const int bn = 64 * tnw;
  const int tiles_n = (p.n + bn - 1) / bn;
  const int tiles_m = (p.m + TC_BIG - 1) / TC_BIG;
  const int64_t blocks = (int64_t)tiles_n * tiles_m * batch;
  // measured on MI355X (profiles/r01_v6_gemm_tile_sweep.txt): one 8-wave block per CU has no second block
  // to hide its prologue/epilogue behind, so the 256-row tile only wins with long K and either many
  // rounds of blocks (the decoder's 256/512-channel 3x3 convolutions) or a grid that fits the 256 CUs once.
  // (r02: wide GEGLU layers -- N = 10240, K = 1280 -- took the 256x320 tile; with two K-steps in flight the 128x128 kernel
  // is ahead there too: 157-160 us vs 163-171 us, profiles/r03_pipe_bench.txt / r03_two_tiles_per_block_ab.txt)
  if (!force) {
    const bool fits = blocks >= 192 && blocks <= 256;
    if (!(p.n >= 256 && p.k >= 2048 && (blocks >= 1024 || fits))) return false;
  }
  const int64_t nblk = (int64_t)tiles_n * 8 * ((tiles_m + 7) / 8);
  if (nblk > 0x7fffffffLL) return false;
  take(r, TC_FAM_WIDE, nblk, 1, batch, 512);
  r->tnw = tnw;
  r->order = tc_gemm_tile_order(p, tiles_n, sw);
  // TC_GEMM_PIPE = 2 only: with one 8-wave block per CU the second barrier per K-step costs more than the deeper
  // prefetch returns (measured, profiles/r03_pipe_bench.txt: the decoder's 512-channel convolutions 0.91x, the
  // N = 10240 GEGLU layer 0.95x), so the default keeps the plain loop
  r->pipe = sw.pipe == 2;
  return true;
}

// ---- 128 / 64 tiles (gemm.hip)
// Split-K factor (1 = no split).  Candidates: one problem (no batching), vector epilogue, no GEGLU, so few
// 128x128 tiles that most of the 512 block slots (2 per CU) would idle, and a K long enough to pay for
// the partial tiles and the reduction pass (~12 us): measured on the M = 1280 layers
// (profiles/r01_v6_gemm_splitk.txt) the 3x3 convolutions (K = 11520 / 23040) gain 1.28x / 1.51x over
// their 64x64-tile launch, while K <= 5120 (linear, temporal conv) loses -- those keep the 64x64 tiles.
static int tc_gemm_splits(const TcGemmParams& p, const TcGemmSwitches& sw) {
  const int force = sw.splitk;
  const int batch = p.batch > 0 ? p.batch : 1;
  if (force == 0 || batch != 1 || p.act == TC_ACT_GEGLU || (p.n & 7) != 0) return 1;
  const int nk = (p.k + TC_BK - 1) / TC_BK;
  const int64_t tiles = (int64_t)((p.n + 127) / 128) * ((p.m + 127) / 128);
  if (tiles >= 200 || (force < 0 && nk < 128)) return 1;
  int s = force > 0 ? force : (int)(512 / tiles);
  if (s > 8) s = 8;
  if (s > nk / 8) s = nk / 8;
  // a power of two: at 100 tiles (the level-3 convolutions) 4 slices measured 1.33-1.41x faster than 5
  // (profiles/r03_gemm_autotune_unet.txt: 61.5 vs 82.3 us at K = 11520, 101.9 vs 143.9 us at K = 23040)
  if (force <= 0) while (s & (s - 1)) s &= s - 1;
  return s < 2 ? 1 : s;
}

// Tile family for the 4-wave kernel: (64 tm) x (64 tn).  The sweep (profiles/r01_v6_gemm_tile_sweep.txt)
// has 128x128 ahead on every UNet/decoder shape -- 128x64 and 64x128 lose 5-45 % to their higher LDS/L1
// traffic per FLOP even where they would fill the CUs more evenly -- except the lowest-resolution layers
// (M = 1280 rows), whose 100 128-tiles leave most of the 256 CUs idle: those take 64x64 (+32-37 %).
static void pick_tile(int m, int n, int batch, bool geglu, int* tm, int* tn) {
  const int64_t big_tiles = (int64_t)((n + 127) / 128) * ((m + 127) / 128) * batch;
  const bool small = !geglu && big_tiles < 384;
  *tm = small ? 1 : 2;
  *tn = small ? 1 : 2;
  // the 3- / 4-channel output convolutions: a 64-column tile wastes half as many MFMAs on padding (measured,
  // profiles/r03_gemm_autotune_*.txt: decoder conv_out 1362 -> 701 us with 128x64, UNet out 106 -> 67 us with 64x64)
  if (!geglu && n <= 64) {
    *tn = 1;
    *tm = m >= 262144 ? 2 : 1;
  }
}

static int route_tile(const TcGemmParams& p, const TcGemmSwitches& sw, int batch, bool gn_ok, TcGemmRoute* r) {
  const bool geglu = p.act == TC_ACT_GEGLU;
  const int force = sw.tile;
  int tm = 2, tn = 2;
  int splits = (p.workspace && force == 0) ? tc_gemm_splits(p, sw) : 1;
  if (splits > 1 && p.workspace_bytes < (int64_t)splits * p.m * p.n * (int64_t)sizeof(float)) splits = 1;
  if (force > 1) {
    tm = force / 10;
    tn = geglu ? 2 : force % 10;
  } else if (splits == 1) {
    pick_tile(p.m, p.n, batch, geglu, &tm, &tn);
  }
  // statistics come from the 128x128 tile without split-K only
  r->gn_rows = (gn_ok && splits == 1 && tm == 2 && tn == 2) ? 128 : 0;
  if (p.gn_part && !r->gn_rows) return TC_ESHAPE;
  if (splits > 1 && !aligned16(p.workspace)) return TC_EALIGN;
  const int bm = 64 * tm, bn = 64 * tn;
  const int tiles_n = (p.n + bn - 1) / bn;
  const int tiles_m = (p.m + bm - 1) / bm;
  // -1 (W-stationary walk) for the lowest-resolution layers (M <= 2048 rows) whose weight matrix outweighs
  // their activation rows.  Measured (profiles/r02_nmajor_ab.txt): +5-7 % on the level-3 convolutions and qkv, neutral
  // on the rest of level 3, 3-7 % SLOWER on the level-2 convolutions (40 M-tiles: the A halo re-reads cost more than
  // the W re-reads the Infinity Cache was already absorbing) -- hence the row limit.
  const bool nmajor = sw.nmajor != 0 && p.batch <= 1 && (sw.nmajor == 2 || (p.m <= 2048 && tc_w_extent(p) > tc_a_extent(p)));
  const int64_t nblk = nmajor ? 8 * (((int64_t)tiles_m * tiles_n + 7) / 8) : (int64_t)tiles_n * 8 * ((tiles_m + 7) / 8);
  if (nblk > 0x7fffffffLL || batch > 65535) return TC_ESHAPE;
  take(r, TC_FAM_TILE, nblk, splits, batch, 256);
  r->tm = tm, r->tn = tn, r->splits = splits;
  r->order = nmajor ? -1 : tc_gemm_tile_order(p, tiles_n, sw);
  r->pipe = sw.pipe != 0, r->late_epi = sw.epi_late;      // pipe 0: the one-K-step-in-flight loop; default: two in flight
  return TC_OK;
}

int tc_gemm_route(const TcGemmParams& p, const TcGemmSwitches& sw, int cus, TcGemmRoute* r) {
  *r = TcGemmRoute{};
  const int batch = p.batch > 0 ? p.batch : 1;
  // gn_part (ABI 9): which problems can carry it at all; forced tile families are tuning runs only
  const bool gn_ok = batch == 1 && p.act != TC_ACT_GEGLU && !p.out_f32 && (p.n & 7) == 0 && !p.a_norm && !sw.tile_set && sw.gn_part;
  if (p.gn_part && !gn_ok) return TC_ESHAPE;
  const auto emits = [&](int rows) {          // the family is chosen: can it emit the statistics the call asks for?
    r->gn_rows = gn_ok ? rows : 0;
    return (p.gn_part && !r->gn_rows) ? TC_ESHAPE : TC_OK;
  };
  const int force = sw.tile;
  if (force == 0 && tc_gemm_ws_takes(p, sw, batch)) return route_ws(p, sw, r), emits(0);      // K = 320 linear layers of level 0: W in registers
  if (p.a_norm) return TC_ESHAPE;                                      // only the weight-stationary kernel normalises A rows
  // tap-reuse patches: the default route of the 3x3 convolutions of levels 0-2.  A call that asks for producer statistics
  // keeps the implicit GEMM, whose epilogue emits them -- so TC_GN_PART=1 measures what profiles/r04_gn_part_ab.txt
  // measured, statistics from every 160 / 128-tile convolution, and not only from the few the halo route leaves over
  // (ADVICE r5); tc_gemm_gn_rows therefore asks with gn_part set
  if (force == 0 && !p.gn_part) {
    const int h = route_halo(p, sw, batch, r);
    if (h < 0) return TC_ESHAPE;                                       // strict mode (tests): a convolution it could not take
    if (h > 0) return TC_OK;
  }
  if (force == 0 && route_gemm8(p, sw, batch, cus, r)) return emits(0);      // long-K / wide-N problems
  if (force == 0 && route_tile16(p, sw, batch, r)) return emits(TC_T16);     // widths 320 k at levels 0 / 1
  if (force <= 1 && route_wide(p, sw, batch, force == 1, r)) return emits(0);   // big-M layers
  return route_tile(p, sw, batch, gn_ok, r);
}

// ---- the C ABI's questions about the route (include/tooncrafter_hip.h)
extern "C" int64_t tc_gemm_workspace(const TcGemmParams* p) {
  if (!p || p->m <= 0 || p->n <= 0 || p->k <= 0) return 0;
  const int s = tc_gemm_splits(*p, tc_gemm_switches());
  return s > 1 ? (int64_t)s * p->m * p->n * (int64_t)sizeof(float) : 0;
}
extern "C" int tc_gemm_ws_eligible(const TcGemmParams* p) {
  return (p && tc_gemm_ws_takes(*p, tc_gemm_switches(), p->batch > 0 ? p->batch : 1)) ? 1 : 0;
}

// ABI 9: row-block height of gn_part under the route tc_gemm_bf16 takes for a call that carries gn_part
extern "C" int tc_gemm_gn_rows(const TcGemmParams* pp) {
  if (!pp || pp->m <= 0 || pp->n <= 0 || pp->k <= 0) return 0;
  TcGemmParams p = *pp;
  if (!p.gn_part) p.gn_part = reinterpret_cast<float*>(16);          // never dereferenced: the route only asks whether it is set
  TcGemmRoute r;
  tc_gemm_route(p, tc_gemm_switches(), 256, &r);          // (the CU count only sizes a grid)
  return r.gn_rows;
}
