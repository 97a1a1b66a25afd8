// Where a bf16 GEMM goes: the routing switches (one table, gemm_route.cpp) and the pure routing function that maps a
// problem to one kernel family, its template variant, its grid and its scalar arguments.  Host only, no HIP: compiled
// into the library and, by tests/gemm_route_host_check.cpp, with a plain host compiler.  The family files
// (gemm_ws / conv_halo / gemm8 / gemm16 / gemm_wide / gemm .hip) keep the kernels and a launcher that only launches.
#pragma once
#include <stdint.h>

#include "tooncrafter_hip.h"

#ifdef __HIPCC__
#define TC_HD __host__ __device__ __forceinline__
#else
#define TC_HD inline
#endif

constexpr int TC_BK = 64;          // K-step of every GEMM kernel: one 128-byte LDS row per tile row
constexpr int TC_T16 = 160, TC_BIG = 256;       // tile side of gemm16 / conv_halo .hip (tall: 320 rows); of gemm8.hip, rows of gemm_wide.hip
constexpr int TC_WS_K = 320, TC_WS_ROWS = 64;   // gemm_ws.hip: the K it is built for, rows per streamed A tile

// byte extents of one batch item of A (source rows of the gather) and W
TC_HD int64_t tc_a_rows(const TcGemmParams& p) {
  return p.gather == TC_GATHER_CONV3x3 ? (int64_t)p.frames * p.h_in * p.w_in : (int64_t)p.m;
}
TC_HD int64_t tc_a_extent(const TcGemmParams& p) {
  const int kc = p.gather == TC_GATHER_LINEAR ? p.k : p.cin;
  return ((tc_a_rows(p) - 1) * p.lda + kc) * 2;
}
TC_HD int64_t tc_w_extent(const TcGemmParams& p) {
  return ((int64_t)(p.n - 1) * p.ldw + p.k) * 2;
}

// Every routing switch of the family, parsed.  tc_gemm_switches() reads the environment; the names, the defaults and
// what each value means are stated once, in the table of gemm_route.cpp.
struct TcGemmSwitches {
  int tile, tile_set;        // TC_GEMM_TILE: 0 = heuristic, 1 = 256-row, 22 | 21 | 12 | 11 = that 4-wave tile; set to anything non-empty
  int tile16, gemm8, ws, wide, pipe, splitk, nmajor, epi_late;         // TC_GEMM_<name>
  int order;                 // TC_GEMM_ORDER
  int64_t order_bytes;       // TC_GEMM_ORDER_MIB, in bytes
  int ilv_set, ilv, g16_tall, g8_grid, g8_stagger;                     // TC_G16_ILV (set at all?) / TC_G16_TALL / TC_G8_GRID / TC_G8_STAGGER
  int halo, halo_3x3, halo_t3, halo_tall, halo_ksplit, gn_part;        // TC_CONV_HALO, TC_CONV_HALO_<name>, TC_GN_PART
  const char *forcing_name, *forcing_value;   // the first implicit-GEMM switch that carries a non-default value (nullptr: none)
};
TcGemmSwitches tc_gemm_switches();

// in the order tc_gemm_route asks them: gemm_ws.hip | conv_halo.hip | gemm8.hip | gemm16.hip | gemm_wide.hip | gemm.hip
enum TcGemmFamily { TC_FAM_WS = 0, TC_FAM_HALO, TC_FAM_GEMM8, TC_FAM_TILE16, TC_FAM_WIDE, TC_FAM_TILE };

struct TcGemmRoute {
  int family;
  // template variant
  int tm, tn;                // TILE: the tile is (64 tm) x (64 tn)
  int tnw;                   // WIDE: 2 | 4 | 5
  int wm, ks;                // TILE16 / HALO: 2 = 160 rows, 4 = 320 rows (tall); HALO: 2 = K split over two wave groups
  int ilv;                   // TILE16: request loop 0 | 1 | 2
  bool pipe, stats;          // TILE / WIDE / TILE16: two K-steps in flight; TILE16: the epilogue emits gn_part
  bool geglu, res, ln;       // WS flavour
  // launch geometry and the scalar kernel arguments
  unsigned grid[3], block;
  int splits, order, late_epi;        // TILE (order: every tiled family)
  int nchunks, safe;                  // WS
  int total_tiles, stagger;           // GEMM8
  int gn_rows;               // row-block height of gn_part on this route (0: the kernel emits none)
  bool halo_yielded;         // the halo route left this convolution to the kernel TcGemmSwitches.forcing_name selects
};

// Argument validation of tc_gemm_bf16 (TC_OK | TC_EINVAL | TC_EALIGN | TC_ESHAPE), then the route of a valid problem:
// no HIP call, nothing launched; `cus` = compute units of the device (the 8-wave kernel's grid).
int tc_gemm_validate(const TcGemmParams& p);
int tc_gemm_route(const TcGemmParams& p, const TcGemmSwitches& sw, int cus, TcGemmRoute* r);

int tc_gemm_tile_order(const TcGemmParams& p, int tiles_n, const TcGemmSwitches& sw);   // the route's rule, for gemm_mx.hip
