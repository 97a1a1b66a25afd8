// The routing of tc_gemm_bf16 EXECUTED on the host: csrc/gemm_route.cpp compiled with g++ (no HIP, no GPU).  Reads the
// problems of tests/golden/make_gemm_routes.py from stdin, takes the switch setting from the environment and prints, per
// problem, what tc_gemm_bf16 does with the route -- the line the golden's recorder got from the launchers themselves:
// kernel instance, grid, block, scalar arguments, gn_rows, workspace bytes, return code.  tests/test_gemm_route_cpu.py.
#include "../tooncrafter_amd/csrc/gemm_route.cpp"

#include "golden/gemm_route_problems.h"

static const char* b(bool v) { return v ? "true" : "false"; }

static void print_launch(const TcGemmParams& p, const TcGemmRoute& r) {
  char name[96], args[64];
  switch (r.family) {
    case TC_FAM_WS:
      snprintf(name, sizeof name, "gemm_ws_kernel<%d, %s, %s, %s>", r.geglu ? 4 : 5, b(r.geglu), b(r.res && !r.geglu), b(r.ln));
      snprintf(args, sizeof args, " %d %d", r.nchunks, r.safe);
      break;
    case TC_FAM_HALO:
      snprintf(name, sizeof name, "conv_halo_kernel<%d, %d, %d>", p.gather, r.wm, r.wm == 4 ? 1 : r.ks);
      snprintf(args, sizeof args, " %d", r.order);
      break;
    case TC_FAM_GEMM8:
      snprintf(name, sizeof name, "gemm8_kernel<%d, 0>", p.gather);
      snprintf(args, sizeof args, " %d %d", r.total_tiles, r.stagger);
      break;
    case TC_FAM_TILE16:
      snprintf(name, sizeof name, "gemm16_kernel<%d, %s, %s, 0, %d, %d>", p.gather, b(r.pipe), b(r.stats), r.ilv, r.wm);
      snprintf(args, sizeof args, " %d", r.order);
      break;
    case TC_FAM_WIDE:
      snprintf(name, sizeof name, "gemm_wide_kernel<%d, %d, %s>", p.gather, r.tnw, b(r.pipe));
      snprintf(args, sizeof args, " %d", r.order);
      break;
    default:
      snprintf(name, sizeof name, "gemm_kernel<%d, %d, %d, %s>", p.gather, r.tm, r.tn, b(r.pipe));
      snprintf(args, sizeof args, " %d %d %d", r.splits, r.order, r.late_epi);
      break;
  }
  printf(" | %s grid=%u,%u,%u block=%u args=%s", name, r.grid[0], r.grid[1], r.grid[2], r.block, args);
  if (r.family == TC_FAM_TILE && r.splits > 1)
    printf(" | splitk_reduce_kernel grid=%u,1,1 block=256 args= %d", (unsigned)(((int64_t)p.m * (p.n >> 3) + 255) / 256), r.splits);
}

int main() {
  TcGemmParams p;
  for (int i = 0;; ++i) {
    printf("%d ", i);
    if (!tc_read_problem(&p)) break;
    TcGemmRoute r;
    int rc = tc_gemm_validate(p);
    if (rc == TC_OK) rc = tc_gemm_route(p, tc_gemm_switches(), 256, &r);
    if (rc == TC_OK) print_launch(p, r);
    printf(" | rc=%d\n", rc);
  }
  printf("end\n");
  return 0;
}
