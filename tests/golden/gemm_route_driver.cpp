// Driver of the golden's recorder: feeds the problems on stdin to tc_gemm_bf16 of a library tree whose launches
// gemm_route_recorder.h turned into text.  One line per problem; the switch setting is the process environment.
#include "gemm_route_problems.h"

int main() {
  TcGemmParams p;
  for (int i = 0;; ++i) {
    printf("%d ", i);
    if (!tc_read_problem(&p)) break;
    const int rc = tc_gemm_bf16(&p, nullptr);
    printf(" | rc=%d\n", rc);
  }
  printf("end\n");
  return 0;
}
