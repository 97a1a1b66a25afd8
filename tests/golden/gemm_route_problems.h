// Shared by the golden's recorder (gemm_route_driver.cpp) and tests/gemm_route_host_check.cpp: one problem per line of
// stdin, the fields of TcGemmParams in declaration order.  Pointers are flags: 0 = NULL, 1 = set (16-byte aligned),
// 2 = set, misaligned; workspace / gn_part may be -1 = "as tooncrafter_amd/ops.py fills them": the bytes
// tc_gemm_workspace asks for, statistics if tc_gemm_gn_rows offers them.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "tooncrafter_hip.h"

inline void* tc_fake_ptr(long flag, int slot) {
  return flag == 0 ? nullptr : reinterpret_cast<void*>((uintptr_t)0x100000 * (slot + 1) + (flag == 2 ? 8 : 0));
}

// false at end of input
inline bool tc_read_problem(TcGemmParams* p) {
  long a, w, c, bias, rb, res, ws, gn;
  long long sa, sw, sc, wsb;
  *p = TcGemmParams{};
  const int n = scanf("%ld %ld %ld %ld %ld %ld %d %d %d %d %d %d %d %d %d %f %f %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %ld %lld %d %f %ld",
                      &a, &w, &c, &bias, &rb, &res, &p->m, &p->n, &p->k, &p->lda, &p->ldw, &p->ldc, &p->ldr, &p->ldrb, &p->row_div,
                      &p->alpha, &p->out_scale, &p->act, &p->out_f32, &p->gather, &p->cin, &p->frames, &p->t_len, &p->h_out, &p->w_out,
                      &p->h_in, &p->w_in, &p->stride, &p->upsample, &p->pad, &p->batch, &sa, &sw, &sc, &ws, &wsb, &p->a_norm,
                      &p->a_norm_eps, &gn);
  if (n != 39) return false;
  p->a = (const tc_bf16*)tc_fake_ptr(a, 0), p->w = (const tc_bf16*)tc_fake_ptr(w, 1), p->c = tc_fake_ptr(c, 2);
  p->bias = (const float*)tc_fake_ptr(bias, 3), p->row_bias = (const float*)tc_fake_ptr(rb, 4);
  p->residual = (const tc_bf16*)tc_fake_ptr(res, 5);
  p->stride_a = sa, p->stride_w = sw, p->stride_c = sc;
  p->workspace_bytes = wsb;
  p->workspace = ws < 0 ? nullptr : tc_fake_ptr(ws, 6);
  const int64_t want = tc_gemm_workspace(p);
  const int rows = tc_gemm_gn_rows(p);
  printf("ws=%lld gn=%d wse=%d", (long long)want, rows, tc_gemm_ws_eligible(p));
  if (ws < 0 && want > 0) p->workspace = tc_fake_ptr(1, 6), p->workspace_bytes = want;
  p->gn_part = gn < 0 ? (rows > 0 ? (float*)tc_fake_ptr(1, 7) : nullptr) : (float*)tc_fake_ptr(gn, 7);
  return true;
}
