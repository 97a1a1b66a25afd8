// Force-included (-include) in front of the library's GEMM sources when they are compiled for the HOST only
// (hipcc --cuda-host-only): every kernel launch becomes a line of text -- the address of the kernel's host-side handle
// (make_gemm_routes.py resolves it to the instance name with `nm -C`), grid, block and the integer arguments -- and
// nothing is launched.  No GPU is needed.  See make_gemm_routes.py.
#pragma once
#include <hip/hip_runtime.h>

#include <stdio.h>

namespace tc_rec {
inline void arg(const int& v) { printf(" %d", v); }
template <class T>
inline void arg(const T&) {}          // the TcGemmParams block: the driver knows it
template <auto K, class... A>
void launch(dim3 g, dim3 b, const A&... a) {
  printf(" | @%p grid=%u,%u,%u block=%u args=", (void*)K, g.x, g.y, g.z, b.x);
  (arg(a), ...);
}
}  // namespace tc_rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(K, G, B, SH, ST, ...) tc_rec::launch<K>(G, B, __VA_ARGS__)
#define hipGetLastError() hipSuccess
#define hipGetDevice(d) hipErrorNoDevice          /* the recording is made for 256 compute units */
