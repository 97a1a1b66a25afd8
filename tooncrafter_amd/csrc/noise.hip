// tc_randn_clips: per-clip Gaussian noise from a counter-based generator (include/tooncrafter_hip.h states the contract).
// Element j of clip i is a pure function of (seeds[i], stream, j): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel
// random numbers: as easy as 1, 2, 3", SC'11) keyed by the clip's seed, counter (j >> 2, 0, stream, 0), then Box-Muller on
// word pairs.  Nothing here depends on the batch size, the clip's slot, the launch chunking or the grid.
#include "common.h"

namespace {

// the seeds of one launch travel as kernel arguments: no device copy, nothing to keep alive after the call returns
struct RandnSeeds { uint32_t lo[TC_RANDN_CLIPS], hi[TC_RANDN_CLIPS]; };

struct Philox4 { uint32_t w0, w1, w2, w3; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1;
    c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += W0; k1 += W1;                                   // the key is bumped between rounds (the tenth bump is unused)
  }
  return {c0, c1, c2, c3};
}

// Box-Muller on one word pair.  u = (2 (wa >> 9) + 1) 2^-24 is exact in fp32 and inside [2^-24, 1 - 2^-24], so logf(u) is
// finite and negative; 2 v = (wb >> 9) 2^-22 is exact.  The accurate logf / sincospif, not the fast intrinsics.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float scale, float& z0, float& z1) {
  const float u = (float)(2u * (wa >> 9) + 1u) * 0x1p-24f;
  const float v2 = (float)(wb >> 9) * 0x1p-22f;
  const float r = sqrtf(-2.0f * logf(u));
  float s, c;
  sincospif(v2, &s, &c);
  z0 = (r * c) * scale;
  z1 = (r * s) * scale;
}

// grid (blocks over the clip's 4-element groups, clips of this launch); one thread = one Philox block = one 16-byte store.
// `out` is the row of the launch's first clip.  The last group of a row whose n % 4 != 0, and every group of a row that
// does not start on a 16-byte boundary, are stored element by element.
template <bool RAW>
__global__ __launch_bounds__(256) void randn_clips_kernel(float* __restrict__ out, int64_t n, RandnSeeds seeds, uint32_t stream,
                                                          float scale) {
  const int clip = blockIdx.y;
  const uint32_t k0 = seeds.lo[clip], k1 = seeds.hi[clip];
  float* row = out + (int64_t)clip * n;
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int64_t groups = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
    const Philox4 w = philox4x32_10((uint32_t)q, 0u, stream, 0u, k0, k1);
    float4 z;
    if (RAW) {
      z = {__uint_as_float(w.w0), __uint_as_float(w.w1), __uint_as_float(w.w2), __uint_as_float(w.w3)};
    } else {
      box_muller(w.w0, w.w1, scale, z.x, z.y);
      box_muller(w.w2, w.w3, scale, z.z, z.w);
    }
    const int64_t j = q << 2;
    if (aligned && j + 4 <= n) {
      *reinterpret_cast<float4*>(row + j) = z;
    } else {
      const float e[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (j + m < n) row[j + m] = e[m];
    }
  }
}

}  // namespace

extern "C" int tc_randn_clips(const TcRandnParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  const TcRandnParams& p = *pp;
  if (!p.out || !p.seeds || p.b <= 0 || p.n <= 0) return TC_EINVAL;
  if (p.n > ((int64_t)1 << 34)) return TC_ESHAPE;                      // q = j >> 2 must fit counter word 0
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t groups = (p.n + 3) >> 2;
  int64_t gx = (groups + 255) / 256;
  if (gx > 4096) gx = 4096;
  for (int32_t first = 0; first < p.b; first += TC_RANDN_CLIPS) {
    const int32_t clips = p.b - first < TC_RANDN_CLIPS ? p.b - first : TC_RANDN_CLIPS;
    RandnSeeds seeds = {};
    for (int32_t i = 0; i < clips; ++i) {
      seeds.lo[i] = (uint32_t)(p.seeds[first + i] & 0xFFFFFFFFull);
      seeds.hi[i] = (uint32_t)(p.seeds[first + i] >> 32);
    }
    float* row = p.out + (int64_t)first * p.n;
    if (p.raw)
      hipLaunchKernelGGL(randn_clips_kernel<true>, dim3((unsigned)gx, (unsigned)clips), dim3(256), 0, s, row, p.n, seeds, p.stream, p.scale);
    else
      hipLaunchKernelGGL(randn_clips_kernel<false>, dim3((unsigned)gx, (unsigned)clips), dim3(256), 0, s, row, p.n, seeds, p.stream, p.scale);
    TC_LAUNCH_CHECK();
  }
  return TC_OK;
}
