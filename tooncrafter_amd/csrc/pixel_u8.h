// The two pieces of pixel arithmetic that more than one file states: a decoded fp32 sample as a byte (tc_video_to_u8 in
// elementwise.hip, tc_frames_to_u8 in pixel_back.hip) and one axis of PIL's 8-bit resample at one output index
// (tc_frames_from_u8 in pixel_front.hip, tc_frames_to_u8).  Each stands here once, so the files cannot drift apart.
#pragma once
#include "common.h"

namespace {

// scripts/evaluation/inference.py:148-153 for one sample: clamp(x, -1, 1), (v + 1) / 2, * 255, fp32 -> u8 truncates like
// Tensor.to(uint8).  Every operation is rounded on its own, in this order.
__device__ __forceinline__ uint8_t sample_to_u8(float v) {
  v = fminf(fmaxf(v, -1.f), 1.f);
  v = (v + 1.0f) / 2.0f;
  return (uint8_t)(v * 255.f);
}

// One axis of PIL's 8-bit resample at one output index: sum coefs[k] * src[(first + k) * step] over the taps, rounded and
// clipped as ImagingResampleHorizontal_8bpc does.  The sum, the shift and the clip are signed: filters with negative lobes
// (bicubic, Lanczos) take it below zero.  The bounds are clamped to [0, extent): a wrong table cannot reach outside the
// image.
__device__ __forceinline__ uint32_t resample_u8(const uint8_t* __restrict__ src, int64_t step, int extent,
                                                const int32_t* __restrict__ bounds, const int32_t* __restrict__ coefs,
                                                int kmax, int idx) {
  int first = bounds[2 * idx], cnt = bounds[2 * idx + 1];
  first = min(max(first, 0), extent - 1);
  cnt = min(min(cnt, kmax), extent - first);
  const int32_t* k = coefs + (int64_t)idx * kmax;
  int32_t ss = 1 << 21;
  for (int i = 0; i < cnt; ++i) ss += k[i] * (int32_t)src[(int64_t)(first + i) * step];
  return (uint32_t)min(max(ss >> 22, 0), 255);
}

}  // namespace
