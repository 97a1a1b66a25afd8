// The pixel arithmetic that more than one file states: a decoded fp32 sample as a byte (tc_video_to_u8 in elementwise.hip,
// tc_frames_to_u8 in pixel_back.hip) and PIL's 8-bit two-pass resample as the front end (tc_frames_from_u8 in
// pixel_front.hip) and the back end (tc_frames_to_u8) both run it: one axis at one output index, the horizontal pass, and
// the pixel under (row, col) of the resized image, with the grid rule of their launches.  Each stands here once, so the files
// cannot drift apart.
#pragma once
#include "common.h"

namespace {

// blocks of 256 threads for n elements of a grid-stride kernel
inline unsigned pixel_grid(int64_t n, unsigned cap = 8192) {
  const int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

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

// horizontal pass: n images (sh, sw, 3), rows `pitch` and images `image_stride` bytes apart -> the packed uint8
// intermediate (n, sh, rw, 3), one thread per pixel of it
__global__ __launch_bounds__(256) void resample_hpass_kernel(const uint8_t* __restrict__ src, int64_t image_stride, int pitch,
                                                             int sh, int sw, int rw, const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ coefs, int kmax,
                                                             uint8_t* __restrict__ mid, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % rw);
    const int64_t row = i / rw;                                  // image * sh + y
    const int64_t img = row / sh, y = row - img * sh;
    const uint8_t* line = src + img * image_stride + y * pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) mid[i * 3 + c] = (uint8_t)resample_u8(line + c, 3, sw, bounds, coefs, kmax, x);
  }
}

// The pixel under (row, col) of the resized image, from one image `img` whose rows are `pitch` bytes apart.  RESAMPLE: img
// has ih rows and is resampled over them; else img is the resized image already and is read as it is.
template <bool RESAMPLE>
__device__ __forceinline__ void resized_pixel(const uint8_t* __restrict__ img, int64_t pitch, int ih,
                                              const int32_t* __restrict__ bounds, const int32_t* __restrict__ coefs, int kmax,
                                              int row, int col, int32_t* rgb) {
  const uint8_t* base = img + (int64_t)col * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rgb[c] = RESAMPLE ? (int32_t)resample_u8(base + c, pitch, ih, bounds, coefs, kmax, row) : (int32_t)base[row * pitch + c];
}

}  // namespace
