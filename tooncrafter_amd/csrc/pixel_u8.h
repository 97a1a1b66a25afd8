// The pixel arithmetic that more than one file states: a decoded fp32 sample as a byte (tc_video_to_u8 in elementwise.hip,
// tc_frames_to_u8 in pixel_back.hip) and PIL's 8-bit two-pass resample as the front end (tc_frames_from_u8 in
// pixel_front.hip) and the back end (tc_frames_to_u8, tc_frames_to_yuv) both run it: one axis at one output index, the
// horizontal pass, and the pixel under (row, col) of the resized image, with the grid rule of their launches.  Each stands
// here once, for uint8 and for the uint16 samples of the 10-bit output alike, so the files and the depths cannot drift apart.
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

// The resample's two sample types: uint8 frames summed in int32 (PIL's 8bpc arithmetic, what both ends run) and the uint16
// frames of the back end's 10-bit output summed in int64 (65535 * 1.6 * 2^22 does not fit int32).  `top` clips the result.
template <typename T> struct Resample;
template <> struct Resample<uint8_t> { using Acc = int32_t; static constexpr int32_t top = 255; };
template <> struct Resample<uint16_t> { using Acc = int64_t; static constexpr int32_t top = 65535; };

// One axis of PIL's 8-bit resample at one output index: sum coefs[k] * src[(first + k) * step] over the taps, rounded and
// clipped as ImagingResampleHorizontal_8bpc does (to 65535 for uint16 samples, same tables).  The sum, the shift and the clip
// are signed: filters with negative lobes (bicubic, Lanczos) take it below zero.  The bounds are clamped to [0, extent): a
// wrong table cannot reach outside the image.  `step` counts samples.
template <typename T>
__device__ __forceinline__ int32_t resample_axis(const T* __restrict__ src, int64_t step, int extent,
                                                 const int32_t* __restrict__ bounds, const int32_t* __restrict__ coefs,
                                                 int kmax, int idx) {
  using Acc = typename Resample<T>::Acc;
  int first = bounds[2 * idx], cnt = bounds[2 * idx + 1];
  first = min(max(first, 0), extent - 1);
  cnt = min(min(cnt, kmax), extent - first);
  const int32_t* k = coefs + (int64_t)idx * kmax;
  Acc ss = (Acc)1 << 21;
  for (int i = 0; i < cnt; ++i) ss += (Acc)k[i] * (Acc)src[(int64_t)(first + i) * step];
  ss >>= 22;
  return (int32_t)(ss < 0 ? (Acc)0 : ss > (Acc)Resample<T>::top ? (Acc)Resample<T>::top : ss);
}

// horizontal pass: n images (sh, sw, 3), rows `pitch` and images `image_stride` samples apart -> the packed intermediate
// (n, sh, rw, 3) of the same sample type, one thread per pixel of it
template <typename T>
__global__ __launch_bounds__(256) void resample_hpass_kernel(const T* __restrict__ src, int64_t image_stride, int pitch,
                                                             int sh, int sw, int rw, const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ coefs, int kmax,
                                                             T* __restrict__ mid, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % rw);
    const int64_t row = i / rw;                                  // image * sh + y
    const int64_t img = row / sh, y = row - img * sh;
    const T* line = src + img * image_stride + y * pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) mid[i * 3 + c] = (T)resample_axis(line + c, 3, sw, bounds, coefs, kmax, x);
  }
}

// The pixel under (row, col) of the resized image, from one image `img` whose rows are `pitch` samples apart.  RESAMPLE: img
// has ih rows and is resampled over them; else img is the resized image already and is read as it is.
template <bool RESAMPLE, typename T>
__device__ __forceinline__ void resized_pixel(const T* __restrict__ img, int64_t pitch, int ih,
                                              const int32_t* __restrict__ bounds, const int32_t* __restrict__ coefs, int kmax,
                                              int row, int col, int32_t* rgb) {
  const T* base = img + (int64_t)col * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rgb[c] = RESAMPLE ? resample_axis(base + c, pitch, ih, bounds, coefs, kmax, row) : (int32_t)base[row * pitch + c];
}

}  // namespace
