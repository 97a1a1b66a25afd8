// Pixel front end, gfx950: uint8 frames -> the model's fp32 frames (tc_frames_from_u8; tc_frames_from_yuv for a decoder's
// planar 4:2:0 surfaces, which converts to packed RGB and runs the same plan) and fp32 frames -> the CLIP image
// tower's patch rows (tc_clip_patches).  All run a handful of times per clip on at most a few megabytes, so every kernel
// here is one thread per output element, written for the arithmetic to be read off the code: the integer resample must give
// PIL's bytes and the blur / bicubic must stay within a bf16 ulp of kornia's, near zero too.  See include/tooncrafter_hip.h.
#include "common.h"
#include "pixel_u8.h"

#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------- tc_frames_from_u8

// The grid rule, one axis of PIL's 8-bit resample, the horizontal pass and the pixel under (row, col) of the resized image are
// pixel_u8.h's: the back end runs them too.

struct FrameSlots { int32_t v[TC_FRAMES_U8_MAX]; };

// The vertical pass and everything behind it: for each pixel of the (H, W) crop window, the pixel of the resized image under
// it (RESAMPLE: `img` (ih rows) resampled over rows; else `img` is that image already), 0 outside, through the value table
// into frame slots.v[image] of the (b, 3, t, H, W) output.
template <bool RESAMPLE>
__global__ __launch_bounds__(256) void frames_final_kernel(const uint8_t* __restrict__ img, int64_t image_stride, int pitch,
                                                           int ih, int rh, int rw, const int32_t* __restrict__ bounds,
                                                           const int32_t* __restrict__ coefs, int kmax, int top, int left,
                                                           FrameSlots slots, float* __restrict__ out, int t, int h, int w,
                                                           int64_t total) {
  // ToTensor + Normalize(0.5, 0.5) of the 256 byte values, as torch rounds them: a correctly rounded fp32 division, then a
  // subtraction and a division by 0.5 (exact), none contracted
  __shared__ float value[256];
  {
#pragma clang fp contract(off)
    const float a = (float)threadIdx.x / 255.0f;
    const float d = a - 0.5f;
    value[threadIdx.x] = d / 0.5f;
  }
  __syncthreads();
  const int64_t hw = (int64_t)h * w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % w);
    const int64_t r = i / w;
    const int y = (int)(r % h);
    const int64_t n = r / h;
    const int ry = y + top, rx = x + left;
    int32_t px[3] = {0, 0, 0};
    if (ry >= 0 && ry < rh && rx >= 0 && rx < rw)
      resized_pixel<RESAMPLE>(img + n * image_stride, pitch, ih, bounds, coefs, kmax, ry, rx, px);
    const int64_t frame = slots.v[n];                            // batch * t + frame index
    const int64_t bb = frame / t, ff = frame - bb * t;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((bb * 3 + c) * t + ff) * hw + (int64_t)y * w + x] = value[px[c]];
  }
}

// Python's round(d / 2.0): halves go to the even neighbour
inline int32_t half_even(int32_t d) {
  int32_t q = d >> 1;                                            // floor(d / 2)
  if ((d & 1) && (q & 1)) ++q;
  return q;
}

// ------------------------------------------------------------------------------------------------ tc_clip_patches

// Everything between the fp32 frames and the bf16 rows is summed in double: the CLIP mean cancels the pixel value, and for
// the outputs that land near zero one bf16 ulp is smaller than the rounding error of an fp32 sum of O(1) terms.

struct BlurTaps { double w[TC_CLIP_BLUR_TAPS]; };

// kornia's Gaussian for one axis: (sigma, odd kernel size) from the scale factor, weights normalised to sum one
struct BlurRule { double sigma; int ks; };
inline BlurRule blur_rule(double factor) {
  BlurRule r;
  r.sigma = (factor - 1.0) / 2.0 > 0.001 ? (factor - 1.0) / 2.0 : 0.001;
  const double k = 2.0 * 2.0 * r.sigma > 3.0 ? 2.0 * 2.0 * r.sigma : 3.0;
  r.ks = k > 1e6 ? 1000001 : (int)k;
  if (r.ks % 2 == 0) ++r.ks;
  return r;
}
inline void blur_taps(const BlurRule& r, BlurTaps* t) {      // r.ks <= TC_CLIP_BLUR_TAPS
  double sum = 0.0;
  for (int i = 0; i < TC_CLIP_BLUR_TAPS; ++i) {
    const double x = i - r.ks / 2;
    t->w[i] = i < r.ks ? exp(-(x * x) / (2.0 * r.sigma * r.sigma)) : 0.0;
    sum += t->w[i];
  }
  for (int i = 0; i < r.ks; ++i) t->w[i] /= sum;
}

__device__ __forceinline__ int reflect(int i, int n) {          // torch's 'reflect' padding: the edge sample is not repeated
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// one axis of the blur over planes of (h, w); ALONG_X: along a row, else along a column.  ks / 2 < the extent.
template <bool ALONG_X, typename In>
__global__ __launch_bounds__(256) void blur_kernel(const In* __restrict__ x, double* __restrict__ y, int h, int w, int ks,
                                                   BlurTaps taps, int64_t total) {
  const int half = ks / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int col = (int)(i % w);
    const int64_t r = i / w;
    const int row = (int)(r % h);
    const In* plane = x + (r / h) * ((int64_t)h * w);
    double acc = 0.0;
    for (int k = 0; k < ks; ++k) {
      const double v = ALONG_X ? plane[(int64_t)row * w + reflect(col + k - half, w)]
                               : plane[(int64_t)reflect(row + k - half, h) * w + col];
      acc += taps.w[k] * v;
    }
    y[i] = acc;
  }
}

// Keys cubic convolution, A = -0.75: weights of the taps at offsets -1, 0, 1, 2 for the fraction t in [0, 1)
__device__ __forceinline__ void cubic_taps(double t, double* c) {
  const double A = -0.75;
  const double u = 1.0 - t;
  c[0] = ((A * (t + 1.0) - 5.0 * A) * (t + 1.0) + 8.0 * A) * (t + 1.0) - 4.0 * A;
  c[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
  c[2] = ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0;
  c[3] = ((A * (u + 1.0) - 5.0 * A) * (u + 1.0) + 8.0 * A) * (u + 1.0) - 4.0 * A;
}

// align_corners=True: output index d of `out` samples reads source coordinate d * (in - 1) / (out - 1); its floor from an
// integer division (exact), its fraction from the remainder
__device__ __forceinline__ void source_coord(int d, int in, int out, int& i0, double& t) {
  if (out <= 1) { i0 = 0; t = 0.0; return; }
  const int64_t num = (int64_t)d * (in - 1);
  i0 = (int)(num / (out - 1));
  t = (double)(num - (int64_t)i0 * (out - 1)) / (double)(out - 1);
}

// double -> bf16 in ONE rounding: to fp32 toward zero with the inexact bit kept in the last place (round to odd), then the
// hardware's round-to-nearest-even to bf16, which that sticky bit makes the rounding of the double itself
__device__ __forceinline__ bf16_t bf16_once(double v) {
  float f = __double2float_rz(v);
  if ((double)f != v) f = __uint_as_float(__float_as_uint(f) | 1u);
  return (bf16_t)f;
}

// bicubic + CLIP normalisation + unfold: one thread per element of the [b * g * g, ld] rows
template <typename In>
__global__ __launch_bounds__(256) void clip_rows_kernel(const In* __restrict__ x, bf16_t* __restrict__ out, int h, int w,
                                                        int size, int patch, int ld, float m0, float m1, float m2, float s0,
                                                        float s1, float s2, int64_t total) {
  const int g = size / patch, pp = patch * patch;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int col = (int)(i % ld);
    if (col >= 3 * pp) {                                         // the K padding of the GEMM operand
      out[i] = (bf16_t)0.f;
      continue;
    }
    const int64_t row = i / ld;                                  // (sample, patch row, patch column)
    const int gx = (int)(row % g), gy = (int)((row / g) % g);
    const int64_t n = row / ((int64_t)g * g);
    const int c = col / pp, py = (col - c * pp) / patch, px = col - c * pp - py * patch;
    const int oy = gy * patch + py, ox = gx * patch + px;
    int y0, x0;
    double ty, tx, cy[4], cx[4];
    source_coord(oy, h, size, y0, ty);
    source_coord(ox, w, size, x0, tx);
    cubic_taps(ty, cy);
    cubic_taps(tx, cx);
    const In* plane = x + (n * 3 + c) * ((int64_t)h * w);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const In* line = plane + (int64_t)min(max(y0 - 1 + a, 0), h - 1) * w;
      double r = 0.0;
#pragma unroll
      for (int b = 0; b < 4; ++b) r += cx[b] * (double)line[min(max(x0 - 1 + b, 0), w - 1)];
      acc += cy[a] * r;
    }
    const double mean = c == 0 ? m0 : c == 1 ? m1 : m2, sd = c == 0 ? s0 : c == 1 ? s1 : s2;
    out[i] = bf16_once(((acc + 1.0) / 2.0 - mean) / sd);
  }
}

// what tc_clip_patches runs for a request, or the TC_E* code that refuses it
struct ClipPlan { bool blur; BlurRule ry, rx; int64_t plane_bytes; };
int clip_plan(const TcClipPatchesParams* p, ClipPlan* plan) {
  if (!p || !p->x || !p->out || p->b <= 0 || p->h <= 0 || p->w <= 0 || p->size <= 0 || p->patch <= 0) return TC_EINVAL;
  if (p->size % p->patch != 0) return TC_ESHAPE;
  if ((int64_t)p->ld < 3 * (int64_t)p->patch * p->patch) return TC_EINVAL;
  const double fy = (double)p->h / p->size, fx = (double)p->w / p->size;
  plan->blur = p->antialias != 0 && (fy > 1.0 || fx > 1.0);
  plan->plane_bytes = (int64_t)p->b * 3 * p->h * p->w * (int64_t)sizeof(double);
  if (plan->blur) {
    plan->ry = blur_rule(fy);
    plan->rx = blur_rule(fx);
    if (plan->ry.ks / 2 >= p->h || plan->rx.ks / 2 >= p->w) return TC_ESHAPE;          // the reflect border does not fit
    if (plan->ry.ks > TC_CLIP_BLUR_TAPS || plan->rx.ks > TC_CLIP_BLUR_TAPS) return TC_ESHAPE;
  }
  return TC_OK;
}

}  // namespace

extern "C" int tc_frames_from_u8_resized(int32_t sh, int32_t sw, int32_t h, int32_t w, int32_t* rh, int32_t* rw) {
  if (sh <= 0 || sw <= 0 || h <= 0 || w <= 0 || !rh || !rw) return TC_EINVAL;
  const int32_t s = h < w ? h : w;
  *rh = sh;
  *rw = sw;
  if ((sw <= sh ? sw : sh) == s) return TC_OK;                   // the shorter side is s already: PIL is not called
  // int(s * long / short) of the transform: a correctly rounded double division, truncated
  const bool portrait = sw < sh;
  const double other = portrait ? (double)((int64_t)s * sh) / (double)sw : (double)((int64_t)s * sw) / (double)sh;
  if (other >= 2147483647.0) return TC_EINVAL;
  *(portrait ? rw : rh) = s;
  *(portrait ? rh : rw) = (int32_t)other;
  return TC_OK;
}

namespace {

// What a request for n (sh, sw) images into a (b, 3, t, h, w) tensor runs, or TC_EINVAL: everything of TcFramesU8Params
// that does not describe the source's memory or the workspace.  Both front ends ask it.
struct FramesPlan { FrameSlots slots; int32_t rh, rw; bool resized; int64_t mid_bytes; };

// the sizing part, which the workspace query asks on its own: it reads n and the four sizes, nothing else
int frames_sizes(const TcFramesU8Params& p, FramesPlan* plan) {
  if (p.n <= 0 || tc_frames_from_u8_resized(p.sh, p.sw, p.h, p.w, &plan->rh, &plan->rw) != TC_OK) return TC_EINVAL;
  // the rule resizes both sides or neither: the shorter side changes whenever anything does, and the longer one then moves by
  // at least a pixel (s * long / short is below long for s < short and at least long + 1 for s > short)
  plan->resized = plan->rh != p.sh;
  plan->mid_bytes = plan->resized ? (int64_t)p.n * p.sh * plan->rw * 3 : 0;
  return TC_OK;
}

int frames_plan(const TcFramesU8Params& p, FramesPlan* plan) {
  if (!p.out || !p.slots || p.n > TC_FRAMES_U8_MAX || p.b <= 0 || p.t <= 0 || frames_sizes(p, plan) != TC_OK) return TC_EINVAL;
  plan->slots = {};
  for (int i = 0; i < p.n; ++i) {
    if (p.slots[i] < 0 || (int64_t)p.slots[i] >= (int64_t)p.b * p.t) return TC_EINVAL;
    plan->slots.v[i] = p.slots[i];
  }
  if (plan->resized && (!p.h_bounds || !p.h_coefs || p.h_kmax <= 0 || !p.v_bounds || !p.v_coefs || p.v_kmax <= 0)) return TC_EINVAL;
  return TC_OK;
}

// the launches of a planned request: packed uint8 images at p.src, the intermediate of the horizontal pass at `mid`
int frames_launch(const TcFramesU8Params& p, const FramesPlan& plan, uint8_t* mid, hipStream_t s) {
  const int32_t rh = plan.rh, rw = plan.rw;
  const int32_t top = half_even(rh - p.h), left = half_even(rw - p.w);
  const int64_t total = (int64_t)p.n * p.h * p.w;
  const dim3 grid(pixel_grid(total)), block(256);
  if (plan.resized) {
    const int64_t mid_total = (int64_t)p.n * p.sh * rw;
    hipLaunchKernelGGL(resample_hpass_kernel<uint8_t>, dim3(pixel_grid(mid_total)), block, 0, s, p.src, p.image_stride, p.pitch, p.sh, p.sw, rw,
                       p.h_bounds, p.h_coefs, p.h_kmax, mid, mid_total);
    TC_LAUNCH_CHECK();
    hipLaunchKernelGGL(frames_final_kernel<true>, grid, block, 0, s, (const uint8_t*)mid, (int64_t)p.sh * rw * 3, rw * 3, p.sh, rh,
                       rw, p.v_bounds, p.v_coefs, p.v_kmax, top, left, plan.slots, p.out, p.t, p.h, p.w, total);
  } else {
    hipLaunchKernelGGL(frames_final_kernel<false>, grid, block, 0, s, p.src, p.image_stride, p.pitch, p.sh, rh, rw,
                       (const int32_t*)nullptr, (const int32_t*)nullptr, 0, top, left, plan.slots, p.out, p.t, p.h, p.w, total);
  }
  TC_LAUNCH_CHECK();
  return TC_OK;
}

}  // namespace

extern "C" int64_t tc_frames_from_u8_workspace(const TcFramesU8Params* p) {
  FramesPlan plan;
  return p && frames_sizes(*p, &plan) == TC_OK ? plan.mid_bytes : 0;
}

extern "C" int tc_frames_from_u8(const TcFramesU8Params* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  const TcFramesU8Params& p = *pp;
  FramesPlan plan;
  if (!p.src || frames_plan(p, &plan) != TC_OK) return TC_EINVAL;
  if ((int64_t)p.pitch < 3 * (int64_t)p.sw || p.image_stride < (int64_t)p.sh * p.pitch) return TC_EINVAL;
  if (plan.mid_bytes > 0 && (!p.workspace || p.workspace_bytes < plan.mid_bytes)) return TC_EWORKSPACE;
  return frames_launch(p, plan, reinterpret_cast<uint8_t*>(p.workspace), reinterpret_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------------------------- tc_frames_from_yuv

namespace {

// n planar 4:2:0 images as the kernel addresses them: Cb and Cr are planes of their own (I420) or one plane read at element
// 2 i and 2 i + 1 (NV12, P010), which `cstep` and the Cr pointer say; `wide`: 16-bit words whose sample is word >> 6
struct YuvPlanes {
  const uint8_t* y; const uint8_t* cb; const uint8_t* cr;
  int64_t image_stride_y, image_stride_c;
  int pitch_y, pitch_c, cstep, wide;
};
struct YuvMatrix { int32_t cy, crv, cgu, cgv, cbu, yoff, coff; };

__device__ __forceinline__ int sample_at(const uint8_t* row, int idx, int wide) {
  return wide ? (int)(reinterpret_cast<const uint16_t*>(row)[idx] >> 6) : (int)row[idx];
}

// chroma sample (j, i) of one image's Cb or Cr plane of (ch, cw) samples, both indices clamped to the plane
__device__ __forceinline__ int chroma_at(const uint8_t* plane, const YuvPlanes& s, int ch, int cw, int j, int i) {
  j = min(max(j, 0), ch - 1);
  i = min(max(i, 0), cw - 1);
  return sample_at(plane + (int64_t)j * s.pitch_c, i * s.cstep, s.wide);
}

// the chroma value under luma pixel (y, x), at the source bit depth
__device__ __forceinline__ int chroma_up(const uint8_t* plane, const YuvPlanes& s, int ch, int cw, int siting, int y, int x) {
  const int j = y >> 1, i = x >> 1;
  if (siting == TC_CHROMA_NEAREST) return chroma_at(plane, s, ch, cw, j, i);
  const int jn = (y & 1) ? j + 1 : j - 1;                        // the other row the pixel lies between
  if (siting == TC_CHROMA_CENTER) {
    const int in = (x & 1) ? i + 1 : i - 1;
    return (9 * chroma_at(plane, s, ch, cw, j, i) + 3 * chroma_at(plane, s, ch, cw, j, in) + 3 * chroma_at(plane, s, ch, cw, jn, i) +
            chroma_at(plane, s, ch, cw, jn, in) + 8) >> 4;
  }
  // TC_CHROMA_LEFT: an even column sits on its sample, an odd one halfway to the next
  if (!(x & 1)) return (3 * chroma_at(plane, s, ch, cw, j, i) + chroma_at(plane, s, ch, cw, jn, i) + 2) >> 2;
  return (3 * chroma_at(plane, s, ch, cw, j, i) + 3 * chroma_at(plane, s, ch, cw, j, i + 1) + chroma_at(plane, s, ch, cw, jn, i) +
          chroma_at(plane, s, ch, cw, jn, i + 1) + 4) >> 3;
}

__device__ __forceinline__ uint8_t clip_u8(int32_t v) { return (uint8_t)min(max(v, 0), 255); }

// one thread per source pixel: n planar images (sh, sw) -> the packed RGB image (n, sh, sw, 3)
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(YuvPlanes s, int sh, int sw, int siting, YuvMatrix m,
                                                         uint8_t* __restrict__ rgb, int64_t total) {
  const int ch = (sh + 1) / 2, cw = (sw + 1) / 2;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int x = (int)(p % sw);
    const int64_t r = p / sw;
    const int y = (int)(r % sh);
    const int64_t img = r / sh;
    const int32_t c = sample_at(s.y + img * s.image_stride_y + (int64_t)y * s.pitch_y, x, s.wide) - m.yoff;
    const int32_t d = chroma_up(s.cb + img * s.image_stride_c, s, ch, cw, siting, y, x) - m.coff;
    const int32_t e = chroma_up(s.cr + img * s.image_stride_c, s, ch, cw, siting, y, x) - m.coff;
    rgb[p * 3 + 0] = clip_u8((m.cy * c + m.crv * e + 32768) >> 16);
    rgb[p * 3 + 1] = clip_u8((m.cy * c - m.cgu * d - m.cgv * e + 32768) >> 16);
    rgb[p * 3 + 2] = clip_u8((m.cy * c + m.cbu * d + 32768) >> 16);
  }
}

// the request as tc_frames_from_u8 sees it once the RGB image stands at `rgb`
TcFramesU8Params yuv_as_u8(const TcFramesYuvParams& p, const uint8_t* rgb) {
  TcFramesU8Params u = {};
  u.src = rgb; u.pitch = 3 * p.sw; u.image_stride = (int64_t)p.sh * p.sw * 3;
  u.n = p.n; u.sh = p.sh; u.sw = p.sw; u.slots = p.slots; u.out = p.out; u.b = p.b; u.t = p.t; u.h = p.h; u.w = p.w;
  u.h_bounds = p.h_bounds; u.h_coefs = p.h_coefs; u.h_kmax = p.h_kmax;
  u.v_bounds = p.v_bounds; u.v_coefs = p.v_coefs; u.v_kmax = p.v_kmax;
  return u;
}

}  // namespace

extern "C" int tc_yuv_matrix(int32_t standard, int32_t range, int32_t bits, int32_t m[7]) {
  if (!m || (standard != TC_YUV_BT601 && standard != TC_YUV_BT709) || (range != TC_YUV_LIMITED && range != TC_YUV_FULL) ||
      (bits != 8 && bits != 10))
    return TC_EINVAL;
  const double kr = standard == TC_YUV_BT601 ? 0.299 : 0.2126, kb = standard == TC_YUV_BT601 ? 0.114 : 0.0722;
  const double kg = 1.0 - kr - kb, q = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
  const double gy = range == TC_YUV_LIMITED ? 255.0 / (219.0 * q) : 255.0 / top;
  const double s = range == TC_YUV_LIMITED ? 255.0 / (224.0 * q) : 255.0 / top;
  const double v[5] = {gy, 2.0 * (1.0 - kr) * s, 2.0 * kb * (1.0 - kb) / kg * s, 2.0 * kr * (1.0 - kr) / kg * s, 2.0 * (1.0 - kb) * s};
  for (int i = 0; i < 5; ++i) m[i] = (int32_t)floor(v[i] * 65536.0 + 0.5);
  m[5] = range == TC_YUV_LIMITED ? 16 << (bits - 8) : 0;
  m[6] = 128 << (bits - 8);
  return TC_OK;
}

extern "C" int64_t tc_frames_from_yuv_workspace(const TcFramesYuvParams* p) {
  if (!p || p->n <= 0 || p->sh <= 0 || p->sw <= 0 || p->h <= 0 || p->w <= 0) return 0;
  const TcFramesU8Params u = yuv_as_u8(*p, nullptr);
  return (int64_t)p->n * p->sh * p->sw * 3 + tc_frames_from_u8_workspace(&u);
}

extern "C" int tc_frames_from_yuv(const TcFramesYuvParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  const TcFramesYuvParams& p = *pp;
  if (!p.y || !p.c0) return TC_EINVAL;
  if (p.format != TC_PIXFMT_I420 && p.format != TC_PIXFMT_NV12 && p.format != TC_PIXFMT_P010) return TC_EINVAL;
  if (p.siting != TC_CHROMA_NEAREST && p.siting != TC_CHROMA_CENTER && p.siting != TC_CHROMA_LEFT) return TC_EINVAL;
  const bool planar = p.format == TC_PIXFMT_I420, wide = p.format == TC_PIXFMT_P010;
  if (planar != (p.c1 != nullptr)) return TC_EINVAL;
  TcFramesU8Params u = yuv_as_u8(p, nullptr);
  FramesPlan plan;
  if (frames_plan(u, &plan) != TC_OK) return TC_EINVAL;              // n, sizes, slots, tables
  const int64_t ch = (p.sh + 1) / 2, cw = (p.sw + 1) / 2, bytes = wide ? 2 : 1;
  if ((int64_t)p.pitch_y < bytes * p.sw || (int64_t)p.pitch_c < (planar ? 1 : 2) * bytes * cw) return TC_EINVAL;
  if (p.image_stride_y < (int64_t)p.sh * p.pitch_y || p.image_stride_c < ch * p.pitch_c) return TC_EINVAL;
  if (p.m[0] <= 0) return TC_EINVAL;
  if (wide && (((reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.c0)) & 1u) || ((p.pitch_y | p.pitch_c) & 1) ||
               ((p.image_stride_y | p.image_stride_c) & 1)))
    return TC_EALIGN;
  const int64_t rgb_bytes = (int64_t)p.n * p.sh * p.sw * 3;
  if (!p.workspace || p.workspace_bytes < rgb_bytes + plan.mid_bytes) return TC_EWORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* rgb = reinterpret_cast<uint8_t*>(p.workspace);
  YuvPlanes src;
  src.y = reinterpret_cast<const uint8_t*>(p.y);
  src.cb = reinterpret_cast<const uint8_t*>(p.c0);
  src.cr = planar ? reinterpret_cast<const uint8_t*>(p.c1) : src.cb + bytes;      // the second sample of each pair
  src.image_stride_y = p.image_stride_y; src.image_stride_c = p.image_stride_c;
  src.pitch_y = p.pitch_y; src.pitch_c = p.pitch_c; src.cstep = planar ? 1 : 2; src.wide = wide ? 1 : 0;
  const YuvMatrix m = {p.m[0], p.m[1], p.m[2], p.m[3], p.m[4], p.m[5], p.m[6]};
  const int64_t total = (int64_t)p.n * p.sh * p.sw;
  hipLaunchKernelGGL(yuv_to_rgb_kernel, dim3(pixel_grid(total)), dim3(256), 0, s, src, p.sh, p.sw, p.siting, m, rgb, total);
  TC_LAUNCH_CHECK();
  u.src = rgb;
  return frames_launch(u, plan, rgb + rgb_bytes, s);
}

extern "C" int64_t tc_clip_patches_workspace(const TcClipPatchesParams* p) {
  ClipPlan plan;
  if (clip_plan(p, &plan) != TC_OK) return 0;
  return plan.blur ? 2 * plan.plane_bytes : 0;
}

extern "C" int tc_clip_patches(const TcClipPatchesParams* pp, void* stream) {
  ClipPlan plan;
  const int rc = clip_plan(pp, &plan);
  if (rc != TC_OK) return rc;
  const TcClipPatchesParams& p = *pp;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int g = p.size / p.patch;
  const int64_t rows_total = (int64_t)p.b * g * g * p.ld;
  bf16_t* out = reinterpret_cast<bf16_t*>(p.out);
  if (plan.blur) {
    if (!p.workspace || p.workspace_bytes < 2 * plan.plane_bytes) return TC_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(p.workspace) & 7u) return TC_EALIGN;
    double* rows = reinterpret_cast<double*>(p.workspace);
    double* cols = rows + plan.plane_bytes / (int64_t)sizeof(double);
    const int64_t total = (int64_t)p.b * 3 * p.h * p.w;
    BlurTaps taps;
    blur_taps(plan.rx, &taps);
    hipLaunchKernelGGL((blur_kernel<true, float>), dim3(pixel_grid(total)), dim3(256), 0, s, p.x, rows, p.h, p.w, plan.rx.ks, taps, total);
    TC_LAUNCH_CHECK();
    blur_taps(plan.ry, &taps);
    hipLaunchKernelGGL((blur_kernel<false, double>), dim3(pixel_grid(total)), dim3(256), 0, s, (const double*)rows, cols, p.h, p.w,
                       plan.ry.ks, taps, total);
    TC_LAUNCH_CHECK();
    hipLaunchKernelGGL(clip_rows_kernel<double>, dim3(pixel_grid(rows_total)), dim3(256), 0, s, (const double*)cols, out, p.h, p.w, p.size,
                       p.patch, p.ld, p.mean[0], p.mean[1], p.mean[2], p.std[0], p.std[1], p.std[2], rows_total);
  } else {
    hipLaunchKernelGGL(clip_rows_kernel<float>, dim3(pixel_grid(rows_total)), dim3(256), 0, s, p.x, out, p.h, p.w, p.size, p.patch, p.ld,
                       p.mean[0], p.mean[1], p.mean[2], p.std[0], p.std[1], p.std[2], rows_total);
  }
  TC_LAUNCH_CHECK();
  return TC_OK;
}
