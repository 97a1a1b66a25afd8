// Pixel back end, gfx950: the decoder's fp32 clips -> uint8 frames at a chosen size, as packed RGB, I420 or NV12, written
// to named places of a longer video (tc_frames_to_u8).  It runs once per clip batch on a few megabytes, so, like the front
// end, every kernel is one thread per output element (per 2 x 2 block for the YUV write), written for the arithmetic to be
// read off the code: the resample must give PIL's bytes and the colour conversion the integers of the header.
// See include/tooncrafter_hip.h.
#include "common.h"
#include "pixel_u8.h"

namespace {

// Where image m = clip * nf + j (frame f0 + j of its clip) starts in a destination: the caller's `out`, or a packed staging
// buffer (frame_stride = one image, clip_stride = nf images).
struct Place { int nf; int64_t frame_stride, clip_stride; };
__device__ __forceinline__ int64_t place_of(const Place& pl, int64_t m) {
  const int64_t clip = m / pl.nf;
  return clip * pl.clip_stride + (m - clip * pl.nf) * pl.frame_stride;
}

// value: frames f0 .. f0 + nf - 1 of x (b, 3, t, h, w) fp32 -> uint8 HWC images with a row pitch, one thread per pixel
__global__ __launch_bounds__(256) void frames_value_kernel(const float* __restrict__ x, int t, int f0, int h, int w,
                                                           uint8_t* __restrict__ dst, Place pl, int64_t pitch, int64_t total) {
  const int64_t hw = (int64_t)h * w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int col = (int)(i % w);
    const int64_t r = i / w;
    const int row = (int)(r % h);
    const int64_t m = r / h, clip = m / pl.nf, f = f0 + (m - clip * pl.nf);
    uint8_t* px = dst + place_of(pl, m) + row * pitch + (int64_t)col * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = sample_to_u8(x[((clip * 3 + c) * t + f) * hw + (int64_t)row * w + col]);
  }
}

// The horizontal pass (resample_hpass_kernel) and the pixel under (row, col) of the (oh, ow) frame (resized_pixel<VRES>:
// resampled over the ih rows of a packed image of ow columns, or that image is the frame already) are pixel_u8.h's: the
// front end runs them too.

// vertical pass (or none) + RGB24 write, one thread per output pixel
template <bool VRES>
__global__ __launch_bounds__(256) void frames_out_rgb_kernel(const uint8_t* __restrict__ img, int ih, int oh, int ow,
                                                             const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ coefs, int kmax,
                                                             uint8_t* __restrict__ out, Place pl, int pitch, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int col = (int)(i % ow);
    const int64_t r = i / ow;
    const int row = (int)(r % oh);
    const int64_t m = r / oh;
    int32_t rgb[3];
    resized_pixel<VRES>(img + m * ((int64_t)ih * ow * 3), (int64_t)ow * 3, ih, bounds, coefs, kmax, row, col, rgb);
    uint8_t* px = out + place_of(pl, m) + (int64_t)row * pitch + (int64_t)col * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (uint8_t)rgb[c];
  }
}

// BT.601 limited range in integers (the header states the rows); every shifted quantity is non-negative
__device__ __forceinline__ uint8_t luma_601(const int32_t* p) {
  return (uint8_t)min((16829 * p[0] + 33039 * p[1] + 6416 * p[2] + (16 << 16) + (1 << 15)) >> 16, 255);
}
__device__ __forceinline__ uint8_t chroma_601(int32_t kr, int32_t kg, int32_t kb, const int32_t* s) {
  return (uint8_t)min(max((kr * s[0] + kg * s[1] + kb * s[2] + (128 << 18) + (1 << 17)) >> 18, 0), 255);
}

// vertical pass (or none) + the YUV write, one thread per 2 x 2 block: four Y samples, one Cb, one Cr.  I420: Cb and Cr
// planes with rows pitch / 2 apart; NV12: one plane of Cb, Cr pairs with rows `pitch` apart.
template <bool VRES, bool NV12>
__global__ __launch_bounds__(256) void frames_out_yuv_kernel(const uint8_t* __restrict__ img, int ih, int oh, int ow,
                                                             const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ coefs, int kmax,
                                                             uint8_t* __restrict__ out, Place pl, int pitch, int64_t total) {
  const int cw = ow / 2, ch = oh / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int bx = (int)(i % cw);
    const int64_t r = i / cw;
    const int by = (int)(r % ch);
    const int64_t m = r / ch;
    const uint8_t* image = img + m * ((int64_t)ih * ow * 3);
    uint8_t* frame = out + place_of(pl, m);
    int32_t sum[3] = {0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int32_t rgb[3];
        resized_pixel<VRES>(image, (int64_t)ow * 3, ih, bounds, coefs, kmax, 2 * by + dy, 2 * bx + dx, rgb);
        frame[(int64_t)(2 * by + dy) * pitch + 2 * bx + dx] = luma_601(rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += rgb[c];
      }
    const uint8_t cb = chroma_601(-9714, -19070, 28784, sum), cr = chroma_601(28784, -24103, -4681, sum);
    uint8_t* chroma = frame + (int64_t)pitch * oh;
    if (NV12) {
      chroma[(int64_t)by * pitch + 2 * bx] = cb;
      chroma[(int64_t)by * pitch + 2 * bx + 1] = cr;
    } else {
      const int64_t cpitch = pitch / 2;
      chroma[by * cpitch + bx] = cb;
      chroma[cpitch * ch + by * cpitch + bx] = cr;
    }
  }
}

// what tc_frames_to_u8 runs for a request, or the TC_E* code that refuses it
struct OutPlan { bool hres, vres, staged; int64_t stage_bytes, mid_bytes; };
int out_plan(const TcFramesOutParams* pp, OutPlan* plan) {
  if (!pp) return TC_EINVAL;
  const TcFramesOutParams& p = *pp;
  if (!p.x || !p.out || p.b <= 0 || p.t <= 0 || p.h <= 0 || p.w <= 0 || p.oh <= 0 || p.ow <= 0) return TC_EINVAL;
  if (p.f0 < 0 || p.nf < 1 || (int64_t)p.f0 + p.nf > p.t) return TC_EINVAL;
  if (p.format != TC_PIXFMT_RGB24 && p.format != TC_PIXFMT_I420 && p.format != TC_PIXFMT_NV12) return TC_EINVAL;
  const bool rgb = p.format == TC_PIXFMT_RGB24;
  if (!rgb && ((p.oh | p.ow) & 1)) return TC_ESHAPE;
  if (p.format == TC_PIXFMT_I420 && (p.pitch & 1)) return TC_ESHAPE;
  if ((int64_t)p.pitch < (rgb ? 3 * (int64_t)p.ow : (int64_t)p.ow)) return TC_EINVAL;
  const int64_t plane = (int64_t)p.pitch * p.oh;
  const int64_t frame_bytes = rgb ? plane : p.format == TC_PIXFMT_I420 ? plane + 2 * (int64_t)(p.pitch / 2) * (p.oh / 2)
                                                                        : plane + (int64_t)p.pitch * (p.oh / 2);
  if (p.frame_stride < frame_bytes) return TC_EINVAL;
  if (p.b > 1 && p.clip_stride < (int64_t)p.nf * p.frame_stride) return TC_EINVAL;
  plan->hres = p.ow != p.w;
  plan->vres = p.oh != p.h;
  if (plan->hres && (!p.h_bounds || !p.h_coefs || p.h_kmax <= 0)) return TC_EINVAL;
  if (plan->vres && (!p.v_bounds || !p.v_coefs || p.v_kmax <= 0)) return TC_EINVAL;
  plan->staged = plan->hres || plan->vres || !rgb;
  const int64_t n = (int64_t)p.b * p.nf;
  plan->stage_bytes = plan->staged ? n * p.h * p.w * 3 : 0;
  plan->mid_bytes = plan->hres ? n * p.h * p.ow * 3 : 0;
  return TC_OK;
}

}  // namespace

extern "C" int64_t tc_frames_to_u8_workspace(const TcFramesOutParams* p) {
  OutPlan plan;
  return out_plan(p, &plan) == TC_OK ? plan.stage_bytes + plan.mid_bytes : 0;
}

extern "C" int tc_frames_to_u8(const TcFramesOutParams* pp, void* stream) {
  OutPlan plan;
  const int rc = out_plan(pp, &plan);
  if (rc != TC_OK) return rc;
  const TcFramesOutParams& p = *pp;
  if (plan.staged && (!p.workspace || p.workspace_bytes < plan.stage_bytes + plan.mid_bytes)) return TC_EWORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 block(256);
  const int64_t n = (int64_t)p.b * p.nf;
  const Place to_out = {p.nf, p.frame_stride, p.clip_stride};
  const int64_t src_total = n * p.h * p.w;
  if (!plan.staged) {                                            // packed RGB at the source size: the value pass writes `out`
    hipLaunchKernelGGL(frames_value_kernel, dim3(pixel_grid(src_total)), block, 0, s, p.x, p.t, p.f0, p.h, p.w, p.out, to_out,
                       (int64_t)p.pitch, src_total);
    TC_LAUNCH_CHECK();
    return TC_OK;
  }
  uint8_t* stage = reinterpret_cast<uint8_t*>(p.workspace);
  const int64_t image = (int64_t)p.h * p.w * 3;
  const Place packed = {p.nf, image, (int64_t)p.nf * image};
  hipLaunchKernelGGL(frames_value_kernel, dim3(pixel_grid(src_total)), block, 0, s, p.x, p.t, p.f0, p.h, p.w, stage, packed,
                     (int64_t)p.w * 3, src_total);
  TC_LAUNCH_CHECK();
  const uint8_t* img = stage;                                    // n packed images of p.h rows and p.ow columns from here on
  if (plan.hres) {
    uint8_t* mid = stage + plan.stage_bytes;
    const int64_t mid_total = n * p.h * p.ow;
    hipLaunchKernelGGL(resample_hpass_kernel, dim3(pixel_grid(mid_total)), block, 0, s, (const uint8_t*)stage, image, p.w * 3, p.h, p.w,
                       p.ow, p.h_bounds, p.h_coefs, p.h_kmax, mid, mid_total);
    TC_LAUNCH_CHECK();
    img = mid;
  }
  const int64_t total = p.format == TC_PIXFMT_RGB24 ? n * p.oh * p.ow : n * (p.oh / 2) * (p.ow / 2);
  const dim3 grid(pixel_grid(total));
#define TC_FRAMES_OUT_LAUNCH(kernel) \
  hipLaunchKernelGGL(kernel, grid, block, 0, s, img, p.h, p.oh, p.ow, p.v_bounds, p.v_coefs, p.v_kmax, p.out, to_out, p.pitch, total)
  if (p.format == TC_PIXFMT_RGB24) {
    if (plan.vres) TC_FRAMES_OUT_LAUNCH(frames_out_rgb_kernel<true>); else TC_FRAMES_OUT_LAUNCH(frames_out_rgb_kernel<false>);
  } else if (p.format == TC_PIXFMT_I420) {
    if (plan.vres) TC_FRAMES_OUT_LAUNCH((frames_out_yuv_kernel<true, false>)); else TC_FRAMES_OUT_LAUNCH((frames_out_yuv_kernel<false, false>));
  } else {
    if (plan.vres) TC_FRAMES_OUT_LAUNCH((frames_out_yuv_kernel<true, true>)); else TC_FRAMES_OUT_LAUNCH((frames_out_yuv_kernel<false, true>));
  }
#undef TC_FRAMES_OUT_LAUNCH
  TC_LAUNCH_CHECK();
  return TC_OK;
}
