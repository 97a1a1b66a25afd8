// Pixel back end, gfx950: the decoder's fp32 clips -> uint8 frames at a chosen size, as packed RGB, I420 or NV12, written
// to named places of a longer video (tc_frames_to_u8), and the same planes in a colour the caller names -- any integer
// matrix, centre or left chroma siting, 8 bit or 10-bit P010 (tc_frames_to_yuv).  It runs once per clip batch on a few
// megabytes, so, like the front end, every kernel is one thread per output element (per 2 x 2 block for the YUV write),
// written for the arithmetic to be read off the code: the resample must give PIL's bytes and the colour conversion the
// integers of the header.  See include/tooncrafter_hip.h.
#include "common.h"
#include "pixel_u8.h"

#include <math.h>

namespace {

// Where image m = clip * nf + j (frame f0 + j of its clip) starts in a destination: the caller's `out`, or a packed staging
// buffer (frame_stride = one image, clip_stride = nf images).  Strides count samples of the destination's type.
struct Place { int nf; int64_t frame_stride, clip_stride; };
__device__ __forceinline__ int64_t place_of(const Place& pl, int64_t m) {
  const int64_t clip = m / pl.nf;
  return clip * pl.clip_stride + (m - clip * pl.nf) * pl.frame_stride;
}

// A decoded sample as the 16-bit intermediate of the 10-bit output: clamp, (v + 1) / 2, * 65535, round half up.  Every
// operation is rounded on its own, in this order: the product and the + 0.5 must not become one fma.
__device__ __forceinline__ uint16_t sample_to_u16(float v) {
#pragma clang fp contract(off)
  v = fminf(fmaxf(v, -1.f), 1.f);
  v = (v + 1.0f) / 2.0f;
  const float s = v * 65535.0f;
  return (uint16_t)floorf(s + 0.5f);
}
__device__ __forceinline__ void sample_to(float v, uint8_t* q) { *q = sample_to_u8(v); }
__device__ __forceinline__ void sample_to(float v, uint16_t* q) { *q = sample_to_u16(v); }

// value: frames f0 .. f0 + nf - 1 of x (b, 3, t, h, w) fp32 -> HWC images of uint8 or uint16 samples with a row pitch (in
// samples), one thread per pixel
template <typename T>
__global__ __launch_bounds__(256) void frames_value_kernel(const float* __restrict__ x, int t, int f0, int h, int w,
                                                           T* __restrict__ dst, Place pl, int64_t pitch, int64_t total) {
  const int64_t hw = (int64_t)h * w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int col = (int)(i % w);
    const int64_t r = i / w;
    const int row = (int)(r % h);
    const int64_t m = r / h, clip = m / pl.nf, f = f0 + (m - clip * pl.nf);
    T* px = dst + place_of(pl, m) + row * pitch + (int64_t)col * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) sample_to(x[((clip * 3 + c) * t + f) * hw + (int64_t)row * w + col], px + c);
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

// ------------------------------------------------------------------------------------------------- tc_frames_to_yuv

// the request's matrix as the kernel takes it: one row per output component
struct OutMatrix { int32_t y[3], cb[3], cr[3], yoff, coff; };

// What the RGB sample type says about the colour step: F = 8 + its bits, the top code, and how a code is stored (as it is, or
// in the upper ten bits of a P010 word)
template <typename T> struct Depth;
template <> struct Depth<uint8_t> { static constexpr int F = 16, top = 255, low_bits = 0; };
template <> struct Depth<uint16_t> { static constexpr int F = 24, top = 1023, low_bits = 6; };

// clip((k . p + (off << shift) + (1 << (shift - 1))) >> shift, 0, top) as the stored sample; the sum is signed, the shift
// arithmetic, the clip two-sided
template <typename T, typename P>
__device__ __forceinline__ T colour_code(const int32_t* k, const P* p, int32_t off, int shift) {
  using Acc = typename Resample<T>::Acc;
  Acc v = (Acc)k[0] * (Acc)p[0] + (Acc)k[1] * (Acc)p[1] + (Acc)k[2] * (Acc)p[2] + ((Acc)off << shift) + ((Acc)1 << (shift - 1));
  v >>= shift;
  v = v < 0 ? (Acc)0 : v > (Acc)Depth<T>::top ? (Acc)Depth<T>::top : v;
  return (T)(v << Depth<T>::low_bits);
}

// vertical pass (or none) + the YUV write by the request's matrix, one thread per chroma sample (bx, by): the four Y samples
// of its 2 x 2 block, one Cb, one Cr.  Chroma from the block's sums (centre siting, weights 1 1 / 1 1, shift F + 2) or,
// `left`, from columns 2 bx - 1 (clamped to 0), 2 bx, 2 bx + 1 of both rows with weights 1 2 1 (shift F + 3): six resized
// pixels instead of four.  `pitch` and the places count samples; I420 / `nv12` as in frames_out_yuv_kernel.
template <bool VRES, typename T>
__global__ __launch_bounds__(256) void frames_out_colour_kernel(const T* __restrict__ img, int ih, int oh, int ow,
                                                                const int32_t* __restrict__ bounds,
                                                                const int32_t* __restrict__ coefs, int kmax,
                                                                T* __restrict__ out, Place pl, int64_t pitch, int nv12, int left,
                                                                OutMatrix mat, int64_t total) {
  using Acc = typename Resample<T>::Acc;
  constexpr int F = Depth<T>::F;
  const int cw = ow / 2, ch = oh / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int bx = (int)(i % cw);
    const int64_t r = i / cw;
    const int by = (int)(r % ch);
    const int64_t m = r / ch;
    const T* image = img + m * ((int64_t)ih * ow * 3);
    T* frame = out + place_of(pl, m);
    Acc sum[3] = {0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int row = 2 * by + dy;
      int32_t rgb[3];
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        resized_pixel<VRES>(image, (int64_t)ow * 3, ih, bounds, coefs, kmax, row, 2 * bx + dx, rgb);
        frame[row * pitch + 2 * bx + dx] = colour_code<T>(mat.y, rgb, mat.yoff, F);
        const int32_t weight = left && dx == 0 ? 2 : 1;          // left: the sample sits on column 2 bx
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += weight * rgb[c];
      }
      if (left) {
        resized_pixel<VRES>(image, (int64_t)ow * 3, ih, bounds, coefs, kmax, row, max(2 * bx - 1, 0), rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += rgb[c];
      }
    }
    const int shift = F + (left ? 3 : 2);
    const T cb = colour_code<T>(mat.cb, sum, mat.coff, shift), cr = colour_code<T>(mat.cr, sum, mat.coff, shift);
    T* chroma = frame + pitch * oh;
    if (nv12) {
      chroma[by * pitch + 2 * bx] = cb;
      chroma[by * pitch + 2 * bx + 1] = cr;
    } else {
      const int64_t cpitch = pitch / 2;
      chroma[by * cpitch + bx] = cb;
      chroma[cpitch * ch + by * cpitch + bx] = cr;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ requests

// What a back-end request runs, or the TC_E* code that refuses it.  Both entry points ask it: tc_frames_to_yuv hands its
// fields over as a TcFramesOutParams with `sample` = the bytes of one output sample (2 for P010, which is then laid out as
// NV12 in words); stage_bytes / mid_bytes hold samples of that size.
struct OutPlan { bool hres, vres, staged; int64_t stage_bytes, mid_bytes; };
int out_plan(const TcFramesOutParams* pp, OutPlan* plan, int64_t sample = 1) {
  if (!pp) return TC_EINVAL;
  const TcFramesOutParams& p = *pp;
  if (!p.x || !p.out || p.b <= 0 || p.t <= 0 || p.h <= 0 || p.w <= 0 || p.oh <= 0 || p.ow <= 0) return TC_EINVAL;
  if (p.f0 < 0 || p.nf < 1 || (int64_t)p.f0 + p.nf > p.t) return TC_EINVAL;
  if (p.format != TC_PIXFMT_RGB24 && p.format != TC_PIXFMT_I420 && p.format != TC_PIXFMT_NV12) return TC_EINVAL;
  const bool rgb = p.format == TC_PIXFMT_RGB24;
  if (!rgb && ((p.oh | p.ow) & 1)) return TC_ESHAPE;
  if (p.format == TC_PIXFMT_I420 && (p.pitch & 1)) return TC_ESHAPE;
  if ((int64_t)p.pitch < sample * (rgb ? 3 * (int64_t)p.ow : (int64_t)p.ow)) return TC_EINVAL;
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
  plan->stage_bytes = plan->staged ? n * p.h * p.w * 3 * sample : 0;
  plan->mid_bytes = plan->hres ? n * p.h * p.ow * 3 * sample : 0;
  return TC_OK;
}

// The value pass into the packed staging buffer at `stage` and, where the width changes, the horizontal pass into `mid` behind
// it; *img: the n packed images of p.h rows and p.ow columns that the write kernels read
template <typename T>
int stage_frames(const TcFramesOutParams& p, const OutPlan& plan, T* stage, hipStream_t s, const T** img) {
  const dim3 block(256);
  const int64_t n = (int64_t)p.b * p.nf, src_total = n * p.h * p.w, image = (int64_t)p.h * p.w * 3;
  const Place packed = {p.nf, image, (int64_t)p.nf * image};
  hipLaunchKernelGGL(frames_value_kernel<T>, dim3(pixel_grid(src_total)), block, 0, s, p.x, p.t, p.f0, p.h, p.w, stage, packed,
                     (int64_t)p.w * 3, src_total);
  TC_LAUNCH_CHECK();
  *img = stage;
  if (plan.hres) {
    T* mid = stage + plan.stage_bytes / (int64_t)sizeof(T);
    const int64_t mid_total = n * p.h * p.ow;
    hipLaunchKernelGGL(resample_hpass_kernel<T>, dim3(pixel_grid(mid_total)), block, 0, s, (const T*)stage, image, p.w * 3, p.h, p.w,
                       p.ow, p.h_bounds, p.h_coefs, p.h_kmax, mid, mid_total);
    TC_LAUNCH_CHECK();
    *img = mid;
  }
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
    hipLaunchKernelGGL(frames_value_kernel<uint8_t>, dim3(pixel_grid(src_total)), block, 0, s, p.x, p.t, p.f0, p.h, p.w, p.out,
                       to_out, (int64_t)p.pitch, src_total);
    TC_LAUNCH_CHECK();
    return TC_OK;
  }
  const uint8_t* img;                                            // n packed images of p.h rows and p.ow columns
  const int staged = stage_frames(p, plan, reinterpret_cast<uint8_t*>(p.workspace), s, &img);
  if (staged != TC_OK) return staged;
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

extern "C" int tc_yuv_out_matrix(int32_t standard, int32_t range, int32_t bits, int32_t m[11]) {
  if (!m || (standard != TC_YUV_BT601 && standard != TC_YUV_BT709) || (range != TC_YUV_LIMITED && range != TC_YUV_FULL) ||
      (bits != 8 && bits != 10))
    return TC_EINVAL;
  const double kr = standard == TC_YUV_BT601 ? 0.299 : 0.2126, kb = standard == TC_YUV_BT601 ? 0.114 : 0.0722;
  const int bits_in = bits == 8 ? 8 : 16;
  const double one = (double)((int64_t)1 << (8 + bits_in)), inmax = (double)((1 << bits_in) - 1), q = (double)(1 << (bits - 8));
  const double gy = range == TC_YUV_LIMITED ? 219.0 * q / inmax : (double)((1 << bits) - 1) / inmax;
  const double gc = range == TC_YUV_LIMITED ? 224.0 * q / inmax : gy;
  auto r = [one](double v) { return (int32_t)floor(v * one + 0.5); };
  m[0] = r(kr * gy);
  m[2] = r(kb * gy);
  m[1] = r(gy) - m[0] - m[2];                                    // white lands exactly
  m[5] = m[6] = r(gc / 2.0);
  m[3] = r(-kr / (2.0 * (1.0 - kb)) * gc);
  m[4] = -(m[5] + m[3]);                                         // the chroma rows sum to 0: grey is neutral
  m[8] = r(-kb / (2.0 * (1.0 - kr)) * gc);
  m[7] = -(m[6] + m[8]);
  m[9] = range == TC_YUV_LIMITED ? 16 << (bits - 8) : 0;
  m[10] = 128 << (bits - 8);
  return TC_OK;
}

namespace {

// tc_frames_to_yuv's request as out_plan sees it (P010 as NV12 in 2-byte samples), or the code that refuses it for anything
// but its workspace
int yuv_out_plan(const TcFramesYuvOutParams* pp, TcFramesOutParams* base, OutPlan* plan) {
  if (!pp) return TC_EINVAL;
  const TcFramesYuvOutParams& p = *pp;
  if (p.format != TC_PIXFMT_I420 && p.format != TC_PIXFMT_NV12 && p.format != TC_PIXFMT_P010) return TC_EINVAL;
  if (p.siting != TC_CHROMA_CENTER && p.siting != TC_CHROMA_LEFT) return TC_EINVAL;
  if (p.m[0] <= 0 || p.m[1] <= 0 || p.m[2] <= 0) return TC_EINVAL;
  const bool wide = p.format == TC_PIXFMT_P010;
  TcFramesOutParams& u = *base;
  u = {};
  u.x = p.x; u.out = reinterpret_cast<uint8_t*>(p.out);
  u.b = p.b; u.t = p.t; u.h = p.h; u.w = p.w; u.f0 = p.f0; u.nf = p.nf; u.oh = p.oh; u.ow = p.ow;
  u.format = wide ? (int32_t)TC_PIXFMT_NV12 : p.format;
  u.pitch = p.pitch; u.frame_stride = p.frame_stride; u.clip_stride = p.clip_stride;
  u.h_bounds = p.h_bounds; u.h_coefs = p.h_coefs; u.h_kmax = p.h_kmax;
  u.v_bounds = p.v_bounds; u.v_coefs = p.v_coefs; u.v_kmax = p.v_kmax;
  u.workspace = p.workspace; u.workspace_bytes = p.workspace_bytes;
  const int rc = out_plan(base, plan, wide ? 2 : 1);
  if (rc != TC_OK) return rc;
  if (wide && (((reinterpret_cast<uintptr_t>(p.out) | reinterpret_cast<uintptr_t>(p.workspace)) & 1u) || (p.pitch & 1) ||
               ((p.frame_stride | p.clip_stride) & 1)))
    return TC_EALIGN;
  return TC_OK;
}

// the write kernel of a planned request on samples of type T
template <typename T>
int yuv_out_launch(const TcFramesYuvOutParams& p, const TcFramesOutParams& u, const OutPlan& plan, hipStream_t s) {
  const T* img;
  const int staged = stage_frames(u, plan, reinterpret_cast<T*>(p.workspace), s, &img);
  if (staged != TC_OK) return staged;
  const int64_t bytes = (int64_t)sizeof(T), total = (int64_t)p.b * p.nf * (p.oh / 2) * (p.ow / 2);
  const Place to_out = {p.nf, p.frame_stride / bytes, p.clip_stride / bytes};
  const OutMatrix mat = {{p.m[0], p.m[1], p.m[2]}, {p.m[3], p.m[4], p.m[5]}, {p.m[6], p.m[7], p.m[8]}, p.m[9], p.m[10]};
  const int nv12 = p.format != TC_PIXFMT_I420, left = p.siting == TC_CHROMA_LEFT;
  const dim3 grid(pixel_grid(total)), block(256);
#define TC_FRAMES_YUV_LAUNCH(VRES) \
  hipLaunchKernelGGL((frames_out_colour_kernel<VRES, T>), grid, block, 0, s, img, p.h, p.oh, p.ow, p.v_bounds, p.v_coefs, p.v_kmax, \
                     reinterpret_cast<T*>(p.out), to_out, (int64_t)p.pitch / bytes, nv12, left, mat, total)
  if (plan.vres) TC_FRAMES_YUV_LAUNCH(true); else TC_FRAMES_YUV_LAUNCH(false);
#undef TC_FRAMES_YUV_LAUNCH
  TC_LAUNCH_CHECK();
  return TC_OK;
}

}  // namespace

extern "C" int64_t tc_frames_to_yuv_workspace(const TcFramesYuvOutParams* p) {
  TcFramesOutParams base;
  OutPlan plan;
  return yuv_out_plan(p, &base, &plan) == TC_OK ? plan.stage_bytes + plan.mid_bytes : 0;
}

extern "C" int tc_frames_to_yuv(const TcFramesYuvOutParams* pp, void* stream) {
  TcFramesOutParams base;
  OutPlan plan;
  const int rc = yuv_out_plan(pp, &base, &plan);
  if (rc != TC_OK) return rc;
  const TcFramesYuvOutParams& p = *pp;
  if (!p.workspace || p.workspace_bytes < plan.stage_bytes + plan.mid_bytes) return TC_EWORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return p.format == TC_PIXFMT_P010 ? yuv_out_launch<uint16_t>(p, base, plan, s) : yuv_out_launch<uint8_t>(p, base, plan, s);
}
