// tc_resize_tables / tc_resize_tables_filter: the coefficient tables of PIL's 8-bit resample for one axis, host code in
// double precision (Pillow src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc).  The device side
// (csrc/pixel_u8.h, run by csrc/pixel_front.hip and csrc/pixel_back.hip) only multiplies and adds these integers.  See
// include/tooncrafter_hip.h for the rule.
#include <math.h>

#include "tooncrafter_hip.h"

namespace {

// Pillow's filter functions (Resample.c: bilinear_filter, bicubic_filter, lanczos_filter, box_filter), 0 outside the support
double filter_bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
double filter_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double filter_lanczos(double x) { return -3.0 <= x && x < 3.0 ? sinc(x) * sinc(x / 3) : 0.0; }
double filter_box(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }

// The tables of one axis in_size -> out_size for the filter F of support S, or kmax alone when bounds is NULL.  The tap
// argument is multiplied by 1 / fs, as Pillow does.  Dividing by fs instead, as the numpy statement of
// tests/test_pixel_front_cpu.py does, gives the bilinear filter the same bounds, kmax and integer coefficients for every
// pair in, out in 1 .. 768 and for in in 1 .. 4320 with out in {224, 256, 320, 384, 512, 576, 640, 720, 1024, 1080} (checked
// on the host), so the one form serves both entry points.
int32_t resize_tables(double (*F)(double), double S, int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs,
                      int64_t coefs_len) {
  if (in_size <= 0 || out_size <= 0 || (bounds == nullptr) != (coefs == nullptr)) return TC_EINVAL;
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;                  // the filter is stretched when downscaling
  const double support = S * fs;
  const double kd = ceil(support) * 2.0 + 1.0;
  if (kd > 1e9) return TC_EINVAL;
  const int32_t kmax = (int32_t)kd;
  if (!bounds) return kmax;                                     // sizing query
  if (coefs_len < (int64_t)out_size * kmax) return TC_EWORKSPACE;
  const double ss = 1.0 / fs;
  for (int32_t xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int32_t xmin = (int32_t)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int32_t xmax = (int32_t)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int32_t cnt = xmax - xmin;
    int32_t* k = coefs + (int64_t)xx * kmax;
    double ww = 0.0;                                            // summed in tap order, as PIL does
    for (int32_t x = 0; x < cnt; ++x) ww += F((x + xmin - center + 0.5) * ss);
    for (int32_t x = 0; x < kmax; ++x) {
      double w = 0.0;
      if (x < cnt) {
        w = F((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
      }
      // the cast truncates toward zero, so a negative lobe rounds with -0.5
      k[x] = w < 0.0 ? (int32_t)(-0.5 + w * (double)(1 << 22)) : (int32_t)(0.5 + w * (double)(1 << 22));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = cnt;
  }
  return kmax;
}

}  // namespace

extern "C" int32_t tc_resize_tables(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs, int64_t coefs_len) {
  return resize_tables(filter_bilinear, 1.0, in_size, out_size, bounds, coefs, coefs_len);
}

extern "C" int32_t tc_resize_tables_filter(int32_t filter, int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs,
                                           int64_t coefs_len) {
  switch (filter) {
    case TC_RESIZE_BILINEAR: return resize_tables(filter_bilinear, 1.0, in_size, out_size, bounds, coefs, coefs_len);
    case TC_RESIZE_BICUBIC: return resize_tables(filter_bicubic, 2.0, in_size, out_size, bounds, coefs, coefs_len);
    case TC_RESIZE_LANCZOS: return resize_tables(filter_lanczos, 3.0, in_size, out_size, bounds, coefs, coefs_len);
    case TC_RESIZE_BOX: return resize_tables(filter_box, 0.5, in_size, out_size, bounds, coefs, coefs_len);
    default: return TC_EINVAL;
  }
}
