// tc_resize_tables: the coefficient tables of PIL's 8-bit BILINEAR resample for one axis, host code in double precision
// (Pillow src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc).  The device side (csrc/pixel_front.hip)
// only multiplies and adds these integers.  See include/tooncrafter_hip.h for the rule.
#include <math.h>

#include "tooncrafter_hip.h"

extern "C" int32_t tc_resize_tables(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coefs, int64_t coefs_len) {
  if (in_size <= 0 || out_size <= 0 || (bounds == nullptr) != (coefs == nullptr)) return TC_EINVAL;
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;                  // bilinear: support 1, stretched when downscaling
  const double support = fs;
  const double kd = ceil(support) * 2.0 + 1.0;
  if (kd > 1e9) return TC_EINVAL;
  const int32_t kmax = (int32_t)kd;
  if (!bounds) return kmax;                                     // sizing query
  if (coefs_len < (int64_t)out_size * kmax) return TC_EWORKSPACE;
  for (int32_t xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int32_t xmin = (int32_t)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int32_t xmax = (int32_t)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int32_t cnt = xmax - xmin;
    int32_t* k = coefs + (int64_t)xx * kmax;
    // the weights are summed in tap order, as PIL does (Pillow multiplies by 1 / fs where this divides; the integer tables
    // of the two forms are equal for every size pair 1 .. 128 and the frame sizes of tests/test_pixel_front_cpu.py)
    double ww = 0.0;
    for (int32_t x = 0; x < cnt; ++x) {
      double a = (x + xmin - center + 0.5) / fs;
      if (a < 0.0) a = -a;
      ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int32_t x = 0; x < kmax; ++x) {
      double w = 0.0;
      if (x < cnt) {
        double a = (x + xmin - center + 0.5) / fs;
        if (a < 0.0) a = -a;
        w = a < 1.0 ? 1.0 - a : 0.0;
        if (ww != 0.0) w /= ww;
      }
      k[x] = (int32_t)(w * (double)(1 << 22) + 0.5);           // bilinear weights are never negative
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = cnt;
  }
  return kmax;
}
