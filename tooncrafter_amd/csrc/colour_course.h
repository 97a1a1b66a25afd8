// The course of a clip's frames through its knots (the rule: include/tooncrafter_hip.h, tc_colour_match), stated once for the
// two kernels that follow it: the coefficient kernel of tc_colour_match_knots (csrc/colour_match.hip) and the table kernel of
// tc_colour_transfer_knots (csrc/colour_hist.hip).  The knots are host values that travel in the kernel arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tooncrafter_hip.h"

// the knots as the launchers hand them to a kernel: checked (1 <= nk <= TC_TEMPORAL_MAX_FRAMES, strictly increasing, in [0, t))
struct TcColourKnots {
  int32_t nk;
  int32_t knot[TC_TEMPORAL_MAX_FRAMES];
};

// where frame f stands: `single` (before or on the first knot, on any knot, on or after the last) -- the target is knot j
// itself and w is 0; otherwise the target lies between knots j and j + 1 at w = (f - k_j) / (k_{j+1} - k_j), 0 < w < 1
struct TcColourCourse {
  int j;
  bool single;
  double w;
};

__host__ __device__ inline TcColourCourse tc_colour_course(const TcColourKnots& k, int f) {
  TcColourCourse c;
  c.j = 0;
  for (int i = 1; i < k.nk; ++i)
    if (k.knot[i] <= f) c.j = i;                                   // the last knot with k_j <= f (0 when there is none)
  c.single = f <= k.knot[c.j] || c.j == k.nk - 1;
  c.w = c.single ? 0.0 : (double)(f - k.knot[c.j]) / (double)(k.knot[c.j + 1] - k.knot[c.j]);
  return c;
}

// TC_OK for knots that the rule allows on a clip of t frames, TC_EINVAL otherwise
inline int tc_colour_knots_check(int32_t nk, const int32_t* knot, int32_t t) {
  if (nk < 1 || nk > TC_TEMPORAL_MAX_FRAMES) return TC_EINVAL;
  for (int i = 0; i < nk; ++i)
    if (knot[i] < 0 || knot[i] >= t || (i > 0 && knot[i] <= knot[i - 1])) return TC_EINVAL;
  return TC_OK;
}
