// What the two colour files ask of a request before they launch (tc_colour_stats / tc_colour_match* in colour_match.hip,
// tc_colour_hist / tc_colour_transfer* in colour_hist.hip; the rule: include/tooncrafter_hip.h): the clamp, the frame slots of a
// statistics or histogram request, and the clip request that match and transfer share -- its TC_EINVAL rules, chunks, vector
// loads and knots.  Each stands here once, so the two files cannot drift apart; the course through the knots is
// csrc/colour_course.h.  A file keeps what is its own: its alignment, its limits, its workspace, its kernels.
#pragma once
#include <cmath>

#include "common.h"
#include "colour_course.h"

namespace {

constexpr int COLOUR_THREADS = 256;               // the block of every streaming kernel of the two files
constexpr int COLOUR_MAX_CHUNKS = 64;

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

// Frame slots: frames f0, f0 + fstep, ... (nf of them) of every clip, slot = clip * nf + j.  TC_OK for the slots that P
// (TcColourStatsParams, TcColourHistParams) asks for into `result`, TC_EINVAL otherwise
template <typename P>
inline int colour_slots_check(const P& p, const void* result) {
  if (!p.x || !result || p.b <= 0 || p.t <= 0 || p.h <= 0 || p.w <= 0 || p.nf <= 0) return TC_EINVAL;
  if (p.f0 < 0 || p.f0 >= p.t || (p.nf > 1 && p.fstep < 1)) return TC_EINVAL;
  if (p.nf > 1 && (int64_t)p.f0 + (int64_t)(p.nf - 1) * p.fstep > (int64_t)p.t - 1) return TC_EINVAL;
  return TC_OK;
}

// the step as the kernels take it: a single frame has none
inline int colour_fstep(int nf, int fstep) { return nf > 1 ? fstep : 1; }

struct ColourSlot { int clip, f; };

__device__ __forceinline__ ColourSlot colour_slot(int slot, int f0, int nf, int fstep) {
  const int clip = slot / nf;
  return {clip, f0 + (slot - clip * nf) * fstep};
}

// parts of a frame of hw pixels: a function of hw alone (where sums are floating point their order is part of the result)
inline int colour_parts(int64_t hw, int64_t part_pixels, int max_parts) {
  const int64_t p = (hw + part_pixels - 1) / part_pixels;
  return (int)(p < 1 ? 1 : p > max_parts ? max_parts : p);
}

inline bool colour_overlap(uintptr_t a, uintptr_t b, uintptr_t bytes) { return a < b + bytes && b < a + bytes; }

// The clip request of a match or a transfer (P: TcColourMatchKnotsParams, TcColourTransferKnotsParams), the TC_EINVAL rules both
// share: pointers (`result`: coefs or table) and sizes, strength finite in [0, 1], reference pixels, the knots; out may be exactly
// x and overlap it in no other way, and a `base` (transfer only, else null) not at all.
template <typename P>
inline int colour_clip_check(const P& p, const void* result, const float* base) {
  if (!p.x || !p.out || !p.src || !p.ref || !result || p.b <= 0 || p.t <= 0 || p.h <= 0 || p.w <= 0) return TC_EINVAL;
  if (!std::isfinite(p.strength) || p.strength < 0.f || p.strength > 1.f || p.ref_pixels <= 0) return TC_EINVAL;
  if (const int rc = tc_colour_knots_check(p.nk, p.knot, p.t)) return rc;
  const uintptr_t bytes = (uintptr_t)p.b * p.t * 3 * (uintptr_t)p.h * p.w * sizeof(float);
  const uintptr_t a = reinterpret_cast<uintptr_t>(p.x), o = reinterpret_cast<uintptr_t>(p.out);
  if (a != o && colour_overlap(a, o, bytes)) return TC_EINVAL;              // an overlap other than out == x
  if (base && colour_overlap(reinterpret_cast<uintptr_t>(base), o, bytes)) return TC_EINVAL;
  return TC_OK;
}

// The launch geometry of the apply pass over a checked clip: `chunks` blocks per frame (a quad per thread and round where it
// fits, 64 at the most), float4 loads (`vec`) where hw % 4 == 0 and every clip is 16-byte aligned, and the knots as kernels take them
struct ColourClip { int64_t hw, frames; int chunks; bool vec; TcColourKnots knots; };

// TC_OK and the geometry, or TC_ESHAPE for a grid past INT32_MAX
template <typename P>
inline int colour_clip_geometry(const P& p, const float* base, ColourClip* g) {
  g->hw = (int64_t)p.h * p.w;
  g->frames = (int64_t)p.b * p.t;
  const int64_t chunks = ((g->hw + 3) / 4 + COLOUR_THREADS - 1) / COLOUR_THREADS;
  g->chunks = (int)(chunks > COLOUR_MAX_CHUNKS ? COLOUR_MAX_CHUNKS : chunks);
  if (g->frames * g->chunks > INT32_MAX) return TC_ESHAPE;
  g->vec = (g->hw & 3) == 0 && tc_aligned16(p.x) && tc_aligned16(p.out) && (!base || tc_aligned16(base));
  g->knots = {};
  g->knots.nk = p.nk;
  for (int i = 0; i < p.nk; ++i) g->knots.knot[i] = p.knot[i];
  return TC_OK;
}

// An old params struct P in its knots form K, the fields they share: the knots are {0, t - 1} ({0} when t = 1) of the clip's two
// reference images.  What only one family has (method, coefs, max_gain; base, table) is the caller's to copy.
template <typename K, typename P>
inline K colour_two_ends(const P& p) {
  K k = {};
  k.x = p.x; k.out = p.out;
  k.b = p.b; k.t = p.t; k.h = p.h; k.w = p.w;
  k.src = p.src; k.ref = p.ref;
  k.ref_pixels = p.ref_pixels; k.strength = p.strength;
  k.nk = p.t > 1 ? 2 : 1;
  k.knot[0] = 0; k.knot[1] = p.t - 1;
  return k;
}

}  // namespace
