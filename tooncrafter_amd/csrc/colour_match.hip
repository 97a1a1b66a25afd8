// Colour match of decoded frames to their keyframes (tc_colour_stats, tc_colour_match, tc_colour_match_knots; the rule:
// include/tooncrafter_hip.h).
// Three streaming passes over the three channel planes of a frame, t * h * w floats apart, and one thread of double
// arithmetic per frame between them:
//   colour_stats_kernel   nine double sums per (frame, part), parts fixed by h * w alone      -> workspace
//   colour_finish_kernel  the parts of a frame added in index order                           -> stats
//   colour_coefs_kernel   (m, C) of frame and target (its course through the knots: csrc/colour_course.h), the 3 x 3 map and
//                         its optional gain limit, twelve fp32 numbers                         -> coefs
//   colour_apply_kernel   y = o' + A' clamp(x), every operation rounded on its own            -> out
// No atomics, no allocation, no synchronisation.  What a request has in common with the histogram transfer's -- the clamp, the frame
// slots, the clip request and its knots -- is csrc/colour_request.h; here are the method, the gain limit, the 8-byte alignment of
// the float64 sums and the solve.
#include "colour_request.h"

namespace {

constexpr int CM_THREADS = COLOUR_THREADS;
constexpr int CM_MAX_PARTS = 64;
constexpr int64_t CM_PART_PIXELS = 2048;
constexpr double CM_EPS = 1.0 / 65536.0;          // 2^-16, value^2 units

__device__ __forceinline__ void stats_add(double* s, float rf, float gf, float bf) {
  const double r = clamp1(rf), g = clamp1(gf), b = clamp1(bf);
  s[0] += r; s[1] += g; s[2] += b;
  s[3] += r * r; s[4] += r * g; s[5] += r * b;
  s[6] += g * g; s[7] += g * b; s[8] += b * b;
}

// One block per (frame slot, part).  Thread j of part p takes the pixel quads q = p * 256 + j, q + 256 P, ...; VEC (every plane
// base 16-byte aligned, hw % 4 == 0) reads a quad as one float4 per plane, otherwise as four floats -- the same pixels in the
// same order, so the sums do not depend on the alignment.
template <bool VEC>
__global__ __launch_bounds__(CM_THREADS) void colour_stats_kernel(const float* __restrict__ x, int t, int64_t hw, int f0, int nf,
                                                                  int fstep, int parts, double* __restrict__ part) {
  __shared__ double red[CM_THREADS / 64][TC_COLOUR_STATS];
  const int slot = blockIdx.x / parts, p = blockIdx.x - slot * parts;
  const ColourSlot at = colour_slot(slot, f0, nf, fstep);
  const float* pr = x + ((int64_t)at.clip * 3 * t + at.f) * hw;
  const float* pg = pr + (int64_t)t * hw;
  const float* pb = pg + (int64_t)t * hw;
  double s[TC_COLOUR_STATS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t quads = (hw + 3) >> 2;
  for (int64_t q = (int64_t)p * CM_THREADS + threadIdx.x; q < quads; q += (int64_t)parts * CM_THREADS) {
    const int64_t i = q << 2;
    if (VEC) {
      const float4 r = *reinterpret_cast<const float4*>(pr + i);
      const float4 g = *reinterpret_cast<const float4*>(pg + i);
      const float4 b = *reinterpret_cast<const float4*>(pb + i);
      stats_add(s, r.x, g.x, b.x);
      stats_add(s, r.y, g.y, b.y);
      stats_add(s, r.z, g.z, b.z);
      stats_add(s, r.w, g.w, b.w);
    } else {
      const int64_t end = i + 4 < hw ? i + 4 : hw;
      for (int64_t k = i; k < end; ++k) stats_add(s, pr[k], pg[k], pb[k]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < TC_COLOUR_STATS; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < TC_COLOUR_STATS)
    part[(int64_t)blockIdx.x * TC_COLOUR_STATS + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// the parts of a slot, in index order: one thread per (slot, statistic)
__global__ __launch_bounds__(CM_THREADS) void colour_finish_kernel(const double* __restrict__ part, int parts, int64_t total,
                                                                   double* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t slot = i / TC_COLOUR_STATS;
  const int k = (int)(i - slot * TC_COLOUR_STATS);
  double v = 0.0;
  for (int p = 0; p < parts; ++p) v += part[(slot * parts + p) * TC_COLOUR_STATS + k];
  stats[i] = v;
}

// ---- the 3 x 3 solve.  Matrices are scalars-in-arrays with compile-time indices only (no scratch).

// symmetric 3 x 3 as a[6] = {00, 01, 02, 11, 12, 22}
__device__ __forceinline__ constexpr int sym_at(int i, int j) { return i <= j ? (i == 0 ? j : i + j + 1) : sym_at(j, i); }

// m = S1 / n, C = S2 / n - m m^T
__device__ __forceinline__ void moments(const double* __restrict__ s, double n, double* m, double* c) {
  m[0] = s[0] / n; m[1] = s[1] / n; m[2] = s[2] / n;
  c[0] = s[3] / n - m[0] * m[0]; c[1] = s[4] / n - m[0] * m[1]; c[2] = s[5] / n - m[0] * m[2];
  c[3] = s[6] / n - m[1] * m[1]; c[4] = s[7] / n - m[1] * m[2];
  c[5] = s[8] / n - m[2] * m[2];
}

// one Jacobi rotation that annihilates a[P][Q]; v gathers the rotations (columns = eigenvectors)
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double* a, double* v) {
  constexpr int R = 3 - P - Q;
  const double apq = a[sym_at(P, Q)];
  if (apq == 0.0) return;
  const double theta = (a[sym_at(Q, Q)] - a[sym_at(P, P)]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
  a[sym_at(P, P)] -= tt * apq;
  a[sym_at(Q, Q)] += tt * apq;
  a[sym_at(P, Q)] = 0.0;
  const double arp = a[sym_at(R, P)], arq = a[sym_at(R, Q)];
  a[sym_at(R, P)] = c * arp - s * arq;
  a[sym_at(R, Q)] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = v[3 * k + P], vq = v[3 * k + Q];
    v[3 * k + P] = c * vp - s * vq;
    v[3 * k + Q] = s * vp + c * vq;
  }
}

// eigenvalues (a's diagonal afterwards) and eigenvectors of a symmetric 3 x 3: cyclic Jacobi, eight sweeps
__device__ __forceinline__ void jacobi_eig(double* a, double* v) {
  v[0] = 1.0; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0; v[4] = 1.0; v[5] = 0.0; v[6] = 0.0; v[7] = 0.0; v[8] = 1.0;
#pragma unroll 1
  for (int sweep = 0; sweep < 8; ++sweep) {
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
}

// out (symmetric, full 3 x 3 row-major) = V diag(d) V^T
__device__ __forceinline__ void from_eig(const double* v, double d0, double d1, double d2, double* out) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = (v[3 * i] * d0 * v[3 * j] + v[3 * i + 1] * d1 * v[3 * j + 1]) + v[3 * i + 2] * d2 * v[3 * j + 2];
}

__device__ __forceinline__ void mat3_mul(const double* a, const double* b, double* out) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// A = S^(-1/2) (S^(1/2) T S^(1/2))^(1/2) S^(-1/2) with S = cs + eps I, T = ct + eps I (full row-major 3 x 3 out)
__device__ __forceinline__ void mkl_map(const double* cs, const double* ct, double* A) {
  double s[6] = {cs[0] + CM_EPS, cs[1], cs[2], cs[3] + CM_EPS, cs[4], cs[5] + CM_EPS};
  double v[9], half[9], ihalf[9], tfull[9], tmp[9], mid[9];
  jacobi_eig(s, v);
  const double e0 = sqrt(fmax(s[0], 0.5 * CM_EPS)), e1 = sqrt(fmax(s[3], 0.5 * CM_EPS)), e2 = sqrt(fmax(s[5], 0.5 * CM_EPS));
  from_eig(v, e0, e1, e2, half);
  from_eig(v, 1.0 / e0, 1.0 / e1, 1.0 / e2, ihalf);
  tfull[0] = ct[0] + CM_EPS; tfull[1] = ct[1]; tfull[2] = ct[2];
  tfull[3] = ct[1]; tfull[4] = ct[3] + CM_EPS; tfull[5] = ct[4];
  tfull[6] = ct[2]; tfull[7] = ct[4]; tfull[8] = ct[5] + CM_EPS;
  mat3_mul(half, tfull, tmp);
  mat3_mul(tmp, half, mid);
  double m[6] = {mid[0], 0.5 * (mid[1] + mid[3]), 0.5 * (mid[2] + mid[6]), mid[4], 0.5 * (mid[5] + mid[7]), mid[8]};
  jacobi_eig(m, v);
  from_eig(v, sqrt(fmax(m[0], 0.0)), sqrt(fmax(m[3], 0.0)), sqrt(fmax(m[5], 0.0)), mid);
  mat3_mul(ihalf, mid, tmp);
  mat3_mul(tmp, ihalf, A);
}

// A held inside the gain limit g (lo = 1 / g): the eigenvalues of its symmetric part clamped to [lo, g], by the same Jacobi
__device__ __forceinline__ void mkl_limit(double* A, double lo, double g) {
  double a[6] = {A[0], 0.5 * (A[1] + A[3]), 0.5 * (A[2] + A[6]), A[4], 0.5 * (A[5] + A[7]), A[8]};
  double v[9];
  jacobi_eig(a, v);
  from_eig(v, fmin(fmax(a[0], lo), g), fmin(fmax(a[3], lo), g), fmin(fmax(a[5], lo), g), A);
}

// The twelve numbers of frame f of a clip: `src` its nine sums over n_src pixels, `ref` those of the clip's reference images
// (n_ref pixels each) in knot order; the frame's course through the knots picks the one or the two that make its target.
__device__ __forceinline__ void frame_coefs(const double* __restrict__ src, const double* __restrict__ ref, const TcColourKnots& knots,
                                            int f, double n_src, double n_ref, int method, float strength, float max_gain,
                                            float* __restrict__ out) {
  double ms[3], cs[6], m0[3], c0[6], mt[3], ct[6], A[9];
  moments(src, n_src, ms, cs);
  const TcColourCourse at = tc_colour_course(knots, f);
  moments(ref + (int64_t)at.j * TC_COLOUR_STATS, n_ref, m0, c0);
  if (at.single) {
#pragma unroll
    for (int k = 0; k < 3; ++k) mt[k] = m0[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) ct[k] = c0[k];
  } else {
    double m1[3], c1[6];
    moments(ref + (int64_t)(at.j + 1) * TC_COLOUR_STATS, n_ref, m1, c1);
    const double w = at.w, u = 1.0 - w;
#pragma unroll
    for (int k = 0; k < 3; ++k) mt[k] = u * m0[k] + w * m1[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) ct[k] = u * c0[k] + w * c1[k];
  }
  if (method == TC_COLOUR_MKL) {
    mkl_map(cs, ct, A);
  } else {
    A[1] = A[2] = A[3] = A[5] = A[6] = A[7] = 0.0;
    A[0] = sqrt((ct[0] + CM_EPS) / (cs[0] + CM_EPS));
    A[4] = sqrt((ct[3] + CM_EPS) / (cs[3] + CM_EPS));
    A[8] = sqrt((ct[5] + CM_EPS) / (cs[5] + CM_EPS));
  }
  if (max_gain > 0.f) {
    const double g = (double)max_gain, lo = 1.0 / g;
    if (method == TC_COLOUR_MKL) {
      mkl_limit(A, lo, g);
    } else {
      A[0] = fmin(fmax(A[0], lo), g);
      A[4] = fmin(fmax(A[4], lo), g);
      A[8] = fmin(fmax(A[8], lo), g);
    }
  }
  const double s = (double)strength;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double o = mt[i] - ((A[3 * i] * ms[0] + A[3 * i + 1] * ms[1]) + A[3 * i + 2] * ms[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double id = i == j ? 1.0 : 0.0;
      out[3 * i + j] = (float)(id + s * (A[3 * i + j] - id));
    }
    out[9 + i] = (float)(s * o);
  }
}

// one thread per frame of the batch; a clip's reference images are rows clip * ref_rows .. of `ref` (ref_rows >= knots.nk)
__global__ __launch_bounds__(64) void colour_coefs_kernel(const double* __restrict__ src, const double* __restrict__ ref, int frames,
                                                          int t, double n_src, double n_ref, int method, float strength,
                                                          float max_gain, int ref_rows, TcColourKnots knots,
                                                          float* __restrict__ coefs) {
  const int fr = blockIdx.x * 64 + threadIdx.x;
  if (fr >= frames) return;
  const int clip = fr / t;
  frame_coefs(src + (int64_t)fr * TC_COLOUR_STATS, ref + (int64_t)clip * ref_rows * TC_COLOUR_STATS, knots, fr - clip * t, n_src,
              n_ref, method, strength, max_gain, coefs + (int64_t)fr * 12);
}

// y = ((o + a0 r) + a1 g) + a2 b on clamped inputs; each operation is an expression of its own and nothing is contracted (the
// library is built with -ffp-contract=on)
__device__ __forceinline__ float affine_one(float o, float a0, float a1, float a2, float r, float g, float b) {
#pragma clang fp contract(off)
  const float p0 = a0 * r;
  const float s0 = o + p0;
  const float p1 = a1 * g;
  const float s1 = s0 + p1;
  const float p2 = a2 * b;
  return s1 + p2;
}

struct Affine { float a[12]; };

__device__ __forceinline__ void affine_pixel(const Affine& c, float r, float g, float b, float& yr, float& yg, float& yb) {
  r = clamp1(r); g = clamp1(g); b = clamp1(b);
  yr = affine_one(c.a[9], c.a[0], c.a[1], c.a[2], r, g, b);
  yg = affine_one(c.a[10], c.a[3], c.a[4], c.a[5], r, g, b);
  yb = affine_one(c.a[11], c.a[6], c.a[7], c.a[8], r, g, b);
}

// `chunks` blocks per frame, grid-stride over the frame's pixels (VEC: quads).  out may be exactly x: every element is read and
// then written by the same thread, so neither pointer is __restrict__.
template <bool VEC>
__global__ __launch_bounds__(CM_THREADS) void colour_apply_kernel(const float* x, float* out, const float* __restrict__ coefs, int t,
                                                                  int64_t hw, int chunks) {
  const int fr = blockIdx.x / chunks, chunk = blockIdx.x - fr * chunks;
  const int clip = fr / t, f = fr - clip * t;
  Affine c;
#pragma unroll
  for (int k = 0; k < 12; ++k) c.a[k] = coefs[(int64_t)fr * 12 + k];
  const int64_t base = ((int64_t)clip * 3 * t + f) * hw, plane = (int64_t)t * hw;
  const float* pr = x + base;
  float* qr = out + base;
  const int64_t start = (int64_t)chunk * CM_THREADS + threadIdx.x, stride = (int64_t)chunks * CM_THREADS;
  if (VEC) {
    for (int64_t q = start; q < (hw >> 2); q += stride) {
      const float4 r = reinterpret_cast<const float4*>(pr)[q];
      const float4 g = reinterpret_cast<const float4*>(pr + plane)[q];
      const float4 b = reinterpret_cast<const float4*>(pr + 2 * plane)[q];
      float4 yr, yg, yb;
      affine_pixel(c, r.x, g.x, b.x, yr.x, yg.x, yb.x);
      affine_pixel(c, r.y, g.y, b.y, yr.y, yg.y, yb.y);
      affine_pixel(c, r.z, g.z, b.z, yr.z, yg.z, yb.z);
      affine_pixel(c, r.w, g.w, b.w, yr.w, yg.w, yb.w);
      reinterpret_cast<float4*>(qr)[q] = yr;
      reinterpret_cast<float4*>(qr + plane)[q] = yg;
      reinterpret_cast<float4*>(qr + 2 * plane)[q] = yb;
    }
  } else {
    for (int64_t i = start; i < hw; i += stride) {
      float yr, yg, yb;
      affine_pixel(c, pr[i], pr[plane + i], pr[2 * plane + i], yr, yg, yb);
      qr[i] = yr;
      qr[plane + i] = yg;
      qr[2 * plane + i] = yb;
    }
  }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// TC_OK and the launch geometry of a statistics request, or its refusal (the workspace is the caller's to check)
int stats_request(const TcColourStatsParams* pp, int* parts, int64_t* slots, int64_t* workspace_bytes) {
  if (!pp) return TC_EINVAL;
  const TcColourStatsParams& p = *pp;
  if (const int rc = colour_slots_check(p, p.stats)) return rc;
  if (!aligned8(p.stats)) return TC_EALIGN;
  *parts = colour_parts((int64_t)p.h * p.w, CM_PART_PIXELS, CM_MAX_PARTS);   // the summation order is part of the result
  *slots = (int64_t)p.b * p.nf;
  if (*slots * *parts > INT32_MAX) return TC_ESHAPE;
  *workspace_bytes = *slots * *parts * TC_COLOUR_STATS * (int64_t)sizeof(double);
  return TC_OK;
}

}  // namespace

extern "C" int64_t tc_colour_stats_workspace(const TcColourStatsParams* p) {
  int parts = 0;
  int64_t slots = 0, bytes = 0;
  return stats_request(p, &parts, &slots, &bytes) == TC_OK ? bytes : 0;
}

extern "C" int tc_colour_stats(const TcColourStatsParams* pp, void* stream) {
  int parts = 0;
  int64_t slots = 0, bytes = 0;
  if (const int rc = stats_request(pp, &parts, &slots, &bytes)) return rc;
  const TcColourStatsParams& p = *pp;
  if (!p.workspace) return TC_EWORKSPACE;
  if (!aligned8(p.workspace)) return TC_EALIGN;
  if (p.workspace_bytes < bytes) return TC_EWORKSPACE;
  const int64_t hw = (int64_t)p.h * p.w;
  const bool vec = (hw & 3) == 0 && tc_aligned16(p.x);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(p.workspace);
  const int fstep = colour_fstep(p.nf, p.fstep);
  const dim3 grid((unsigned)(slots * parts));
  if (vec) hipLaunchKernelGGL(colour_stats_kernel<true>, grid, dim3(CM_THREADS), 0, s, p.x, p.t, hw, p.f0, p.nf, fstep, parts, part);
  else hipLaunchKernelGGL(colour_stats_kernel<false>, grid, dim3(CM_THREADS), 0, s, p.x, p.t, hw, p.f0, p.nf, fstep, parts, part);
  TC_LAUNCH_CHECK();
  const int64_t total = slots * TC_COLOUR_STATS;
  hipLaunchKernelGGL(colour_finish_kernel, dim3((unsigned)((total + CM_THREADS - 1) / CM_THREADS)), dim3(CM_THREADS), 0, s, part, parts,
                     total, p.stats);
  TC_LAUNCH_CHECK();
  return TC_OK;
}

namespace {

// The match of p: its checks and its two launches.  ref_rows: reference images per clip in p.ref (p.nk for the knots call; 2
// for tc_colour_match, also when t = 1 and only the first is a knot).
int colour_match_launch(const TcColourMatchKnotsParams& p, int ref_rows, void* stream) {
  if (const int rc = colour_clip_check(p, p.coefs, nullptr)) return rc;
  if (p.method != TC_COLOUR_MEAN_STD && p.method != TC_COLOUR_MKL) return TC_EINVAL;
  if (!std::isfinite(p.max_gain) || p.max_gain < 0.f || (p.max_gain > 0.f && p.max_gain < 1.f)) return TC_EINVAL;
  if (!aligned8(p.src) || !aligned8(p.ref)) return TC_EALIGN;
  ColourClip g;
  if (const int rc = colour_clip_geometry(p, nullptr, &g)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(colour_coefs_kernel, dim3((unsigned)((g.frames + 63) / 64)), dim3(64), 0, s, p.src, p.ref, (int)g.frames, p.t,
                     (double)g.hw, (double)p.ref_pixels, p.method, p.strength, p.max_gain, ref_rows, g.knots, p.coefs);
  TC_LAUNCH_CHECK();
  const dim3 grid((unsigned)(g.frames * g.chunks));
  if (g.vec) hipLaunchKernelGGL(colour_apply_kernel<true>, grid, dim3(CM_THREADS), 0, s, p.x, p.out, p.coefs, p.t, g.hw, g.chunks);
  else hipLaunchKernelGGL(colour_apply_kernel<false>, grid, dim3(CM_THREADS), 0, s, p.x, p.out, p.coefs, p.t, g.hw, g.chunks);
  TC_LAUNCH_CHECK();
  return TC_OK;
}

}  // namespace

// the two ends of the clip's two reference images, no gain limit
extern "C" int tc_colour_match(const TcColourMatchParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  TcColourMatchKnotsParams k = colour_two_ends<TcColourMatchKnotsParams>(*pp);
  k.method = pp->method;
  k.coefs = pp->coefs;
  k.max_gain = 0.f;
  return colour_match_launch(k, 2, stream);
}

extern "C" int tc_colour_match_knots(const TcColourMatchKnotsParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  return colour_match_launch(*pp, pp->nk, stream);
}
