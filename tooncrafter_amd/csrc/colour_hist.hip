// Histogram colour transfer of decoded frames to their keyframes (tc_colour_hist, tc_colour_transfer, tc_colour_transfer_knots;
// the rule: include/tooncrafter_hip.h).  Counts are integers, so nothing here depends on an order of summation:
//   colour_hist_kernel         one block per (frame slot, channel, part): a 1024-bin LDS histogram per wave (integer LDS
//                              atomics), the four added through LDS                                        -> workspace
//   colour_hist_finish_kernel  the parts of a (slot, channel) added                                       -> hist
//   colour_table_kernel        one block per (frame, channel), one thread per bin: three scans, two binary searches on
//                              int64 products, the displacement in double, rounded to fp32 once           -> table
//   colour_lut_kernel          y = beta + s ((c + D[bin(c)]) - beta), every operation rounded on its own  -> out
// No global atomics, no memset, no allocation, no synchronisation.
//
// Toon content puts most lanes of a wave into one bin, and LDS atomics on one address serialise.  So a lane merges equal
// neighbouring bins of its pixel quad into one add, and a wave whose lanes all hold one and the same bin adds its total once.
//
// What a request has in common with the linear match's -- the clamp, the frame slots, the clip request and its knots -- is
// csrc/colour_request.h; here are `base`, the 4-byte alignment of the int32 counts, the 2^26 limit and the tables.
#include "colour_request.h"

namespace {

constexpr int CH_THREADS = COLOUR_THREADS;
constexpr int CH_WAVES = CH_THREADS / 64;
constexpr int CH_MAX_PARTS = 16;
constexpr int64_t CH_PART_PIXELS = 1024;
constexpr int64_t CH_MAX_PIXELS = (int64_t)1 << 26;   // P_i m and A_j 2 n stay below 2^53: exact in int64 and in double

// bin of a CLAMPED value: the add is rounded, the multiply by 512 is exact; c + 1 >= 0
__device__ __forceinline__ int bin_of(float c) {
#pragma clang fp contract(off)
  const float u = c + 1.0f;
  const int b = (int)floorf(u * 512.0f);
  return b < TC_COLOUR_BINS - 1 ? b : TC_COLOUR_BINS - 1;
}

// One block per (slot, channel, part), blockIdx.x = (slot * 3 + k) * parts + p.  Thread j of part p takes the pixel quads
// q = p * 256 + j, q + 256 P, ...; VEC (plane bases 16-byte aligned, hw % 4 == 0) reads a quad as one float4.
template <bool VEC>
__global__ __launch_bounds__(CH_THREADS) void colour_hist_kernel(const float* __restrict__ x, int t, int64_t hw, int f0, int nf,
                                                                 int fstep, int parts, int32_t* __restrict__ part) {
  __shared__ int32_t h[CH_WAVES][TC_COLOUR_BINS];
  const int sk = blockIdx.x / parts, p = blockIdx.x - sk * parts;
  const int slot = sk / 3, k = sk - slot * 3;
  const ColourSlot at = colour_slot(slot, f0, nf, fstep);
  const float* px = x + (((int64_t)at.clip * 3 + k) * t + at.f) * hw;
  for (int i = threadIdx.x; i < CH_WAVES * TC_COLOUR_BINS; i += CH_THREADS) (&h[0][0])[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int32_t* mine = h[threadIdx.x >> 6];
  const int64_t quads = (hw + 3) >> 2;
  for (int64_t q = (int64_t)p * CH_THREADS + threadIdx.x; q < quads; q += (int64_t)parts * CH_THREADS) {
    const int64_t i = q << 2;
    int b0, b1, b2, b3;                                                   // -1: past the end of the plane
    if (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(px + i);
      b0 = bin_of(clamp1(v.x)); b1 = bin_of(clamp1(v.y)); b2 = bin_of(clamp1(v.z)); b3 = bin_of(clamp1(v.w));
    } else {
      b0 = bin_of(clamp1(px[i]));
      b1 = i + 1 < hw ? bin_of(clamp1(px[i + 1])) : -1;
      b2 = i + 2 < hw ? bin_of(clamp1(px[i + 2])) : -1;
      b3 = i + 3 < hw ? bin_of(clamp1(px[i + 3])) : -1;
    }
    const bool one = b1 == b0 && b2 == b0 && b3 == b0;
    const int first = __builtin_amdgcn_readfirstlane(b0);
    const unsigned long long active = __ballot(1);
    if (__ballot(one && b0 == first) == active) {                         // the whole wave in one bin: one add
      if (lane == __ffsll(active) - 1) atomicAdd(&mine[first], 4 * __popcll(active));
    } else {                                                              // runs of equal neighbours: one add each
      int cur = b0, cnt = 1;
      if (b1 == cur) ++cnt; else { atomicAdd(&mine[cur], cnt); cur = b1; cnt = 1; }
      if (b2 == cur) ++cnt; else { if (cur >= 0) atomicAdd(&mine[cur], cnt); cur = b2; cnt = 1; }
      if (b3 == cur) ++cnt; else { if (cur >= 0) atomicAdd(&mine[cur], cnt); cur = b3; cnt = 1; }
      if (cur >= 0) atomicAdd(&mine[cur], cnt);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TC_COLOUR_BINS; i += CH_THREADS)
    part[(int64_t)blockIdx.x * TC_COLOUR_BINS + i] = (h[0][i] + h[1][i]) + (h[2][i] + h[3][i]);
}

// the parts of a (slot, channel): one thread per count
__global__ __launch_bounds__(CH_THREADS) void colour_hist_finish_kernel(const int32_t* __restrict__ part, int parts, int64_t total,
                                                                        int32_t* __restrict__ hist) {
  const int64_t i = (int64_t)blockIdx.x * CH_THREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t sk = i / TC_COLOUR_BINS;
  const int bin = (int)(i - sk * TC_COLOUR_BINS);
  int32_t v = 0;
  for (int p = 0; p < parts; ++p) v += part[(sk * parts + p) * TC_COLOUR_BINS + bin];
  hist[i] = v;
}

// The reference quantile of midpoint rank P / 2n in bin units: cum[j] = A_j = sum_{i < j} r_i (cum[0] = 0), pm = P m, n2 = 2 n.
// j is the smallest index in [1, 1024] with A_j n2 >= pm; the search stays inside [1, 1024] whatever the counts are.
__device__ __forceinline__ double ref_quantile(const int32_t* cum, int64_t pm, int64_t n2) {
#pragma clang fp contract(off)
  int lo = 1, hi = TC_COLOUR_BINS;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)cum[mid] * n2 >= pm) hi = mid; else lo = mid + 1;
  }
  const int64_t below = (int64_t)cum[lo - 1] * n2, r = (int64_t)cum[lo] - (int64_t)cum[lo - 1];
  const double frac = (double)(pm - below) / (double)(r * n2);
  return (double)(lo - 1) + frac;
}

// One block per (frame, channel), thread i = bin i.  Inclusive scans of s, a, b: an up-shuffle scan per wave, then the totals of
// the waves before it.  The frame's course through the knots (csrc/colour_course.h) picks the one or the two of the clip's
// reference histograms (rows clip * ref_rows .. of `ref`, ref_rows >= knots.nk) that make its target.
__global__ __launch_bounds__(TC_COLOUR_BINS) void colour_table_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ ref,
                                                                      int t, int64_t n, int64_t m, int ref_rows, TcColourKnots knots,
                                                                      float* __restrict__ table) {
#pragma clang fp contract(off)
  __shared__ int32_t total[TC_COLOUR_BINS / 64][3];
  __shared__ int32_t cum[2][TC_COLOUR_BINS + 1];
  const int fk = blockIdx.x, fr = fk / 3, k = fk - fr * 3;
  const int clip = fr / t, f = fr - clip * t;
  const TcColourCourse at = tc_colour_course(knots, f);                   // the same for the whole block
  const int ja = at.j, jb = at.single ? at.j : at.j + 1;
  const int i = threadIdx.x, lane = i & 63, wave = i >> 6;
  const int32_t s = src[(int64_t)fk * TC_COLOUR_BINS + i];
  int32_t v0 = s;
  int32_t v1 = ref[(((int64_t)clip * ref_rows + ja) * 3 + k) * TC_COLOUR_BINS + i];
  int32_t v2 = ref[(((int64_t)clip * ref_rows + jb) * 3 + k) * TC_COLOUR_BINS + i];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t u0 = __shfl_up(v0, off, 64), u1 = __shfl_up(v1, off, 64), u2 = __shfl_up(v2, off, 64);
    if (lane >= off) { v0 += u0; v1 += u1; v2 += u2; }
  }
  if (lane == 63) { total[wave][0] = v0; total[wave][1] = v1; total[wave][2] = v2; }
  __syncthreads();
  for (int w = 0; w < wave; ++w) { v0 += total[w][0]; v1 += total[w][1]; v2 += total[w][2]; }
  cum[0][i + 1] = v1;
  cum[1][i + 1] = v2;
  if (i == 0) cum[0][0] = cum[1][0] = 0;
  __syncthreads();
  float d = 0.0f;
  if (s > 0) {
    const int64_t pm = (2 * (int64_t)v0 - (int64_t)s) * m, n2 = 2 * n;
    double T = ref_quantile(cum[0], pm, n2);                              // a frame that takes one knot: that knot's q itself
    if (!at.single) {
      const double qa = T, qb = ref_quantile(cum[1], pm, n2);
      const double step = at.w * (qb - qa);
      T = qa + step;
    }
    const double centre = (double)i + 0.5;
    d = (float)((T - centre) / 512.0);
  }
  table[(int64_t)fk * TC_COLOUR_BINS + i] = d;
}

template <bool BASE>
__device__ __forceinline__ float lut_one(float x, float base, const float* D, float s) {
#pragma clang fp contract(off)
  const float c = clamp1(x);
  const float v = c + D[bin_of(c)];
  const float beta = BASE ? clamp1(base) : c;
  const float diff = v - beta;
  const float scaled = s * diff;
  return beta + scaled;
}

// `chunks` blocks per frame, grid-stride over the frame's pixels (VEC: quads), the frame's three tables in LDS.  out may be
// exactly x: every element is read and then written by the same thread, so neither pointer is __restrict__.
template <bool VEC, bool BASE>
__global__ __launch_bounds__(CH_THREADS) void colour_lut_kernel(const float* x, const float* base, float* out,
                                                                const float* __restrict__ table, float s, int t, int64_t hw, int chunks) {
  __shared__ float D[3][TC_COLOUR_BINS];
  const int fr = blockIdx.x / chunks, chunk = blockIdx.x - fr * chunks;
  const int clip = fr / t, f = fr - clip * t;
  for (int i = threadIdx.x; i < 3 * TC_COLOUR_BINS; i += CH_THREADS) (&D[0][0])[i] = table[(int64_t)fr * 3 * TC_COLOUR_BINS + i];
  __syncthreads();
  const int64_t first = ((int64_t)clip * 3 * t + f) * hw, plane = (int64_t)t * hw;
  const int64_t start = (int64_t)chunk * CH_THREADS + threadIdx.x, stride = (int64_t)chunks * CH_THREADS;
  if (VEC) {
    for (int64_t q = start; q < (hw >> 2); q += stride) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int64_t at = first + k * plane;
        const float4 v = reinterpret_cast<const float4*>(x + at)[q];
        float4 bv = v;
        if (BASE) bv = reinterpret_cast<const float4*>(base + at)[q];
        float4 y;
        y.x = lut_one<BASE>(v.x, bv.x, D[k], s);
        y.y = lut_one<BASE>(v.y, bv.y, D[k], s);
        y.z = lut_one<BASE>(v.z, bv.z, D[k], s);
        y.w = lut_one<BASE>(v.w, bv.w, D[k], s);
        reinterpret_cast<float4*>(out + at)[q] = y;
      }
    }
  } else {
    for (int64_t i = start; i < hw; i += stride) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int64_t at = first + k * plane + i;
        const float v = x[at];
        out[at] = lut_one<BASE>(v, BASE ? base[at] : v, D[k], s);
      }
    }
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// TC_OK and the launch geometry of a histogram request, or its refusal (the workspace is the caller's to check)
int hist_request(const TcColourHistParams* pp, int* parts, int64_t* slots, int64_t* workspace_bytes) {
  if (!pp) return TC_EINVAL;
  const TcColourHistParams& p = *pp;
  if (const int rc = colour_slots_check(p, p.hist)) return rc;
  if (!aligned4(p.hist)) return TC_EALIGN;
  const int64_t hw = (int64_t)p.h * p.w;
  if (hw > CH_MAX_PIXELS) return TC_ESHAPE;
  *parts = colour_parts(hw, CH_PART_PIXELS, CH_MAX_PARTS);                   // counts do not depend on it; the workspace does
  *slots = (int64_t)p.b * p.nf;
  if (*slots * 3 * *parts > INT32_MAX) return TC_ESHAPE;
  *workspace_bytes = *slots * 3 * *parts * TC_COLOUR_BINS * (int64_t)sizeof(int32_t);
  return TC_OK;
}

template <bool VEC>
void launch_lut(const TcColourTransferKnotsParams& p, const ColourClip& g, hipStream_t s) {
  const dim3 grid((unsigned)(g.frames * g.chunks));
  if (p.base) hipLaunchKernelGGL((colour_lut_kernel<VEC, true>), grid, dim3(CH_THREADS), 0, s, p.x, p.base, p.out, p.table, p.strength, p.t, g.hw, g.chunks);
  else hipLaunchKernelGGL((colour_lut_kernel<VEC, false>), grid, dim3(CH_THREADS), 0, s, p.x, p.base, p.out, p.table, p.strength, p.t, g.hw, g.chunks);
}

}  // namespace

extern "C" int64_t tc_colour_hist_workspace(const TcColourHistParams* p) {
  int parts = 0;
  int64_t slots = 0, bytes = 0;
  return hist_request(p, &parts, &slots, &bytes) == TC_OK ? bytes : 0;
}

extern "C" int tc_colour_hist(const TcColourHistParams* pp, void* stream) {
  int parts = 0;
  int64_t slots = 0, bytes = 0;
  if (const int rc = hist_request(pp, &parts, &slots, &bytes)) return rc;
  const TcColourHistParams& p = *pp;
  if (!p.workspace) return TC_EWORKSPACE;
  if (!aligned4(p.workspace)) return TC_EALIGN;
  if (p.workspace_bytes < bytes) return TC_EWORKSPACE;
  const int64_t hw = (int64_t)p.h * p.w;
  const bool vec = (hw & 3) == 0 && tc_aligned16(p.x);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int32_t* part = reinterpret_cast<int32_t*>(p.workspace);
  const int fstep = colour_fstep(p.nf, p.fstep);
  const dim3 grid((unsigned)(slots * 3 * parts));
  if (vec) hipLaunchKernelGGL(colour_hist_kernel<true>, grid, dim3(CH_THREADS), 0, s, p.x, p.t, hw, p.f0, p.nf, fstep, parts, part);
  else hipLaunchKernelGGL(colour_hist_kernel<false>, grid, dim3(CH_THREADS), 0, s, p.x, p.t, hw, p.f0, p.nf, fstep, parts, part);
  TC_LAUNCH_CHECK();
  const int64_t total = slots * 3 * TC_COLOUR_BINS;
  hipLaunchKernelGGL(colour_hist_finish_kernel, dim3((unsigned)((total + CH_THREADS - 1) / CH_THREADS)), dim3(CH_THREADS), 0, s, part,
                     parts, total, p.hist);
  TC_LAUNCH_CHECK();
  return TC_OK;
}

namespace {

// The transfer of p: its checks and its two launches.  ref_rows: reference images per clip in p.ref (p.nk for the knots call; 2
// for tc_colour_transfer, also when t = 1 and only the first is a knot).
int colour_transfer_launch(const TcColourTransferKnotsParams& p, int ref_rows, void* stream) {
  if (const int rc = colour_clip_check(p, p.table, p.base)) return rc;
  if (!aligned4(p.src) || !aligned4(p.ref) || !aligned4(p.table)) return TC_EALIGN;
  ColourClip g;
  if (const int rc = colour_clip_geometry(p, p.base, &g)) return rc;
  if (g.hw > CH_MAX_PIXELS || p.ref_pixels > CH_MAX_PIXELS || g.frames * 3 > INT32_MAX) return TC_ESHAPE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(colour_table_kernel, dim3((unsigned)(g.frames * 3)), dim3(TC_COLOUR_BINS), 0, s, p.src, p.ref, p.t, g.hw, p.ref_pixels,
                     ref_rows, g.knots, p.table);
  TC_LAUNCH_CHECK();
  if (g.vec) launch_lut<true>(p, g, s);
  else launch_lut<false>(p, g, s);
  TC_LAUNCH_CHECK();
  return TC_OK;
}

}  // namespace

// the two ends of the clip's two reference images
extern "C" int tc_colour_transfer(const TcColourTransferParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  TcColourTransferKnotsParams k = colour_two_ends<TcColourTransferKnotsParams>(*pp);
  k.base = pp->base;
  k.table = pp->table;
  return colour_transfer_launch(k, 2, stream);
}

extern "C" int tc_colour_transfer_knots(const TcColourTransferKnotsParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  return colour_transfer_launch(*pp, pp->nk, stream);
}
