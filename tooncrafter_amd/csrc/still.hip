// Still regions: where the two keyframes of a clip agree, and the decoded clip held to the keyframes there (tc_still_map,
// tc_still_composite; the rule: include/tooncrafter_hip.h, restated in numpy by tests/still_ref.py).
//   still_scan_kernel       one block per 16 cells of a cell row: 8 x 8 pixels x 3 channels x 2 keyframes each as float4
//                           loads, a cell's "moved" flag OR-ed in LDS                                   -> dist (as 0 / 1)
//   still_dist_kernel       one block per clip: the flags into LDS, the capped Chebyshev distance as a separable min filter
//                           (along rows, then along columns), in place                                  -> dist, mask
//   still_alpha_kernel      one thread per four pixels: the 2 x 2 cells around them, integer bilinear taps in sixteenths per
//                           axis, one correctly rounded division                                        -> alpha
//   still_composite_kernel  one thread per four pixels of a channel and up to four frames: alpha and the keyframes read once,
//                           out = v | key | v + alpha (key - v), every operation rounded on its own     -> out
// The flags live in `dist` between the first two launches, so there is no workspace.  No global atomics, no memset, no
// allocation, no synchronisation: the launches are ordered by the stream and can be captured in a hipGraph.
#include "common.h"

namespace {

constexpr int ST_CELL = TC_STILL_CELL;
constexpr int ST_SCAN_CELLS = 16;                          // cells of a cell row per block of the scan
constexpr int ST_SCAN_THREADS = ST_SCAN_CELLS * ST_CELL;   // one thread per pixel row of a cell
constexpr int ST_DIST_THREADS = 256;
constexpr int ST_MAX_CELLS = 16384;                        // a clip's cell map twice in LDS: 32 KB
constexpr int ST_FRAMES = 4;                               // frames per thread of the composite

static_assert(ST_CELL == 8, "a pixel row of a cell is two float4");

// a NaN stays a NaN (fminf / fmaxf would turn it into a bound), so that it differs from everything
__device__ __forceinline__ float st_clamp(float v) { return v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v; }

__device__ __forceinline__ bool st_moved(float a, float b, float thr) {
  const float d = st_clamp(a) - st_clamp(b);
  return !(fabsf(d) <= thr);
}

__device__ __forceinline__ bool st_moved4(const float4& a, const float4& b, float thr) {
  return st_moved(a.x, b.x, thr) | st_moved(a.y, b.y, thr) | st_moved(a.z, b.z, thr) | st_moved(a.w, b.w, thr);
}

// grid (ceil(w / 16), h, b), h x w cells.  Thread (r = tid / 16, c = tid % 16): pixel row r of cell c of the block, 8 floats of
// each of the 6 planes.  flag[c] = any of its pixels moved.
__global__ __launch_bounds__(ST_SCAN_THREADS) void still_scan_kernel(const float* __restrict__ ends, uint8_t* __restrict__ dist,
                                                                     int h, int w, float thr) {
  __shared__ int flag[ST_SCAN_CELLS];
  const int c = threadIdx.x & (ST_SCAN_CELLS - 1), r = threadIdx.x / ST_SCAN_CELLS;
  const int cx = blockIdx.x * ST_SCAN_CELLS + c, cy = blockIdx.y, clip = blockIdx.z;
  if (threadIdx.x < ST_SCAN_CELLS) flag[threadIdx.x] = 0;
  __syncthreads();
  if (cx < w) {
    const int64_t plane = (int64_t)h * w * (ST_CELL * ST_CELL);                  // H * W
    const int64_t at = ((int64_t)cy * ST_CELL + r) * ((int64_t)w * ST_CELL) + (int64_t)cx * ST_CELL;
    const float* p = ends + (int64_t)clip * 6 * plane + at;
    bool moved = false;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float4* a = reinterpret_cast<const float4*>(p + (2 * ch) * plane);
      const float4* b = reinterpret_cast<const float4*>(p + (2 * ch + 1) * plane);
      const float4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
      moved = moved | st_moved4(a0, b0, thr) | st_moved4(a1, b1, thr);
    }
    if (moved) atomicOr(&flag[c], 1);                                            // LDS
  }
  __syncthreads();
  if (threadIdx.x < ST_SCAN_CELLS && cx < w) dist[((int64_t)clip * h + cy) * w + cx] = (uint8_t)flag[threadIdx.x];
}

// one block per clip, h * w <= ST_MAX_CELLS.  row[i][j] = min(D, the distance along row i from j to a moved cell);
// d[i][j] = min over |di| < D of max(|di|, row[i + di][j]), capped at D: the Chebyshev distance to the nearest moved cell.
__global__ __launch_bounds__(ST_DIST_THREADS) void still_dist_kernel(uint8_t* dist, float* __restrict__ mask, int h, int w,
                                                                     int grow, int cap) {
  __shared__ uint8_t moved[ST_MAX_CELLS];
  __shared__ uint8_t row[ST_MAX_CELLS];
  const int cells = h * w;
  uint8_t* d = dist + (int64_t)blockIdx.x * cells;
  float* m = mask + (int64_t)blockIdx.x * cells;
  for (int i = threadIdx.x; i < cells; i += ST_DIST_THREADS) moved[i] = d[i];
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += ST_DIST_THREADS) {
    const int y = i / w, x = i - y * w;
    int best = cap;
    if (moved[i]) {
      best = 0;
    } else {
      for (int k = 1; k < cap; ++k) {
        const bool hit = (x - k >= 0 && moved[i - k]) || (x + k < w && moved[i + k]);
        if (hit) { best = k; break; }
      }
    }
    row[i] = (uint8_t)best;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += ST_DIST_THREADS) {
    const int y = i / w, x = i - y * w;
    int best = row[i];
    for (int k = 1; k < best; ++k) {                                             // a row k away cannot give less than k
      int v = cap;
      if (y - k >= 0) v = min(v, (int)row[i - k * w]);
      if (y + k < h) v = min(v, (int)row[i + k * w]);
      best = min(best, max(k, v));
    }
    d[i] = (uint8_t)best;
    m[i] = best > grow ? 1.0f : 0.0f;
  }
}

// The two cells and the two weights in sixteenths of pixel p = 8 i + r along one axis of n cells, centres at 8 i + 3.5, edges
// replicated: r < 4 lies between the centres of cells i - 1 and i, r >= 4 between those of i and i + 1.
__device__ __forceinline__ void st_taps(int p, int n, int& i0, int& i1, int& w0, int& w1) {
  const int i = p >> 3, r = p & 7;
  if (r < 4) { i0 = max(i - 1, 0); i1 = i; w1 = 2 * r + 9; }
  else { i0 = i; i1 = min(i + 1, n - 1); w1 = 2 * r - 7; }
  w0 = 16 - w1;
}

__device__ __forceinline__ int st_weight(int d, int grow, int feather) { return min(max(d - grow - 1, 0), feather); }

// thread = four pixels of a row (inside one half of a cell: one pair of cell columns); total = b * H * W / 4
__global__ __launch_bounds__(256) void still_alpha_kernel(const uint8_t* __restrict__ dist, float* __restrict__ alpha, int h, int w,
                                                          int grow, int feather, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int wq = w * 2;                                                          // groups of four per pixel row
  const int64_t line = i / wq;                                                   // clip * H + y
  const int x = (int)(i - line * wq) * 4;
  const int64_t clip = line / (h * ST_CELL);
  const int y = (int)(line - clip * (h * ST_CELL));
  int y0, y1, wy0, wy1, x0, x1, wx0, wx1;
  st_taps(y, h, y0, y1, wy0, wy1);
  st_taps(x, w, x0, x1, wx0, wx1);
  const uint8_t* d = dist + clip * ((int64_t)h * w);
  const int a00 = st_weight(d[y0 * w + x0], grow, feather), a01 = st_weight(d[y0 * w + x1], grow, feather);
  const int a10 = st_weight(d[y1 * w + x0], grow, feather), a11 = st_weight(d[y1 * w + x1], grow, feather);
  const int left = wy0 * a00 + wy1 * a10, right = wy0 * a01 + wy1 * a11;         // sixteenths along y
  const float den = (float)(256 * feather);
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = (wx0 - 2 * k) * left + (wx1 + 2 * k) * right;                  // the x weights move by 2 / 16 per pixel
    r[k] = __fdiv_rn((float)n, den);
  }
  reinterpret_cast<float4*>(alpha)[i] = float4{r[0], r[1], r[2], r[3]};
}

struct StCompositeArgs {
  const float* video;
  const float* ends;
  const float* alpha;
  float* out;
  int32_t t, f0, nf;
  int64_t plane4;                                                                // H * W / 4
  float s[TC_TEMPORAL_MAX_FRAMES];                                               // s[j] = float(j) / float(t - 1), host values
};

__device__ __forceinline__ float st_blend(float v, float e0, float e1, float s, float a) {
#pragma clang fp contract(off)
  if (a == 0.0f) return v;
  const float span = e1 - e0;
  const float step = s * span;
  const float key = e0 + step;
  if (a == 1.0f) return key;
  const float diff = key - v;
  const float move = a * diff;
  return v + move;
}

// grid (ceil(H W / 4 / 256), 3 * ceil(nf / 4), b).  INPLACE: out == video, so a group whose four alphas are zero is left alone.
template <bool INPLACE>
__global__ __launch_bounds__(256) void still_composite_kernel(const StCompositeArgs g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.plane4) return;
  const int ch = blockIdx.y % 3, part = blockIdx.y / 3, clip = blockIdx.z;
  const float4 a = reinterpret_cast<const float4*>(g.alpha)[(int64_t)clip * g.plane4 + i];
  const bool none = a.x == 0.0f && a.y == 0.0f && a.z == 0.0f && a.w == 0.0f;
  if (INPLACE && none) return;
  float4 e0 = float4{0.f, 0.f, 0.f, 0.f}, e1 = e0;
  if (!none) {                                                                   // the keyframes are not read where alpha is 0
    const float4* e = reinterpret_cast<const float4*>(g.ends) + ((int64_t)clip * 3 + ch) * 2 * g.plane4 + i;
    e0 = e[0];
    e1 = e[g.plane4];
  }
  const int64_t base = ((int64_t)clip * 3 + ch) * g.t * g.plane4 + i;
  const float4* vin = reinterpret_cast<const float4*>(g.video);                  // may be out itself: no __restrict__
  float4* vout = reinterpret_cast<float4*>(g.out);
  const int j0 = g.f0 + part * ST_FRAMES, j1 = min(g.f0 + g.nf, j0 + ST_FRAMES);
  for (int j = j0; j < j1; ++j) {
    const float s = g.s[j];
    const float4 v = vin[base + (int64_t)j * g.plane4];
    float4 r;
    r.x = st_blend(v.x, e0.x, e1.x, s, a.x);
    r.y = st_blend(v.y, e0.y, e1.y, s, a.y);
    r.z = st_blend(v.z, e0.z, e1.z, s, a.z);
    r.w = st_blend(v.w, e0.w, e1.w, s, a.w);
    vout[base + (int64_t)j * g.plane4] = r;
  }
}

inline bool st_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

}  // namespace

extern "C" int tc_still_map(const TcStillMapParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  const TcStillMapParams& p = *pp;
  if (!p.ends || !p.mask || !p.alpha || !p.dist) return TC_EINVAL;
  if (p.b <= 0 || p.h <= 0 || p.w <= 0) return TC_EINVAL;
  if (p.tau < 0 || p.tau > 255 || p.grow < 0 || p.feather < 1) return TC_EINVAL;
  if ((int64_t)p.grow + p.feather + 1 > TC_STILL_MAX_DIST) return TC_EINVAL;
  if (p.h % ST_CELL || p.w % ST_CELL) return TC_ESHAPE;
  const int h = p.h / ST_CELL, w = p.w / ST_CELL;
  if ((int64_t)h * w > ST_MAX_CELLS || p.b > 65535 || h > 65535) return TC_ESHAPE;
  if (!tc_aligned16(p.ends) || !tc_aligned16(p.alpha) || (reinterpret_cast<uintptr_t>(p.mask) & 3u)) return TC_EALIGN;
  const int cap = p.grow + p.feather + 1;
  const float thr = (float)p.tau / 127.5f;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(still_scan_kernel, dim3((unsigned)((w + ST_SCAN_CELLS - 1) / ST_SCAN_CELLS), (unsigned)h, (unsigned)p.b),
                     dim3(ST_SCAN_THREADS), 0, s, p.ends, p.dist, h, w, thr);
  TC_LAUNCH_CHECK();
  hipLaunchKernelGGL(still_dist_kernel, dim3((unsigned)p.b), dim3(ST_DIST_THREADS), 0, s, p.dist, p.mask, h, w, p.grow, cap);
  TC_LAUNCH_CHECK();
  const int64_t total = (int64_t)p.b * p.h * p.w / 4;                            // at most 65535 * 16384 * 16
  hipLaunchKernelGGL(still_alpha_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p.dist, p.alpha, h, w, p.grow,
                     p.feather, total);
  TC_LAUNCH_CHECK();
  return TC_OK;
}

extern "C" int tc_still_composite(const TcStillCompositeParams* pp, void* stream) {
  if (!pp) return TC_EINVAL;
  const TcStillCompositeParams& p = *pp;
  if (!p.video || !p.ends || !p.alpha || !p.out) return TC_EINVAL;
  if (p.b <= 0 || p.h <= 0 || p.w <= 0 || p.t <= 0) return TC_EINVAL;
  if (p.nf < 1 || p.f0 < 0 || p.f0 >= p.t || p.nf > p.t - p.f0) return TC_EINVAL;
  if (p.h % ST_CELL || p.w % ST_CELL || p.t < 2 || p.t > TC_TEMPORAL_MAX_FRAMES || p.b > 65535) return TC_ESHAPE;
  const int64_t plane = (int64_t)p.h * p.w;
  if (plane / 4 > (int64_t)INT32_MAX * 256) return TC_ESHAPE;
  if (!tc_aligned16(p.video) || !tc_aligned16(p.ends) || !tc_aligned16(p.alpha) || !tc_aligned16(p.out)) return TC_EALIGN;
  const int64_t clip_bytes = (int64_t)p.b * 3 * p.t * plane * (int64_t)sizeof(float);
  const bool inplace = p.out == p.video;
  if (!inplace && st_overlap(p.out, clip_bytes, p.video, clip_bytes)) return TC_EINVAL;
  if (st_overlap(p.out, clip_bytes, p.ends, (int64_t)p.b * 6 * plane * (int64_t)sizeof(float))) return TC_EINVAL;
  if (st_overlap(p.out, clip_bytes, p.alpha, (int64_t)p.b * plane * (int64_t)sizeof(float))) return TC_EINVAL;
  StCompositeArgs g;
  g.video = p.video; g.ends = p.ends; g.alpha = p.alpha; g.out = p.out;
  g.t = p.t; g.f0 = p.f0; g.nf = p.nf;
  g.plane4 = plane / 4;
  const float last = (float)(p.t - 1);
  for (int j = 0; j < TC_TEMPORAL_MAX_FRAMES; ++j) g.s[j] = j < p.t ? (float)j / last : 0.0f;
  const dim3 grid((unsigned)((g.plane4 + 255) / 256), (unsigned)(3 * ((p.nf + ST_FRAMES - 1) / ST_FRAMES)), (unsigned)p.b);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (inplace) hipLaunchKernelGGL(still_composite_kernel<true>, grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL(still_composite_kernel<false>, grid, dim3(256), 0, s, g);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
