// Frame deltas: 64-bin histograms of n images on a decoder's surfaces and, per pair (p, p + lag) and component, the sum of
// absolute differences, the count of samples that moved by more than tau and the L1 distance of the two histograms
// (tc_frame_deltas; the rule: include/tooncrafter_hip.h).  Everything is an integer, so nothing here depends on an order of
// summation:
//   frame_delta_kernel         one block per (image, plane, part): image p as `a` (its histogram, a private one per wave in LDS)
//                              and image p + lag as `b`, so a sample is read once in each role          -> workspace
//   frame_delta_finish_kernel  one block per (image, component): the parts added in int64, hist_l1      -> hist, delta
// No global atomics, no memset, no allocation, no synchronisation.
//
// A plane is rows of bytes whose components repeat with a fixed period: one (Y, Cb, Cr planes), two (NV12 chroma), three
// (packed RGB), or the upper bytes of 2-byte words (P010: one or two components).  A thread takes a chunk of 16 bytes (48 for
// RGB, so that a chunk always starts on a pixel) as dwords: |a - b| per component is v_sad_u8 on masked dwords, the histogram
// and the moved count go byte by byte.  As in colour_hist.hip, toon content puts most lanes into one bin and LDS atomics on
// one address serialise: a lane merges runs of equal bins into one add, and a wave whose lanes all hold one bin adds once.
#include "common.h"

namespace {

constexpr int FD_THREADS = 256;
constexpr int FD_WAVES = FD_THREADS / 64;
constexpr int FD_BINS = TC_DELTA_BINS;
constexpr int FD_ENTRIES = FD_BINS + 2;                    // a part's counts per component: the bins, sad, changed
constexpr int FD_PART_BYTES = 32768;                       // whole rows up to this many bytes make a part ...
constexpr int FD_SEG_BYTES = 3 << 18;                      // ... and a longer row is cut into segments: 255 * 3 * 2^18 < 2^31
constexpr int64_t FD_MAX_PIXELS = (int64_t)1 << 26;

static_assert(FD_SEG_BYTES % 48 == 0 && FD_PART_BYTES <= FD_SEG_BYTES, "a segment starts on a chunk; a part is at most a segment");
static_assert((int64_t)255 * FD_SEG_BYTES < INT32_MAX, "int32 part counters");

struct FdPlane {
  const uint8_t* base;
  int64_t image_stride;
  int32_t pitch, rows, row_bytes;
  int32_t kind;                                            // FD_K1 ..
  int32_t comp0;                                           // the component of the first sample of a row
  int32_t rows_per_part, col_parts;
  int32_t first, blocks;                                   // its blocks among an image's
};

struct FdArgs {
  FdPlane plane[3];
  int32_t planes, blocks_per_image;
  int32_t n, lag, tau;
  int32_t* part;                                           // [n * blocks_per_image][3][FD_ENTRIES]
};

struct FdFinishArgs {
  int32_t lo[3], hi[3];                                    // the blocks of an image that count component c
  int32_t blocks_per_image, n, lag;
  const int32_t* part;
  int32_t* hist;
  int64_t* delta;
};

enum { FD_K1 = 0, FD_K2 = 1, FD_K3 = 2, FD_W1 = 3, FD_W2 = 4 };

// the component (relative to the row's first) of byte k of a chunk, -1: the lower byte of a P010 word
template <int NCOMP, bool WIDE>
constexpr int fd_comp(int k) { return WIDE ? ((k & 1) ? (k >> 1) % NCOMP : -1) : k % NCOMP; }

// the bytes of dword d of a chunk that belong to component j
template <int NCOMP, bool WIDE>
constexpr uint32_t fd_mask(int d, int j) {
  uint32_t m = 0;
  for (int kk = 0; kk < 4; ++kk)
    if (fd_comp<NCOMP, WIDE>(4 * d + kk) == j) m |= 0xFFu << (8 * kk);
  return m;
}

template <int NCOMP, bool WIDE, int CHUNK>
constexpr int fd_count(int j) {
  int c = 0;
  for (int k = 0; k < CHUNK; ++k) c += fd_comp<NCOMP, WIDE>(k) == j;
  return c;
}

// `valid` bytes at p as CHUNK / 4 dwords, zero past them.  VEC: p is 16-byte aligned; a 16-byte load only where all of it is valid
template <bool VEC, int CHUNK>
__device__ __forceinline__ void fd_load(const uint8_t* __restrict__ p, int valid, uint32_t (&v)[CHUNK / 4]) {
#pragma unroll
  for (int q = 0; q < CHUNK / 16; ++q) {
    if (VEC && valid >= 16 * q + 16) {
      const uint4 t = *reinterpret_cast<const uint4*>(p + 16 * q);
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t w = 0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int k = 16 * q + 4 * d + kk;
          if (k < valid) w |= (uint32_t)p[k] << (8 * kk);
        }
        v[4 * q + d] = w;
      }
    }
  }
}

// One chunk: a's histogram into the wave's `h` (rows of FD_BINS, the row's first component at 0), |a - b| and the moved count
// into the lane's sums.  Bytes past `valid` are zero in a and b alike: no difference, not moved, and not counted in h.
template <int NCOMP, bool WIDE, int CHUNK, bool PAIR, bool FULL>
__device__ __forceinline__ void fd_chunk(const uint32_t (&a)[CHUNK / 4], const uint32_t (&b)[CHUNK / 4], int valid, int tau,
                                         int32_t* h, uint32_t (&sad)[NCOMP], uint32_t (&chg)[NCOMP]) {
  int cur[NCOMP], cnt[NCOMP];
#pragma unroll
  for (int j = 0; j < NCOMP; ++j) { cur[j] = -1; cnt[j] = 0; }
#pragma unroll
  for (int d = 0; d < CHUNK / 4; ++d) {
    if (PAIR) {
#pragma unroll
      for (int j = 0; j < NCOMP; ++j) {
        const uint32_t m = fd_mask<NCOMP, WIDE>(d, j);
        if (m != 0u) sad[j] = __builtin_amdgcn_sad_u8(a[d] & m, b[d] & m, sad[j]);
      }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = 4 * d + kk;
      const int j = fd_comp<NCOMP, WIDE>(k);
      if (j < 0) continue;
      if (!FULL && k >= valid) continue;
      const int va = (int)((a[d] >> (8 * kk)) & 0xFFu);
      if (PAIR) {
        const int vb = (int)((b[d] >> (8 * kk)) & 0xFFu);
        const int diff = va > vb ? va - vb : vb - va;
        chg[j] += diff > tau ? 1u : 0u;
      }
      const int bin = va >> 2;
      if (bin == cur[j]) {
        ++cnt[j];
      } else {
        if (cur[j] >= 0) atomicAdd(&h[j * FD_BINS + cur[j]], cnt[j]);
        cur[j] = bin;
        cnt[j] = 1;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NCOMP; ++j) {
    if (FULL) {                                                            // every lane here holds at least one run of j
      const int all = fd_count<NCOMP, WIDE, CHUNK>(j);
      const int first = __builtin_amdgcn_readfirstlane(cur[j]);
      const unsigned long long active = __ballot(1);
      if (__ballot(cnt[j] == all && cur[j] == first) == active) {          // the whole wave in one bin: one add
        if ((int)(threadIdx.x & 63) == __ffsll(active) - 1) atomicAdd(&h[j * FD_BINS + first], all * __popcll(active));
      } else {
        atomicAdd(&h[j * FD_BINS + cur[j]], cnt[j]);
      }
    } else if (cur[j] >= 0) {
      atomicAdd(&h[j * FD_BINS + cur[j]], cnt[j]);
    }
  }
}

__device__ __forceinline__ uint32_t fd_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The rows [r0, r1) x bytes [c0, c1) of plane `pl` of image `image` (and of image + lag): chunk idx = row * chunks + chunk
template <int NCOMP, bool WIDE, bool VEC, bool PAIR>
__device__ __forceinline__ void fd_part(const FdPlane& pl, int image, int lag, int tau, int r0, int r1, int c0, int c1, int32_t* h,
                                        uint32_t (&red)[FD_WAVES][6], int32_t* __restrict__ out) {
  constexpr int CHUNK = NCOMP == 3 ? 48 : 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t* mine = h + wave * 3 * FD_BINS;                                  // h: the four waves' histograms, 3 * FD_BINS each
  uint32_t sad[NCOMP], chg[NCOMP];
#pragma unroll
  for (int j = 0; j < NCOMP; ++j) sad[j] = chg[j] = 0;
  const int chunks = (c1 - c0 + CHUNK - 1) / CHUNK;
  const int total = (r1 - r0) * chunks;                                    // at most FD_SEG_BYTES / 16
  const uint8_t* pa = pl.base + (int64_t)image * pl.image_stride;
  const uint8_t* pb = pa + (int64_t)lag * pl.image_stride;                 // used with PAIR only
  for (int idx = threadIdx.x; idx < total; idx += FD_THREADS) {
    const int r = idx / chunks, c = idx - r * chunks;
    const int at = c0 + c * CHUNK;
    const int valid = min(CHUNK, c1 - at);
    const int64_t off = (int64_t)(r0 + r) * pl.pitch + at;
    uint32_t a[CHUNK / 4], b[CHUNK / 4];
    fd_load<VEC, CHUNK>(pa + off, valid, a);
    if (PAIR) {
      fd_load<VEC, CHUNK>(pb + off, valid, b);
    } else {
#pragma unroll
      for (int d = 0; d < CHUNK / 4; ++d) b[d] = a[d];
    }
    if (valid == CHUNK) fd_chunk<NCOMP, WIDE, CHUNK, PAIR, true>(a, b, valid, tau, mine, sad, chg);
    else fd_chunk<NCOMP, WIDE, CHUNK, PAIR, false>(a, b, valid, tau, mine, sad, chg);
  }
#pragma unroll
  for (int j = 0; j < NCOMP; ++j) {
    const uint32_t s = fd_wave_sum(sad[j]), m = fd_wave_sum(chg[j]);
    if (lane == 0) { red[wave][2 * j] = s; red[wave][2 * j + 1] = m; }
  }
  __syncthreads();                                                         // the waves' histograms and sums are complete
  for (int i = threadIdx.x; i < NCOMP * FD_BINS; i += FD_THREADS) {
    const int j = i / FD_BINS, k = i - j * FD_BINS;
    int32_t v = 0;
#pragma unroll
    for (int w = 0; w < FD_WAVES; ++w) v += h[w * 3 * FD_BINS + i];
    out[j * FD_ENTRIES + k] = v;
  }
  if (threadIdx.x < 2 * NCOMP) {
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < FD_WAVES; ++w) v += red[w][threadIdx.x];
    out[(threadIdx.x >> 1) * FD_ENTRIES + FD_BINS + (threadIdx.x & 1)] = (int32_t)v;
  }
}

template <bool VEC, bool PAIR>
__device__ __forceinline__ void fd_kind(const FdPlane& pl, int image, int lag, int tau, int r0, int r1, int c0, int c1, int32_t* h,
                                        uint32_t (&red)[FD_WAVES][6], int32_t* out) {
  switch (pl.kind) {                                                       // the same for the whole block
    case FD_K1: fd_part<1, false, VEC, PAIR>(pl, image, lag, tau, r0, r1, c0, c1, h, red, out); break;
    case FD_K2: fd_part<2, false, VEC, PAIR>(pl, image, lag, tau, r0, r1, c0, c1, h, red, out); break;
    case FD_K3: fd_part<3, false, VEC, PAIR>(pl, image, lag, tau, r0, r1, c0, c1, h, red, out); break;
    case FD_W1: fd_part<1, true, VEC, PAIR>(pl, image, lag, tau, r0, r1, c0, c1, h, red, out); break;
    default: fd_part<2, true, VEC, PAIR>(pl, image, lag, tau, r0, r1, c0, c1, h, red, out); break;
  }
}

// blockIdx.x = image * blocks_per_image + j; block j of an image is part (j - first) of the plane whose blocks hold j, parts
// ordered row part by row part, a long row's segments side by side.  A part's counts go to part[blockIdx.x][component].
template <bool VEC>
__global__ __launch_bounds__(FD_THREADS) void frame_delta_kernel(const FdArgs g) {
  __shared__ int32_t h[FD_WAVES][3][FD_BINS];
  __shared__ uint32_t red[FD_WAVES][6];
  const int image = blockIdx.x / g.blocks_per_image, j = blockIdx.x - image * g.blocks_per_image;
  const int which = (g.planes > 2 && j >= g.plane[2].first) ? 2 : (g.planes > 1 && j >= g.plane[1].first) ? 1 : 0;
  const FdPlane& pl = g.plane[which];
  const int jp = j - pl.first;
  const int rp = jp / pl.col_parts, cp = jp - rp * pl.col_parts;
  const int r0 = rp * pl.rows_per_part, r1 = min(pl.rows, r0 + pl.rows_per_part);
  const int c0 = cp * FD_SEG_BYTES, c1 = (int)min((int64_t)pl.row_bytes, (int64_t)c0 + FD_SEG_BYTES);
  for (int i = threadIdx.x; i < FD_WAVES * 3 * FD_BINS; i += FD_THREADS) (&h[0][0][0])[i] = 0;
  __syncthreads();
  int32_t* out = g.part + ((int64_t)blockIdx.x * 3 + pl.comp0) * FD_ENTRIES;
  if (image + g.lag < g.n) {
    fd_kind<VEC, true>(pl, image, g.lag, g.tau, r0, r1, c0, c1, &h[0][0][0], red, out);
  } else {
    fd_kind<VEC, false>(pl, image, g.lag, g.tau, r0, r1, c0, c1, &h[0][0][0], red, out);
  }
}

// One block per (image, component).  Wave w adds the parts lo + w, lo + w + 4, ... of its image, lane k bin k and lanes 0, 1
// sad and changed; for a pair also the bins of image + lag, which its own block adds once more for hist -- the price of
// having no third launch.
__global__ __launch_bounds__(FD_THREADS) void frame_delta_finish_kernel(const FdFinishArgs g) {
  __shared__ int32_t ha[FD_WAVES][FD_BINS], hb[FD_WAVES][FD_BINS];
  __shared__ int64_t two[FD_WAVES][2];
  const int image = blockIdx.x / 3, c = blockIdx.x - image * 3;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool pair = image + g.lag < g.n;
  int32_t a = 0, b = 0;
  int64_t s = 0;
  for (int p = g.lo[c] + wave; p < g.hi[c]; p += FD_WAVES) {
    const int32_t* pa = g.part + (((int64_t)image * g.blocks_per_image + p) * 3 + c) * FD_ENTRIES;
    a += pa[lane];
    if (lane < 2) s += pa[FD_BINS + lane];
    if (pair) b += g.part[(((int64_t)(image + g.lag) * g.blocks_per_image + p) * 3 + c) * FD_ENTRIES + lane];
  }
  ha[wave][lane] = a;
  hb[wave][lane] = b;
  if (lane < 2) two[wave][lane] = s;
  __syncthreads();
  if (wave != 0) return;
  a = (ha[0][lane] + ha[1][lane]) + (ha[2][lane] + ha[3][lane]);
  g.hist[((int64_t)image * 3 + c) * FD_BINS + lane] = a;
  if (!pair) return;
  b = (hb[0][lane] + hb[1][lane]) + (hb[2][lane] + hb[3][lane]);
  int64_t l1 = a > b ? (int64_t)a - b : (int64_t)b - a;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) l1 += __shfl_xor(l1, off, 64);
  int64_t* out = g.delta + ((int64_t)image * 3 + c) * 3;
  if (lane < 2) out[lane] = (two[0][lane] + two[1][lane]) + (two[2][lane] + two[3][lane]);
  if (lane == 2) out[2] = l1;
}

inline bool fd_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// a plane's share of an image's blocks
void fd_plan(FdPlane* pl, const void* base, int64_t image_stride, int32_t pitch, int32_t rows, int64_t row_bytes, int kind, int comp0,
             int64_t* blocks) {
  pl->base = static_cast<const uint8_t*>(base);
  pl->image_stride = image_stride;
  pl->pitch = pitch;
  pl->rows = rows;
  pl->row_bytes = (int32_t)row_bytes;
  pl->kind = kind;
  pl->comp0 = comp0;
  pl->col_parts = (int32_t)((row_bytes + FD_SEG_BYTES - 1) / FD_SEG_BYTES);
  pl->rows_per_part = pl->col_parts > 1 ? 1 : (int32_t)(FD_PART_BYTES / row_bytes > 0 ? FD_PART_BYTES / row_bytes : 1);
  const int64_t row_parts = ((int64_t)rows + pl->rows_per_part - 1) / pl->rows_per_part;
  pl->first = (int32_t)*blocks;
  pl->blocks = (int32_t)(row_parts * pl->col_parts);
  *blocks += pl->blocks;
}

// TC_OK and the launches' arguments, or the refusal of a request (the workspace is the caller's to check)
int fd_request(const TcFrameDeltaParams* pp, FdArgs* g, FdFinishArgs* f, bool* vec, int64_t* workspace_bytes) {
  if (!pp) return TC_EINVAL;
  const TcFrameDeltaParams& p = *pp;
  if (!p.y || !p.hist) return TC_EINVAL;
  if (p.n <= 0 || p.lag < 1 || p.tau < 0 || p.tau > 255 || p.h <= 0 || p.w <= 0) return TC_EINVAL;
  if (p.n > p.lag && !p.delta) return TC_EINVAL;
  const bool rgb = p.format == TC_PIXFMT_RGB24, wide = p.format == TC_PIXFMT_P010;
  if (!rgb && p.format != TC_PIXFMT_I420 && p.format != TC_PIXFMT_NV12 && !wide) return TC_EINVAL;
  if ((p.c0 != nullptr) != !rgb || (p.c1 != nullptr) != (p.format == TC_PIXFMT_I420)) return TC_EINVAL;
  const int64_t ch = ((int64_t)p.h + 1) / 2, cw = ((int64_t)p.w + 1) / 2;
  const int64_t row_y = rgb ? 3 * (int64_t)p.w : wide ? 2 * (int64_t)p.w : p.w;
  const int64_t row_c = p.format == TC_PIXFMT_I420 ? cw : wide ? 4 * cw : 2 * cw;
  if (p.pitch_y < row_y || p.image_stride_y < (int64_t)p.h * p.pitch_y) return TC_EINVAL;
  if (!rgb && (p.pitch_c < row_c || p.image_stride_c < ch * p.pitch_c)) return TC_EINVAL;
  if (wide && (!fd_aligned(p.y, 2) || !fd_aligned(p.c0, 2) || (p.pitch_y | p.pitch_c | p.image_stride_y | p.image_stride_c) & 1))
    return TC_EALIGN;
  if (!fd_aligned(p.hist, 4) || (p.n > p.lag && !fd_aligned(p.delta, 8))) return TC_EALIGN;
  if ((int64_t)p.h * p.w > FD_MAX_PIXELS) return TC_ESHAPE;
  int64_t blocks = 0;
  *vec = tc_aligned16(p.y) && p.pitch_y % 16 == 0 && p.image_stride_y % 16 == 0;
  if (rgb) {
    g->planes = 1;
    fd_plan(&g->plane[0], p.y, p.image_stride_y, p.pitch_y, p.h, row_y, FD_K3, 0, &blocks);
    g->plane[1] = g->plane[2] = g->plane[0];
  } else {
    *vec = *vec && tc_aligned16(p.c0) && p.pitch_c % 16 == 0 && p.image_stride_c % 16 == 0;
    fd_plan(&g->plane[0], p.y, p.image_stride_y, p.pitch_y, p.h, row_y, wide ? FD_W1 : FD_K1, 0, &blocks);
    if (p.format == TC_PIXFMT_I420) {
      *vec = *vec && tc_aligned16(p.c1);
      g->planes = 3;
      fd_plan(&g->plane[1], p.c0, p.image_stride_c, p.pitch_c, (int32_t)ch, row_c, FD_K1, 1, &blocks);
      fd_plan(&g->plane[2], p.c1, p.image_stride_c, p.pitch_c, (int32_t)ch, row_c, FD_K1, 2, &blocks);
    } else {
      g->planes = 2;
      fd_plan(&g->plane[1], p.c0, p.image_stride_c, p.pitch_c, (int32_t)ch, row_c, wide ? FD_W2 : FD_K2, 1, &blocks);
      g->plane[2] = g->plane[1];
    }
  }
  if (blocks * p.n > INT32_MAX || (int64_t)p.n * 3 > INT32_MAX) return TC_ESHAPE;
  g->blocks_per_image = (int32_t)blocks;
  g->n = p.n; g->lag = p.lag; g->tau = p.tau;
  for (int c = 0; c < 3; ++c) {                              // the plane that holds component c
    const FdPlane& pl = g->plane[rgb ? 0 : g->planes == 3 ? c : c > 0];
    f->lo[c] = pl.first;
    f->hi[c] = pl.first + pl.blocks;
  }
  f->blocks_per_image = g->blocks_per_image;
  f->n = p.n; f->lag = p.lag;
  f->hist = p.hist;
  f->delta = p.delta;
  *workspace_bytes = (int64_t)p.n * blocks * 3 * FD_ENTRIES * (int64_t)sizeof(int32_t);
  return TC_OK;
}

}  // namespace

extern "C" int64_t tc_frame_deltas_workspace(const TcFrameDeltaParams* p) {
  FdArgs g;
  FdFinishArgs f;
  bool vec = false;
  int64_t bytes = 0;
  return fd_request(p, &g, &f, &vec, &bytes) == TC_OK ? bytes : 0;
}

extern "C" int tc_frame_deltas(const TcFrameDeltaParams* pp, void* stream) {
  FdArgs g;
  FdFinishArgs f;
  bool vec = false;
  int64_t bytes = 0;
  if (const int rc = fd_request(pp, &g, &f, &vec, &bytes)) return rc;
  const TcFrameDeltaParams& p = *pp;
  if (!p.workspace) return TC_EWORKSPACE;
  if (!fd_aligned(p.workspace, 8)) return TC_EALIGN;
  if (p.workspace_bytes < bytes) return TC_EWORKSPACE;
  g.part = reinterpret_cast<int32_t*>(p.workspace);
  f.part = g.part;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((int64_t)p.n * g.blocks_per_image));
  if (vec) hipLaunchKernelGGL(frame_delta_kernel<true>, grid, dim3(FD_THREADS), 0, s, g);
  else hipLaunchKernelGGL(frame_delta_kernel<false>, grid, dim3(FD_THREADS), 0, s, g);
  TC_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_delta_finish_kernel, dim3((unsigned)(p.n * 3)), dim3(FD_THREADS), 0, s, f);
  TC_LAUNCH_CHECK();
  return TC_OK;
}
