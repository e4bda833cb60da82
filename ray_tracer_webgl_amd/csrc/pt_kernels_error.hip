// pt_kernels_error.hip — the PER-PIXEL ERROR ESTIMATE (pt_set_option PT_OPT_ERROR_ESTIMATE; include/ptrace.h, DESIGN.md
// §error estimate), a translation unit and gfx950 code object of its own: the HIP runtime loads it when the estimate is
// first turned on, so a context that never asks for it pays nothing.  Seven kernels, none of them a trace kernel:
//   pt_fold_error_kernel     takes pt_accumulate_kernel's place: the same four fp32 adds per pass in the same order (accum
//                            keeps its bits) and, beside them, Welford's update of the pass sums' mean and M2 per channel
//   pt_resolve_error_kernel  the standard error of each pixel's mean as linear radiance
//   pt_error_tiles_kernel    per 8x8 tile of the local rows, one wave64: sums of se^2 and mean^2 over the counted pixels
//   pt_partition_order_kernel, pt_fold_error_tiles_kernel   a partial round of pt_render_adaptive: the queue's tile table with
//                            the active tiles first, and the fold over those tiles' pixels only
//   pt_filter_kernel         the variance-guided filtered read-out (pt_resolve_filtered): each pixel's mean averaged with the
//                            neighbours whose means differ by no more than the standard errors explain
//   pt_filter_patch_kernel   the same read-out with the test summed over the patches around the two pixels
//                            (pt_resolve_filtered_patch)
// The arithmetic is a contract (tests/error_ref.py restates it statement by statement): ONE IEEE fp32 operation per
// statement, nothing fused (-ffp-contract=off), `/` and sqrtf correctly rounded.  pt_api.hip reaches the kernels through
// pt_error_kernel() only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_error_plan.hpp"
#include "pt_extra.h"
#include "pt_sigs.h"

// state per pixel i: est[2 i] = A = {mean.r, mean.g, mean.b, n}, est[2 i + 1] = B = {M2.r, M2.g, M2.b, k}
// (n passes folded, k their samples: both live in the buffer, like accum.w, so a hipGraph replay keeps them right)
__device__ __forceinline__ void welford(float x, float n, float& mean, float& m2) {
  const float d = x - mean;
  const float q = d / n;
  mean = mean + q;
  const float e = x - mean;
  const float t = d * e;
  m2 = m2 + t;
}

// one pixel's fold over the launch's slabs: the statements of the contract, shared by the two fold kernels below
__device__ __forceinline__ void fold_pixel(float4* accum, float4* est, const float4* slab, size_t i, size_t n_pix, uint32_t n_passes) {
  float4 acc = accum[i];
  float4 a = est[2 * i], b = est[2 * i + 1];
  for (uint32_t p = 0; p < n_passes; p++) {
    const float4 s = slab[(size_t)p * n_pix + i];
    acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w;
    a.w = a.w + 1.0f;
    b.w = b.w + s.w;
    welford(s.x, a.w, a.x, b.x);
    welford(s.y, a.w, a.y, b.y);
    welford(s.z, a.w, a.z, b.z);
  }
  accum[i] = acc;
  est[2 * i] = a;
  est[2 * i + 1] = b;
}

extern "C" __global__ __launch_bounds__(256) void pt_fold_error_kernel(float4* accum, float4* est, const float4* slab,
                                                                       uint32_t n_pix, uint32_t n_passes) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) fold_pixel(accum, est, slab, i, n_pix, n_passes);
}

// The fold of a PARTIAL round (pt_render_adaptive): one wave64 per table position j < n_active, its tile order[j], lane l owns
// local pixel (8 tx + l % 8, 8 ty + l / 8) as in the tile kernel below; a lane inside the image folds its pixel exactly as
// pt_fold_error_kernel does.  Pixels of the other tiles are neither read nor written (their slab slots are stale).
extern "C" __global__ __launch_bounds__(256) void pt_fold_error_tiles_kernel(float4* accum, float4* est, const float4* slab,
                                                                             const uint32_t* order, uint32_t n_active,
                                                                             uint32_t width, uint32_t rows, uint32_t tiles_x,
                                                                             uint32_t n_passes) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  const size_t n_pix = (size_t)width * rows;
  for (uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n_active; j += waves) {
    const uint32_t t = order[j];
    const uint32_t x = 8u * (t % tiles_x) + (lane & 7u), y = 8u * (t / tiles_x) + (lane >> 3);
    if (x < width && y < rows) fold_pixel(accum, est, slab, (size_t)y * width + x, n_pix, n_passes);
  }
}

// The tile table of a partial round: a STABLE PARTITION of the queue's current order by flags[tile] — the flagged tiles first in
// their present relative order, then the rest, a full permutation again (every tile_order[...] read of the refill stays valid);
// `base` receives the order as it was found.  One 1024-thread workgroup: thread t owns a run of ceil(n / 1024) positions,
// counts its flagged ones, an inclusive scan of the counts in the LDS gives every run its two starts.
extern "C" __global__ __launch_bounds__(1024) void pt_partition_order_kernel(const uint32_t* order, const uint32_t* flags,
                                                                             uint32_t* part, uint32_t* base, uint32_t n_tiles) {
  __shared__ uint32_t s_scan[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n_tiles + 1023u) / 1024u;
  const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
  uint32_t cnt = 0;
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t tile = order[i];
    cnt += (tile < n_tiles && flags[tile] != 0u) ? 1u : 0u;
  }
  s_scan[t] = cnt;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint32_t v = t >= off ? s_scan[t - off] : 0u;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  const uint32_t total = s_scan[1023];
  uint32_t a = s_scan[t] - cnt;      // flagged tiles before this run
  uint32_t r = total + (lo - a);     // the rest start behind all flagged ones
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t tile = order[i];
    base[i] = tile;
    if (tile < n_tiles && flags[tile] != 0u) part[a++] = tile; else part[r++] = tile;
  }
}

// what a pixel's state reads as: se = sqrt(M2 / (n (n - 1))) n / k, the estimate's own mean m = mean n / k
struct PixelError { float se[3], m[3]; bool known; };
__device__ __forceinline__ PixelError pixel_error(const float4 a, const float4 b) {
  PixelError r;
  const float n = a.w, k = b.w;
  r.known = (n >= 2.0f) && (k > 0.0f);
  const float q = n / k;
  const float n1 = n - 1.0f;
  const float nn = n * n1;
  const float mean[3] = {a.x, a.y, a.z}, m2[3] = {b.x, b.y, b.z};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float v = m2[c] / nn;
    const float s = __builtin_sqrtf(v);
    r.se[c] = r.known ? s * q : 0.0f;
    r.m[c] = r.known ? mean[c] * q : 0.0f;
  }
  return r;
}

extern "C" __global__ __launch_bounds__(256) void pt_resolve_error_kernel(const float4* est, float4* out, uint32_t n_pix) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    const float4 a = est[2 * (size_t)i], b = est[2 * (size_t)i + 1];
    const PixelError r = pixel_error(a, b);
    out[i] = make_float4(r.se[0], r.se[1], r.se[2], a.w);
  }
}

__device__ __forceinline__ bool finite3(const float v[3]) {
  return __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]);
}

// One wave64 per 8x8 tile (the work queue's tiles, of the context's LOCAL rows); lane l owns pixel (8 tx + l % 8, 8 ty + l / 8).
// The wave reduces with the fixed tree  for off in 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l + off] (l < off)  through cross-lane
// moves (__shfl_down: a lane at or above `off` computes something nobody reads), so a tile's record depends on the state
// alone — not on the launch shape, which only decides which wave takes which tile.
//   tiles[t] = {sum e, sum m2, counted lanes, min n over counted lanes (0 if none)}
//   aux[t]   = {lanes with !(n >= 2), lanes with n >= 2 that are not counted (k <= 0 or NaN, se or m not finite),
//               max n over counted lanes (0 if none), 0}                                   (what pt_error_stats adds up)
extern "C" __global__ __launch_bounds__(256) void pt_error_tiles_kernel(const float4* est, float4* tiles, float4* aux,
                                                                        uint32_t width, uint32_t rows, uint32_t tiles_x,
                                                                        uint32_t n_tiles) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n_tiles; t += waves) {
    const uint32_t x = 8u * (t % tiles_x) + (lane & 7u), y = 8u * (t / tiles_x) + (lane >> 3);
    const bool inside = x < width && y < rows;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (inside) {
      const size_t i = (size_t)y * width + x;
      a = est[2 * i];
      b = est[2 * i + 1];
    }
    const PixelError r = pixel_error(a, b);
    const bool counted = inside && r.known && finite3(r.se) && finite3(r.m);
    const float e01 = r.se[0] * r.se[0], e1 = r.se[1] * r.se[1], e2 = r.se[2] * r.se[2];
    const float m01 = r.m[0] * r.m[0], m1 = r.m[1] * r.m[1], m2 = r.m[2] * r.m[2];
    const float es = e01 + e1, ms = m01 + m1;
    float e = counted ? es + e2 : 0.0f;
    float m = counted ? ms + m2 : 0.0f;
    float cnt = counted ? 1.0f : 0.0f;
    float nmin = counted ? a.w : __builtin_inff();
    float nmax = counted ? a.w : 0.0f;
    const bool is_short = inside && !(a.w >= 2.0f);
    float n_short = is_short ? 1.0f : 0.0f;
    float n_bad = (inside && !is_short && !counted) ? 1.0f : 0.0f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      e = e + __shfl_down(e, off, 64);
      m = m + __shfl_down(m, off, 64);
      cnt = cnt + __shfl_down(cnt, off, 64);
      n_short = n_short + __shfl_down(n_short, off, 64);
      n_bad = n_bad + __shfl_down(n_bad, off, 64);
      nmin = fminf(nmin, __shfl_down(nmin, off, 64));
      nmax = fmaxf(nmax, __shfl_down(nmax, off, 64));
    }
    if (lane == 0u) {
      tiles[t] = make_float4(e, m, cnt, cnt > 0.0f ? nmin : 0.0f);
      aux[t] = make_float4(n_short, n_bad, nmax, 0.0f);
    }
  }
}

// THE FILTERED READ-OUT (pt_resolve_filtered; the statements: include/ptrace.h, DESIGN.md §4.8d, tests/filter_ref.py).  A
// 256-thread workgroup owns a 32x8 tile of output pixels, thread t the pixel (t % 32, t / 32) of it.  It stages the tile and a halo
// of PT_FILTER_MAX_RADIUS texels into the LDS as seven planes — m.rgb, v.rgb = se.rgb^2 and the counted flag — so the read-out
// (three divisions, three square roots, the finiteness tests) is evaluated once per staged texel, not per tap; texels outside
// the image are staged as not counted.  After one barrier every pixel runs the tap loop from the LDS in the contract's order
// (dy ascending, then dx ascending); a tap row outside the pixel's chunk of band rows is rejected by comparing it with the
// chunk's first and last local row, computed once per pixel.
// Row stride 40 = the staged width, no padding: every LDS access here is a ds_read_b32 / ds_write_b32, which the LDS serves in
// two groups of 32 lanes with 32 banks.  A group is one 32-pixel row of the tile: 32 consecutive dwords, conflict-free whatever
// the stride; and the staging stores of 32 consecutive texels are 32 consecutive dwords only without padding.
#define FILTER_TW 32
#define FILTER_TH 8
#define FILTER_SW (FILTER_TW + 2 * PT_FILTER_MAX_RADIUS)
#define FILTER_SH (FILTER_TH + 2 * PT_FILTER_MAX_RADIUS)
struct FilterTile {
  float m[3][FILTER_SH * FILTER_SW], v[3][FILTER_SH * FILTER_SW];
  uint32_t counted[FILTER_SH * FILTER_SW];
};

// one pixel's taps, the loops over the launch-uniform radius at run time: a tap is seven LDS reads and some twenty VALU
// operations, beside which its address arithmetic does not count; one instantiation per radius with both loops unrolled made
// the scheduler hoist the 567 reads of radius 4 (512 registers, spills, one wave per SIMD)
__device__ __forceinline__ float4 filter_taps(const FilterTile& s, int centre, int y, int first_row, int last_row, int R, float k2) {
  const float mp[3] = {s.m[0][centre], s.m[1][centre], s.m[2][centre]};
  const float vp[3] = {s.v[0][centre], s.v[1][centre], s.v[2][centre]};
  float sum[3] = {0.0f, 0.0f, 0.0f};
  float cnt = 0.0f;
  for (int dy = -R; dy <= R; dy++) {
    if (y + dy < first_row || y + dy > last_row) continue;   // (uniform over a row of the tile: half a wave)
    for (int dx = -R; dx <= R; dx++) {
      const int q = centre + dy * FILTER_SW + dx;
      const float mq[3] = {s.m[0][q], s.m[1][q], s.m[2][q]};
      const float vq[3] = {s.v[0][q], s.v[1][q], s.v[2][q]};
      const float d0 = mp[0] - mq[0], d1 = mp[1] - mq[1], d2 = mp[2] - mq[2];
      const float e0 = d0 * d0, e1 = d1 * d1, e2 = d2 * d2;
      const float t01 = e0 + e1;
      const float t = t01 + e2;
      const float s0 = vp[0] + vq[0], s1 = vp[1] + vq[1], s2 = vp[2] + vq[2];
      const float u01 = s0 + s1;
      const float u = u01 + s2;
      const float rhs = k2 * u;
      const bool ok = s.counted[q] != 0u && ((dx == 0 && dy == 0) || t <= rhs);   // the centre is accepted untested
      const float a0 = sum[0] + mq[0], a1 = sum[1] + mq[1], a2 = sum[2] + mq[2];
      const float c1 = cnt + 1.0f;
      sum[0] = ok ? a0 : sum[0];
      sum[1] = ok ? a1 : sum[1];
      sum[2] = ok ? a2 : sum[2];
      cnt = ok ? c1 : cnt;
    }
  }
  return make_float4(sum[0] / cnt, sum[1] / cnt, sum[2] / cnt, cnt);
}

// grid: ceil(width / 32) x ceil(rows / 8) workgroups.  band_rows: the chunk height of a band context, 0 for a context that is no
// band (pt_error_plan.hpp chunk_rows).
extern "C" __global__ __launch_bounds__(256) void pt_filter_kernel(const float4* est, float4* out, uint32_t width, uint32_t rows,
                                                                   uint32_t band_rows, uint32_t radius, float kappa, int gamma) {
  __shared__ FilterTile s;
  const int x0 = (int)(blockIdx.x * FILTER_TW), y0 = (int)(blockIdx.y * FILTER_TH);
  for (int i = (int)threadIdx.x; i < FILTER_SH * FILTER_SW; i += 256) {
    const int gx = x0 + i % FILTER_SW - PT_FILTER_MAX_RADIUS, gy = y0 + i / FILTER_SW - PT_FILTER_MAX_RADIUS;
    const bool inside = gx >= 0 && gx < (int)width && gy >= 0 && gy < (int)rows;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (inside) {
      const size_t j = (size_t)gy * width + (size_t)gx;
      a = est[2 * j];
      b = est[2 * j + 1];
    }
    const PixelError r = pixel_error(a, b);
    s.counted[i] = (inside && r.known && finite3(r.se) && finite3(r.m)) ? 1u : 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      s.m[c][i] = r.m[c];
      s.v[c][i] = r.se[c] * r.se[c];
    }
  }
  __syncthreads();
  const int tx = (int)(threadIdx.x % FILTER_TW), ty = (int)(threadIdx.x / FILTER_TW);
  const int x = x0 + tx, y = y0 + ty;
  if (x >= (int)width || y >= (int)rows) return;
  const int centre = (ty + PT_FILTER_MAX_RADIUS) * FILTER_SW + tx + PT_FILTER_MAX_RADIUS;
  float4 f = make_float4(s.m[0][centre], s.m[1][centre], s.m[2][centre], 0.0f);   // an uncounted centre passes through
  if (s.counted[centre] != 0u) {
    const pterr::ChunkRows ch = pterr::chunk_rows((uint32_t)y, band_rows, rows);
    const int first_row = (int)ch.first, last_row = (int)ch.last;
    const float k2 = kappa * kappa;
    f = filter_taps(s, centre, y, first_row, last_row, (int)radius, k2);
  }
  if (gamma != 0) {
    f.x = __builtin_sqrtf(f.x);
    f.y = __builtin_sqrtf(f.y);
    f.z = __builtin_sqrtf(f.z);
  }
  out[(size_t)y * width + (size_t)x] = f;
}

// THE PATCH-WISE FILTERED READ-OUT (pt_resolve_filtered_patch; the statements: include/ptrace.h, DESIGN.md §4.8f,
// tests/patch_filter_ref.py).  pt_filter_kernel's shape — a 256-thread workgroup per 32x8 tile, the seven planes staged once, one
// barrier — with a halo of PT_FILTER_MAX_RADIUS + PT_FILTER_MAX_PATCH = 5 texels: b = q + (ox, oy) lies up to radius + patch
// from the pixel.  42x18 texels, 21 168 B static.  Each pixel evaluates the (2P+1)^2 pair terms of a tap from the LDS (form (a)
// of §4.8f); a term whose row a.y or b.y lies outside the pixel's chunk is rejected by the same two compares as a tap row,
// a term outside the image by its staged counted flag.
// Row stride 42, no padding: every LDS access is again a dword access, served in two groups of 32 lanes over 32 banks, and a
// group is one 32-pixel row of the tile at ONE offset (dx + ox, dy + oy): 32 consecutive dwords, conflict-free at any stride,
// 42 included.
#define PATCH_HALO (PT_FILTER_MAX_RADIUS + PT_FILTER_MAX_PATCH)
#define PATCH_SW (FILTER_TW + 2 * PATCH_HALO)
#define PATCH_SH (FILTER_TH + 2 * PATCH_HALO)
struct PatchTile {
  float m[3][PATCH_SH * PATCH_SW], v[3][PATCH_SH * PATCH_SW];
  uint32_t counted[PATCH_SH * PATCH_SW];
};

// one pixel's taps; all four loops run over launch-uniform bounds at run time (pt_filter_kernel's finding: unrolled, the
// scheduler hoists the loads).  A pair term is thirteen LDS reads (the flags of a and b beside the twelve operands) and some
// twenty VALU operations.
__device__ __forceinline__ float4 filter_patch_taps(const PatchTile& s, int centre, int y, int first_row, int last_row, int R, int P,
                                                    float k2) {
  float sum[3] = {0.0f, 0.0f, 0.0f};
  float cnt = 0.0f;
  for (int dy = -R; dy <= R; dy++) {
    if (y + dy < first_row || y + dy > last_row) continue;   // (uniform over a row of the tile: half a wave)
    for (int dx = -R; dx <= R; dx++) {
      const int q = centre + dy * PATCH_SW + dx;
      float T = 0.0f, U = 0.0f;
      for (int oy = -P; oy <= P; oy++) {
        if (y + oy < first_row || y + oy > last_row || y + dy + oy < first_row || y + dy + oy > last_row) continue;
        for (int ox = -P; ox <= P; ox++) {
          const int a = centre + oy * PATCH_SW + ox, b = q + oy * PATCH_SW + ox;
          const float d0 = s.m[0][a] - s.m[0][b], d1 = s.m[1][a] - s.m[1][b], d2 = s.m[2][a] - s.m[2][b];
          const float e0 = d0 * d0, e1 = d1 * d1, e2 = d2 * d2;
          const float t01 = e0 + e1;
          const float t = t01 + e2;
          const float s0 = s.v[0][a] + s.v[0][b], s1 = s.v[1][a] + s.v[1][b], s2 = s.v[2][a] + s.v[2][b];
          const float u01 = s0 + s1;
          const float u = u01 + s2;
          const bool both = s.counted[a] != 0u && s.counted[b] != 0u;
          const float Tt = T + t, Uu = U + u;
          T = both ? Tt : T;
          U = both ? Uu : U;
        }
      }
      const float rhs = k2 * U;
      const bool ok = s.counted[q] != 0u && ((dx == 0 && dy == 0) || T <= rhs);   // the centre is accepted untested
      const float mq[3] = {s.m[0][q], s.m[1][q], s.m[2][q]};
      const float a0 = sum[0] + mq[0], a1 = sum[1] + mq[1], a2 = sum[2] + mq[2];
      const float c1 = cnt + 1.0f;
      sum[0] = ok ? a0 : sum[0];
      sum[1] = ok ? a1 : sum[1];
      sum[2] = ok ? a2 : sum[2];
      cnt = ok ? c1 : cnt;
    }
  }
  return make_float4(sum[0] / cnt, sum[1] / cnt, sum[2] / cnt, cnt);
}

// grid and band_rows as pt_filter_kernel's; radius <= PT_FILTER_MAX_RADIUS and patch <= PT_FILTER_MAX_PATCH (the host checks
// both: the halo is sized by them)
extern "C" __global__ __launch_bounds__(256) void pt_filter_patch_kernel(const float4* est, float4* out, uint32_t width, uint32_t rows,
                                                                         uint32_t band_rows, uint32_t radius, uint32_t patch, float kappa,
                                                                         int gamma) {
  __shared__ PatchTile s;
  const int x0 = (int)(blockIdx.x * FILTER_TW), y0 = (int)(blockIdx.y * FILTER_TH);
  for (int i = (int)threadIdx.x; i < PATCH_SH * PATCH_SW; i += 256) {
    const int gx = x0 + i % PATCH_SW - PATCH_HALO, gy = y0 + i / PATCH_SW - PATCH_HALO;
    const bool inside = gx >= 0 && gx < (int)width && gy >= 0 && gy < (int)rows;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (inside) {
      const size_t j = (size_t)gy * width + (size_t)gx;
      a = est[2 * j];
      b = est[2 * j + 1];
    }
    const PixelError r = pixel_error(a, b);
    s.counted[i] = (inside && r.known && finite3(r.se) && finite3(r.m)) ? 1u : 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      s.m[c][i] = r.m[c];
      s.v[c][i] = r.se[c] * r.se[c];
    }
  }
  __syncthreads();
  const int tx = (int)(threadIdx.x % FILTER_TW), ty = (int)(threadIdx.x / FILTER_TW);
  const int x = x0 + tx, y = y0 + ty;
  if (x >= (int)width || y >= (int)rows) return;
  const int centre = (ty + PATCH_HALO) * PATCH_SW + tx + PATCH_HALO;
  float4 f = make_float4(s.m[0][centre], s.m[1][centre], s.m[2][centre], 0.0f);   // an uncounted centre passes through
  if (s.counted[centre] != 0u) {
    const pterr::ChunkRows ch = pterr::chunk_rows((uint32_t)y, band_rows, rows);
    const float k2 = kappa * kappa;
    f = filter_patch_taps(s, centre, y, (int)ch.first, (int)ch.last, (int)radius, (int)patch, k2);
  }
  if (gamma != 0) {
    f.x = __builtin_sqrtf(f.x);
    f.y = __builtin_sqrtf(f.y);
    f.z = __builtin_sqrtf(f.z);
  }
  out[(size_t)y * width + (size_t)x] = f;
}

extern "C" const void* pt_error_kernel(int id) {
  switch (id) {
    case PT_E_FILTER_PATCH: return ptcall::handle(ptsig::FilterPatch{}, pt_filter_patch_kernel);
    case PT_E_FILTER: return ptcall::handle(ptsig::Filter{}, pt_filter_kernel);
    case PT_E_FOLD: return ptcall::handle(ptsig::FoldError{}, pt_fold_error_kernel);
    case PT_E_RESOLVE: return ptcall::handle(ptsig::ResolveError{}, pt_resolve_error_kernel);
    case PT_E_TILES: return ptcall::handle(ptsig::ErrorTiles{}, pt_error_tiles_kernel);
    case PT_E_FOLD_TILES: return ptcall::handle(ptsig::FoldErrorTiles{}, pt_fold_error_tiles_kernel);
    case PT_E_PARTITION: return ptcall::handle(ptsig::PartitionOrder{}, pt_partition_order_kernel);
    default: return nullptr;
  }
}
