// pt_glare.hpp — THE GLARE (BLOOM) PYRAMID (include/ptrace.h pt_glare has the statement list), written once for
// the device and the host: pt_kernels_glare.hip runs the statements per thread over device memory (its down kernel through the
// LDS, which changes the order of nothing: the x pass's result is an fp32 either way), tests/glare_shim.cpp and
// tests/glare_main.cpp run ptglare::run over host arrays (the latter exactly sized, under the sanitizers).
// fp32, ONE IEEE operation per statement, nothing fused (-ffp-contract=off), `/` correctly rounded.  No HIP header needed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_tone.hpp"

#if defined(__HIPCC__)
#define PT_GLARE_HD __host__ __device__ __forceinline__
#else
#define PT_GLARE_HD inline
#endif

namespace ptglare {

using pttone::F4;

// the size of the next level: (n + 1) / 2, without the sum that could wrap
PT_GLARE_HD uint32_t half_up(uint32_t n) { return n / 2u + (n & 1u); }
// w_k (or h_k) of a frame of n_0 = n
PT_GLARE_HD uint32_t level_size(uint32_t n, uint32_t k) {
  for (uint32_t i = 0; i < k; i++) n = half_up(n);
  return n;
}
// the texels of levels 1 .. levels of a (w, h) frame; a frame without pixels has none
PT_GLARE_HD size_t pyramid_texels(uint32_t w, uint32_t h, uint32_t levels) {
  size_t n = 0;
  if (w == 0u || h == 0u) return n;
  for (uint32_t k = 0; k < levels; k++) {
    w = half_up(w);
    h = half_up(h);
    n += (size_t)w * h;
  }
  return n;
}

PT_GLARE_HD bool is_finite(float v) { return v - v == 0.0f; }

// PT_ERR_INVALID's cases of PtGlareOptions (a weight past `levels` is not read)
PT_GLARE_HD bool options_valid(const PtGlareOptions& o) {
  if (!is_finite(o.strength) || !(o.strength >= 0.0f) || !(o.strength <= 1.0f)) return false;
  if (!is_finite(o.threshold) || !(o.threshold >= 0.0f)) return false;
  if (o.levels < 1u || o.levels > (uint32_t)PT_GLARE_MAX_LEVELS) return false;
  for (uint32_t k = 0; k < o.levels; k++)
    if (!is_finite(o.weight[k]) || !(o.weight[k] >= 0.0f)) return false;
  return true;
}

// bright: the linear colour x of a source texel and the part b of it that spills
PT_GLARE_HD void bright(const F4 v, bool from_accum, float threshold, float x[3], float b[3]) {
  pttone::source_colour(v, from_accum, x);
  const float Y = pttone::luminance(x);
  const float z = Y - Y;
  if (!(z == 0.0f)) {  // NaN or infinite: one bad pixel must not veil the frame
    b[0] = b[1] = b[2] = 0.0f;
  } else if (threshold == 0.0f) {
    b[0] = x[0]; b[1] = x[1]; b[2] = x[2];
  } else {
    const float t = Y - threshold;
    if (!(t > 0.0f)) {
      b[0] = b[1] = b[2] = 0.0f;
    } else {
      const float m = t / Y;
      b[0] = x[0] * m; b[1] = x[1] * m; b[2] = x[2] * m;
    }
  }
}

// down, one axis: the taps at 2X-1, 2X, 2X+1, 2X+2 weighted 1 3 3 1 over 8
PT_GLARE_HD float down_tap(float t0, float t1, float t2, float t3) {
  const float o = t0 + t3;
  float i = t1 + t2;
  i = 3.0f * i;
  const float s = o + i;
  return s * 0.125f;
}

// up, one axis: the nearer texel p weighted 3, the other neighbour q weighted 1, over 4
PT_GLARE_HD float up_tap(float ap, float aq) {
  float t = 3.0f * ap;
  t = t + aq;
  return t * 0.25f;
}

// an index clamped to [0, n - 1] (n >= 1)
PT_GLARE_HD uint32_t clamp_index(int64_t i, uint32_t n) { return i < 0 ? 0u : (i > (int64_t)n - 1 ? n - 1u : (uint32_t)i); }

// up's two taps of X on an axis of N texels
PT_GLARE_HD void up_pair(uint32_t X, uint32_t N, uint32_t& p, uint32_t& q) {
  const int64_t p0 = (int64_t)(X >> 1);
  p = clamp_index(p0, N);
  q = clamp_index((X & 1u) ? p0 + 1 : p0 - 1, N);
}

// up(A) at (X, Y): A is a (W, H) level; first along x (on the two rows), then along y
PT_GLARE_HD void up_at(const F4* A, uint32_t W, uint32_t H, uint32_t X, uint32_t Y, float v[3]) {
  uint32_t px, qx, py, qy;
  up_pair(X, W, px, qx);
  up_pair(Y, H, py, qy);
  const F4 pp = A[(size_t)py * W + px], pq = A[(size_t)py * W + qx];
  const F4 qp = A[(size_t)qy * W + px], qq = A[(size_t)qy * W + qx];
  const float rp[3] = {up_tap(pp.x, pq.x), up_tap(pp.y, pq.y), up_tap(pp.z, pq.z)};
  const float rq[3] = {up_tap(qp.x, qq.x), up_tap(qp.y, qq.y), up_tap(qp.z, qq.z)};
  for (int c = 0; c < 3; c++) v[c] = up_tap(rp[c], rq[c]);
}

// gather: U_k at one texel from D_k there and, below the top level, up(U_{k+1})
PT_GLARE_HD F4 gather_at(const F4 d, float weight, const F4* above, uint32_t W, uint32_t H, uint32_t X, uint32_t Y) {
  float a[3] = {weight * d.x, weight * d.y, weight * d.z};
  if (above) {
    float u[3];
    up_at(above, W, H, X, Y, u);
    for (int c = 0; c < 3; c++) a[c] = a[c] + u[c];
  }
  const F4 r = {a[0], a[1], a[2], 0.0f};
  return r;
}

// composite: the output texel of source texel v at (X, Y); u1 is U_1, a (W, H) level
PT_GLARE_HD F4 composite_at(const F4 v, bool from_accum, float threshold, float strength, const F4* u1, uint32_t W, uint32_t H, uint32_t X,
                            uint32_t Y) {
  float x[3], b[3], G[3], o[3];
  bright(v, from_accum, threshold, x, b);
  up_at(u1, W, H, X, Y, G);
  for (int c = 0; c < 3; c++) {
    float d = G[c] - b[c];
    d = d * strength;
    o[c] = x[c] + d;
  }
  const F4 r = {o[0], o[1], o[2], 1.0f};
  return r;
}

// down at (X, Y) of a (sw, sh) image given by fetch(x, y, t[3]): the x pass on the four rows, then the y pass
template <class Fetch>
PT_GLARE_HD F4 down_at(const Fetch& fetch, uint32_t sw, uint32_t sh, uint32_t X, uint32_t Y) {
  float row[4][3];
  for (int r = 0; r < 4; r++) {
    const uint32_t sy = clamp_index(2 * (int64_t)Y - 1 + r, sh);
    float t[4][3];
    for (int k = 0; k < 4; k++) fetch(clamp_index(2 * (int64_t)X - 1 + k, sw), sy, t[k]);
    for (int c = 0; c < 3; c++) row[r][c] = down_tap(t[0][c], t[1][c], t[2][c], t[3][c]);
  }
  F4 v;
  v.x = down_tap(row[0][0], row[1][0], row[2][0], row[3][0]);
  v.y = down_tap(row[0][1], row[1][1], row[2][1], row[3][1]);
  v.z = down_tap(row[0][2], row[1][2], row[2][2], row[3][2]);
  v.w = 0.0f;
  return v;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole glare of a (w, h) image on the host.  src: w*h texels, accumulation texels when from_accum; out: w*h texels, may be
// src; scratch: pyramid_texels(w, h, o.levels) texels.  `o` has passed options_valid.  An image without pixels writes nothing.
inline void run(const F4* src, uint32_t w, uint32_t h, bool from_accum, const PtGlareOptions& o, F4* out, F4* scratch) {
  if (w == 0u || h == 0u) return;
  F4* level[PT_GLARE_MAX_LEVELS + 1] = {nullptr};
  uint32_t lw[PT_GLARE_MAX_LEVELS + 1], lh[PT_GLARE_MAX_LEVELS + 1];
  lw[0] = w; lh[0] = h;
  F4* next = scratch;
  for (uint32_t k = 1; k <= o.levels; k++) {
    lw[k] = half_up(lw[k - 1]); lh[k] = half_up(lh[k - 1]);
    level[k] = next;
    next += (size_t)lw[k] * lh[k];
  }
  const float threshold = o.threshold;
  for (uint32_t k = 1; k <= o.levels; k++) {
    const uint32_t sw = lw[k - 1], sh = lh[k - 1];
    for (uint32_t Y = 0; Y < lh[k]; Y++)
      for (uint32_t X = 0; X < lw[k]; X++) {
        F4& d = level[k][(size_t)Y * lw[k] + X];
        if (k == 1u) {
          d = down_at([&](uint32_t x, uint32_t y, float t[3]) { float c[3]; bright(src[(size_t)y * sw + x], from_accum, threshold, c, t); }, sw, sh, X, Y);
        } else {
          const F4* s = level[k - 1];
          d = down_at([&](uint32_t x, uint32_t y, float t[3]) { const F4 v = s[(size_t)y * sw + x]; t[0] = v.x; t[1] = v.y; t[2] = v.z; }, sw, sh, X, Y);
        }
      }
  }
  for (uint32_t k = o.levels; k >= 1u; k--) {  // U_k over D_k: a texel of U_k reads D_k only at itself
    const F4* above = k < o.levels ? level[k + 1] : nullptr;
    const uint32_t W = k < o.levels ? lw[k + 1] : 0u, H = k < o.levels ? lh[k + 1] : 0u;
    for (uint32_t Y = 0; Y < lh[k]; Y++)
      for (uint32_t X = 0; X < lw[k]; X++) {
        F4& d = level[k][(size_t)Y * lw[k] + X];
        d = gather_at(d, o.weight[k - 1], above, W, H, X, Y);
      }
  }
  for (uint32_t Y = 0; Y < h; Y++)
    for (uint32_t X = 0; X < w; X++) {
      const size_t i = (size_t)Y * w + X;
      out[i] = composite_at(src[i], from_accum, threshold, o.strength, level[1], lw[1], lh[1], X, Y);
    }
}
#endif

}  // namespace ptglare
