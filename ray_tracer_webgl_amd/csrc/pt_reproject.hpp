// pt_reproject.hpp — ONE PIXEL of temporal reprojection (include/ptrace.h pt_reproject has the statement list),
// written once for the device and the host: pt_kernels_reproject.hip runs it per thread over device memory,
// tests/reproject_plan_shim.cpp and tests/reproject_main.cpp run it over host arrays (the latter bounds-checked, under the
// sanitizers), so the index guard below is proven on the CPU before any GPU sees hostile operands.  The same pixel with the error
// estimate's state (pt_reproject_estimate, §4.8h) follows it: reproject_pixel_estimate, for pt_reproject_estimate_kernel,
// tests/reproject_estimate_shim.cpp and tests/reproject_estimate_main.cpp.
// fp32, ONE IEEE operation per statement, nothing fused (-ffp-contract=off), `/` correctly rounded.  No HIP header needed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_REP_HD __host__ __device__ __forceinline__
#else
#define PT_REP_HD inline
#endif

namespace ptrep {

struct alignas(16) F4 { float x, y, z, w; };
struct alignas(16) I4 { int32_t x, y, z, w; };

// the history view's constants (pt_reproject_plan.hpp, out16 in its order) and the caps of the call
struct Consts {
  float O[3], N[3], A[3], B[3];
  float ea, eb, k, cap_diffuse, cap_other;
};
// the frame both views share: the image, this context's local rows and its row partition (band_count <= 1: every row)
struct Frame {
  uint32_t width, height, rows;
  uint32_t band_rows, band_index, band_count;
};

// the inverse of pt_band_row: is image row y one of this context's, and which local row?
PT_REP_HD bool local_row_of(const Frame& f, uint32_t y, uint32_t* lq) {
  if (f.band_count <= 1u || f.band_rows == 0u) { *lq = y; return y < f.rows; }
  const uint32_t chunk = y / f.band_rows;
  if (chunk % f.band_count != f.band_index) return false;
  *lq = (chunk / f.band_count) * f.band_rows + y % f.band_rows;
  return *lq < f.rows;  // (always, for y < height: the guard of the gather's index)
}

PT_REP_HD float dot_n(const float w[3], const float n[3]) {
  const float x = w[0] * n[0], y = w[1] * n[1], z = w[2] * n[2];
  const float xy = x + y;
  return xy + z;
}

// `Mem`: hids(i), hpnt(i), acc(i) -> the history ids, the history point and the accumulation of local texel i < rows * width.
// ids, Pn: the CURRENT planes' texels of the pixel.  Returns out = {col.rgb * nq, nq}, all +0 when nothing is kept.
template <class Mem>
PT_REP_HD F4 reproject_pixel(const I4 ids, const F4 Pn, const Consts& K, const Frame& f, const Mem& mem) {
  const F4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  if (ids.x < 0) return zero;                               // a miss: sky needs no history
  const float P[3] = {Pn.x, Pn.y, Pn.z};
  float w[3];
  for (int c = 0; c < 3; c++) w[c] = P[c] - K.O[c];
  const float lam = dot_n(w, K.N);
  if (!(lam > 0.0f)) return zero;                           // behind the history camera (or NaN)
  const float ws = dot_n(w, K.A), wt = dot_n(w, K.B);
  float s = ws / lam;
  s = s - K.ea;
  float t = wt / lam;
  t = t - K.eb;
  const float wf = (float)f.width, hf = (float)f.height;
  float fx = s * wf;
  fx = fx - 0.5f;
  float fy = t * hf;
  fy = fy - 0.5f;
  if (!(fx > -1.0f && fx < wf && fy > -1.0f && fy < hf)) return zero;   // outside the history frame (NaN: outside)
  const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
  const float ax = fx - x0f, ay = fy - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;                   // in [-1, width - 1] x [-1, height - 1]: only now an integer
  const float lam2 = lam * lam;
  const float rhs = K.k * lam2;
  const float cap = ids.z == 0 /* PT_DIFFUSE */ ? K.cap_diffuse : K.cap_other;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  float cnt = 0.0f, wsum = 0.0f;
  for (int dy = 0; dy < 2; dy++) {
    for (int dx = 0; dx < 2; dx++) {
      const int qx = x0 + dx, qy = y0 + dy;
      if (qx < 0 || qx >= (int)f.width || qy < 0 || qy >= (int)f.height) continue;
      uint32_t lq;
      if (!local_row_of(f, (uint32_t)qy, &lq)) continue;    // a row another band owns
      const size_t q = (size_t)lq * f.width + (size_t)qx;
      const I4 hid = mem.hids(q);
      if (!(hid.x == ids.x && hid.w == ids.w)) continue;    // another sphere, or its other side
      const F4 hp = mem.hpnt(q);
      const float d[3] = {hp.x - P[0], hp.y - P[1], hp.z - P[2]};
      const float d2 = dot_n(d, d);
      if (!(d2 <= rhs)) continue;                           // farther than tolerance_px footprints at that depth (NaN: skipped)
      const F4 a = mem.acc(q);
      if (!(a.w > 0.0f)) continue;
      const float wx = dx ? ax : 1.0f - ax, wy = dy ? ay : 1.0f - ay;
      const float g = wx * wy;
      if (!(g > 0.0f)) continue;
      const float m[3] = {a.x / a.w, a.y / a.w, a.z / a.w};
      for (int c = 0; c < 3; c++) {
        const float gm = g * m[c];
        sum[c] = sum[c] + gm;
      }
      const float ga = g * a.w;
      cnt = cnt + ga;
      wsum = wsum + g;
    }
  }
  if (!(wsum > 0.0f)) return zero;
  float nq = cnt / wsum;
  nq = __builtin_floorf(nq);
  if (nq > cap) nq = cap;
  if (!(nq >= 1.0f)) return zero;
  const float col[3] = {sum[0] / wsum, sum[1] / wsum, sum[2] / wsum};
  const F4 out = {col[0] * nq, col[1] * nq, col[2] * nq, nq};
  return out;
}

// ---- the same pixel WITH the error estimate's state (include/ptrace.h pt_reproject_estimate) -----------------
// the estimate's host constants: S = the samples_per_pixel of the folded passes, the caps in passes
struct EstConsts {
  float Sf, S2, capP_diffuse, capP_other;
};
// on the host, once per call: S > 0, the caps as the call takes them (whole numbers in [0, 2^24))
PT_REP_HD EstConsts est_consts(int S, float cap_diffuse, float cap_other) {
  const float Sf = (float)S;
  const float S2 = Sf * Sf;
  const float cd = cap_diffuse / Sf, co = cap_other / Sf;
  const EstConsts E = {Sf, S2, __builtin_floorf(cd), __builtin_floorf(co)};
  return E;
}
// what one pixel leaves: the accumulation's texel — reproject_pixel's bits — and the estimate's two, A' = {mean', nE}, B' = {M2', kE}
struct Carried {
  F4 acc, A, B;
};

// `Mem` as above, and errA(i), errB(i) -> the estimate's state of local texel i.  The tap tests both gathers share (range, row,
// ids, distance, weight) are evaluated once; `a.w > 0` gates the accumulation's sums only, `Aq.w >= 2 && Bq.w > 0` the estimate's.
template <class Mem>
PT_REP_HD Carried reproject_pixel_estimate(const I4 ids, const F4 Pn, const Consts& K, const EstConsts& E, const Frame& f,
                                           const Mem& mem) {
  const F4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  Carried r = {zero, zero, zero};
  if (ids.x < 0) return r;
  const float P[3] = {Pn.x, Pn.y, Pn.z};
  float w[3];
  for (int c = 0; c < 3; c++) w[c] = P[c] - K.O[c];
  const float lam = dot_n(w, K.N);
  if (!(lam > 0.0f)) return r;
  const float ws = dot_n(w, K.A), wt = dot_n(w, K.B);
  float s = ws / lam;
  s = s - K.ea;
  float t = wt / lam;
  t = t - K.eb;
  const float wf = (float)f.width, hf = (float)f.height;
  float fx = s * wf;
  fx = fx - 0.5f;
  float fy = t * hf;
  fy = fy - 0.5f;
  if (!(fx > -1.0f && fx < wf && fy > -1.0f && fy < hf)) return r;
  const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
  const float ax = fx - x0f, ay = fy - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float lam2 = lam * lam;
  const float rhs = K.k * lam2;
  const bool diffuse = ids.z == 0 /* PT_DIFFUSE */;
  const float cap = diffuse ? K.cap_diffuse : K.cap_other;
  const float capP = diffuse ? E.capP_diffuse : E.capP_other;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  float cnt = 0.0f, wsum = 0.0f;
  float mu[3] = {0.0f, 0.0f, 0.0f}, W[3] = {0.0f, 0.0f, 0.0f};
  float cntE = 0.0f, wsumE = 0.0f;
  for (int dy = 0; dy < 2; dy++) {
    for (int dx = 0; dx < 2; dx++) {
      const int qx = x0 + dx, qy = y0 + dy;
      if (qx < 0 || qx >= (int)f.width || qy < 0 || qy >= (int)f.height) continue;
      uint32_t lq;
      if (!local_row_of(f, (uint32_t)qy, &lq)) continue;
      const size_t q = (size_t)lq * f.width + (size_t)qx;
      const I4 hid = mem.hids(q);
      if (!(hid.x == ids.x && hid.w == ids.w)) continue;
      const F4 hp = mem.hpnt(q);
      const float d[3] = {hp.x - P[0], hp.y - P[1], hp.z - P[2]};
      const float d2 = dot_n(d, d);
      if (!(d2 <= rhs)) continue;
      const float wx = dx ? ax : 1.0f - ax, wy = dy ? ay : 1.0f - ay;
      const float g = wx * wy;
      if (!(g > 0.0f)) continue;
      const F4 a = mem.acc(q);
      if (a.w > 0.0f) {                                      // the accumulation's sums: reproject_pixel's statements
        const float m[3] = {a.x / a.w, a.y / a.w, a.z / a.w};
        for (int c = 0; c < 3; c++) {
          const float gm = g * m[c];
          sum[c] = sum[c] + gm;
        }
        const float ga = g * a.w;
        cnt = cnt + ga;
        wsum = wsum + g;
      }
      const F4 Aq = mem.errA(q), Bq = mem.errB(q);
      if (Aq.w >= 2.0f && Bq.w > 0.0f) {                     // the estimate's sums: a texel whose read-out is "known" (NaN: skipped)
        const float qq = Aq.w / Bq.w;
        const float qq2 = qq * qq;
        const float n1 = Aq.w - 1.0f;
        const float Am[3] = {Aq.x, Aq.y, Aq.z}, Bm[3] = {Bq.x, Bq.y, Bq.z};
        for (int c = 0; c < 3; c++) {
          const float m = Am[c] * qq;
          const float gm = g * m;
          mu[c] = mu[c] + gm;
          float pv = Bm[c] / n1;
          pv = pv * qq2;
          const float gp = g * pv;
          W[c] = W[c] + gp;
        }
        const float gn = g * Aq.w;
        cntE = cntE + gn;
        wsumE = wsumE + g;
      }
    }
  }
  if (wsum > 0.0f) {
    float nq = cnt / wsum;
    nq = __builtin_floorf(nq);
    if (nq > cap) nq = cap;
    if (nq >= 1.0f) {
      const float col[3] = {sum[0] / wsum, sum[1] / wsum, sum[2] / wsum};
      const F4 out = {col[0] * nq, col[1] * nq, col[2] * nq, nq};
      r.acc = out;
    }
  }
  if (wsumE > 0.0f) {
    float nE = cntE / wsumE;
    nE = __builtin_floorf(nE);
    if (nE > capP) nE = capP;
    if (nE >= 2.0f) {
      const float n1 = nE - 1.0f;
      const float kE = nE * E.Sf;
      float mean[3], M2[3];
      for (int c = 0; c < 3; c++) {
        const float a = mu[c] / wsumE;
        mean[c] = a * E.Sf;
        float b = W[c] / wsumE;
        b = b * n1;
        M2[c] = b * E.S2;
      }
      const F4 An = {mean[0], mean[1], mean[2], nE}, Bn = {M2[0], M2[1], M2[2], kE};
      r.A = An;
      r.B = Bn;
    }
  }
  return r;
}

}  // namespace ptrep
