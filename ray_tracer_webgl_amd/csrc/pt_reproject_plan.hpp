// pt_reproject_plan.hpp — the host constants of temporal reprojection (include/ptrace.h pt_reproject_constants; DESIGN.md
// §4.8g): what pt_reproject's kernel needs of the HISTORY camera to project a world point into its image and to measure a
// distance in its pixel footprints.  Pure host arithmetic, no HIP: pt_api.hip calls it, tests/reproject_plan_shim.cpp puts it
// in front of ctypes, tests/reproject_main.cpp runs it under the sanitizers.
//
// Computed in double from the float fields of the history view's uniforms, one IEEE operation per statement (the build has
// -ffp-contract=off), every result narrowed to float ONCE:
//     O = camera_origin; Hh = horizontal; V = vertical; L = lower_left_corner
//     e = L - O;  n = Hh x V;  N = n / (e.n)
//     A = (V x n) / (Hh.(V x n));  B = (n x Hh) / (V.(n x Hh))
//     ea = e.A;  eb = e.B                               (A and B as doubles, before they are narrowed)
//     k = tolerance_px^2 * (Hh.Hh) / width^2
//     out16 = {O.xyz, N.xyz, A.xyz, B.xyz, ea, eb, k, 0}
// with  a x b = {a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x}  and  a.b = (a.x*b.x + a.y*b.y) + a.z*b.z.
// A pixel (s, t) of that view looks along d = e + s Hh + t V; for a point P = O + lam d:  N.(P - O) = lam,
// A.(P - O) / lam = ea + s,  B.(P - O) / lam = eb + t.  The lens does not enter: the feature planes are pinhole.
#pragma once
#include <cmath>
#include <cstdint>

namespace ptrep {

enum { K_O = 0, K_N = 3, K_A = 6, K_B = 9, K_EA = 12, K_EB = 13, K_K = 14, K_COUNT = 16 };

inline void cross3(const double a[3], const double b[3], double out[3]) {
  const double yz = a[1] * b[2], zy = a[2] * b[1];
  const double zx = a[2] * b[0], xz = a[0] * b[2];
  const double xy = a[0] * b[1], yx = a[1] * b[0];
  out[0] = yz - zy;
  out[1] = zx - xz;
  out[2] = xy - yx;
}
inline double dot3(const double a[3], const double b[3]) {
  const double x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
  const double xy = x + y;
  return xy + z;
}

// false (out16 untouched) when e.n or either denominator is 0, or when any result is not finite
inline bool constants(const float origin[3], const float horizontal[3], const float vertical[3], const float lower_left_corner[3],
                      uint32_t width, float tolerance_px, float out16[K_COUNT]) {
  double O[3], Hh[3], V[3], e[3];
  for (int c = 0; c < 3; c++) {
    O[c] = (double)origin[c];
    Hh[c] = (double)horizontal[c];
    V[c] = (double)vertical[c];
    e[c] = (double)lower_left_corner[c] - O[c];
  }
  double n[3], vn[3], nh[3];
  cross3(Hh, V, n);
  const double en = dot3(e, n);
  cross3(V, n, vn);
  const double da = dot3(Hh, vn);
  cross3(n, Hh, nh);
  const double db = dot3(V, nh);
  if (en == 0.0 || da == 0.0 || db == 0.0) return false;
  double N[3], A[3], B[3];
  for (int c = 0; c < 3; c++) {
    N[c] = n[c] / en;
    A[c] = vn[c] / da;
    B[c] = nh[c] / db;
  }
  const double ea = dot3(e, A), eb = dot3(e, B);
  const double tol = (double)tolerance_px, w = (double)width;
  const double t2 = tol * tol, hh = dot3(Hh, Hh), w2 = w * w;
  const double th = t2 * hh;
  const double k = th / w2;
  float out[K_COUNT];
  for (int c = 0; c < 3; c++) {
    out[K_O + c] = origin[c];
    out[K_N + c] = (float)N[c];
    out[K_A + c] = (float)A[c];
    out[K_B + c] = (float)B[c];
  }
  out[K_EA] = (float)ea;
  out[K_EB] = (float)eb;
  out[K_K] = (float)k;
  out[15] = 0.0f;
  for (int i = 0; i < K_COUNT; i++)
    if (!std::isfinite(out[i])) return false;
  for (int i = 0; i < K_COUNT; i++) out16[i] = out[i];
  return true;
}

}  // namespace ptrep
