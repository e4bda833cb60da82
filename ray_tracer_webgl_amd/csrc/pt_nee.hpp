// pt_nee.hpp — NEXT-EVENT ESTIMATION (PT_OPT_NEXT_EVENT; include/ptrace.h has the contract, DESIGN.md §4.8m the argument), its
// arithmetic written once for the device and the host: pt_shade.hpp runs the statements per lane in the _nee builds
// (pt_kernels_nee.hip), pt_api.hip makes the light table with lights_of, tests/nee_shim.cpp and tests/nee_main.cpp run the same
// functions on the CPU.  fp32, ONE IEEE operation per statement, every fused multiply-add an explicit __builtin_fmaf
// (-ffp-contract=off), `/` and sqrt correctly rounded.  No HIP header needed.
//
//   lights      the spheres of the list with type == PT_EMISSIVE, a finite centre, a finite non-zero radius and a finite albedo, in
//               list order; per light {centre, r * r, albedo, list index}: 32 bytes
//   choose      k = min((int)(u0 * L), L - 1)                                       (u0 can be 1: hash3 rounds 2^31 - 1 up)
//   reach       w = c_k - x; d2 = fma(w.z, w.z, fma(w.y, w.y, w.x * w.x)); P(x, k) := d2 > r2
//   cone        q = r2 / d2; cosmax = sqrt(max(0, 1 - q)); om = 1 - cosmax; cos_t = 1 - u1 * om;
//               sin_t = sqrt(max(0, fma(-cos_t, cos_t, 1)))                           (s, c) = sincos2pi(u2), the caller's
//   frame       i = 1 / sqrt(d2); z = w * i; sg = copysign(1, z.z); a = -1 / (sg + z.z); b = (z.x * z.y) * a;
//               t = (fma(sg * (z.x * z.x), a, 1), sg * b, -sg * z.x); bt = (b, fma(z.y * z.y, a, sg), -z.y)
//               branch-free and finite for every unit z: sg + z.z has magnitude >= 1, (0, 0, -1) gives a = 1 / 2
//   direction   sx = sin_t * c; sy = sin_t * s; omega = fma(z, cos_t, fma(bt, sy, t * sx)) per component
//   weight      cos_s = dot(n, omega); wgt = ((float)L * (2 * om)) * cos_s           dot as fma(n.z, o.z, fma(n.y, o.y, n.x * o.x))
//   add         sum.c = sum.c + (throughput.c * albedo_k.c) * wgt                    when the shadow ray's closest hit is light k
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_NEE_HD __host__ __device__ __forceinline__
#else
#define PT_NEE_HD inline
#endif

namespace ptnee {

struct Light {
  float c[3];
  float r2;
  float albedo[3];
  int32_t index;  // the light's place in the sphere list
};
static_assert(sizeof(Light) == 32, "a light is two 16-byte loads");

enum { TYPE_EMISSIVE = 3 };  // PT_EMISSIVE (include/ptrace.h)

PT_NEE_HD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
PT_NEE_HD bool is_finite(float v) { return v - v == 0.0f; }

// Is the sphere a light?  (A sphere a ray HIT has a finite centre and a finite r * r already; pt_shade.hpp asks the rest.)
PT_NEE_HD bool is_light(int32_t type, const float centre[3], float radius, const float albedo[3]) {
  return type == TYPE_EMISSIVE && is_finite(centre[0]) && is_finite(centre[1]) && is_finite(centre[2]) && is_finite(radius) && radius != 0.0f &&
         is_finite(albedo[0]) && is_finite(albedo[1]) && is_finite(albedo[2]);
}

// The table of a list: geom = n x {cx, cy, cz, r * r} (the kernels' own record: the same r * r bits), mat = n shading records
// with .albedo[3], .type and .radius (PtMatRec).  Writes at most n lights to out (NULL: count only) and returns L.
template <class Mat>
inline uint32_t lights_of(const float* geom, const Mat* mat, uint32_t n, Light* out) {
  uint32_t L = 0;
  for (uint32_t i = 0; i < n; i++) {
    const float* a = mat[i].albedo;
    if (!is_light(mat[i].type, geom + 4 * (size_t)i, mat[i].radius, a)) continue;
    if (out) {
      Light& l = out[L];
      l.c[0] = geom[4 * (size_t)i]; l.c[1] = geom[4 * (size_t)i + 1]; l.c[2] = geom[4 * (size_t)i + 2];
      l.r2 = geom[4 * (size_t)i + 3];
      l.albedo[0] = a[0]; l.albedo[1] = a[1]; l.albedo[2] = a[2];
      l.index = (int32_t)i;
    }
    L++;
  }
  return L;
}

PT_NEE_HD int choose(float u0, int L) {
  const int k = (int)(u0 * (float)L);
  return k < L - 1 ? k : L - 1;
}

// w = c - x, d2 = |w|^2; returns P(x, light): can the light be sampled from x?
PT_NEE_HD bool reach(const float x[3], const float c[3], float r2, float w[3], float& d2) {
  w[0] = c[0] - x[0]; w[1] = c[1] - x[1]; w[2] = c[2] - x[2];
  d2 = fma_(w[2], w[2], fma_(w[1], w[1], w[0] * w[0]));
  return d2 > r2;
}

// One cone sample of a light that P holds for: the direction omega, and om = 1 - cosmax (the cone's solid angle is 2 pi om).
// (s, c) = sincos2pi(u2).
PT_NEE_HD void sample(const float w[3], float d2, float r2, float u1, float s, float c, float omega[3], float& om) {
  const float q = r2 / d2;
  const float m = 1.0f - q;
  const float cosmax = __builtin_sqrtf(m > 0.0f ? m : 0.0f);
  om = 1.0f - cosmax;
  const float cos_t = 1.0f - u1 * om;
  const float s2 = fma_(-cos_t, cos_t, 1.0f);
  const float sin_t = __builtin_sqrtf(s2 > 0.0f ? s2 : 0.0f);
  const float i = 1.0f / __builtin_sqrtf(d2);
  const float zx = w[0] * i, zy = w[1] * i, zz = w[2] * i;
  const float sg = __builtin_copysignf(1.0f, zz);
  const float a = -1.0f / (sg + zz);
  const float b = (zx * zy) * a;
  const float tx = fma_(sg * (zx * zx), a, 1.0f), ty = sg * b, tz = -sg * zx;
  const float bx = b, by = fma_(zy * zy, a, sg), bz = -zy;
  const float sx = sin_t * c, sy = sin_t * s;
  omega[0] = fma_(zx, cos_t, fma_(bx, sy, tx * sx));
  omega[1] = fma_(zy, cos_t, fma_(by, sy, ty * sx));
  omega[2] = fma_(zz, cos_t, fma_(bz, sy, tz * sx));
}

PT_NEE_HD float cos_at(const float n[3], const float omega[3]) { return fma_(n[2], omega[2], fma_(n[1], omega[1], n[0] * omega[0])); }
PT_NEE_HD float weight(int L, float om, float cos_s) { return ((float)L * (2.0f * om)) * cos_s; }
PT_NEE_HD void add(float sum[3], const float throughput[3], const float albedo[3], float wgt) {
  sum[0] = sum[0] + (throughput[0] * albedo[0]) * wgt;
  sum[1] = sum[1] + (throughput[1] * albedo[1]) * wgt;
  sum[2] = sum[2] + (throughput[2] * albedo[2]) * wgt;
}

}  // namespace ptnee
