// pt_gather.hpp — GATHER QUERIES (pt_gather_irradiance, pt_bake_probes; include/ptrace.h has the contract, DESIGN.md §4.8n the
// argument), their arithmetic written once for the device and the host: the generator and the reduce kernel of
// pt_kernels_gather.hip run the statements per lane, pt_api.hip sizes its batches with the integer helpers,
// tests/gather_shim.cpp and tests/gather_main.cpp run the same functions on the CPU.  fp32, ONE IEEE operation per statement,
// every fused multiply-add an explicit __builtin_fmaf (-ffp-contract=off), `/` and sqrt correctly rounded.  No HIP header needed:
// sincos2pi's result is the caller's (pt_arith.hpp on the device, the oracle's on the host).
//
//   the set       D directions, D a multiple of 64 in [64, 4096]; for j < D:
//                 a = float(2 j + 1) / float(D)                                  (a_j = (2 j + 1) / D)
//                 u = float(((j * 0x9E3779B97F4A7C15) mod 2^64) >> 40) * 2^-24   (frac(j * 0.61803398875) cut to 24 bits, in
//                                                                                 integers: the constant is 2^64 / the golden ratio)
//                 (s, c) = sincos2pi(u), the caller's
//   sphere        y = 1 - a; r2 = fma(-y, y, 1); r = sqrt(r2); omega = (r * c, y, r * s)
//   hemisphere    h = a * 0.5; sh = sqrt(h); lx = sh * c; ly = sh * s; m = 1 - h; lz = sqrt(m)
//   normal        g = max(|n.x|, |n.y|, |n.z|); p = n / g per component (a tiny or a huge normal: |p| has a component of 1);
//                 d2 = fma(p.z, p.z, fma(p.y, p.y, p.x * p.x)); i = 1 / sqrt(d2); z = p * i
//   frame         pt_nee.hpp's (Duff et al.): sg = copysign(1, z.z); a = -1 / (sg + z.z); b = (z.x * z.y) * a;
//                 t = (fma(sg * (z.x * z.x), a, 1), sg * b, -sg * z.x); bt = (b, fma(z.y * z.y, a, sg), -z.y)
//                 omega = fma(z, lz, fma(bt, ly, t * lx)) per component
//   basis         Y0 = 0.282095; Y1 = 0.488603 * y; Y2 = 0.488603 * z; Y3 = 0.488603 * x; Y4 = 1.092548 * (x * y);
//                 Y5 = 1.092548 * (y * z); Y6 = 0.315392 * fma(3, z * z, -1); Y7 = 1.092548 * (x * z);
//                 Y8 = 0.546274 * fma(x, x, -(y * y))
//   lane          lane l < 64 of an item starts from 28 (probe) or 4 (irradiance) accumulators of +0 and takes the records
//                 j = l, l + 64, l + 128, ... in ascending order: mean.c = sum.c / samples;
//                 irradiance: acc[c] = acc[c] + mean.c;  probe: acc[3 k + c] = fma(mean.c, Y_k, acc[3 k + c]);
//                 the last accumulator: acc = acc + samples
//   tree          for o = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l xor o], every lane at once, per accumulator; the item's is v[0]
//   record        irradiance: e.c = v.c * (3.14159265 / float(D));  probe: sh[k][c] = v[3 k + c] * (12.5663706 / float(D));
//                 samples = the last accumulator
// The order of the sum is the lane's ascending j and then the tree: no launch shape, no batch boundary and no atomic enters it
// (a lane's partial sum is carried from batch to batch where an item straddles one: the same adds in the same order).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ptrace.h"

#if defined(__HIPCC__)
#define PT_GTH_HD __host__ __device__ __forceinline__
#else
#define PT_GTH_HD inline
#endif

namespace ptgather {

enum { kLanes = 64, kIrrAcc = 4, kProbeAcc = 28, kMaxAcc = 28, kMinDirections = 64, kMaxDirections = 4096 };
enum Kind { IRRADIANCE = 0, PROBE = 1 };

PT_GTH_HD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
PT_GTH_HD uint32_t bits_of(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, sizeof u);
  return u;
}
PT_GTH_HD bool finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }
PT_GTH_HD bool zero_bits(uint32_t u) { return (u & 0x7fffffffu) == 0u; }

// ---- what a call may ask ----------------------------------------------------------------------------------------------------
PT_GTH_HD bool directions_valid(uint32_t D) { return D >= kMinDirections && D <= kMaxDirections && D % kLanes == 0u; }
// the rays of a call, or 0 where n * D is beyond 2^32 - 1 (n > 0, D valid)
PT_GTH_HD uint64_t total_rays(uint32_t n, uint32_t D) {
  const uint64_t t = (uint64_t)n * D;
  return t <= 0xffffffffull ? t : 0ull;
}
// the items a batch of at most `batch` rays can touch: whole ones, and a straddling one at either end
PT_GTH_HD uint32_t items_per_batch(uint32_t batch) { return batch / kMinDirections + 2u; }
// The items of D rays each that the batch of rays [first, first + m) touches (m >= 1, first + m <= 2^32 - 1: the sum is taken in
// 64 bits all the same): `items` of them from item0 on, at most items_per_batch(m), of which [done0, done1) END in the batch —
// their records are written; the last one touched goes on into the next batch where done1 < item0 + items.
struct ItemSpan {
  uint32_t item0, items, done0, done1;
};
PT_GTH_HD ItemSpan item_span(uint32_t first, uint32_t m, uint32_t D) {
  const uint64_t end = (uint64_t)first + m;
  const uint32_t item0 = first / D;
  return {item0, (uint32_t)((end - 1u) / D) - item0 + 1u, item0, (uint32_t)(end / D)};
}

// THE VALIDITY PREDICATE of an item: a non-finite position component; for irradiance also a non-finite normal component or a
// normal of three zeros of either sign
PT_GTH_HD bool item_valid(const PtGatherPoint& p, int kind) {
  const bool pos = finite_bits(bits_of(p.position[0])) && finite_bits(bits_of(p.position[1])) && finite_bits(bits_of(p.position[2]));
  if (kind == PROBE) return pos;
  const uint32_t n0 = bits_of(p.normal[0]), n1 = bits_of(p.normal[1]), n2 = bits_of(p.normal[2]);
  return pos && finite_bits(n0) && finite_bits(n1) && finite_bits(n2) && !(zero_bits(n0) && zero_bits(n1) && zero_bits(n2));
}

// ---- the set ----------------------------------------------------------------------------------------------------------------
PT_GTH_HD float stratum(uint32_t j, uint32_t D) { return (float)(2u * j + 1u) / (float)D; }
PT_GTH_HD float turn(uint32_t j) { return (float)(uint32_t)(((uint64_t)j * 0x9E3779B97F4A7C15ull) >> 40) * (1.0f / 16777216.0f); }

// (s, c) = sincos2pi(turn(j))
PT_GTH_HD void sphere_direction(float a, float s, float c, float omega[3]) {
  const float y = 1.0f - a;
  const float r2 = fma_(-y, y, 1.0f);
  const float r = __builtin_sqrtf(r2);
  omega[0] = r * c;
  omega[1] = y;
  omega[2] = r * s;
}

// the unit normal of a valid irradiance item
PT_GTH_HD void unit_normal(const float n[3], float z[3]) {
  const float ax = __builtin_fabsf(n[0]), ay = __builtin_fabsf(n[1]), az = __builtin_fabsf(n[2]);
  const float gxy = ax > ay ? ax : ay;
  const float g = gxy > az ? gxy : az;
  const float px = n[0] / g, py = n[1] / g, pz = n[2] / g;
  const float d2 = fma_(pz, pz, fma_(py, py, px * px));
  const float i = 1.0f / __builtin_sqrtf(d2);
  z[0] = px * i; z[1] = py * i; z[2] = pz * i;
}

PT_GTH_HD void hemisphere_direction(const float z[3], float a, float s, float c, float omega[3]) {
  const float h = a * 0.5f;
  const float sh = __builtin_sqrtf(h);
  const float lx = sh * c, ly = sh * s;
  const float m = 1.0f - h;
  const float lz = __builtin_sqrtf(m);
  const float zx = z[0], zy = z[1], zz = z[2];
  const float sg = __builtin_copysignf(1.0f, zz);
  const float q = -1.0f / (sg + zz);
  const float b = (zx * zy) * q;
  const float tx = fma_(sg * (zx * zx), q, 1.0f), ty = sg * b, tz = -sg * zx;
  const float bx = b, by = fma_(zy * zy, q, sg), bz = -zy;
  omega[0] = fma_(zx, lz, fma_(bx, ly, tx * lx));
  omega[1] = fma_(zy, lz, fma_(by, ly, ty * lx));
  omega[2] = fma_(zz, lz, fma_(bz, ly, tz * lx));
}

// Ray j of an item: {position, omega}; of an invalid item: the null ray (an invalid ray of pt_query_radiance: nothing is traced)
PT_GTH_HD PtRay ray_of(const PtGatherPoint& p, int kind, uint32_t j, uint32_t D, float s, float c) {
  PtRay r;
  r._pad0 = 0.0f; r._pad1 = 0.0f;
  if (!item_valid(p, kind)) {
    r.origin[0] = r.origin[1] = r.origin[2] = 0.0f;
    r.direction[0] = r.direction[1] = r.direction[2] = 0.0f;
    return r;
  }
  r.origin[0] = p.position[0]; r.origin[1] = p.position[1]; r.origin[2] = p.position[2];
  const float a = stratum(j, D);
  if (kind == PROBE) {
    sphere_direction(a, s, c, r.direction);
  } else {
    float z[3];
    unit_normal(p.normal, z);
    hemisphere_direction(z, a, s, c, r.direction);
  }
  return r;
}

// ---- the basis --------------------------------------------------------------------------------------------------------------
PT_GTH_HD void sh_basis(const float w[3], float Y[9]) {
  const float x = w[0], y = w[1], z = w[2];
  Y[0] = 0.282095f;
  Y[1] = 0.488603f * y;
  Y[2] = 0.488603f * z;
  Y[3] = 0.488603f * x;
  Y[4] = 1.092548f * (x * y);
  Y[5] = 1.092548f * (y * z);
  Y[6] = 0.315392f * fma_(3.0f, z * z, -1.0f);
  Y[7] = 1.092548f * (x * z);
  Y[8] = 0.546274f * fma_(x, x, -(y * y));
}

// ---- the reduction ----------------------------------------------------------------------------------------------------------
PT_GTH_HD void lane_add_irradiance(float acc[kIrrAcc], const PtRayRadiance& r) {
  acc[0] = acc[0] + r.sum[0] / r.samples;
  acc[1] = acc[1] + r.sum[1] / r.samples;
  acc[2] = acc[2] + r.sum[2] / r.samples;
  acc[3] = acc[3] + r.samples;
}
PT_GTH_HD void lane_add_probe(float acc[kProbeAcc], const PtRayRadiance& r, const float Y[9]) {
  const float m0 = r.sum[0] / r.samples, m1 = r.sum[1] / r.samples, m2 = r.sum[2] / r.samples;
  for (int k = 0; k < 9; k++) {
    acc[3 * k] = fma_(m0, Y[k], acc[3 * k]);
    acc[3 * k + 1] = fma_(m1, Y[k], acc[3 * k + 1]);
    acc[3 * k + 2] = fma_(m2, Y[k], acc[3 * k + 2]);
  }
  acc[27] = acc[27] + r.samples;
}
PT_GTH_HD float irradiance_scale(uint32_t D) { return 3.14159265f / (float)D; }
PT_GTH_HD float probe_scale(uint32_t D) { return 12.5663706f / (float)D; }

PT_GTH_HD PtIrradiance irradiance_record(const float v[kIrrAcc], uint32_t D) {
  const float k = irradiance_scale(D);
  PtIrradiance e;
  e.e[0] = v[0] * k; e.e[1] = v[1] * k; e.e[2] = v[2] * k;
  e.samples = v[3];
  return e;
}
PT_GTH_HD PtProbeSH probe_record(const float v[kProbeAcc], uint32_t D) {
  const float k = probe_scale(D);
  PtProbeSH p;
  for (int i = 0; i < 9; i++) {
    p.sh[i][0] = v[3 * i] * k; p.sh[i][1] = v[3 * i + 1] * k; p.sh[i][2] = v[3 * i + 2] * k;
  }
  p.samples = v[27];
  return p;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host's whole item, for the tests: rec[0 .. D) are the item's records, sc[2 j], sc[2 j + 1] = sincos2pi(turn(j)); out
// holds 4 (irradiance: the PtIrradiance) or 28 floats (probe: the PtProbeSH).  The tree is the kernel's butterfly, lane by lane.
inline void reduce_item(int kind, const PtRayRadiance* rec, uint32_t D, const float* sc, float* out) {
  const int n_acc = kind == PROBE ? kProbeAcc : kIrrAcc;
  float lanes[kLanes][kMaxAcc];
  for (uint32_t l = 0; l < kLanes; l++) {
    for (int a = 0; a < n_acc; a++) lanes[l][a] = 0.0f;
    for (uint32_t j = l; j < D; j += kLanes) {
      if (kind == PROBE) {
        float w[3], Y[9];
        sphere_direction(stratum(j, D), sc[2 * j], sc[2 * j + 1], w);
        sh_basis(w, Y);
        lane_add_probe(lanes[l], rec[j], Y);
      } else {
        lane_add_irradiance(lanes[l], rec[j]);
      }
    }
  }
  for (uint32_t o = kLanes / 2; o >= 1; o /= 2) {
    float next[kLanes][kMaxAcc];
    for (uint32_t l = 0; l < kLanes; l++)
      for (int a = 0; a < n_acc; a++) next[l][a] = lanes[l][a] + lanes[l ^ o][a];
    for (uint32_t l = 0; l < kLanes; l++)
      for (int a = 0; a < n_acc; a++) lanes[l][a] = next[l][a];
  }
  if (kind == PROBE) {
    const PtProbeSH p = probe_record(lanes[0], D);
    __builtin_memcpy(out, &p, sizeof p);
  } else {
    const PtIrradiance e = irradiance_record(lanes[0], D);
    __builtin_memcpy(out, &e, sizeof e);
  }
}
#endif

}  // namespace ptgather
