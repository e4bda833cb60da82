// pt_probe.hpp — PROBE LATTICES (pt_bake_lattice, pt_shade_probes; include/ptrace.h has the contract, DESIGN.md §4.8p the
// argument), their arithmetic written once for the device and the host: the generator and the shading kernel of
// pt_kernels_probe.hip run the statements per lane, pt_api.hip asks the checks, tests/probe_shim.cpp and tests/probe_main.cpp
// run the same functions on the CPU.  fp32, ONE IEEE operation per statement, every fused multiply-add an explicit
// __builtin_fmaf (-ffp-contract=off), `/` and sqrt correctly rounded.  dot, the unit vectors and the basis Y_j are pt_gather.hpp's.
//
//   node          i = (iz * ny + iy) * nx + ix;  position.c = fma(float(i_c), step.c, origin.c)
//   buried        (PT_LATTICE_SKIP_BURIED) for some sphere with type != PT_GLASS: w = position - centre;
//                 d2 = fma(w.z, w.z, fma(w.y, w.y, w.x * w.x));  d2 < r * r  (strict; r * r the bits the kernels intersect; a NaN
//                 centre never buries) — the node's position becomes NaN: an invalid item of pt_bake_probes
//   pixel         miss (ids.x < 0) and PT_EMISSIVE: {albedo plane rgb, 1};  a type outside the four: {0, 0, 0, 1};  otherwise
//   look-up       q.c = fma(normal_bias, n.c, hp.c);  g.c = (q.c - origin.c) / step.c;  i.c = clamp(int(floor(g.c)), 0, n_c - 2)
//                 (a NaN g takes cell 0);  t.c = g.c - float(i.c);  f.c = min(max(t.c, 0), 1)  (max(t, 0) is t > 0 ? t : 0,
//                 min(t, 1) is t < 1 ? t : 1: a NaN gives 0)
//   direction     DIFFUSE: omega = n, b = (3.14159265f, 2.09439510f x3, 0.785398163f x5)  (pi, 2 pi / 3, pi / 4)
//                 METAL:   v.c = hp.c - camera_origin.c;  d = dot(v, n);  k = 2 * d;  m.c = k * n.c;  r.c = v.c - m.c;
//                          omega = unit(r), b = 1                      (the mirror direction: fuzz does not enter)
//                 GLASS:   omega = unit(v), b = 1                      (straight through: refraction does not enter)
//                 B_j = b_j * Y_j(omega)
//   corners       k = 0 .. 7 ascending, bit 0 = x, bit 1 = y, bit 2 = z:  wx = bit ? f.x : 1 - f.x (y, z likewise);
//                 w_k = (wx * wy) * wz;  kept iff w_k > 0, under PT_PROBE_HALFSPACE e.c = pos_k.c - hp.c and dot(e, n) > 0, and
//                 the record's samples > 0;  for a kept corner
//                 E_k.c = fma(B_8, sh[8].c, ... fma(B_0, sh[0].c, +0)) (j ascending);  W = W + w_k;  S.c = fma(w_k, E_k.c, S.c)
//   result        W > 0:  v.c = max(S.c / W, 0);  DIFFUSE out.c = albedo.c * (v.c * 0.318309886f);  METAL out.c = albedo.c * v.c;
//                 GLASS out.c = v.c;  alpha 1.     W == 0: {0, 0, 0, 0} — alpha 0 is the mark of "no usable probe"
// dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), the order of pt_gather.hpp's d2.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ptrace.h"
#include "pt_gather.hpp"

#if defined(__HIPCC__)
#define PT_PRB_HD __host__ __device__ __forceinline__
#else
#define PT_PRB_HD inline
#endif

namespace ptprobe {

enum { kMinNodes = 2, kMaxNodes = 256, kMaxTotal = 1 << 20, kRecordFloats = 28 };

PT_PRB_HD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
PT_PRB_HD float dot(const float a[3], const float b[3]) { return fma_(a[2], b[2], fma_(a[1], b[1], a[0] * b[0])); }
PT_PRB_HD float quiet_nan() {
  const uint32_t u = 0x7fc00000u;
  float f;
  __builtin_memcpy(&f, &u, sizeof f);
  return f;
}

// ---- what a call may ask ----------------------------------------------------------------------------------------------------
// nullptr for a lattice the calls take, else what is wrong with it (the words of PT_ERR_INVALID)
PT_PRB_HD const char* lattice_error(const PtProbeLattice& L) {
  if (L.nx < kMinNodes || L.nx > kMaxNodes || L.ny < kMinNodes || L.ny > kMaxNodes || L.nz < kMinNodes || L.nz > kMaxNodes)
    return "nx, ny and nz lie in [2, 256]";
  if ((uint64_t)L.nx * L.ny * L.nz > (uint64_t)kMaxTotal) return "nx * ny * nz is at most 2^20";
  for (int k = 0; k < 3; k++)
    if (!ptgather::finite_bits(ptgather::bits_of(L.step[k])) || !(L.step[k] > 0.0f)) return "every step is finite and > 0";
  for (int k = 0; k < 3; k++)
    if (!ptgather::finite_bits(ptgather::bits_of(L.origin[k]))) return "every origin component is finite";
  if (L.flags & ~(uint32_t)PT_LATTICE_SKIP_BURIED) return "flags holds PT_LATTICE_SKIP_BURIED or nothing";
  return nullptr;
}
PT_PRB_HD uint32_t node_count(const PtProbeLattice& L) { return L.nx * L.ny * L.nz; }
// the slice [first, first + count) lies in the lattice
PT_PRB_HD bool slice_valid(const PtProbeLattice& L, uint32_t first, uint32_t count) { return (uint64_t)first + count <= (uint64_t)node_count(L); }
PT_PRB_HD const char* options_error(uint32_t flags, float normal_bias) {
  if (flags & ~(uint32_t)PT_PROBE_HALFSPACE) return "flags holds PT_PROBE_HALFSPACE or nothing";
  if (!ptgather::finite_bits(ptgather::bits_of(normal_bias))) return "normal_bias is finite";
  return nullptr;
}

// ---- the nodes --------------------------------------------------------------------------------------------------------------
PT_PRB_HD void node_position(const PtProbeLattice& L, uint32_t ix, uint32_t iy, uint32_t iz, float pos[3]) {
  pos[0] = fma_((float)ix, L.step[0], L.origin[0]);
  pos[1] = fma_((float)iy, L.step[1], L.origin[1]);
  pos[2] = fma_((float)iz, L.step[2], L.origin[2]);
}
PT_PRB_HD void node_position(const PtProbeLattice& L, uint32_t i, float pos[3]) {
  const uint32_t ix = i % L.nx, t = i / L.nx;
  node_position(L, ix, t % L.ny, t / L.ny, pos);
}
// geom: {cx, cy, cz, r * r} as the kernels intersect it; type: the sphere's, as uploaded
PT_PRB_HD bool buried_by(const float pos[3], const float geom[4], int32_t type) {
  if (type == PT_GLASS) return false;
  const float w[3] = {pos[0] - geom[0], pos[1] - geom[1], pos[2] - geom[2]};
  const float d2 = dot(w, w);
  return d2 < geom[3];
}

// ---- the shading ------------------------------------------------------------------------------------------------------------
// the look-up of a DIFFUSE, METAL or GLASS pixel: its cell, its fractions and its basis with the band factors
struct Lookup {
  uint32_t i[3];
  float f[3];
  float B[9];
};

PT_PRB_HD uint32_t cell_of(float g, uint32_t n) {
  const float fl = __builtin_floorf(g);
  const float last = (float)(n - 2u);
  if (!(fl > 0.0f)) return 0u;  // (below the lattice, and a NaN)
  if (fl >= last) return n - 2u;
  return (uint32_t)(int32_t)fl;
}
PT_PRB_HD float fraction_of(float g, uint32_t i) {
  const float t = g - (float)i;
  const float lo = t > 0.0f ? t : 0.0f;
  return lo < 1.0f ? lo : 1.0f;
}

PT_PRB_HD void lookup(int32_t type, const float n[3], const float hp[3], const PtProbeLattice& L, float bias, const float cam[3], Lookup& k) {
  const uint32_t nn[3] = {L.nx, L.ny, L.nz};
  for (int c = 0; c < 3; c++) {
    const float q = fma_(bias, n[c], hp[c]);
    const float d = q - L.origin[c];
    const float g = d / L.step[c];
    k.i[c] = cell_of(g, nn[c]);
    k.f[c] = fraction_of(g, k.i[c]);
  }
  float omega[3] = {n[0], n[1], n[2]};
  if (type != PT_DIFFUSE) {
    const float v[3] = {hp[0] - cam[0], hp[1] - cam[1], hp[2] - cam[2]};
    if (type == PT_METAL) {
      const float d = dot(v, n);
      const float t = 2.0f * d;
      const float m[3] = {t * n[0], t * n[1], t * n[2]};
      const float r[3] = {v[0] - m[0], v[1] - m[1], v[2] - m[2]};
      ptgather::unit_normal(r, omega);
    } else {
      ptgather::unit_normal(v, omega);
    }
  }
  float Y[9];
  ptgather::sh_basis(omega, Y);
  const float b0 = type == PT_DIFFUSE ? 3.14159265f : 1.0f, b1 = type == PT_DIFFUSE ? 2.09439510f : 1.0f, b2 = type == PT_DIFFUSE ? 0.785398163f : 1.0f;
  k.B[0] = b0 * Y[0];
  k.B[1] = b1 * Y[1]; k.B[2] = b1 * Y[2]; k.B[3] = b1 * Y[3];
  k.B[4] = b2 * Y[4]; k.B[5] = b2 * Y[5]; k.B[6] = b2 * Y[6]; k.B[7] = b2 * Y[7]; k.B[8] = b2 * Y[8];
}

// corner `corner` of the look-up's cell: its weight
PT_PRB_HD float corner_weight(const Lookup& k, int corner) {
  const float wx = (corner & 1) ? k.f[0] : 1.0f - k.f[0];
  const float wy = (corner & 2) ? k.f[1] : 1.0f - k.f[1];
  const float wz = (corner & 4) ? k.f[2] : 1.0f - k.f[2];
  const float wxy = wx * wy;
  return wxy * wz;
}
PT_PRB_HD uint32_t corner_node(const Lookup& k, const PtProbeLattice& L, int corner) {
  const uint32_t ix = k.i[0] + (uint32_t)(corner & 1), iy = k.i[1] + (uint32_t)((corner >> 1) & 1), iz = k.i[2] + (uint32_t)((corner >> 2) & 1);
  return (iz * L.ny + iy) * L.nx + ix;
}
// what of "kept" needs no record: the weight and the half-space
PT_PRB_HD bool corner_wanted(const Lookup& k, const PtProbeLattice& L, uint32_t flags, const float n[3], const float hp[3], int corner, float w) {
  if (!(w > 0.0f)) return false;
  if (!(flags & PT_PROBE_HALFSPACE)) return true;
  float pos[3];
  node_position(L, k.i[0] + (uint32_t)(corner & 1), k.i[1] + (uint32_t)((corner >> 1) & 1), k.i[2] + (uint32_t)((corner >> 2) & 1), pos);
  const float e[3] = {pos[0] - hp[0], pos[1] - hp[1], pos[2] - hp[2]};
  return dot(e, n) > 0.0f;
}
// a wanted corner's record (28 floats: sh[9][3], samples) into the sums {S.r, S.g, S.b, W}
PT_PRB_HD void corner_add(const Lookup& k, float w, const float rec[kRecordFloats], float sums[4]) {
  if (!(rec[27] > 0.0f)) return;
  float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
  for (int j = 0; j < 9; j++) {
    e0 = fma_(k.B[j], rec[3 * j], e0);
    e1 = fma_(k.B[j], rec[3 * j + 1], e1);
    e2 = fma_(k.B[j], rec[3 * j + 2], e2);
  }
  sums[3] = sums[3] + w;
  sums[0] = fma_(w, e0, sums[0]);
  sums[1] = fma_(w, e1, sums[1]);
  sums[2] = fma_(w, e2, sums[2]);
}
PT_PRB_HD float clamp0(float v) { return v > 0.0f ? v : 0.0f; }
PT_PRB_HD void finish(int32_t type, const float albedo[3], const float sums[4], float out[4]) {
  if (!(sums[3] > 0.0f)) {
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    return;
  }
  for (int c = 0; c < 3; c++) {
    const float q = sums[c] / sums[3];
    const float v = clamp0(q);
    if (type == PT_DIFFUSE) {
      const float s = v * 0.318309886f;
      out[c] = albedo[c] * s;
    } else if (type == PT_METAL) {
      out[c] = albedo[c] * v;
    } else {
      out[c] = v;
    }
  }
  out[3] = 1.0f;
}

// the pixels that need no probe: true, and `out` is the texel
PT_PRB_HD bool flat_pixel(const float albedo[3], int32_t index, int32_t type, float out[4]) {
  if (index < 0 || type == PT_EMISSIVE) {
    out[0] = albedo[0]; out[1] = albedo[1]; out[2] = albedo[2]; out[3] = 1.0f;
    return true;
  }
  if (type != PT_DIFFUSE && type != PT_METAL && type != PT_GLASS) {
    out[0] = out[1] = out[2] = 0.0f; out[3] = 1.0f;
    return true;
  }
  return false;
}

// The corners of a look-up blended into the texel: `load(node, corner, rec)` fetches a wanted corner's 28 floats (the kernel:
// seven 16-byte loads, or the wave's staged copy of the cell; the host: a copy).  A corner that is not wanted is not fetched.
template <class Load>
PT_PRB_HD void blend(const Lookup& k, int32_t type, const float albedo[3], const float n[3], const float hp[3], const PtProbeLattice& L, uint32_t flags,
                     Load load, float out[4]) {
  float sums[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int corner = 0; corner < 8; corner++) {
    const float w = corner_weight(k, corner);
    if (!corner_wanted(k, L, flags, n, hp, corner, w)) continue;
    float rec[kRecordFloats];
    load(corner_node(k, L, corner), corner, rec);
    corner_add(k, w, rec, sums);
  }
  finish(type, albedo, sums, out);
}

// One pixel, whole.
template <class Load>
PT_PRB_HD void shade_pixel(const float albedo[3], const float n[3], const float hp[3], int32_t index, int32_t type, const PtProbeLattice& L,
                           uint32_t flags, float bias, const float cam[3], Load load, float out[4]) {
  if (flat_pixel(albedo, index, type, out)) return;
  Lookup k;
  lookup(type, n, hp, L, bias, cam, k);
  blend(k, type, albedo, n, hp, L, flags, load, out);
}

}  // namespace ptprobe
