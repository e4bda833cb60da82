// pt_query.hpp — the ARITHMETIC of ray queries (include/ptrace.h pt_query_rays), written once for the device
// and the host: which rays are invalid, how a call's n rays fall into launches and how many tile rows a launch covers, how a
// PtRay becomes two texels of the query planes and how four texels become a PtRayHit.  The query builds of the trace kernel
// (pt_refill.hpp start_sample QRY) and the pack and unpack kernels of pt_kernels_query.hip run it per lane, pt_api.hip runs it
// for host pointers, tests/query_plan_shim.cpp pins it and tests/query_main.cpp drives it over bounds-checked buffers under the
// sanitizers.  No HIP header needed; integers and bit tests only, no floating-point operation.
#pragma once
#include <stdint.h>

#include "../../include/ptrace.h"

#if defined(__HIPCC__)
#define PT_QRY_HD __host__ __device__ __forceinline__
#else
#define PT_QRY_HD inline
#endif

namespace ptq {

struct alignas(16) F4 { float x, y, z, w; };
struct alignas(16) I4 { int32_t x, y, z, w; };

PT_QRY_HD uint32_t bits_of(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, sizeof u);
  return u;
}
// neither NaN nor an infinity: the exponent field is not all ones
PT_QRY_HD bool finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }
// +0 or -0
PT_QRY_HD bool zero_bits(uint32_t u) { return (u & 0x7fffffffu) == 0u; }

// THE VALIDITY PREDICATE: a ray is invalid when a component of its origin or direction is not finite, or when its three
// direction components are all zeros of either sign.  Everything else is answered (denormal directions included).
PT_QRY_HD bool ray_valid(float ox, float oy, float oz, float dx, float dy, float dz) {
  const uint32_t o0 = bits_of(ox), o1 = bits_of(oy), o2 = bits_of(oz), d0 = bits_of(dx), d1 = bits_of(dy), d2 = bits_of(dz);
  const bool finite = finite_bits(o0) && finite_bits(o1) && finite_bits(o2) && finite_bits(d0) && finite_bits(d1) && finite_bits(d2);
  const bool null_direction = zero_bits(d0) && zero_bits(d1) && zero_bits(d2);
  return finite && !null_direction;
}

// ---- batches: a call's n rays in launches of at most `batch` (the local pixel count, > 0) ---------------------------------------
PT_QRY_HD uint32_t n_batches(uint32_t n, uint32_t batch) { return n / batch + (n % batch ? 1u : 0u); }
// rays of launch k < n_batches: a full batch, the last one what is left
PT_QRY_HD uint32_t batch_rays(uint32_t n, uint32_t batch, uint32_t k) {
  const uint64_t first = (uint64_t)k * batch;
  const uint64_t left = (uint64_t)n - first;
  return left < batch ? (uint32_t)left : batch;
}
// ray i of a launch is local pixel i: m rays occupy the first ceil(m / width) rows, i.e. the first ceil(rows / 8) rows of 8x8 tiles
PT_QRY_HD uint32_t tile_rows_covered(uint32_t m, uint32_t width) {
  const uint32_t rows = m / width + (m % width ? 1u : 0u);
  return rows / 8u + (rows % 8u ? 1u : 0u);
}
// ... and in the identity order (tile = tile row * tiles per row + tile column) those are the first this many tiles
PT_QRY_HD uint32_t tiles_covered(uint32_t m, uint32_t width) { return tile_rows_covered(m, width) * ((width + 7u) / 8u); }

// ---- the record -----------------------------------------------------------------------------------------------------------------
// a ray as its two texels (origin: PT_FEAT_POINT's plane, direction: PT_FEAT_NORMAL's); the pads are not carried
PT_QRY_HD void pack_ray(const PtRay& r, F4* origin, F4* direction) {
  const F4 o = {r.origin[0], r.origin[1], r.origin[2], 0.0f};
  const F4 d = {r.direction[0], r.direction[1], r.direction[2], 0.0f};
  *origin = o;
  *direction = d;
}
// four texels as the record, field for field
PT_QRY_HD PtRayHit unpack_hit(const F4 albedo, const F4 normal, const F4 point, const I4 ids) {
  PtRayHit h;
  h.albedo[0] = albedo.x; h.albedo[1] = albedo.y; h.albedo[2] = albedo.z; h.t = albedo.w;
  h.normal[0] = normal.x; h.normal[1] = normal.y; h.normal[2] = normal.z; h._pad0 = normal.w;
  h.point[0] = point.x; h.point[1] = point.y; h.point[2] = point.z; h._pad1 = point.w;
  h.index = ids.x; h.uuid = ids.y; h.type = ids.z; h.front_face = ids.w;
  return h;
}
// the texels of an invalid ray: all +0, ids {PT_RAY_INVALID x3, 0}
PT_QRY_HD void invalid_texels(F4* albedo, F4* normal, F4* point, I4* ids) {
  const F4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  const I4 bad = {PT_RAY_INVALID, PT_RAY_INVALID, PT_RAY_INVALID, 0};
  *albedo = zero; *normal = zero; *point = zero; *ids = bad;
}

// m rays into the planes of `plane` texels each, and back: what the pack and unpack kernels do per thread and the host does for
// host pointers.  i < m <= plane.
PT_QRY_HD void pack_at(const PtRay* rays, uint32_t i, F4* planes, uint32_t plane) {
  pack_ray(rays[i], planes + (size_t)PT_FEAT_POINT * plane + i, planes + (size_t)PT_FEAT_NORMAL * plane + i);
}
PT_QRY_HD void unpack_at(const F4* planes, uint32_t plane, uint32_t i, PtRayHit* hits) {
  const I4* ids = reinterpret_cast<const I4*>(planes + (size_t)PT_FEAT_IDS * plane);
  hits[i] = unpack_hit(planes[(size_t)PT_FEAT_ALBEDO * plane + i], planes[(size_t)PT_FEAT_NORMAL * plane + i],
                       planes[(size_t)PT_FEAT_POINT * plane + i], ids[i]);
}

}  // namespace ptq
