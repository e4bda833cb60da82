// pt_kernels_gather.hip — GATHER QUERIES (pt_gather_irradiance, pt_bake_probes; include/ptrace.h), a
// translation unit and gfx950 code object of its own: the HIP runtime loads it at the first gather call of a process, so a
// context that never asks pays nothing.  Two kernels around the radiance builds and their fold, which run as they are:
//   pt_gather_rays_kernel     THE GENERATOR, in the pack kernel's place: one thread per ray of a batch.  Ray `first + i` of the
//                             call is direction j = (first + i) % D of item (first + i) / D; its two texels go where the radiance
//                             builds read them (the point and normal planes of the query planes).  An invalid item's rays are the
//                             null ray: the builds trace nothing for them and the fold answers the zero record.
//   pt_gather_reduce_kernel   THE REDUCE: one wave per item a batch touches, four waves per workgroup.  Lane l takes the item's
//                             records j = l, l + 64, ... that lie in the batch, in ascending order, starting from +0 — or, where the
//                             item began in an earlier batch, from the lane's partial sums that batch left in `carry_in`.  An item
//                             that ends in the batch is folded across the lanes by the xor butterfly (DPP row and bank moves via
//                             __shfl_xor: every lane ends with the same bits) and stored by lane 0 with plain vector stores; an
//                             item that goes on leaves its partial sums in `carry_out`.  Only the first item of a batch reads and
//                             only the last writes, but in a batch that holds both they are different waves of ONE launch, in no
//                             order: carry_in and carry_out are therefore two slots, which the host swaps from batch to batch
//                             (the launches of a stream are ordered: a slot is read only by the launch after the one that wrote
//                             it).  One item that spans a whole batch reads the one and writes the other in the same wave.
//                             No LDS, no atomics, no scratch.
// The per-lane statements are pt_gather.hpp's, shared with the host.  pt_api.hip reaches the kernels through pt_gather_kernel().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_arith.hpp"
#include "pt_extra.h"
#include "pt_sigs.h"
#include "pt_gather.hpp"
#include "pt_query.hpp"

namespace {

typedef float Vec4 __attribute__((ext_vector_type(4)));
// the caller's arrays are arrays of floats: four at a time, but no alignment beyond a float's is assumed
typedef float Vec4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void store4(void* p, float x, float y, float z, float w) {
  const Vec4u v = {x, y, z, w};
  *reinterpret_cast<Vec4u*>(p) = v;
}
__device__ __forceinline__ PtGatherPoint load_point(const PtGatherPoint* p) {
  const Vec4u a = reinterpret_cast<const Vec4u*>(p)[0], b = reinterpret_cast<const Vec4u*>(p)[1];
  PtGatherPoint g;
  g.position[0] = a.x; g.position[1] = a.y; g.position[2] = a.z; g._pad0 = 0.0f;
  g.normal[0] = b.x; g.normal[1] = b.y; g.normal[2] = b.z; g._pad1 = 0.0f;
  return g;
}

}  // namespace

// grid = ceil(m / 256) workgroups of 256 threads; m <= plane.  points[k] is item item0 + k of the call: every item the rays
// [first, first + m) touch is in it.  Writes texel i < m of the point and the normal plane and nothing else.
extern "C" __global__ __launch_bounds__(256) void pt_gather_rays_kernel(const PtGatherPoint* points, uint32_t item0, uint32_t first, uint32_t m,
                                                                        uint32_t D, int kind, ptq::F4* planes, uint32_t plane) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  const uint32_t ray = first + i;  // (< n * D <= 2^32 - 1: no wrap)
  const uint32_t item = ray / D, j = ray % D;
  const PtGatherPoint p = load_point(points + (item - item0));
  float s, c;
  ptd::sincos2pi(ptgather::turn(j), s, c);
  const PtRay r = ptgather::ray_of(p, kind, j, D, s, c);
  store4(planes + (size_t)PT_FEAT_POINT * plane + i, r.origin[0], r.origin[1], r.origin[2], 0.0f);
  store4(planes + (size_t)PT_FEAT_NORMAL * plane + i, r.direction[0], r.direction[1], r.direction[2], 0.0f);
}

// grid = ceil(items / 4) workgroups of 256 threads, items = the items the rays [first, first + m) touch (item0 the first of
// them).  rec[i], i < m: the folded record of ray first + i.  points as above.  carry_in, carry_out: two different slots of 64 * 28 floats, lane l's at 28 l.
// out[k]: the record of item out0 + k (a PtIrradiance or a PtProbeSH); only items that END in this batch are written.
extern "C" __global__ __launch_bounds__(256) void pt_gather_reduce_kernel(const PtRayRadiance* rec, const PtGatherPoint* points, uint32_t item0,
                                                                          uint32_t items, uint32_t first, uint32_t m, uint32_t D, int kind,
                                                                          const float* carry_in, float* carry_out, void* out, uint32_t out0) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
  if (k >= items) return;
  const uint32_t item = item0 + k;
  const uint64_t base = (uint64_t)item * D, end = (uint64_t)first + m;  // the item's first ray; the batch's end
  const uint32_t ja = base < first ? (uint32_t)(first - base) : 0u;      // the item's records [ja, jb) lie in this batch
  const uint32_t jb = base + D <= end ? D : (uint32_t)(end - base);
  const bool ends_here = jb == D;
  const bool valid = ptgather::item_valid(load_point(points + k), kind);
  const int n_acc = kind == ptgather::PROBE ? ptgather::kProbeAcc : ptgather::kIrrAcc;  // (launch-uniform)
  float acc[ptgather::kMaxAcc];
#pragma unroll
  for (int a = 0; a < ptgather::kMaxAcc; a++) acc[a] = 0.0f;
  if (valid) {
    if (ja > 0u) {
#pragma unroll
      for (int a = 0; a < ptgather::kMaxAcc; a++)
        if (a < n_acc) acc[a] = carry_in[lane * ptgather::kMaxAcc + a];
    }
    // the lane's first j at or behind ja: ja + ((lane - ja) mod 64)
    for (uint32_t j = ja + ((lane - ja) & 63u); j < jb; j += 64u) {
      const Vec4 t = *reinterpret_cast<const Vec4*>(rec + (size_t)(base + j - first));
      PtRayRadiance r;
      r.sum[0] = t.x; r.sum[1] = t.y; r.sum[2] = t.z; r.samples = t.w;
      if (kind == ptgather::PROBE) {
        float s, c, w[3], Y[9];
        ptd::sincos2pi(ptgather::turn(j), s, c);
        ptgather::sphere_direction(ptgather::stratum(j, D), s, c, w);
        ptgather::sh_basis(w, Y);
        ptgather::lane_add_probe(acc, r, Y);
      } else {
        ptgather::lane_add_irradiance(acc, r);
      }
    }
    if (!ends_here) {
#pragma unroll
      for (int a = 0; a < ptgather::kMaxAcc; a++)
        if (a < n_acc) carry_out[lane * ptgather::kMaxAcc + a] = acc[a];
      return;
    }
    // (the wave is whole here: `valid`, `ends_here` and the item are wave-uniform)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
      for (int a = 0; a < ptgather::kMaxAcc; a++)
        if (a < n_acc) acc[a] = acc[a] + __shfl_xor(acc[a], o, 64);
    }
  } else if (!ends_here) {
    return;  // (an invalid item: all +0 when it ends)
  }
  if (lane != 0u) return;
  if (kind == ptgather::PROBE) {
    const PtProbeSH p = ptgather::probe_record(acc, D);
    float* dst = reinterpret_cast<float*>(reinterpret_cast<PtProbeSH*>(out) + (item - out0));
#pragma unroll
    for (int q = 0; q < 7; q++) {
      const float* src = &p.sh[0][0] + 4 * q;
      store4(dst + 4 * q, src[0], src[1], src[2], q == 6 ? p.samples : src[3]);
    }
  } else {
    const PtIrradiance e = ptgather::irradiance_record(acc, D);
    store4(reinterpret_cast<PtIrradiance*>(out) + (item - out0), e.e[0], e.e[1], e.e[2], e.samples);
  }
}

extern "C" const void* pt_gather_kernel(int id) {
  switch (id) {
    case PT_GATHER_RAYS: return ptcall::handle(ptsig::GatherRays{}, pt_gather_rays_kernel);
    case PT_GATHER_REDUCE: return ptcall::handle(ptsig::GatherReduce{}, pt_gather_reduce_kernel);
  }
  return nullptr;
}
