// pt_kernels_probe.hip — PROBE LATTICES (pt_bake_lattice, pt_shade_probes; include/ptrace.h), a translation
// unit and gfx950 code object of its own: the HIP runtime loads it at the first of the two calls of a process, so a context that
// never asks pays nothing.  Two kernels:
//   pt_probe_points_kernel    THE GENERATOR: one thread per node of a bake's slice.  Node first + i becomes PtGatherPoint i of the
//                             buffer the gather calls' host body then reads in place: {position, 0, 0, 0, 0, 0}, or a NaN position
//                             where PT_LATTICE_SKIP_BURIED finds the node inside a sphere that is not GLASS (the installed list's
//                             {centre, r * r} records and types, read by every lane at the same address: scalar loads).
//   pt_probe_shade_kernel     THE SHADING, the hot path: one lane per pixel, a wave covers an 8 x 8 block of pixels (a workgroup
//   pt_probe_shade_shared_kernel  four such blocks, consecutive in the work queue's tile order: tile t = ty * tiles_x + tx), so that
//                             the lanes of a wave fall into one or two cells of the lattice and their record loads hit the same
//                             lines.  A lane reads its four feature texels (64 bytes), then the records of the corners its weight
//                             and the half-space test want — seven 16-byte loads each — and writes one 16-byte texel with a
//                             plain vector store.  The lattice (at most a few megabytes in practice) lives in L2.  No atomics, no
//                             scratch.  Partial blocks at the right and top edges: the lanes outside write nothing.  The first
//                             form loads per lane and uses no LDS; the second, which pt_shade_probes launches (it won every
//                             measured case: DESIGN.md §4.8p, profiles/r33_probe_lit.txt), stages a coherent wave's cell in the
//                             wave's own 896 bytes of LDS (shade_body below).  The same bits either way.
// The per-lane statements are pt_probe.hpp's, shared with the host.  pt_api.hip reaches the kernels through pt_lattice_kernel().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_extra.h"
#include "pt_sigs.h"
#include "pt_kernel_args.h"
#include "pt_probe.hpp"

namespace {

typedef float Vec4 __attribute__((ext_vector_type(4)));
typedef int IVec4 __attribute__((ext_vector_type(4)));
// the caller's arrays are arrays of floats: four at a time, but no alignment beyond a float's is assumed
typedef float Vec4u __attribute__((ext_vector_type(4), aligned(4)));

// a node's record: seven 16-byte loads
struct LoadRecord {
  const float* probes;
  __device__ __forceinline__ void operator()(uint32_t node, int, float rec[ptprobe::kRecordFloats]) const {
    const Vec4u* src = reinterpret_cast<const Vec4u*>(probes + (size_t)node * ptprobe::kRecordFloats);
#pragma unroll
    for (int q = 0; q < 7; q++) {
      const Vec4u v = src[q];
      rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
    }
  }
};
// a corner's record out of the wave's staged cell: seven 16-byte LDS reads, every lane at one address (a broadcast)
struct LoadStaged {
  const float* cell;  // 8 x 28 floats
  __device__ __forceinline__ void operator()(uint32_t, int corner, float rec[ptprobe::kRecordFloats]) const {
    const Vec4* src = reinterpret_cast<const Vec4*>(cell + corner * ptprobe::kRecordFloats);
#pragma unroll
    for (int q = 0; q < 7; q++) {
      const Vec4 v = src[q];
      rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
    }
  }
};

// The body of both shading kernels.  kShared: a wave whose lit lanes all share one cell (a readfirstlane compare and a ballot)
// fetches the cell's eight records ONCE — lanes 0 .. 55 one 16-byte load each, into the wave's 896 bytes of LDS — and every lane
// reads its wanted corners from there; any other wave takes the straight loads.  The LDS copy is the wave's own: no workgroup
// barrier (the four waves of a workgroup take different ways), a wave's DS operations complete in order.  The statements and
// their operands are the same either way: the same bits.
template <bool kShared>
__device__ __forceinline__ void shade_body(const Vec4* planes, uint32_t plane, uint32_t width, uint32_t rows, const PtProbeLattice& L, uint32_t flags, float bias,
                                           const float cam[3], const float* probes, float* out, float* staged, uint32_t* paths) {
  const uint32_t tiles_x = (width + 7u) / 8u, tiles_y = (rows + 7u) / 8u;
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
  if (tile >= tiles_x * tiles_y) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t x = (tile % tiles_x) * 8u + (lane & 7u), y = (tile / tiles_x) * 8u + (lane >> 3);
  const bool inside = x < width && y < rows;
  if (!kShared && !inside) return;
  const size_t p = inside ? (size_t)y * width + x : 0;  // (a lane outside reads texel 0 and writes nothing)
  const Vec4 a = planes[(size_t)PT_FEAT_ALBEDO * plane + p], n4 = planes[(size_t)PT_FEAT_NORMAL * plane + p], h4 = planes[(size_t)PT_FEAT_POINT * plane + p];
  const IVec4 ids = reinterpret_cast<const IVec4*>(planes)[(size_t)PT_FEAT_IDS * plane + p];
  const float albedo[3] = {a.x, a.y, a.z}, n[3] = {n4.x, n4.y, n4.z}, hp[3] = {h4.x, h4.y, h4.z};
  float texel[4];
  if (!kShared) {
    ptprobe::shade_pixel(albedo, n, hp, ids.x, ids.z, L, flags, bias, cam, LoadRecord{probes}, texel);
  } else {
    const bool lit = inside && !ptprobe::flat_pixel(albedo, ids.x, ids.z, texel);
    ptprobe::Lookup k;
    uint32_t cell = 0u;
    if (lit) {
      ptprobe::lookup(ids.z, n, hp, L, bias, cam, k);
      cell = ptprobe::corner_node(k, L, 0);
    }
    const unsigned long long lit_lanes = __ballot(lit);
    bool shared = false;
    uint32_t cell0 = 0u;
    if (lit_lanes) {
      cell0 = (uint32_t)__shfl((int)cell, (int)(__ffsll((long long)lit_lanes) - 1), 64);  // (the first lit lane's cell)
      shared = __ballot(lit && cell != cell0) == 0ull;
    }
    if (shared) {  // (wave-uniform)
      if (lane < 56u) {
        const uint32_t corner = lane / 7u, q = lane % 7u;
        const uint32_t node = cell0 + (corner & 1u) + ((corner >> 1) & 1u) * L.nx + ((corner >> 2) & 1u) * L.nx * L.ny;
        const Vec4u v = reinterpret_cast<const Vec4u*>(probes + (size_t)node * ptprobe::kRecordFloats)[q];
        const Vec4 w = {v.x, v.y, v.z, v.w};
        reinterpret_cast<Vec4*>(staged)[lane] = w;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lit) ptprobe::blend(k, ids.z, albedo, n, hp, L, flags, LoadStaged{staged}, texel);
    } else if (lit) {
      ptprobe::blend(k, ids.z, albedo, n, hp, L, flags, LoadRecord{probes}, texel);
    }
    if (paths && lane == 0u && lit_lanes) paths[tile] = shared ? 2u : 1u;  // (dev tools and tests only: which way the wave went)
    if (!inside) return;
  }
  const Vec4u v = {texel[0], texel[1], texel[2], texel[3]};
  *reinterpret_cast<Vec4u*>(out + 4u * p) = v;
}

}  // namespace

// grid = ceil(count / 256) workgroups of 256 threads.  geom: n_spheres x {cx, cy, cz, r * r}; mat: n_spheres records.
// Writes points[i], i < count, and nothing else.
extern "C" __global__ __launch_bounds__(256) void pt_probe_points_kernel(PtProbeLattice L, uint32_t first, uint32_t count, const float* geom,
                                                                          const PtMatRec* mat, uint32_t n_spheres, PtGatherPoint* points) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  float pos[3];
  ptprobe::node_position(L, first + i, pos);
  if (L.flags & PT_LATTICE_SKIP_BURIED) {
    bool buried = false;
    for (uint32_t s = 0; s < n_spheres; s++) {
      const Vec4 g = *reinterpret_cast<const Vec4*>(geom + 4u * (size_t)s);
      const float rec[4] = {g.x, g.y, g.z, g.w};
      buried = buried || ptprobe::buried_by(pos, rec, mat[s].type);
    }
    if (buried) pos[0] = pos[1] = pos[2] = ptprobe::quiet_nan();
  }
  Vec4* dst = reinterpret_cast<Vec4*>(points + i);
  const Vec4 a = {pos[0], pos[1], pos[2], 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f};
  dst[0] = a;
  dst[1] = b;
}

// grid = ceil(tiles_x * tiles_y / 4) workgroups of 256 threads, tiles_x = ceil(width / 8), tiles_y = ceil(rows / 8).
// planes: the four feature planes, plane k at k * plane texels (plane = rows * width); probes: nx * ny * nz records;
// out: rows * width texels.  Writes out[y * width + x] for every pixel of the frame and nothing else.
extern "C" __global__ __launch_bounds__(256) void pt_probe_shade_kernel(const Vec4* planes, uint32_t plane, uint32_t width, uint32_t rows,
                                                                         PtProbeLattice L, uint32_t flags, float bias, float cam_x, float cam_y,
                                                                         float cam_z, const float* probes, float* out) {
  const float cam[3] = {cam_x, cam_y, cam_z};
  shade_body<false>(planes, plane, width, rows, L, flags, bias, cam, probes, out, nullptr, nullptr);
}

// The same with the shared-cell way for coherent waves (shade_body): 3584 bytes of LDS per workgroup.  paths: NULL, or one word
// per tile that receives 1 (straight loads) or 2 (the staged cell) from every wave with a lit lane.
extern "C" __global__ __launch_bounds__(256) void pt_probe_shade_shared_kernel(const Vec4* planes, uint32_t plane, uint32_t width, uint32_t rows,
                                                                                PtProbeLattice L, uint32_t flags, float bias, float cam_x, float cam_y,
                                                                                float cam_z, const float* probes, float* out, uint32_t* paths) {
  __shared__ __attribute__((aligned(16))) float staged[4][8 * ptprobe::kRecordFloats];
  const float cam[3] = {cam_x, cam_y, cam_z};
  shade_body<true>(planes, plane, width, rows, L, flags, bias, cam, probes, out, staged[threadIdx.x >> 6], paths);
}

extern "C" const void* pt_lattice_kernel(int id) {
  switch (id) {
    case PT_PROBE_POINTS: return ptcall::handle(ptsig::ProbePoints{}, pt_probe_points_kernel);
    case PT_PROBE_SHADE: return ptcall::handle(ptsig::ProbeShade{}, pt_probe_shade_kernel);
    case PT_PROBE_SHADE_SHARED: return ptcall::handle(ptsig::ProbeShadeShared{}, pt_probe_shade_shared_kernel);
  }
  return nullptr;
}
