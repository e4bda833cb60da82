// pt_scene_image.hpp — what pt_set_spheres puts on the device, as far as the host alone decides it (pure: no HIP runtime; the
// library, the host exports of pt_host.cpp and the CPU tests' shims compile the same functions, under -ffp-contract=off):
// the split of a PtSphere list into the records the kernels read, the gather of a per-sphere array into a structure's slot
// order, and the uniform grid in the layout the kernel that will read it wants.  The upload itself is pt_api.hip's.
#pragma once
#include "pt_geom_plan.hpp"
#include "pt_grid.hpp"
#include "pt_grid_records.hpp"

namespace ptscene {

// A sphere list split into the 16-byte geometry record the intersection loop stages into LDS and the 32-byte shading
// record read once per closest hit.
struct Split {
  // PT_LDS_ENTRIES(n) x {cx, cy, cz, r*r}: already padded (multiple of 8 + one prefetch group, unreachable spheres beyond
  // MAX_T) and with r*r precomputed: the fp32 multiply `pow(radius, 2.)` of static/shader.frag:149, performed here
  std::vector<float> geom;
  std::vector<PtMatRec> mat;  // n
  std::vector<float> radii;   // n, signed
  // n x {r0 for the ratio 1 / ri (front face), r0 for the ratio ri}: reflectance()'s r0 = ((1 - ratio) / (1 + ratio))^2
  // (static/shader.frag:205) for both ratios a GLASS sphere is entered with: a subtraction, an addition, an IEEE division and a
  // product in fp32 under -ffp-contract=off give the same bits here as in the kernel.  Read by the small-list kernels only
  // (pt_shade.hpp): in the closed room (config 4) the GLASS branch runs in 95 % of the wave steps for 3.6 lanes, and a division
  // is a dozen instructions for the whole wave (config 4 -0.7 %, State::default within the boxes' spread; the kernels of the
  // large scenes sit at their register limits and measured +1 % with it: they keep the division; profiles/r05_ab_runs.txt)
  std::vector<float> r0;
  std::vector<int32_t> uuid;  // n: PtSphere.uuid in list order
  bool regular = true;        // every |center[k]| and |radius| < 1e15f (NaN fails): the precondition of both structures
};

inline Split split(const PtSphere* s, uint32_t n) {
  Split out;
  const uint32_t n_pad = PT_LDS_ENTRIES(n);
  out.geom.assign((size_t)n_pad * 4, 1e15f);
  for (uint32_t i = n; i < n_pad; i++) out.geom[4 * i + 3] = 0.0f;
  out.mat.resize(n); out.radii.resize(n); out.r0.resize(2 * (size_t)n); out.uuid.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    PtMatRec& m = out.mat[i];
    for (int k = 0; k < 3; k++) {
      out.regular = out.regular && (std::fabs(s[i].center[k]) < 1e15f);
      out.geom[4 * i + k] = s[i].center[k];
      m.albedo[k] = s[i].albedo[k];
    }
    out.regular = out.regular && (std::fabs(s[i].radius) < 1e15f); // NaN fails both
    out.geom[4 * i + 3] = s[i].radius * s[i].radius;
    m.fuzz = s[i].fuzz;
    m.refraction_index = s[i].refraction_index;
    m.type = s[i].type;
    m.radius = out.radii[i] = s[i].radius;
    m.inv_ri = 1.0f / s[i].refraction_index;  // (IEEE division, -ffp-contract=off: what `1.0 / ri` is in the shader's arithmetic contract)
    const float front = m.inv_ri, back = m.refraction_index;
    const float qf = (1.0f - front) / (1.0f + front), qb = (1.0f - back) / (1.0f + back);
    out.r0[2 * i] = qf * qf;
    out.r0[2 * i + 1] = qb * qb;
    out.uuid[i] = s[i].uuid;
  }
  return out;
}

// a per-sphere array in the slot order of a structure (index[k] = the sphere of slot k): the walk kernels shade from a slot
// and need no index look-up.  A slot whose index names no sphere (padding: never hit) gets a value-initialised element.
template <class T>
std::vector<T> per_slot(const uint32_t* index, size_t n_index, const T* src, size_t n_src) {
  std::vector<T> out(n_index);
  for (size_t k = 0; k < n_index; k++)
    if (index[k] < n_src) out[k] = src[index[k]];
  return out;
}

// cell records a build that stages them copies into the LDS: a one-layer grid's in the ring layout (pt_grid_records.hpp; the
// builds that walk such a grid along three axes stage the plain array into the same room)
inline uint64_t staged_cells(const ptgrid::Grid& g) {
  return g.n[1] == 1u ? ptrec::ring_cells(g.n[0], g.n[2]) : (uint64_t)g.n[0] * g.n[1] * g.n[2];
}

// the uniform grid of PT_GEOM_GRID for a scene, laid out for the kernel that will read it
inline bool build_grid(const float* geom, const float* radii, uint32_t n, double near_factor, ptgrid::Grid* grid) {
  if (!ptgrid::build(geom, radii, n, grid, near_factor)) return false;
  // entries that will not be staged in the LDS (pt_api.hip bind_grid) are gathered from L2: their runs in Morton order of the cells
  if (PT_GRID_LDS_CELLS(staged_cells(*grid)) + (size_t)grid->n_entries * 16 > walk_lds_room()) {
    int mode = 2;
#ifdef PT_DEV_KNOBS  // A/B only: PT_PAD_RUNS = 0 plain layout, 1 padded runs in Morton order, 2 Morton order (default), 3 padded runs
    if (getenv("PT_PAD_RUNS")) mode = atoi(getenv("PT_PAD_RUNS"));
#endif
    if (mode) (void)ptgrid::morton_runs(grid, mode != 2, mode != 3);
  }
  // the device record's entry field (pt_grid_records.hpp), checked on the layout that is uploaded (padded runs are longer):
  // no grid, as when the host format overflows
  return ptrec::fits(grid->n_entries);
}

}  // namespace ptscene
