// scene_image_shim.cpp — C entry points over csrc/pt_scene_image.hpp (what pt_set_spheres derives from a sphere list on the
// host: the split, the per-slot gather, the grid in the layout its kernel reads) for tests/test_scene_image.py; host only, no
// HIP runtime.  Compiled by the test with g++ -ffp-contract=off, like the library.
#include "../ray_tracer_webgl_amd/csrc/pt_scene_image.hpp"

#include <algorithm>
#include <cstring>

#define SHIM extern "C" __attribute__((visibility("default")))

// PT_LDS_ENTRIES of csrc/pt_kernel_args.h
SHIM uint32_t scene_lds_entries(uint32_t n) { return PT_LDS_ENTRIES(n); }

// ptscene::split: the vectors' lengths in sizes5 = {geom floats, mat records, radii, r0 floats, uuids}, `regular` as the
// return value; each array (may be NULL) gets what its capacity holds
SHIM int scene_split(const PtSphere* s, uint32_t n, size_t* sizes5, float* geom, size_t geom_cap, PtMatRec* mat, size_t mat_cap,
                     float* radii, size_t radii_cap, float* r0, size_t r0_cap, int32_t* uuid, size_t uuid_cap) {
  const ptscene::Split sp = ptscene::split(s, n);
  sizes5[0] = sp.geom.size(); sizes5[1] = sp.mat.size(); sizes5[2] = sp.radii.size(); sizes5[3] = sp.r0.size(); sizes5[4] = sp.uuid.size();
  if (geom) std::memcpy(geom, sp.geom.data(), std::min(geom_cap, sp.geom.size()) * sizeof(float));
  if (mat) std::memcpy(mat, sp.mat.data(), std::min(mat_cap, sp.mat.size()) * sizeof(PtMatRec));
  if (radii) std::memcpy(radii, sp.radii.data(), std::min(radii_cap, sp.radii.size()) * sizeof(float));
  if (r0) std::memcpy(r0, sp.r0.data(), std::min(r0_cap, sp.r0.size()) * sizeof(float));
  if (uuid) std::memcpy(uuid, sp.uuid.data(), std::min(uuid_cap, sp.uuid.size()) * sizeof(int32_t));
  return sp.regular ? 1 : 0;
}

// ptscene::per_slot for both element types it is used with; out holds n_index elements
SHIM void scene_per_slot_mat(const uint32_t* index, size_t n_index, const PtMatRec* src, size_t n_src, PtMatRec* out) {
  const std::vector<PtMatRec> v = ptscene::per_slot(index, n_index, src, n_src);
  std::memcpy(out, v.data(), v.size() * sizeof(PtMatRec));
}
SHIM void scene_per_slot_i32(const uint32_t* index, size_t n_index, const int32_t* src, size_t n_src, int32_t* out) {
  const std::vector<int32_t> v = ptscene::per_slot(index, n_index, src, n_src);
  std::memcpy(out, v.data(), v.size() * sizeof(int32_t));
}

// ptscene::build_grid on the split of a sphere list, as pt_set_spheres (near_factor 3) and pt_tune (any class) call it:
// counts8, the arrays, the capacities and the return codes as pt_build_grid's (include/ptrace.h)
SHIM int scene_build_grid(const PtSphere* s, uint32_t n, double near_factor, uint32_t* counts8, uint32_t* cells, size_t n_cells,
                          float* entries, size_t entry_floats, uint32_t* entry_index, size_t n_index) {
  const ptscene::Split sp = ptscene::split(s, n);
  ptgrid::Grid g;
  if (!sp.regular || !ptscene::build_grid(sp.geom.data(), sp.radii.data(), n, near_factor, &g)) return PT_ERR_NOT_READY;
  if (counts8) {
    counts8[0] = g.n[0]; counts8[1] = g.n[1]; counts8[2] = g.n[2]; counts8[3] = g.n_cell_entries;
    counts8[4] = g.n_always; counts8[5] = g.n_entries; counts8[6] = g.max_cell_entries; counts8[7] = g.nonempty;
  }
  if ((cells && n_cells < g.cells.size()) || (entries && entry_floats < g.entries.size()) ||
      (entry_index && n_index < g.entry_index.size()))
    return PT_ERR_CAPACITY;
  if (cells) std::copy(g.cells.begin(), g.cells.end(), cells);
  if (entries) std::copy(g.entries.begin(), g.entries.end(), entries);
  if (entry_index) std::copy(g.entry_index.begin(), g.entry_index.end(), entry_index);
  return PT_OK;
}
