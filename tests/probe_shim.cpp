// probe_shim.cpp — csrc/pt_probe.hpp (the probe lattices' checks, node positions, buried rule and shading) and the ProbeSet of
// csrc/pt_buffers.hpp in front of ctypes for tests/test_probe_ref.py: CPU only, no HIP; built with -ffp-contract=off, as the
// library is.  The device allocator pt_buffers.hpp asks of its includer is a stand-in, as in tests/buffers_shim.cpp: malloc / free
// with a counter that makes the k-th allocation fail.
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../ray_tracer_webgl_amd/csrc/pt_buffers.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_probe.hpp"
#include "probe_sweep.hpp"

namespace {
long g_allocs = 0, g_fail_at = 0, g_live = 0;
}  // namespace

int ptbuf::dev_malloc(void** p, size_t bytes) {
  *p = nullptr;
  if (++g_allocs == g_fail_at) return 2;
  *p = std::malloc(bytes ? bytes : 1);
  if (!*p) return 2;
  g_live++;
  return 0;
}
int ptbuf::dev_free(void* p) {
  std::free(p);
  g_live--;
  return 0;
}

extern "C" {
// the checks: NULL, or the words
const char* prb_lattice_error(const PtProbeLattice* L) { return ptprobe::lattice_error(*L); }
const char* prb_options_error(uint32_t flags, float bias) { return ptprobe::options_error(flags, bias); }
int prb_slice_valid(const PtProbeLattice* L, uint32_t first, uint32_t count) { return ptprobe::slice_valid(*L, first, count) ? 1 : 0; }
uint32_t prb_node_count(const PtProbeLattice* L) { return ptprobe::node_count(*L); }
void prb_node_position(const PtProbeLattice* L, uint32_t i, float pos[3]) { ptprobe::node_position(*L, i, pos); }
// geom: {cx, cy, cz, r * r}
int prb_buried_by(const float pos[3], const float geom[4], int32_t type) { return ptprobe::buried_by(pos, geom, type) ? 1 : 0; }

// n pixels: f9 = {albedo, n, hp} per pixel, i2 = {index, type}; probes: 28 floats per node; out: 4 floats per pixel;
// loads: the records fetched, in all (a corner that is not wanted is not read)
void prb_shade(const PtProbeLattice* L, const float* probes, uint32_t flags, float bias, const float cam[3], uint32_t n, const float* f9,
               const int32_t* i2, float* out, uint64_t* loads) {
  uint64_t fetched = 0;
  auto load = [&](uint32_t node, int, float rec[ptprobe::kRecordFloats]) {
    fetched++;
    std::memcpy(rec, probes + (size_t)node * ptprobe::kRecordFloats, sizeof(float) * ptprobe::kRecordFloats);
  };
  for (uint32_t k = 0; k < n; k++)
    ptprobe::shade_pixel(f9 + 9 * (size_t)k, f9 + 9 * (size_t)k + 3, f9 + 9 * (size_t)k + 6, i2[2 * (size_t)k], i2[2 * (size_t)k + 1], *L, flags, bias, cam, load,
                         out + 4 * (size_t)k);
  if (loads) *loads = fetched;
}

// the sweep (tests/probe_sweep.hpp)
void prb_sweep_lattice(PtProbeLattice* L, float cam[3]) {
  *L = probesweep::lattice();
  std::memcpy(cam, probesweep::camera(), 3 * sizeof(float));
}
uint32_t prb_sweep_sets(void) { return probesweep::SET_COUNT; }
void prb_sweep_records(int set, float* out) {
  const std::vector<float> r = probesweep::records(set);
  std::memcpy(out, r.data(), r.size() * sizeof(float));
}
uint32_t prb_sweep_pixels(float* f9, int32_t* i2) {
  const std::vector<probesweep::Pixel> v = probesweep::pixels();
  if (f9 && i2)
    for (size_t k = 0; k < v.size(); k++) {
      std::memcpy(f9 + 9 * k, v[k].albedo, 3 * sizeof(float));
      std::memcpy(f9 + 9 * k + 3, v[k].n, 3 * sizeof(float));
      std::memcpy(f9 + 9 * k + 6, v[k].hp, 3 * sizeof(float));
      i2[2 * k] = v[k].index;
      i2[2 * k + 1] = v[k].type;
    }
  return (uint32_t)v.size();
}

// the set
void alloc_fail_at(long k) { g_allocs = 0; g_fail_at = k; }
long alloc_live() { return g_live; }
ptbuf::ProbeSet* set_new() { return new ptbuf::ProbeSet(); }
void set_delete(ptbuf::ProbeSet* s) { delete s; }
int set_fit_points(ptbuf::ProbeSet* s, uint64_t nodes) { return s->fit_points(nodes).ok() ? 0 : 1; }
int set_fit_stage(ptbuf::ProbeSet* s, uint64_t nodes) { return s->fit_stage(nodes).ok() ? 0 : 1; }
int set_points_in_place(const ptbuf::ProbeSet* s, uint64_t nodes) { return s->points_in_place(nodes) ? 1 : 0; }
int set_stage_in_place(const ptbuf::ProbeSet* s, uint64_t nodes) { return s->stage_in_place(nodes) ? 1 : 0; }
void set_release_points(ptbuf::ProbeSet* s) { s->release_points(); }
void set_release_stage(ptbuf::ProbeSet* s) { s->release_stage(); }
uint64_t set_points_capacity(const ptbuf::ProbeSet* s) { return s->points.capacity(); }
uint64_t set_stage_capacity(const ptbuf::ProbeSet* s) { return s->stage.capacity(); }
}
