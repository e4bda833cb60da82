// gather_shim.cpp — csrc/pt_gather.hpp (the gather queries' direction set, frame, basis and reduction) and the GatherSet of
// csrc/pt_buffers.hpp in front of ctypes for tests/test_gather_ref.py: CPU only, no HIP; built with -ffp-contract=off, as the
// library is.  The device allocator pt_buffers.hpp asks of its includer is a stand-in, as in tests/buffers_shim.cpp: malloc / free
// with a counter that makes the k-th allocation fail.
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../ray_tracer_webgl_amd/csrc/pt_buffers.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_gather.hpp"
#include "gather_sweep.hpp"

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
int gth_directions_valid(uint32_t D) { return ptgather::directions_valid(D) ? 1 : 0; }
uint64_t gth_total_rays(uint32_t n, uint32_t D) { return ptgather::total_rays(n, D); }
uint32_t gth_items_per_batch(uint32_t batch) { return ptgather::items_per_batch(batch); }
// the items the batch of rays [first, first + m) touches: {item0, items, done0, done1}
void gth_item_span(uint32_t first, uint32_t m, uint32_t D, uint32_t out[4]) {
  const ptgather::ItemSpan s = ptgather::item_span(first, m, D);
  out[0] = s.item0; out[1] = s.items; out[2] = s.done0; out[3] = s.done1;
}
int gth_item_valid(const PtGatherPoint* p, int kind) { return ptgather::item_valid(*p, kind) ? 1 : 0; }
float gth_stratum(uint32_t j, uint32_t D) { return ptgather::stratum(j, D); }
float gth_turn(uint32_t j) { return ptgather::turn(j); }
void gth_unit_normal(const float n[3], float z[3]) { ptgather::unit_normal(n, z); }
// ray j of an item: 8 floats {origin, pad, direction, pad}
void gth_ray(const PtGatherPoint* p, int kind, uint32_t j, uint32_t D, float s, float c, float out[8]) {
  const PtRay r = ptgather::ray_of(*p, kind, j, D, s, c);
  std::memcpy(out, &r, sizeof r);
}
void gth_basis(const float w[3], float Y[9]) { ptgather::sh_basis(w, Y); }
// an item's record from its D records; sc: 2 D floats, (sin, cos) of 2 pi turn(j); out: 4 or 28 floats
void gth_reduce(int kind, const PtRayRadiance* rec, uint32_t D, const float* sc, float* out) { ptgather::reduce_item(kind, rec, D, sc, out); }

// the sweep (tests/gather_sweep.hpp)
uint32_t gth_sweep_normals(float* out) {
  const auto& v = gathersweep::normals();
  if (out)
    for (size_t i = 0; i < v.size(); i++) std::memcpy(out + 3 * i, v[i].n, sizeof v[i].n);
  return (uint32_t)v.size();
}
uint32_t gth_sweep_counts(uint32_t* out) {
  const auto& v = gathersweep::direction_counts();
  if (out)
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
  return (uint32_t)v.size();
}
void gth_sweep_records(uint32_t D, int with_nan, PtRayRadiance* out) {
  const std::vector<PtRayRadiance> r = gathersweep::records(D, with_nan != 0);
  std::memcpy(out, r.data(), r.size() * sizeof(PtRayRadiance));
}

// the set
void alloc_fail_at(long k) { g_allocs = 0; g_fail_at = k; }
long alloc_live() { return g_live; }
ptbuf::GatherSet* set_new() { return new ptbuf::GatherSet(); }
void set_delete(ptbuf::GatherSet* s) { delete s; }
int set_fit(ptbuf::GatherSet* s, uint64_t pix) { return s->fit(ptbuf::Extent(pix, 1, 1)).ok() ? 0 : 1; }
int set_in_place(const ptbuf::GatherSet* s, uint64_t pix) { return s->in_place(ptbuf::Extent(pix, 1, 1)) ? 1 : 0; }
void set_release(ptbuf::GatherSet* s) { s->release(); }
uint64_t set_capacity(const ptbuf::GatherSet* s) { return s->work.capacity(); }
// the offsets, in floats, of the carry slot batches 0 .. 3 write
void set_carry_slots(const ptbuf::GatherSet* s, uint64_t out[4]) {
  for (uint32_t k = 0; k < 4; k++) out[k] = (uint64_t)(s->carry(k) - s->carry(0));
}
// the layout for an extent, in floats from the buffer's start: {points, records, end}
void set_layout(const ptbuf::GatherSet* s, uint64_t pix, uint64_t out[3]) {
  const ptbuf::Extent e(pix, 1, 1);
  out[0] = (uint64_t)(s->points() - s->carry(0));
  out[1] = (uint64_t)(s->records(e) - s->carry(0));
  out[2] = ptbuf::GatherSet::floats(e);
}
}
