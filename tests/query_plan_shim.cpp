// query_plan_shim.cpp — csrc/pt_query.hpp (the arithmetic of pt_query_rays) as plain C functions for tests/test_query_plan.py:
// g++, host only, no HIP header.
#include "../ray_tracer_webgl_amd/csrc/pt_query.hpp"

extern "C" {

uint32_t query_n_batches(uint32_t n, uint32_t batch) { return ptq::n_batches(n, batch); }
uint32_t query_batch_rays(uint32_t n, uint32_t batch, uint32_t k) { return ptq::batch_rays(n, batch, k); }
uint32_t query_tile_rows_covered(uint32_t m, uint32_t width) { return ptq::tile_rows_covered(m, width); }
uint32_t query_tiles_covered(uint32_t m, uint32_t width) { return ptq::tiles_covered(m, width); }

int query_ray_valid(const float o[3], const float d[3]) { return ptq::ray_valid(o[0], o[1], o[2], d[0], d[1], d[2]) ? 1 : 0; }

// m rays into planes of `plane` texels each (4 * plane * 16 bytes), as the pack kernel does it
void query_pack(const PtRay* rays, uint32_t m, float* planes, uint32_t plane) {
  for (uint32_t i = 0; i < m; i++) ptq::pack_at(rays, i, reinterpret_cast<ptq::F4*>(planes), plane);
}
// ... and the records out of them, as the unpack kernel does it
void query_unpack(const float* planes, uint32_t plane, uint32_t m, PtRayHit* hits) {
  for (uint32_t i = 0; i < m; i++) ptq::unpack_at(reinterpret_cast<const ptq::F4*>(planes), plane, i, hits);
}
// the four texels of an invalid ray, at texel i of the planes
void query_invalid(float* planes, uint32_t plane, uint32_t i) {
  ptq::F4* p = reinterpret_cast<ptq::F4*>(planes);
  ptq::invalid_texels(p + i, p + plane + i, p + 2 * (size_t)plane + i, reinterpret_cast<ptq::I4*>(p + 3 * (size_t)plane) + i);
}

uint32_t query_sizeof_ray(void) { return (uint32_t)sizeof(PtRay); }
uint32_t query_sizeof_hit(void) { return (uint32_t)sizeof(PtRayHit); }

}  // extern "C"
