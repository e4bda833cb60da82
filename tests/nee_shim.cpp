// nee_shim.cpp — csrc/pt_nee.hpp (next-event estimation's statements and the light table), the side table of
// csrc/pt_nee_table.hpp and the LightSet of csrc/pt_buffers.hpp in front of ctypes for tests/test_nee_ref.py: CPU only, no HIP;
// built with -ffp-contract=off, as the library is.  The device allocator pt_buffers.hpp asks of its includer is a stand-in, as in
// tests/buffers_shim.cpp: malloc / free with a counter that makes the k-th allocation fail.
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../ray_tracer_webgl_amd/csrc/pt_buffers.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_kernel_args.h"
#include "../ray_tracer_webgl_amd/csrc/pt_nee.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_nee_table.hpp"
#include "nee_sweep.hpp"

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

typedef ptbuf::LightSet<ptnee::Light> Set;

extern "C" {
// the table of a PtSphere list, made as pt_set_spheres makes it (the kernels' {centre, r * r} record and the shading record);
// out holds n records of 8 words; returns L
uint32_t nee_lights(const PtSphere* s, uint32_t n, ptnee::Light* out) {
  float* geom = static_cast<float*>(std::malloc((n ? n : 1) * 4 * sizeof(float)));
  PtMatRec* mat = static_cast<PtMatRec*>(std::calloc(n ? n : 1, sizeof(PtMatRec)));
  for (uint32_t i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) { geom[4 * i + k] = s[i].center[k]; mat[i].albedo[k] = s[i].albedo[k]; }
    geom[4 * i + 3] = s[i].radius * s[i].radius;
    mat[i].type = s[i].type;
    mat[i].radius = s[i].radius;
  }
  const uint32_t L = ptnee::lights_of(geom, mat, n, out);
  std::free(geom);
  std::free(mat);
  return L;
}
int nee_choose(float u0, int L) { return ptnee::choose(u0, L); }
// steps 5 .. 9 for light {c, r2} at x with normal n and the draw (u1, sin, cos): out = {P, d2, omega.xyz, om, cos_s, wgt}
void nee_sample(const float x[3], const float n[3], const float c[3], float r2, int L, float u1, float s, float co, float out[8]) {
  float w[3], d2;
  std::memset(out, 0, 8 * sizeof(float));
  const bool P = ptnee::reach(x, c, r2, w, d2);
  out[0] = P ? 1.0f : 0.0f;
  out[1] = d2;
  if (!P) return;
  float om;
  ptnee::sample(w, d2, r2, u1, s, co, out + 2, om);
  out[5] = om;
  out[6] = ptnee::cos_at(n, out + 2);
  out[7] = ptnee::weight(L, om, out[6]);
}
void nee_add(float sum[3], const float throughput[3], const float albedo[3], float wgt) { ptnee::add(sum, throughput, albedo, wgt); }

// the sweep (tests/nee_sweep.hpp): its length, and case i as 14 floats {x, n, c, r2, L, u0, u1, u2}
uint32_t nee_sweep_count(void) { return (uint32_t)neesweep::cases().size(); }
void nee_sweep_read(float* out) {
  for (const neesweep::Case& k : neesweep::cases()) {
    const float v[14] = {k.x[0], k.x[1], k.x[2], k.n[0], k.n[1], k.n[2], k.c[0], k.c[1], k.c[2], k.r2, (float)k.L, k.u0, k.u1, k.u2};
    std::memcpy(out, v, sizeof v);
    out += 14;
  }
}

// the side table: a row's cell
int nee_rows(void) { return ROW_COUNT; }
int nee_cell(int row, int* object, int* id, int* waves, const char** name) {
  if (row < 0 || row >= ROW_COUNT) return 1;
  const TraceCell& k = kNeeKernels[row];
  *object = k.object; *id = k.id; *waves = k.waves; *name = k.name;
  return 0;
}
int nee_plain_waves(int row) { return kTraceKernels[row][BUILD_PLAIN].waves; }
int nee_rr_id(int row) { return kTraceKernels[row][BUILD_RR].id; }
const char* nee_rr_name(int row) { return kTraceKernels[row][BUILD_RR].name; }
int nee_obj_count(void) { return OBJ_COUNT; }
int nee_build_value(void) { return BUILD_NEXT_EVENT; }
int nee_build_count(void) { return BUILD_COUNT; }
int nee_takes_cell(int on, int build) { return takes_nee_cell(on != 0, build) ? 1 : 0; }

// the set
void alloc_fail_at(long k) { g_allocs = 0; g_fail_at = k; }
long alloc_live() { return g_live; }
Set* set_new() { return new Set(); }
void set_delete(Set* s) { delete s; }
void set_on(Set* s, int on) { if (on) s->on = true; else s->release(); }
int set_fit(Set* s, uint32_t n) { return s->fit(n).ok() ? 0 : 1; }
int set_in_place(const Set* s) { return s->in_place() ? 1 : 0; }
uint32_t set_n(const Set* s) { return s->n; }
uint64_t set_capacity(const Set* s) { return s->table.capacity(); }
}
