// glare_shim.cpp — csrc/pt_glare.hpp (the glare pyramid's statements, level sizes, option check and host loop) and the GlareSet of
// csrc/pt_buffers.hpp in front of ctypes for tests/test_glare_ref.py: CPU only, no HIP; built with -ffp-contract=off, as the library
// is.  The device allocator pt_buffers.hpp asks of its includer is a stand-in, as in tests/buffers_shim.cpp: malloc / free with a
// counter that makes the k-th allocation fail.
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../ray_tracer_webgl_amd/csrc/pt_buffers.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_glare.hpp"

namespace {
long g_allocs = 0;   // allocations asked for since alloc_fail_at, refused ones included
long g_fail_at = 0;  // the g_fail_at-th of them is refused (0: none)
long g_live = 0;     // allocations not yet freed
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

typedef ptbuf::GlareSet<ptglare::F4> Set;

extern "C" {
// the whole glare of a (w, h) image: 0 done, 1 the options are refused
int glare_run(const float* src, uint32_t w, uint32_t h, int from_accum, const PtGlareOptions* o, float* out) {
  if (!ptglare::options_valid(*o)) return 1;
  std::vector<ptglare::F4> scratch(ptglare::pyramid_texels(w, h, o->levels));
  ptglare::run(reinterpret_cast<const ptglare::F4*>(src), w, h, from_accum != 0, *o, reinterpret_cast<ptglare::F4*>(out), scratch.data());
  return 0;
}
int glare_options_valid(const PtGlareOptions* o) { return ptglare::options_valid(*o) ? 1 : 0; }
uint32_t glare_level_size(uint32_t n, uint32_t k) { return ptglare::level_size(n, k); }
uint64_t glare_pyramid_texels(uint32_t w, uint32_t h, uint32_t levels) { return ptglare::pyramid_texels(w, h, levels); }

void alloc_fail_at(long k) { g_allocs = 0; g_fail_at = k; }
long alloc_live() { return g_live; }
Set* set_new() { return new Set(); }
void set_delete(Set* s) { delete s; }
// the option turned on as pt_set_option does it — on, fitted, released again if the fit was refused — or turned off: 0 / 1 refused
int set_toggle(Set* s, int on, uint32_t width, uint32_t rows) {
  if (!on) { s->release(); return 0; }
  s->on = true;
  const ptbuf::Fit f = s->fit(width, rows);
  if (!f.ok()) s->release();
  return f.ok() ? 0 : 1;
}
// a refit, as ensure_buffers does it: 0 / 1 refused; *fresh = the fresh bits
int set_fit(Set* s, uint32_t width, uint32_t rows, uint32_t* fresh) {
  const ptbuf::Fit f = s->fit(width, rows);
  *fresh = f.fresh;
  return f.ok() ? 0 : 1;
}
int set_in_place(const Set* s, uint32_t width, uint32_t rows) { return s->in_place(width, rows) ? 1 : 0; }
int set_on(const Set* s) { return s->on ? 1 : 0; }
uint64_t set_capacity(const Set* s) { return s->pyramid.capacity(); }
int set_held(const Set* s) { return s->pyramid.get() != nullptr; }
uint64_t set_texels(uint32_t width, uint32_t rows) { return Set::texels(width, rows); }
}
