// buffers_shim.cpp — csrc/pt_buffers.hpp (the context's buffer sets: sizing, ownership, what a failed allocation leaves) in front
// of ctypes for tests/test_buffers.py: CPU only, no HIP.  The device allocator the header asks of its includer is a stand-in
// here: malloc / free with a counter that makes the k-th allocation fail.  tests/buffers_main.cpp includes this file for its
// sanitizer build.
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../ray_tracer_webgl_amd/csrc/pt_buffers.hpp"

namespace {
long g_allocs = 0;   // allocations asked for since alloc_reset, refused ones included
long g_fail_at = 0;  // the g_fail_at-th of them is refused (0: none)
long g_live = 0;     // allocations not yet freed
}  // namespace

int ptbuf::dev_malloc(void** p, size_t bytes) {
  *p = nullptr;
  if (++g_allocs == g_fail_at) return 2;  // (hipErrorOutOfMemory's value; any non-zero code would do)
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

struct Texel { float x, y, z, w; };
static_assert(sizeof(Texel) == 16, "the library's texel is a float4");

// the five members a context holds
struct Sets {
  ptbuf::FrameSet<Texel> frame;
  ptbuf::EstimateSet<Texel> est;
  ptbuf::FeatureSet<Texel> feat;
  ptbuf::QuerySet<Texel> query;
  ptbuf::HistorySet<Texel> hist;
  Texel bound[4];  // what buf_bind binds: never dereferenced
};
enum { SET_FRAME = 0, SET_ESTIMATE, SET_FEATURES, SET_QUERIES, SET_HISTORY, SET_COUNT };
enum { N_BUFFERS = 16 };

inline ptbuf::Fit fit_set(Sets* s, int set, const ptbuf::Extent& e) {
  switch (set) {
    case SET_FRAME: return s->frame.fit(e);
    case SET_ESTIMATE: return s->est.fit(e, s->hist.on);
    case SET_FEATURES: return s->feat.fit(e);
    case SET_QUERIES: return s->query.fit(e);
    default: return s->hist.fit(e);
  }
}
inline bool set_in_place(const Sets* s, int set, const ptbuf::Extent& e) {
  switch (set) {
    case SET_FRAME: return s->frame.in_place(e);
    case SET_ESTIMATE: return s->est.in_place(e, s->hist.on);
    case SET_FEATURES: return s->feat.in_place(e);
    case SET_QUERIES: return s->query.in_place(e);
    default: return s->hist.in_place(e);
  }
}
inline bool* set_flag(Sets* s, int set) {
  switch (set) {
    case SET_ESTIMATE: return &s->est.on;
    case SET_FEATURES: return &s->feat.on;
    case SET_QUERIES: return &s->query.on;
    case SET_HISTORY: return &s->hist.on;
    default: return nullptr;
  }
}
inline void release_set(Sets* s, int set) {
  switch (set) {
    case SET_ESTIMATE: s->est.release(); break;
    case SET_FEATURES: s->feat.release(); break;
    case SET_QUERIES: s->query.release(); break;
    case SET_HISTORY: s->hist.release(); break;
    default: break;
  }
}
// every buffer of every set, in the order tests/test_buffers.py names them: {pointer held, capacity in elements}
inline void all_buffers(const Sets* s, uint64_t* held, uint64_t* cap) {
  int k = 0;
  auto put = [&](const auto& b) { held[k] = b.get() != nullptr; cap[k] = b.capacity(); k++; };
  put(s->frame.own_accum); put(s->frame.slab); put(s->frame.tile_cost); put(s->frame.tile_order);
  put(s->frame.tex[0]); put(s->frame.tex[1]); put(s->frame.canvas); put(s->frame.resolve);
  put(s->est.state); put(s->est.tiles); put(s->est.stage);
  put(s->feat.planes);
  put(s->query.planes); put(s->query.order);
  put(s->hist.planes); put(s->hist.tally);
}

extern "C" {
void alloc_reset() { g_allocs = 0; g_fail_at = 0; }
void alloc_fail_at(long k) { g_allocs = 0; g_fail_at = k; }
long alloc_count() { return g_allocs; }
long alloc_live() { return g_live; }

Sets* buf_new() { return new Sets(); }
void buf_delete(Sets* s) { delete s; }

// fit one set to {pix, tiles, passes}: 0 done, 1 an allocation was refused, 2 refused above the index cap; out2 = {fresh bits, code}
int buf_fit(Sets* s, int set, uint64_t pix, uint64_t tiles, uint64_t passes, uint32_t* out2) {
  const ptbuf::Fit f = fit_set(s, set, ptbuf::Extent(pix, tiles, passes));
  out2[0] = f.fresh;
  out2[1] = (uint32_t)f.err;
  return f.capped ? 2 : (f.err ? 1 : 0);
}
int buf_in_place(const Sets* s, int set, uint64_t pix, uint64_t tiles, uint64_t passes) {
  return set_in_place(s, set, ptbuf::Extent(pix, tiles, passes)) ? 1 : 0;
}
// an option turned on as pt_set_option does it — on, fitted, and released again if the fit was refused — or turned off
int buf_toggle(Sets* s, int set, int on, uint64_t pix, uint64_t tiles, uint64_t passes) {
  if (!on) { release_set(s, set); return 0; }
  *set_flag(s, set) = true;
  const ptbuf::Fit f = fit_set(s, set, ptbuf::Extent(pix, tiles, passes));
  if (!f.ok()) release_set(s, set);
  return f.capped ? 2 : (f.err ? 1 : 0);
}
void buf_buffers(const Sets* s, uint64_t* held16, uint64_t* cap16) { all_buffers(s, held16, cap16); }
// out8 = {est.on, feat.on, query.on, hist.on, est.spp, feat.valid, hist.valid, hist.ran}
void buf_flags(const Sets* s, int32_t* out8) {
  const int32_t v[8] = {s->est.on, s->feat.on, s->query.on, s->hist.on, s->est.spp, s->feat.valid, s->hist.valid, s->hist.ran};
  for (int k = 0; k < 8; k++) out8[k] = v[k];
}
// what only other calls set: the estimate holds passes of 4 samples, the planes and the history speak, a pt_reproject ran
void buf_mark_valid(Sets* s) {
  s->est.spp = 4;
  s->feat.valid = s->hist.valid = s->hist.ran = true;
}
// the accumulation pointer: 0 null, 1 the own buffer's, 2 the caller's bound buffer, 3 anything else (stale); *pixels = accum_pixels
int buf_accum(const Sets* s, uint64_t* pixels) {
  *pixels = s->frame.accum_pixels;
  if (!s->frame.accum) return 0;
  if (s->frame.accum == s->frame.own_accum.get()) return 1;
  return s->frame.accum == s->bound ? 2 : 3;
}
void buf_bind(Sets* s, int on) {
  s->frame.accum_bound = on != 0;
  s->frame.accum = on ? s->bound : nullptr;
  s->frame.accum_pixels = on ? 4 : 0;
}
// the planes' sizing arithmetic by itself (nothing is allocated)
uint64_t buf_plane_texels(uint64_t pix) { return ptbuf::plane_texels(pix); }
int buf_planes_indexable(uint64_t pix) { return ptbuf::planes_indexable(pix) ? 1 : 0; }
}
