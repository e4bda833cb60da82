// ctx_state_shim.cpp — csrc/pt_ctx_state.hpp (the change table, the accumulation's host tallies, the effective row partition) in
// front of ctypes for tests/test_ctx_state.py: CPU only, no HIP.  The context is a stand-in made of the real sets of
// csrc/pt_buffers.hpp plus the header's Flags; nothing is ever allocated, so the allocator the sets ask of their includer refuses.
// tests/ctx_state_main.cpp includes this file for its sanitizer build.
#include <cstddef>
#include <cstdint>

#include "../ray_tracer_webgl_amd/csrc/pt_buffers.hpp"
#include "../ray_tracer_webgl_amd/csrc/pt_ctx_state.hpp"

int ptbuf::dev_malloc(void** p, size_t) { *p = nullptr; return 2; }
int ptbuf::dev_free(void*) { return 0; }

struct Texel { float x, y, z, w; };

// what changed() needs of a context, and the sets' other fields, which no change may touch
struct Ctx {
  ptbuf::EstimateSet<Texel> est;
  ptbuf::FeatureSet<Texel> feat;
  ptbuf::HistorySet<Texel> hist;
  ptstate::Flags state;
};

// the flags as the tests number them: bit 0 feat.valid, 1 hist.valid, 2 adapt_valid, 3 uuid_valid, 4 grid_cells_build,
// 5 have_spheres, 6 have_params
enum { N_FLAGS = 7 };
inline void set_flags(Ctx& c, uint32_t bits) {
  c.feat.valid = bits & 1u; c.hist.valid = bits & 2u; c.state.adapt_valid = bits & 4u; c.state.uuid_valid = bits & 8u;
  c.state.grid_cells_build = bits & 16u; c.state.have_spheres = bits & 32u; c.state.have_params = bits & 64u;
}
inline uint32_t get_flags(const Ctx& c) {
  return (c.feat.valid ? 1u : 0u) | (c.hist.valid ? 2u : 0u) | (c.state.adapt_valid ? 4u : 0u) | (c.state.uuid_valid ? 8u : 0u) |
         (c.state.grid_cells_build ? 16u : 0u) | (c.state.have_spheres ? 32u : 0u) | (c.state.have_params ? 64u : 0u);
}
// everything else a change could reach: every option on, the estimate holding passes of 4 samples, a pt_reproject's tallies in place
inline void set_rest(Ctx& c) {
  c.est.on = c.feat.on = c.hist.on = c.hist.ran = true;
  c.est.spp = 4;
  c.state.scene_gen = 41;
}
inline bool rest_kept(const Ctx& c) { return c.est.on && !c.est.paused && c.feat.on && c.hist.on && c.hist.ran && c.est.spp == 4; }

enum TallyOp { T_EMPTIED, T_REPARTITIONED, T_OWN_FRESH, T_REBOUND, T_LOADED, T_UNIFORM, T_FRAMES, T_PARTIAL };
inline void tally_op(ptstate::AccumTally& t, int op, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  switch (op) {
    case T_EMPTIED: t.emptied(); break;
    case T_REPARTITIONED: t.repartitioned(); break;
    case T_OWN_FRESH: t.own_fresh(); break;
    case T_REBOUND: t.rebound(); break;
    case T_LOADED: t.loaded((uint32_t)a, b); break;                                  // w, pixels
    case T_UNIFORM: t.uniform_launch(a != 0, b, (uint32_t)c, (uint32_t)d); break;    // capturing, pixels, passes, spp
    case T_FRAMES: t.frames((uint32_t)a, b, (uint32_t)c); break;                     // n, pixels, spp
    default: t.partial_round(a, (uint32_t)b, (uint32_t)c); break;                    // active pixels, passes, spp
  }
}

inline ptstate::Partition partition_of(uint32_t rows, uint32_t index, uint32_t count) {
  PtParams p{};
  p.band_rows = rows; p.band_index = index; p.band_count = count;
  return ptstate::Partition(p);
}

extern "C" {
int ctx_change_count() { return ptstate::CHANGE_COUNT; }

// one change applied to a context whose flags are `bits`: out3 = {the flags after, scene_gen after (41 before), 1 if nothing
// else of the sets moved}
void ctx_changed(int change, uint32_t bits, uint64_t* out3) {
  Ctx c;
  set_flags(c, bits);
  set_rest(c);
  ptstate::changed(c, (ptstate::Change)change);
  out3[0] = get_flags(c);
  out3[1] = c.state.scene_gen;
  out3[2] = rest_kept(c) ? 1 : 0;
}

// one transition from state4 = {total_spp, captured, launches, samples}, in place; returns nothing_rendered() afterwards
int tally_apply(uint64_t* state4, int op, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  ptstate::AccumTally t;
  t.total_spp = (uint32_t)state4[0]; t.captured = state4[1] != 0; t.launches = (uint32_t)state4[2]; t.samples = state4[3];
  tally_op(t, op, a, b, c, d);
  state4[0] = t.total_spp; state4[1] = t.captured; state4[2] = t.launches; state4[3] = t.samples;
  return t.nothing_rendered() ? 1 : 0;
}

// the partition PtParams{band_rows, band_index, band_count} names, normalised; returns every_row()
int partition_get(uint32_t rows, uint32_t index, uint32_t count, uint32_t* out3) {
  const ptstate::Partition p = partition_of(rows, index, count);
  out3[0] = p.rows; out3[1] = p.index; out3[2] = p.count;
  return p.every_row() ? 1 : 0;
}
// 1: == holds and != does not; 0: the reverse; -1: the two operators disagree
int partition_equal(uint32_t r0, uint32_t i0, uint32_t c0, uint32_t r1, uint32_t i1, uint32_t c1) {
  const ptstate::Partition a = partition_of(r0, i0, c0), b = partition_of(r1, i1, c1);
  if ((a == b) == (a != b)) return -1;
  return a == b ? 1 : 0;
}
}
