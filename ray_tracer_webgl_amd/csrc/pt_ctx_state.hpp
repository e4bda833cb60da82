// pt_ctx_state.hpp — what a context knows about its derived products, and which call takes that knowledge away: the change
// table, the accumulation's host tallies and the effective row partition.  Host only: no HIP, no device call, so
// tests/ctx_state_shim.cpp pins every row and every transition on the CPU.  pt_api.hip reports what happened (changed(c, ...),
// c->tally.<transition>) and does the device work — the memsets, the uploads, the launches — itself.
//
// The table records behaviour as it was found, entry by entry; where an entry looks doubtful a comment says so and DESIGN.md §10
// has a line.  Nothing here decides a pixel: a flag that survives too long serves stale planes or tables to a read-out, one that
// drops too early costs a refused call.
#pragma once
#include <cstdint>

#include "../../include/ptrace.h"

namespace ptstate {

// ---- (a) the change table ------------------------------------------------------------------------------------------------
// The plain flags of a context (pt_ctx::state).  Validity that belongs to a buffer set alone stays inside the set
// (pt_buffers.hpp: feat.valid, hist.valid, hist.ran, est.spp — the set's own fit drops it where it reallocates); the table below
// names feat.valid and hist.valid through the context and does not move them.
struct Flags {
  bool have_spheres = false;      // list, hierarchy and grid are one scene's, wholly installed
  bool have_params = false;       // uniforms of the context's size are in place
  bool uuid_valid = false;        // the three uuid arrays match the scene and structures in place
  bool adapt_valid = false;       // the adaptive tables are those of a partial round of the scene and partition in place
  bool grid_cells_build = false;  // pt_tune measured the grid build that gathers its entries from L2 faster on this scene and view
  uint64_t scene_gen = 0;         // counts installed scenes: the frames' cost-sorted tile order is probed per scene
};

// what a change can drop or establish: one bit per product
enum Product : uint32_t {
  FEAT = 1,      // feat.valid: the feature planes speak for the scene, uniforms and partition in place
  HIST = 2,      // hist.valid: the history is usable
  ADAPT = 4,     // adapt_valid
  UUID = 8,      // uuid_valid
  CELLS = 16,    // grid_cells_build
  SPHERES = 32,  // have_spheres
  PARAMS = 64,   // have_params
  GEN = 128,     // scene_gen moves on: what was probed for the previous scene no longer counts
};

// what a context undergoes (the order of kRows)
enum Change {
  SCENE_DROPPED,           // pt_set_spheres from its first device write on, and again when the install was refused
  SCENE_INSTALLED,         // ... and when everything is in place
  UNIFORMS_SAME_ROWS,      // pt_set_params accepted, same row partition
  ROWS_ASKED,              // pt_set_params for other rows, before its buffers are fitted (a refused fit leaves this much)
  UNIFORMS_OTHER_ROWS,     // ... and once the new partition is in place
  RESIZED,                 // pt_resize
  GRID_REBUILT,            // rebuild_grid (pt_refit_grid, pt_tune): another margin class, other slots
  TILE_COUNT_CHANGED,      // ensure_buffers put a fresh tile order in place
  PARTIAL_ROUND_BEGINS,    // pt_render_adaptive writes its tables
  PARTIAL_ROUND_DONE,      // ... and has enqueued the round that reads them
  REPROJECTED,             // pt_reproject / pt_reproject_estimate: one-shot, the history is used up
  UUIDS_UPLOADED,          // upload_uuids succeeded
  CELLS_BUILD_UNMEASURED,  // pt_tune kept a margin class (or its trial of the build failed or lost)
  CELLS_BUILD_CHOSEN,      // pt_tune puts the build on trial, and leaves it on when it won
  CHANGE_COUNT
};

struct Row { uint32_t drops, makes; };

// ONE ROW PER CHANGE.  What a row does not name keeps its value.
constexpr Row kRows[CHANGE_COUNT] = {
    //                            drops                            establishes
    /* SCENE_DROPPED          */ {SPHERES | UUID | FEAT | HIST,    0},  // (the history's list indices would name other spheres); adapt_valid, grid_cells_build
                                                                        // and scene_gen wait for SCENE_INSTALLED: a REFUSED install keeps them — doubtful for the tables
    /* SCENE_INSTALLED        */ {CELLS | ADAPT | GEN,             SPHERES},  // (cells: a measurement of the previous scene); beside it: geom.reset()
    /* UNIFORMS_SAME_ROWS     */ {FEAT,                            PARAMS},   // the planes speak for the uniforms they were rendered with; the history is left alone
    /* ROWS_ASKED             */ {FEAT | HIST,                     0},  // (the history planes held other rows) — also when the fit is then refused and the old rows stay
    /* UNIFORMS_OTHER_ROWS    */ {FEAT | HIST | ADAPT,             PARAMS},   // beside it: accumulation, estimate and textures cleared, tally.repartitioned()
    /* RESIZED                */ {PARAMS | FEAT | HIST | ADAPT,    0},  // uuid arrays and grid_cells_build are the scene's, not the size's; beside it: a bound
                                                                        // accumulation is let go, then as pt_reset_accum
    /* GRID_REBUILT           */ {UUID | FEAT,                     0},  // uuids are uploaded again when wanted; the history and the adaptive tables name list indices
                                                                        // and tiles, not slots.  grid_cells_build is kept as found — doubtful: it was measured on
                                                                        // another class's grid; beside it: geom.list_paths()
    /* TILE_COUNT_CHANGED     */ {ADAPT,                           0},  // the sets' own fits have dropped feat.valid / hist.valid where they reallocated;
                                                                        // beside it: order.reseeded()
    /* PARTIAL_ROUND_BEGINS   */ {ADAPT,                           0},
    /* PARTIAL_ROUND_DONE     */ {0,                               ADAPT},
    /* REPROJECTED            */ {HIST,                            0},  // feat.valid stays: the planes are the new view's; the estimate is cleared, or carried
    /* UUIDS_UPLOADED         */ {0,                               UUID},
    /* CELLS_BUILD_UNMEASURED */ {CELLS,                           0},
    /* CELLS_BUILD_CHOSEN     */ {0,                               CELLS},
};

// apply a row to a context: anything with the sets `feat` and `hist` of pt_buffers.hpp and a Flags member `state`
template <class Ctx>
void changed(Ctx& c, Change ch) {
  const Row r = kRows[ch];
  auto apply = [r](uint32_t bit, bool& flag) { flag = (flag && !(r.drops & bit)) || (r.makes & bit); };
  apply(FEAT, c.feat.valid);
  apply(HIST, c.hist.valid);
  apply(ADAPT, c.state.adapt_valid);
  apply(UUID, c.state.uuid_valid);
  apply(CELLS, c.state.grid_cells_build);
  apply(SPHERES, c.state.have_spheres);
  apply(PARAMS, c.state.have_params);
  if (r.drops & GEN) c.state.scene_gen++;
}

// ---- (b) the accumulation's host tallies -----------------------------------------------------------------------------------
// What the host knows of the accumulation buffer's contents and of the work enqueued since it was last emptied (pt_ctx::tally;
// PtStats.total_spp / samples / render_launches, and "nothing rendered yet").  The transitions are named after what happened;
// each does what its call site did when the fields were written by hand, and the differences are deliberate:
//   emptied        pt_reset_accum: everything starts over
//   repartitioned  pt_set_params for other rows: the image is gone and so is whatever a replayed graph accumulated, but samples
//                  and launches count WORK DONE and go on counting across partitions (only pt_reset_accum restarts them)
//   own_fresh      ensure_buffers reallocated the own buffer: zeroed texels hold no samples; `captured` stays — a caller's graph
//                  may still replay into the new buffer, and only the device will know
//   rebound        pt_bind_accum, both directions: the contents are the caller's (or zeroed), so counting restarts; `captured`
//                  stays for the same reason (the differences to `repartitioned` are as found)
//   loaded         pt_load_accum: the mirrors FOLLOW the checkpoint — the only transition that sets samples rather than adding,
//                  and launches are not part of a checkpoint
//   uniform_launch pt_render_passes: a captured launch runs as often as its graph is replayed, which the host cannot see — it
//                  only marks `captured`; a direct one counts
//   frames         pt_render_frame / pt_render_frames: frames blend into the textures and never touch the accumulation, so
//                  total_spp is not theirs; a series counts a launch per frame
//   partial_round  pt_render_adaptive's partial launch: pixels hold different sample counts from here on, so total_spp — one
//                  number for every pixel — is left to the device's word (pt_get_stats reads pixel 0)
struct AccumTally {
  uint32_t total_spp = 0;  // samples per pixel enqueued directly (not through graph replays)
  bool captured = false;   // some launch was captured into a hipGraph: only the device knows the spp
  uint32_t launches = 0;
  uint64_t samples = 0;

  void emptied() { *this = AccumTally(); }
  void repartitioned() { total_spp = 0; captured = false; }
  void own_fresh() { total_spp = 0; }
  void rebound() { total_spp = 0; }
  void loaded(uint32_t w, uint64_t pixels) { total_spp = w; samples = (uint64_t)w * pixels; captured = false; }
  void uniform_launch(bool capturing, uint64_t pixels, uint32_t passes, uint32_t spp) {
    if (capturing) { captured = true; return; }
    launches++;
    total_spp += passes * spp;
    samples += pixels * passes * (uint64_t)spp;
  }
  void frames(uint32_t n, uint64_t pixels, uint32_t spp) {
    launches += n;
    samples += (uint64_t)n * pixels * (uint64_t)spp;
  }
  void partial_round(uint64_t active_pixels, uint32_t passes, uint32_t spp) {
    launches++;
    samples += active_pixels * passes * (uint64_t)spp;
  }
  bool nothing_rendered() const { return total_spp == 0 && !captured; }
};

// ---- (c) the effective row partition ---------------------------------------------------------------------------------------
// The rows a set of uniforms names (include/ptrace.h: row y belongs to band (y / band_rows) % band_count): band_count <= 1 or
// band_rows == 0 means EVERY ROW whatever the other fields hold, and that is normalised to {0, 0, 1} — what the reprojection
// kernels' frame and the filters' band_rows argument expect.  pt_host.cpp (pt_local_rows, pt_band_row), abi.py and the kernels
// state the rule in their own languages; the ABI tests pin them to each other.
struct Partition {
  uint32_t rows = 0, index = 0, count = 1;

  Partition() = default;
  Partition(uint32_t band_rows, uint32_t band_index, uint32_t band_count) {
    if (band_count > 1 && band_rows != 0) { rows = band_rows; index = band_index; count = band_count; }
  }
  explicit Partition(const PtParams& p) : Partition(p.band_rows, p.band_index, p.band_count) {}
  bool every_row() const { return rows == 0; }
  bool operator==(const Partition& o) const { return rows == o.rows && index == o.index && count == o.count; }
  bool operator!=(const Partition& o) const { return !(*this == o); }
};

}  // namespace ptstate
