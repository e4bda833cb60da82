// pt_geom_plan.hpp — which way a trace launch reads the sphere list (PT_GEOM_AUTO's autotuner) and which margin class and
// build of the uniform grid it walks: the grid's fit to the view, what a walk kernel stages in the LDS, pt_tune's search
// over the classes and pt_refit_grid's decision.  Host only: no runtime call, no context, so tests/geom_plan_shim.cpp can pin
// it.  The API side does the rebuilds, the launches and the timing and asks this header at every turn.  Scheduling only: the
// images are the same bits whatever it decides.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <optional>
#include <vector>

#include "../../include/ptrace.h"
#include "pt_kernel_args.h"

// ---- the ways to read the list (PT_GEOM_AUTO) ----

// what the choice of a path knows about the scene
struct PathScene {
  uint32_t n_spheres = 0;
  bool have_bvh = false, have_grid = false;
  uint32_t grid_max_cell_entries = 0, grid_n_always = 0;  // (with a grid)
};

struct PathChoice {
  int path = 0;
  int trial = -1;  // k when the launch is the autotune measurement of paths[k]
};

struct PathTuner {
  int policy = PT_GEOM_AUTO;  // PT_OPT_GEOMETRY_PATH
  int tuned = 0;              // the path PT_GEOM_AUTO settled on, 0 while measuring
  int last = PT_GEOM_LDS;     // path of the most recent launch
  int paths[4] = {0, 0, 0, 0};  // the paths this scene can use, in measuring order
  int n_paths = 0;
  int state = 0;  // 0: unmeasured first launch (cold), k in 1..n_paths: the next launch measures paths[k-1], n_paths + 1: all enqueued
  double samples[4] = {0.0, 0.0, 0.0, 0.0};  // camera samples of each enqueued trial

  // the geometry paths a scene can use, in measuring order (the first is also the default while PT_GEOM_AUTO has not decided)
  void list_paths(const PathScene& s) {
    n_paths = 0;
    // The list walks test every sphere for every ray: beside a culling structure they can only win
    // on very short lists (measured: 484 spheres 4x, 10 001 spheres 14x slower than the grid), so
    // beyond 64 spheres PT_GEOM_AUTO does not spend launches on measuring them.
    const bool structured = s.have_bvh || s.have_grid;
    if (s.n_spheres <= PT_MAX_SPHERES_SMALL) paths[n_paths++] = PT_GEOM_SMALL;  // the reference's own scene size
    if (!structured || s.n_spheres <= 64u) {
      if (s.n_spheres <= PT_MAX_SPHERES_LDS && n_paths < 4) paths[n_paths++] = PT_GEOM_LDS;
      if (n_paths < 4) paths[n_paths++] = PT_GEOM_SCALAR;
    }
    // The hierarchy beats the grid where a uniform grid is the wrong structure: a dense clump inside one
    // cell of a sparse field (many entries in a cell), or many spheres too large to be gridded (every ray
    // tests those first).  On an even field the grid won every measurement (config 2: 112 against 185 ms,
    // config 5: 123 against 365), and a trial of the hierarchy costs the first frame of such a scene more
    // than anything else (config 5: two 0.4-s launches): not measured there.
    const bool grid_even = s.have_grid && s.grid_max_cell_entries <= 16u && s.grid_n_always <= 8u;
    if (s.have_bvh && !grid_even && n_paths < 4) paths[n_paths++] = PT_GEOM_BVH;
    if (s.have_grid && n_paths < 4) paths[n_paths++] = PT_GEOM_GRID;
    if (n_paths == 1) tuned = paths[0];  // nothing to measure
  }

  // a new scene: PT_GEOM_AUTO measures again (list_paths follows)
  void reset() { tuned = 0; state = 0; }

  // which way PHASE 1 looks at the sphere list (bit-identical results whichever way): the forced path, or PT_GEOM_AUTO's
  // tuned one / the trial this launch is.  The caller has settled what it could first (settle, below).
  PathChoice choose(const PathScene& s, bool allow_trials, bool roulette) {
    PathChoice ch{policy, -1};
    if (policy == PT_GEOM_AUTO) {
      if (tuned) ch.path = tuned;
      else if (!allow_trials) ch.path = paths[0];
      else if (state == 0) { ch.path = paths[0]; state = 1; }  // cold launch: not measured
      else if (state <= n_paths) { ch.trial = state - 1; ch.path = paths[ch.trial]; }
      else ch.path = paths[0];  // trials still in flight
    }
    // a forced path the scene cannot use falls back to the nearest one it can
    int& path = ch.path;
    if (path == PT_GEOM_GRID && !s.have_grid) path = s.have_bvh ? PT_GEOM_BVH : PT_GEOM_SCALAR;
    if (path == PT_GEOM_BVH && !s.have_bvh) path = PT_GEOM_SCALAR;
    if (path == PT_GEOM_SMALL && s.n_spheres > PT_MAX_SPHERES_SMALL) path = PT_GEOM_SCALAR;
    if (path == PT_GEOM_LDS && s.n_spheres > PT_MAX_SPHERES_LDS) path = PT_GEOM_SCALAR;
    if (roulette && path == PT_GEOM_LDS) path = PT_GEOM_SCALAR;  // the roulette builds exist for the other four ways to read the list
    return ch;
  }

  // trial k was enqueued, measuring that many camera samples
  void enqueued(int k, double n_samples) {
    samples[k] = n_samples;
    state = k + 2;
  }

  // every trial enqueued and nothing settled yet: once their launches have finished, settle
  bool awaiting_times() const { return !tuned && n_paths > 0 && state > n_paths; }

  // keep the path with the lowest time per camera sample (`ms[k]`: trial k's kernel time); on a tie the first
  void settle(const double* ms) {
    double best = 0.0;
    int best_path = 0;
    for (int k = 0; k < n_paths; k++) {
      const double per = ms[k] / (samples[k] > 0 ? samples[k] : 1.0);
      if (best_path == 0 || per < best) { best = per; best_path = paths[k]; }
    }
    tuned = best_path;
  }

  // does pt_tune have a path to decide (by one cold launch and one per trial)?
  bool has_path_to_decide() const { return policy == PT_GEOM_AUTO && n_paths >= 2; }

  bool lists(int path) const {
    for (int k = 0; k < n_paths; k++) if (paths[k] == path) return true;
    return false;
  }

  // can the grid be what the next launch walks?
  bool grid_in_use(bool have_grid) const {
    if (!have_grid) return false;
    if (policy == PT_GEOM_GRID) return true;
    return policy == PT_GEOM_AUTO && (tuned == 0 || tuned == PT_GEOM_GRID);
  }

  // may pt_tune time the grid — forced, or one of PT_GEOM_AUTO's trials?  (Unlike grid_in_use, true also once PT_GEOM_AUTO
  // has settled on another path: pt_tune measures the paths again after the grid.)
  bool grid_tried() const { return policy == PT_GEOM_GRID || (policy == PT_GEOM_AUTO && lists(PT_GEOM_GRID)); }
};

// ---- the grid's margin classes and their fit to the view ----

// The margin classes a grid is built for (d_near / s0: rays that start within (factor - 1) s0 of the scene's middle walk the
// cells; pt_grid.hpp).
constexpr double kNearFactors[] = {2.5, 3.0, 4.0, 5.5, 8.0, 12.0, 16.0};
constexpr int kNearClasses = (int)(sizeof kNearFactors / sizeof kNearFactors[0]);
constexpr double kDefaultNearFactor = 3.0;  // what pt_set_spheres builds for: rays that start within 2 s0 of the scene's middle

// the same class (a grid's near_factor is a float; one built under PT_GRID_DNEAR has a factor outside the table)
inline bool same_class(double a, double b) { return std::fabs(a - b) < 1e-6; }

// The smallest class that covers the camera of `p` with its lens, for a grid of middle c0 and radius s0; 0 = a camera that is
// not finite.  A camera farther out than the largest class gets the largest: its primary rays take the far path as before (it
// sees the scene under a small angle: few of them reach the grid's box).
inline double view_need_factor(const PtParams& p, const float c0[3], float s0) {
  double rho = 0.0, reach = 0.0;
  for (int k = 0; k < 3; k++) {
    const double dk = (double)p.camera_origin[k] - (double)c0[k];
    rho += dk * dk;
    reach += std::fabs((double)p.lens_radius) * (std::fabs((double)p.u[k]) + std::fabs((double)p.v[k]));
  }
  rho = std::sqrt(rho) + reach;
  if (!std::isfinite(rho)) return 0.0;
  const double need = ((rho / 0.9999 + (double)s0) / (double)s0) * 1.01;
  double factor = kNearFactors[kNearClasses - 1];
  for (double f : kNearFactors) if (f >= need) { factor = f; break; }
  return factor;
}

// Does the grid in place (built for `have`) fit a view that needs `need` (0: no grid in use / no uniforms)?  0 = it fits,
// 1 = too small: the camera stands outside the near region and every primary ray takes the far path, 2 = looser than needed —
// measured against the default class, not against a class BELOW it: whether 2.5 s0 beats 3 s0 depends on where BOUNCE rays
// start (a camera that sees the ground out to the horizon sends them back from beyond any near region), which only a
// measurement knows (pt_tune); a refit never goes below the default.
inline int grid_fit_state(bool in_use, double need, double have) {
  if (!in_use || need <= 0.0) return 0;
  if (have < need - 1e-6) return 1;
  return have > std::max(need, kDefaultNearFactor) + 1e-6 ? 2 : 0;
}

// pt_refit_grid's decision.  policy: 0 = rebuild whenever another class fits better, 1 = only when the class in place is too
// SMALL; never below the default class either way.  The class to rebuild for, or 0 = leave the grid in place.
inline double refit_factor(int policy, int fit_state, double need) {
  if (fit_state == 0 || (policy == 1 && fit_state != 1)) return 0.0;
  return std::max(need, kDefaultNearFactor);
}

// ---- what a walk kernel stages in the LDS ----

// LDS a walk kernel may fill with its staged scene: what is left beside a 1024-thread workgroup's parked path state
constexpr size_t kWalkLdsMax = (size_t)PT_LDS_ENTRIES(PT_MAX_SPHERES_LDS) * 16;
constexpr size_t walk_lds_room() { return kWalkLdsMax - (size_t)PT_PARK_STRIDE * 4 * 1024; }

struct Staging {
  int kind = 0;      // grid: the build (1 / 2 / 3); hierarchy: what is staged (0 / 1 / 2); pt_trace_table.hpp trace_row makes the kernel's row of it
  size_t bytes = 0;  // staged in the LDS
};

// Which build of the grid kernel a launch gets (PtStats.grid_kernel_build): 1 = cells AND entries staged in the LDS
// (pt_trace_kernel_grid), 2 = the cell records staged, the entries gathered from L2 (…_grid_cells), 3 = nothing staged (…_grid_gmem).
// What fits goes into the LDS — with two exceptions (round 6).  (i) A camera OUTSIDE the near region (grid_fit_state 1: the host
// has not refitted yet) turns every primary ray into a far ray, and the LDS-staged build runs a far ray through the literal loop
// for ONE lane (~12 instructions per sphere of the list), while its siblings hand it to the whole wave, 64 spheres at a time:
// the 1 500-sphere field from five scene radii out renders in 2.2-2.9 ms through the cells build against 8-10 ms (and 0.55 ms once
// refitted).  (ii) pt_tune times both builds on scenes whose entries take a good part of the LDS (fewer workgroups per CU) and
// keeps the faster (`cells_build`; the same field seen from inside: 1.37 against 1.48 ms; config 2, 14 KB of entries: the LDS
// build by 6 %, not measured there).  Scheduling only: the same entries, the same tests, the same bits.
inline Staging grid_staging(uint64_t n_cells, uint32_t n_entries, size_t lds_room, bool cells_build, int fit_state) {
  const size_t need_cells = PT_GRID_LDS_CELLS(n_cells);
  const size_t need_all = need_cells + (size_t)n_entries * 16;
  if (need_all <= lds_room && !cells_build && fit_state != 1) return {1, need_all};
  return need_cells <= lds_room ? Staging{2, need_cells} : Staging{3, 0};
}

// Which WALK the LDS-staged build runs: a grid of one layer of cells along y (pt_grid.hpp collapses a flat axis: a field on a
// ground, configs 2 and 3) gets the two-axis walk of pt_grid_walk.hpp — pt_trace_kernel_grid —, a grid of several layers the
// three-axis one — pt_trace_kernel_grid_layers; both are build 1.  The builds that gather (2, 3) walk three axes whatever the
// grid: no flat scene large enough for them is measured.  The same cells' entries, the same tests, the same bits.
inline bool grid_walk_flat(int build_kind, uint32_t n_layers_y) { return build_kind == 1 && n_layers_y == 1u; }

// the hierarchy: 0 = nodes and slots staged, 1 = the nodes, 2 = nothing
inline Staging hierarchy_staging(uint32_t n_nodes, uint32_t n_slots, size_t lds_room) {
  const size_t need_all = PT_BVH_LDS_BYTES32(n_nodes, n_slots);
  const size_t need_nodes = PT_BVH_LDS_BYTES16(n_nodes);
  if (need_all <= lds_room) return {0, need_all};
  return need_nodes <= lds_room ? Staging{1, need_nodes} : Staging{2, 0};
}

// ---- pt_tune: the grid's class and build ----

// The smallest class that covers the CAMERA is a lower bound, not the answer: bounce rays start wherever the camera's rays end,
// and those that start on an always-tested giant (the ground under a field) beyond the near region and come back into the grid's
// box take the far path — one of them costs what hundreds of walked segments cost (the literal loop over the list for one lane,
// or the whole wave 64 spheres at a time).  Measured on a 1 500-sphere field, camera inside it looking across: the grid for
// 2.5 s0 renders the frame in 1.8 ms, the one for 3 s0 in 0.9 (profiles/r06_ab_runs.txt); on config 5 (camera above the field
// looking down) 2.5 s0 is 3 % faster.  So pt_tune MEASURES (PT_OPT_GRID_FIT 0, the default): one timed launch of the grid walk
// per candidate — the class the camera needs, the default class when that is smaller, and up to two classes wider while the
// launch's own far-ray tally says such rays matter and a wider class keeps winning — and the fastest stays.  PT_OPT_GRID_FIT 1:
// the class the camera needs, unmeasured (no launches).  So is a pt_tune asked for more passes than are reserved.
inline bool grid_class_unmeasured(int fit_mode, uint32_t n_passes, uint32_t reserved_passes) {
  return fit_mode == 1 || n_passes > reserved_passes;
}

// How long a timed launch has to be: long enough to rank grids that differ by 2 % (the device's launch-to-launch spread is
// ~0.5 %), no longer — pt_tune is part of a first frame.  The search's first COLD launch (code load, tile order: never a
// measurement) is ONE pass and doubles as the yardstick: the timed launches get as many passes as make ~4 ms, at most four and
// at most n_passes (config 2: 2 passes, configs 3 and 5: 1; round 6's first version timed 4 passes whatever their length:
// 27 / 90 / 130 ms).  `yard_ms` < 0: no yardstick was taken (the class the camera needs built no grid).
inline uint32_t timed_passes(double yard_ms, uint32_t n_passes) {
  const uint32_t n_most = n_passes < 4u ? n_passes : 4u;
  if (yard_ms < 0.0) return n_most;
  // (an over-estimate: the yardstick carries the code load — so the timed launches come out shorter, never longer)
  const double want = yard_ms > 0.0 ? std::ceil(4.0 / yard_ms) : (double)n_most;
  return want < 1.0 ? 1u : (want > (double)n_most ? n_most : (uint32_t)want);
}

struct ClassProbe {
  double factor, ms, far_share;  // the class, the timed launch's kernel time and the share of its segments that were far rays
};

// The search over the classes, one launch at a time: next() is the class to time (and whether its launch is cold: the first),
// or factor 0 when the search is over and keep() stands; the caller rebuilds the grid, times it and reports the probe — or that
// no grid could be built for the class (not a candidate).
class GridClassSearch {
 public:
  struct Step {
    double factor = 0.0;  // 0: done
    bool cold = false;    // a cold launch of one pass before the timed one (the first: it is also the yardstick)
  };

  explicit GridClassSearch(double need) : need_(need) {}

  Step next() {
    if (stage_ == kNeed) return {need_, true};
    if (stage_ == kDefault) {
      if (need_ < kDefaultNearFactor) return {kDefaultNearFactor, false};
      stage_ = kWiden;
    }
    if (stage_ != kWiden || widened_ >= 2 || probes_.empty()) return {};
    const ClassProbe& b = probes_[best()];
    if (b.far_share < 2e-5) return {};  // (practically no ray takes the far path: a wider class only adds copies)
    for (double f : kNearFactors) {
      bool seen = false;
      for (const ClassProbe& q : probes_) seen = seen || same_class(q.factor, f);
      if (f > b.factor + 1e-6 && !seen) return {f, false};
    }
    return {};
  }

  // the class of the last next() was timed (`probe`), or built no grid (empty)
  void report(const std::optional<ClassProbe>& probe) {
    if (probe) probes_.push_back(*probe);
    if (stage_ == kNeed) { stage_ = kDefault; return; }
    if (stage_ == kDefault) { stage_ = kWiden; return; }
    widened_++;
    if (!probe || probes_[best()].factor != probe->factor) widened_ = 2;  // (no grid for it, or not faster: stop widening)
  }

  bool kept() const { return !probes_.empty(); }
  double keep() const { return probes_[best()].factor; }  // (kept() only)
  double keep_ms() const { return probes_[best()].ms; }

 private:
  enum { kNeed, kDefault, kWiden };
  size_t best() const {  // (the first of equals)
    size_t b = 0;
    for (size_t k = 1; k < probes_.size(); k++) if (probes_[k].ms < probes_[b].ms) b = k;
    return b;
  }
  double need_;
  int stage_ = kNeed, widened_ = 0;
  std::vector<ClassProbe> probes_;
};

// ... and WHICH BUILD walks the kept class (grid_staging): where the staged entries take more than 16 KB of the LDS — fewer
// workgroups per CU — the build that gathers them from L2 is timed against the LDS-staged one (cold first: another kernel, its
// code object's first use), and kept when it is at least 2 % faster
inline bool cells_build_worth_timing(uint32_t n_entries, int build_kind) {
  return (size_t)n_entries * 16 > (size_t)16384 && build_kind == 1;
}
inline bool keep_cells_build(const std::optional<ClassProbe>& cells, double keep_ms) {
  return cells && !(cells->ms > 0.98 * keep_ms);
}
