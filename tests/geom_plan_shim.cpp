// geom_plan_shim.cpp — the geometry-path autotuner and the grid's class and build policy (csrc/pt_geom_plan.hpp) behind C
// entries, for tests/test_geom_plan.py.  Compiled by the tests with g++: the header is host-only arithmetic.
#include "../ray_tracer_webgl_amd/csrc/pt_geom_plan.hpp"

#define GP_API extern "C" __attribute__((visibility("default")))

namespace {
PathScene scene_of(uint32_t n_spheres, int have_bvh, int have_grid, uint32_t max_cell_entries, uint32_t n_always) {
  return {n_spheres, have_bvh != 0, have_grid != 0, max_cell_entries, n_always};
}
}  // namespace

// the paths a new scene lists (out4) and their count; *tuned = what PT_GEOM_AUTO has settled on (a single path: that one)
GP_API int gp_list_paths(uint32_t n_spheres, int have_bvh, int have_grid, uint32_t max_cell_entries, uint32_t n_always, int* out4,
                         int* tuned) {
  PathTuner t;
  t.list_paths(scene_of(n_spheres, have_bvh, have_grid, max_cell_entries, n_always));
  for (int k = 0; k < 4; k++) out4[k] = t.paths[k];
  *tuned = t.tuned;
  return t.n_paths;
}

// A new scene under `policy`, then `n_ops` operations as pt_api.hip performs them: ops[i] 0 / 1 = a launch without / with
// trials allowed (settling first, as prepare_launch does, when the trials' events are `ready`), 2 = every enqueued trial's end
// event has completed, 3 = pt_tune's reset.  A launch that measures trial k enqueues samples[k] camera samples; trial k's kernel
// time is ms[k].  out_path[i] / out_trial[i] per launch (-1 for other ops); out3 = {tuned, state, n_paths} at the end.
GP_API void gp_autotune(uint32_t n_spheres, int have_bvh, int have_grid, uint32_t max_cell_entries, uint32_t n_always, int policy,
                        int roulette, const int* ops, int n_ops, const double* samples, const double* ms, int* out_path,
                        int* out_trial, int* out3) {
  const PathScene s = scene_of(n_spheres, have_bvh, have_grid, max_cell_entries, n_always);
  PathTuner t;
  t.policy = policy;
  t.reset();
  t.list_paths(s);
  bool ready = false;
  for (int i = 0; i < n_ops; i++) {
    out_path[i] = out_trial[i] = -1;
    if (ops[i] == 2) ready = true;
    if (ops[i] == 3) { t.reset(); ready = false; }
    if (ops[i] > 1) continue;
    if (t.policy == PT_GEOM_AUTO && t.awaiting_times() && ready) t.settle(ms);  // (try_finish_tuning)
    const PathChoice ch = t.choose(s, ops[i] == 1, roulette != 0);
    if (ch.trial >= 0) t.enqueued(ch.trial, samples[ch.trial]);
    out_path[i] = ch.path;
    out_trial[i] = ch.trial;
  }
  out3[0] = t.tuned;
  out3[1] = t.state;
  out3[2] = t.n_paths;
}

// out2 = {grid_in_use, grid_tried} of a scene's tuner under `policy` having settled on `tuned`
GP_API void gp_grid_use(uint32_t n_spheres, int have_bvh, int have_grid, uint32_t max_cell_entries, uint32_t n_always, int policy,
                        int tuned, int* out2) {
  PathTuner t;
  t.policy = policy;
  t.list_paths(scene_of(n_spheres, have_bvh, have_grid, max_cell_entries, n_always));
  t.tuned = tuned;
  out2[0] = t.grid_in_use(have_grid != 0);
  out2[1] = t.grid_tried();
}

GP_API double gp_need_factor(const double* origin3, const double* u3, const double* v3, double lens_radius, const double* c03,
                             double s0) {
  PtParams p{};
  float c0[3];
  for (int k = 0; k < 3; k++) {
    p.camera_origin[k] = (float)origin3[k];
    p.u[k] = (float)u3[k];
    p.v[k] = (float)v3[k];
    c0[k] = (float)c03[k];
  }
  p.lens_radius = (float)lens_radius;
  return view_need_factor(p, c0, (float)s0);
}

GP_API int gp_fit_state(int in_use, double need, double have) { return grid_fit_state(in_use != 0, need, have); }

GP_API double gp_refit_factor(int policy, int fit_state, double need) { return refit_factor(policy, fit_state, need); }

GP_API int gp_grid_staging(uint64_t n_cells, uint32_t n_entries, uint64_t lds_room, int cells_build, int fit_state, uint64_t* bytes) {
  const Staging st = grid_staging(n_cells, n_entries, (size_t)lds_room, cells_build != 0, fit_state);
  *bytes = st.bytes;
  return st.kind;
}

GP_API int gp_hierarchy_staging(uint32_t n_nodes, uint32_t n_slots, uint64_t lds_room, uint64_t* bytes) {
  const Staging st = hierarchy_staging(n_nodes, n_slots, (size_t)lds_room);
  *bytes = st.bytes;
  return st.kind;
}

GP_API uint64_t gp_walk_lds_room() { return walk_lds_room(); }

GP_API int gp_classes(double* out) {
  for (int k = 0; k < kNearClasses; k++) out[k] = kNearFactors[k];
  return kNearClasses;
}

GP_API uint32_t gp_timed_passes(double yard_ms, uint32_t n_passes) { return timed_passes(yard_ms, n_passes); }

// pt_tune's grid part as tune_grid_to_view drives the header, against a scripted device.  Class k of kNearFactors builds a grid
// when builds[k] (else the one in place stays), with entries[k] entries in cells[k] cells; a cold launch takes cold_ms[k], a timed
// one ms[k] (cells_ms[k] through the cells build) with far share far[k].  The grid starts at `have`, in use.  log: 3 doubles per
// event, {1, factor, 0} a rebuild, {2, passes, cells build} a launch; returns the number of events.  out3 = {the grid's class at
// the end, the cells build kept, launched}.
GP_API int gp_tune(double need, double have, int fit_mode, uint32_t n_passes, uint32_t reserved_passes, const int* builds,
                   const uint32_t* entries, const uint64_t* cells, const double* cold_ms, const double* ms, const double* cells_ms,
                   const double* far, double* log, double* out3) {
  int n_log = 0;
  double at_factor = have;
  bool cells_build = false, launched = false;
  auto cls = [](double f) { for (int k = 0; k < kNearClasses; k++) if (same_class(kNearFactors[k], f)) return k; return -1; };
  auto event = [&](double a, double b, double c) { log[3 * n_log] = a; log[3 * n_log + 1] = b; log[3 * n_log + 2] = c; n_log++; };
  auto at = [&](double f) { return same_class(f, at_factor); };
  auto rebuild = [&](double f) { if (builds[cls(f)]) { at_factor = f; event(1, f, 0); } };
  auto fit = [&]() { return grid_fit_state(true, need, at_factor); };
  auto finish = [&]() { out3[0] = at_factor; out3[1] = cells_build; out3[2] = launched; return n_log; };
  if (grid_class_unmeasured(fit_mode, n_passes, reserved_passes)) {
    if (!at(need)) rebuild(need);
    return finish();
  }
  uint32_t n_timed = timed_passes(-1.0, n_passes);
  auto measure = [&](double f, bool cold, bool yardstick, std::optional<ClassProbe>* probe) {
    if (!at(f)) rebuild(f);
    if (!at(f)) return;
    const int k = cls(f);
    if (cold) {
      event(2, 1, cells_build);
      if (yardstick) n_timed = timed_passes(cold_ms[k], n_passes);
    }
    event(2, n_timed, cells_build);
    *probe = ClassProbe{f, cells_build ? cells_ms[k] : ms[k], far[k]};
    launched = true;
  };
  GridClassSearch search(need);
  for (GridClassSearch::Step step = search.next(); step.factor != 0.0; step = search.next()) {
    std::optional<ClassProbe> probe;
    measure(step.factor, step.cold, step.cold, &probe);
    search.report(probe);
  }
  if (!search.kept()) return finish();
  const double keep = search.keep();
  if (!at(keep)) rebuild(keep);
  const int k = cls(keep);
  const int kind = grid_staging(cells[k], entries[k], walk_lds_room(), false, fit()).kind;
  if (at(keep) && cells_build_worth_timing(entries[k], kind)) {
    cells_build = true;
    std::optional<ClassProbe> probe;
    measure(keep, true, false, &probe);
    cells_build = keep_cells_build(probe, search.keep_ms());
  }
  return finish();
}
