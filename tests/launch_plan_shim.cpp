// launch_plan_shim.cpp — the trace launch's queue and grid policy (csrc/pt_launch_plan.hpp) behind a C entry, for
// tests/test_launch_plan.py.  Compiled by the tests with g++: the header is host-only integer arithmetic.
#include "../ray_tracer_webgl_amd/csrc/pt_launch_plan.hpp"

// knob_mask bit i set = knob i overridden with knob_vals[i] (as read_launch_knobs assigns atoi's result), in the order
// PT_COOP_MAX, PT_PER_CU, PT_QUEUE_CHUNK, PT_GRID_PERCENT, PT_QUEUE_STATIC, PT_COST_FEEDBACK, PT_FEWER_X10_1,
// PT_FEWER_X10_2, PT_QUEUE_GROUPED.  out7 = {queue_chunk, queue_static, queue_groups, grid, n_waves, cost_feedback,
// coop_max_live}.
extern "C" __attribute__((visibility("default"))) int launch_plan(
    uint64_t items, int spp, uint32_t passes, uint32_t block, int per_cu, uint32_t num_cus, int walk, uint32_t n_spheres,
    uint32_t knob_mask, const int* knob_vals, uint32_t* out7) {
  LaunchPlanIn in;
  in.items = items;
  in.spp = spp;
  in.passes = passes;
  in.block = block;
  in.per_cu = per_cu;
  in.num_cus = num_cus;
  in.walk = walk != 0;
  in.n_spheres = n_spheres;
  LaunchKnobs& k = in.knobs;
  auto knob = [&](int i, auto& field) { if ((knob_mask >> i) & 1u) field = knob_vals[i]; };
  knob(0, k.coop_max);
  knob(1, k.per_cu);
  knob(2, k.queue_chunk);
  knob(3, k.grid_percent);
  knob(4, k.queue_static);
  knob(5, k.cost_feedback);
  knob(6, k.fewer_x10_1);
  knob(7, k.fewer_x10_2);
  knob(8, k.queue_grouped);
  const LaunchPlan P = plan_launch(in);
  const uint32_t out[7] = {P.queue_chunk, (uint32_t)P.deal, P.queue_groups, P.grid, P.n_waves, P.cost_feedback, P.coop_max_live};
  for (int i = 0; i < 7; i++) out7[i] = out[i];
  return 0;
}

extern "C" __attribute__((visibility("default"))) uint32_t launch_list_block_threads(uint64_t lds) {
  return list_block_threads(lds);
}
