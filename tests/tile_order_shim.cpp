// tile_order_shim.cpp — the host's state of the work queue's tile order (csrc/pt_tile_order.hpp) behind a C entry, for
// tests/test_tile_order.py.  Compiled by the tests with g++: the header is host only.  Each event is reported and answered the way
// pt_api.hip does it: ask, "enqueue", report.
#include "../ray_tracer_webgl_amd/csrc/pt_tile_order.hpp"

enum { EV_RESEED, EV_UNIFORM, EV_FRAMES, EV_PARTIAL, EV_NEW_SCENE };

// the uniforms of view `id`: 0 the base view; 1-6 differ from it in one field of the view each; 7 differs in fields that are not
// part of the view; 8 has -0.0 where the base has +0.0 (equal as numbers, another view bytewise)
static PtParams view_params(int id) {
  PtParams p;
  memset(&p, 0, sizeof p);
  p.camera_origin[1] = 2.0f; p.horizontal[0] = 4.0f; p.vertical[1] = 3.0f; p.lower_left_corner[2] = -1.0f;
  p.lens_radius = 0.1f; p.max_depth = 6; p.samples_per_pixel = 4;
  if (id == 1) p.camera_origin[2] = 1.0f;
  if (id == 2) p.horizontal[1] = 1.0f;
  if (id == 3) p.vertical[0] = 1.0f;
  if (id == 4) p.lower_left_corner[0] = 1.0f;
  if (id == 5) p.lens_radius = 0.2f;
  if (id == 6) p.max_depth = 7;
  if (id == 7) { p.time = 9.0f; p.first_pass = 3; p.render_count = 5; p.samples_per_pixel = 25; }
  if (id == 8) p.camera_origin[0] = -0.0f;
  return p;
}

// events: n x 5 ints {kind, a, b, c, d} — EV_UNIFORM: a = cost feedback, b = capturing; EV_FRAMES: a = samples per pixel,
// b = view id, c = frames, d = capturing.  out: n x 7 {order kernel runs, costs zeroed, probe runs; then the state afterwards:
// valid, pending, probed, frames_since_probe}.  The state lives for one call: a fresh context per sequence.
extern "C" __attribute__((visibility("default"))) int tile_order_run(const int* events, int n, uint32_t* out) {
  TileOrder order;
  uint64_t scene_gen = 0;
  for (int i = 0; i < n; i++) {
    const int* e = events + 5 * i;
    bool kernel = false, zero = false, probe = false;
    switch (e[0]) {
      case EV_RESEED: order.reseeded(); break;
      case EV_NEW_SCENE: scene_gen++; break;
      case EV_UNIFORM:
        kernel = order.uniform_wants_order_kernel(e[1] != 0);
        if (kernel) order.uniform_order_kernel_enqueued(e[2] != 0);
        order.uniform_traced(e[1] != 0, e[2] != 0);
        break;
      case EV_PARTIAL:
        kernel = order.partial_wants_order_kernel();
        if (kernel) order.order_kernel_ran();
        break;
      case EV_FRAMES: {
        const PtParams p = view_params(e[2]);
        const TileOrder::FrameStep s = order.frames(e[1], p, scene_gen, (uint32_t)e[3], [e] { return e[4] != 0; });
        kernel = s.order_kernel; zero = s.zero_costs; probe = s.probe;
        if (kernel) order.order_kernel_ran();
        if (probe) order.probed_for(p, scene_gen);
        break;
      }
      default: return -1;
    }
    uint32_t* o = out + 7 * i;
    o[0] = kernel; o[1] = zero; o[2] = probe;
    o[3] = order.valid(); o[4] = order.pending(); o[5] = order.probed(); o[6] = order.frames_since_probe();
  }
  return 0;
}
