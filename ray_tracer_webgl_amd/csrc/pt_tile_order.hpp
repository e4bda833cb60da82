// pt_tile_order.hpp — what the host knows about the work queue's tile order (d_tile_order) and the costs it is sorted by
// (d_tile_cost): whether the order kernel has to run before a launch, whether the frames' cost-sorted order has to be probed
// again.  Host only: no HIP, no context, so tests/tile_order_shim.cpp can pin every transition.  The API side reports what it
// enqueued and asks what to enqueue next; the order kernel, the clearing of the costs and the probe launch stay there.
// Scheduling only: the images are the same bits whatever order the tiles are dealt in, so no rendering test can see a slip here.
//
// The three kinds of launch differ in when the order kernel runs and in whether a captured one counts as run.  The differences
// are the code's history, kept as they were found:
//   uniform (pt_render_passes)   runs iff the launch reports costs or no order is in place; a CAPTURED order kernel has not run, so
//                                it changes nothing here and the next direct launch runs its own
//   frames (pt_render_frame(s))  runs iff no order is in place; the capture status is NOT consulted (for a caller capturing single
//                                frames the order kernel captured with them counts as run)
//   partial round                runs iff costs are pending or no order is in place (never inside a capture: pt_render_adaptive
//                                refuses one)
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/ptrace.h"

// what of the uniforms the tiles' costs depend on
inline bool same_view(const PtParams& a, const PtParams& b) {
  return memcmp(a.camera_origin, b.camera_origin, sizeof a.camera_origin) == 0 && memcmp(a.horizontal, b.horizontal, sizeof a.horizontal) == 0 &&
         memcmp(a.vertical, b.vertical, sizeof a.vertical) == 0 && memcmp(a.lower_left_corner, b.lower_left_corner, sizeof a.lower_left_corner) == 0 &&
         a.lens_radius == b.lens_radius && a.max_depth == b.max_depth;
}

struct TileOrder {
  // what a frame (series) has to enqueue before its own launches, in this order
  struct FrameStep {
    bool zero_costs = false;    // clear d_tile_cost: the order kernel then writes the identity
    bool order_kernel = false;  // run it, then report order_kernel_ran()
    bool probe = false;         // one pass with the cost feedback on and the order kernel after it, then report probed_for()
  };

  // the buffers were reallocated for another tile count: the device holds the identity order and zero costs
  void reseeded() { valid_ = false; probed_ = false; pending_ = false; }

  // ---- a uniform launch
  bool uniform_wants_order_kernel(bool cost_feedback) const { return cost_feedback || !valid_; }
  void uniform_order_kernel_enqueued(bool capturing) { if (!capturing) order_kernel_ran(); }
  void uniform_traced(bool cost_feedback, bool capturing) { if (cost_feedback && !capturing) pending_ = true; }

  // ---- a partial round (its launch reports no costs and keeps the order it finds)
  bool partial_wants_order_kernel() const { return pending_ || !valid_; }

  // ---- a frame or a series of n_frames (they report no costs either).  Below four samples per pixel frames keep — and, after a
  // probed series, restore — the identity order; from four on they want a cost-sorted one, probed when there is none for this
  // scene, and after the view has changed once 64 frames have been drawn since the last probe.  `capturing()` is asked only when
  // the answer decides something (it is a runtime query on the API side): no probe inside a caller's capture.
  template <class Capturing>
  FrameStep frames(int samples_per_pixel, const PtParams& view, uint64_t scene_gen, uint32_t n_frames, Capturing&& capturing) {
    FrameStep s;
    if (samples_per_pixel < 4) {
      if (probed_) {  // (a probe leaves the costs zero, a uniform launch with cost feedback since then does not: the caller clears them)
        probed_ = false; valid_ = false; pending_ = false;
        s.zero_costs = true;
      }
      s.order_kernel = !valid_;
      return s;
    }
    const bool fresh = probed_ && valid_ && scene_gen_ == scene_gen && (same_view(view_, view) || frames_since_probe_ < 64u);
    frames_since_probe_ += n_frames;  // (also when fresh: frames drawn, not frames probed for)
    if (fresh) return s;
    s.order_kernel = !valid_;
    s.probe = !capturing();
    return s;
  }

  // the order kernel of a frame or a partial round has been enqueued
  void order_kernel_ran() { valid_ = true; pending_ = false; }
  // the probe and its order kernel have been enqueued (valid_ is left alone: the frames' own order kernel came before)
  void probed_for(const PtParams& view, uint64_t scene_gen) {
    probed_ = true; pending_ = false;
    view_ = view; scene_gen_ = scene_gen; frames_since_probe_ = 0;
  }

  bool valid() const { return valid_; }
  bool pending() const { return pending_; }
  bool probed() const { return probed_; }
  uint32_t frames_since_probe() const { return frames_since_probe_; }

 private:
  bool valid_ = false;    // d_tile_order holds an order for the current tile count
  bool pending_ = false;  // a direct launch has reported costs that no order kernel has consumed yet
  bool probed_ = false;   // the order in place was probed for view_ and scene_gen_, frames_since_probe_ frames ago
  PtParams view_{};
  uint64_t scene_gen_ = 0;
  uint32_t frames_since_probe_ = 0;
};
