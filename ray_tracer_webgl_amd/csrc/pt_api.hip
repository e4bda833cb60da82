// pt_api.hip — the device-facing entry points of include/ptrace.h: context lifetime, scene and
// uniform upload, kernel launches, read-out, statistics.  Replaces the WebGL2 surface used by
// src/webgl.rs (setup_program :66, create_texture :82, create_framebuffer :153, set_geometry
// :225, Uniforms::run_setters :629, render :180 / draw :169) with HIP on gfx950.
//
// Rules kept here: nothing throws across the C ABI; pt_render* never allocates or synchronises
// (graph-capturable once pt_reserve_passes has sized the workspace); no CPU fallback exists.
#include <hip/hip_runtime.h>

#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ptrace.h"
#include "../../include/ptrace_dev.h"
#include "pt_bvh.hpp"
#include "pt_grid.hpp"
#include "pt_grid_records.hpp"
#include "pt_scene_image.hpp"
#include "pt_extra.h"
#include "pt_sigs.h"
#include "pt_kernel_args.h"
#include "pt_geom_plan.hpp"
#include "pt_launch_plan.hpp"
#include "pt_trace_table.hpp"
#include "pt_nee_table.hpp"
#include "pt_rad_nee_table.hpp"
#include "pt_nee.hpp"
#include "pt_tile_order.hpp"
#include "pt_error_plan.hpp"
#include "pt_reproject_plan.hpp"
#include "pt_reproject.hpp"
#include "pt_query.hpp"
#include "pt_radiance.hpp"
#include "pt_tone.hpp"
#include "pt_glare.hpp"
#include "pt_gather.hpp"
#include "pt_probe.hpp"
#include "pt_buffers.hpp"
#include "pt_ctx_state.hpp"

#define PT_API extern "C" __attribute__((visibility("default")))

// the kernels every context uses are compiled into this object (no -fgpu-rdc needed); the opt-in builds
// (Russian roulette, measuring twins) are the translation unit pt_kernels_extra.hip, the debug-overlay builds
// pt_kernels_debug.hip — code objects of their own, which the HIP runtime loads when one of their kernels is first
// asked for (cell_kernel below)
#include "pt_kernels.hip"

static thread_local std::string g_create_error;

// the allocator of pt_buffers.hpp's DevBuf; its codes are hipError_t values.  A refused allocation is reported by the call that
// asked for it and leaves no error pending for the hipGetLastError() of a later, good launch.
int ptbuf::dev_malloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) (void)hipGetLastError();
  return (int)e;
}
int ptbuf::dev_free(void* p) { return (int)hipFree(p); }
using ptbuf::DevBuf;

// Everything a trace-kernel launch needs, decided from the context's scene and uniforms: the
// argument block, which kernel walks the sphere list, launch geometry.  No HIP call in here that
// enqueues work, allocates or synchronises (capture-safe).
struct Launch {
  PtKernelArgs A;
  const void* kfn = nullptr;
  uint32_t grid = 1, block = 256;
  size_t lds = 0;
  int path = 0;
  int trial = -1;  // k when this launch is the autotune measurement of PathTuner::paths[k]
};

// Everything a frame bakes into its launches: decided BEFORE anything is enqueued (prepare_launch queries
// occupancy and the autotuner's events — not things to do inside a stream capture), and what the cached graph of
// pt_render_frames is keyed on.  Zeroed with memset and compared bytewise, padding included (plan_frame).
struct FramePlan {
  Launch L;
  const uint32_t* ctr = nullptr;  // the device cell holding a frame's number in its series
  uint32_t even_odd0 = 0;
  int max_render_count = 0, render_count0 = 0, should_average = 0;
  float last_frame_weight = 0.f;
  hipStream_t stream = nullptr;
  float4* slab = nullptr;
  uint32_t* tex0 = nullptr; uint32_t* tex1 = nullptr; uint32_t* canvas = nullptr;
  uint32_t n_frames = 1;  // frames traced by the one launch (as its passes), blended one after the other
};

// The scene on the device (pt_set_spheres installs it; pt_scene_image.hpp makes what is uploaded): the sphere list and the two
// culling structures, which tiny and irregular scenes do not get.  Each owns its buffers and keeps its host head.
struct SceneList {
  DevBuf<float> geom, r0;  // r0: PtKernelArgs::mat_r0
  DevBuf<PtMatRec> mat;
  DevBuf<int32_t> uuid;    // n: PtSphere.uuid in list order (debug overlay: upload_uuids)
  uint32_t n = 0;
  ptscene::Split host;     // what was uploaded: pt_tune rebuilds the grid from it (fit_grid_to_view), the uuid arrays are made from it
};
// what the walk kernels read per slot of a structure (index_n slots in use), and whether the structure is in place
struct SceneSlots {
  bool present = false;
  DevBuf<uint32_t> index;  // the slot's sphere
  DevBuf<PtMatRec> mat;    // ... its material
  DevBuf<int32_t> uuid;    // ... its uuid (debug overlay)
  size_t index_n = 0;
};
// (the heads: host copies of the scalars, the arrays released after upload)
struct SceneBvh : SceneSlots { ptbvh::Bvh head; DevBuf<uint32_t> nodes; DevBuf<float> nodes32, slots; };
// ring: a one-layer grid's records once more, in the ring layout the two-axis walk reads (pt_grid_records.hpp); entries: 16 B each
struct SceneGrid : SceneSlots { ptgrid::Grid head; DevBuf<uint32_t> cells, ring; DevBuf<float> entries; };

// pt_shade_probes' kernel form unless pt_debug_probe_form says otherwise: 0 straight loads, 1 the shared-cell way for coherent
// waves (pt_kernels_probe.hip; profiles/r33_probe_lit.txt has the measurement that chose it)
constexpr int kProbeFormDefault = 1;

struct pt_ctx {
  int device = 0;
  uint32_t width = 0, height = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr; // own_stream or the caller's
  // scene
  SceneList list;
  SceneBvh bvh;
  SceneGrid grid;
  // what the context knows of its derived products and of its accumulation (pt_ctx_state.hpp: the plain flags with the table
  // of what each change drops — applied with changed(*c, ...) —, and the host tallies with their named transitions)
  ptstate::Flags state;
  ptstate::AccumTally tally;
  PtParams params{};
  uint32_t local_rows = 0;
  // The buffers sized for the row partition, in five sets, and a sixth of a fixed size (pt_buffers.hpp: what each holds, how it is sized, what a failed
  // allocation leaves; ensure_buffers fits them).  frame: what every context has — the accumulation (own or caller-bound), the
  // per-pass slabs, the work queue's per-tile cost and order (with `order` below), the reference's frame (two RGBA8 textures +
  // canvas) and the read-out staging.  The opt-in sets hold their `on` flag and validity beside their buffers: est
  // (PT_OPT_ERROR_ESTIMATE; pt_kernels_error.hip: the state folded by pt_fold_error_kernel in pt_accumulate_kernel's place, the
  // tile records then their tallies), feat (PT_OPT_FEATURES; pt_kernels_features.hip: written by pt_render_features, which also
  // needs the uuid arrays below), query (PT_OPT_RAY_QUERIES; pt_kernels_query.hip: rays staged into the point and normal planes,
  // records read back from all four; the frame's own tile order belongs to the render launches; pt_query_rays also needs the
  // uuid arrays) and hist (PT_OPT_REPROJECT; pt_kernels_reproject.hip: pt_keep_history / pt_load_history).  expo (PT_OPT_TONEMAP;
  // pt_kernels_display.hip: pt_meter's tallies and the exposure record) is the one set no extent sizes: resizes leave it alone.
  // glare (PT_OPT_GLARE; pt_kernels_glare.hip: pt_glare's pyramid) is sized from the width and the rows in place; scratch, no state.
  ptbuf::FrameSet<float4> frame;
  ptbuf::EstimateSet<float4> est;
  ptbuf::FeatureSet<float4> feat;
  ptbuf::QuerySet<float4> query;
  ptbuf::HistorySet<float4> hist;
  ptbuf::ExposureSet expo;
  ptbuf::GlareSet<float4> glare;
  // the gather queries' workspace (pt_gather_irradiance, pt_bake_probes): fitted by the first call, released with the query planes
  ptbuf::GatherSet gather;
  // the probe lattices' two buffers (pt_bake_lattice's points: released with the query planes; pt_shade_probes' staging of host
  // records: released with the feature planes), each fitted by the first call that needs it; scratch
  ptbuf::ProbeSet probe;
  int probe_form = kProbeFormDefault;   // which shading kernel pt_shade_probes launches (include/ptrace_dev.h pt_debug_probe_form)
  uint32_t* probe_paths = nullptr;      // ... and the caller's per-tile path words, form 1 only
  uint32_t reserved_passes = 1;
  // geometry path (include/ptrace.h PT_GEOM_*): policy, autotune state
  PathTuner geom;
  hipEvent_t trial_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // begin/end per trial
  int grid_fit_mode = 0;  // PT_OPT_GRID_FIT: 0 pt_tune measures the margin classes, 1 it takes the one the camera needs unmeasured
  int count_work = 0; // PT_OPT_COUNT_WORK: launch the measuring twin of the walk kernel
  DevBuf<uint32_t> d_cell_hist;           // grid twins: leaf-round lanes per entry run + coherence bins (pt_debug_cell_hist)
  size_t cell_hist_n = 0;
  DevBuf<unsigned long long> d_wave_log;  // measuring twins: per-wave {start, queue dry, end}
  size_t wave_log_n = 0;
  uint32_t carry_lanes = 12;
  uint32_t refill_min = 4;
  int rr_min_depth = 0;  // PT_OPT_RUSSIAN_ROULETTE: 0 = off (the reference's estimator, bit-exact against the oracle)
  // PT_OPT_NEXT_EVENT: the light table of the scene in place (pt_buffers.hpp LightSet: built when the option comes on over a scene
  // and by pt_set_spheres while it is on, never otherwise)
  ptbuf::LightSet<ptnee::Light> lights;
  // debug overlay (pt_set_debug_overlay): the shader's u_enable_debugging / u_selected_object / u_cursor_point, and the uuids
  // its outline test compares — uploaded when the overlay is first turned on for a scene (upload_uuids), never before
  bool dbg_enable = false;
  int32_t dbg_selected = 0;
  float dbg_cursor[3] = {0.f, 0.f, 0.f};
  int last_build = 0;              // which build the most recent trace launch was (pt_last_trace_build)
  // work-queue ordering feedback, one entry per tile: what the host knows of frame.tile_cost and frame.tile_order
  TileOrder order;  // (pt_tile_order.hpp): when the order kernel runs, when the frames' order is probed
  // adaptive sampling (pt_render_adaptive): a partial round's tables — 3 x tiles words: the flags as uploaded, the partition the
  // trace launch and the masked fold read, the cost order it was made from — and the host's copy of the flags
  DevBuf<uint32_t> d_adapt;
  std::vector<uint32_t> h_adapt_flags;
  uint32_t adapt_tiles = 0, adapt_active = 0;  // (while state.adapt_valid: pt_adaptive_tiles)
  // the reference's frame (pt_render_frame / pt_render_frames): the device-side frame counter ([0] frames replayed since the
  // series began, [1] a cell that stays 0)
  DevBuf<uint32_t> d_frame_ctr;
  // captured frames, one graph per group size (kFrameGroups: 64, 16, 4, 1 frames — a group is ONE trace launch of that many passes,
  // one kernel for their blends, one advance; a single frame is trace + blend + advance), each captured once per plan
  hipGraphExec_t frame_exec[4] = {nullptr, nullptr, nullptr, nullptr};
  FramePlan frame_plan[4];               // the plan each cached graph was captured from (copied and compared bytewise)
  DevBuf<float4> d_frame_slab;           // a group's slabs (up to 16 passes), allocated by the first pt_render_frames that needs them
  // counters + timing
  DevBuf<unsigned long long> d_counters;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events; // pool
  size_t events_used = 0;
  double kernel_ms = 0.0;
  // device properties
  int num_cus = 256;
  // host-clock durations of the set-up calls, ms (include/ptrace_dev.h pt_debug_setup_times: where a first frame's time goes)
  double setup_ms[PT_SETUP_COUNT] = {0};
  std::string error;

  // what the context owns besides its buffers (those free themselves); the caller's stream is left alone
  ~pt_ctx() {
    for (auto& ev : events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (hipEvent_t e : trial_ev) if (e) (void)hipEventDestroy(e);
    for (hipGraphExec_t e : frame_exec) if (e) (void)hipGraphExecDestroy(e);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

namespace {

// the pixels a context owns (its local rows) and the work queue's 8x8 tiles over them
inline size_t n_pixels(const pt_ctx* c) { return (size_t)c->local_rows * c->width; }
inline uint32_t tiles_x(const pt_ctx* c) { return (c->width + 7) / 8; }
inline uint32_t tiles_y(const pt_ctx* c) { return (c->local_rows + 7) / 8; }
inline uint32_t n_tiles(const pt_ctx* c) { return tiles_x(c) * tiles_y(c); }

inline uint32_t grid_for(uint32_t n, uint32_t block, uint32_t cap) {
  uint32_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  return g > cap ? cap : g;
}
// the grid of a kernel that strides 256-thread workgroups over the pixels
inline uint32_t pixel_grid(uint32_t n_pix) { return grid_for(n_pix, 256, 2048); }
// ... and of one whose wave64s take a tile each: four waves, hence four tiles, per 256-thread workgroup
inline uint32_t tile_grid(uint32_t n) { return grid_for(n, 4, 4096); }

// the work queue's heads start a launch at zero: the shared head, or the grouped queue's (pt_refill.hpp)
inline hipError_t zero_queue_heads(pt_ctx* c, uint32_t queue_static) {
  if (queue_static == 2u)
    return hipMemsetAsync(c->d_counters.get() + PT_CTR_GROUP_HEADS, 0, 8 * PT_QUEUE_GROUPS_MAX * sizeof(unsigned long long), c->stream);
  if (queue_static == 0u) return hipMemsetAsync(c->d_counters.get() + PT_CTR_HEAD, 0, sizeof(unsigned long long), c->stream);
  return hipSuccess;
}

inline double host_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int fail(pt_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->error = buf; else g_create_error = buf;
  return code;
}

#define PT_HIP(c, call)                                                                     \
  do {                                                                                      \
    hipError_t e_ = static_cast<hipError_t>(call); /* (DevBuf::reserve hands the code on as an int) */ \
    if (e_ != hipSuccess)                                                                   \
      return fail((c), PT_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
                  __FILE__, __LINE__);                                                      \
  } while (0)

// frames per replayed graph (pt_render_frames; measured on the reference's 1280x702 1-spp frame: 1 / 2 / 4 / 8 / 16 / 32 frames
// per graph -> 8 190 / 12 690 / 18 960 / 21 040 / 21 790 / 21 000 frames per second)
// 960 frames with the group's blends as one kernel: 8 / 12 / 16 / 24 per graph -> 22 640 / 23 020 / 23 940 / 24 250; 16 it is (230 MB of slabs
// at that size), with groups of 4 and single frames for what is left of a series
// frames per replayed graph, largest first.  Round 4 (separate blends, static deal): 1 / 2 / 4 / 8 / 16 / 32 frames -> 8 190 ... 21 790 /
// 21 000 frames per second, hence 16.  Round 5, with the group's launch dealt through the grouped queue and every wave resident
// (bench.py --config default, 1 920 frames): 16 / 24 / 32 / 48 / 64 frames per group -> 28 530 / 29 880 / 30 930 / 31 760 / 32 020:
// a longer launch amortises its start and drain, hence 64 — while its slabs stay below kFrameSlabCap (64 x 1280 x 702 x 16 B =
// 0.92 GB; a 1920x1080 series uses groups of 16: 0.53 GB)
constexpr int kFrameLevels = 4;
#ifdef PT_DEV_KNOBS
static uint32_t kFrameGroups[kFrameLevels] = {64u, 16u, 4u, 1u};
struct FrameGroupKnob { FrameGroupKnob() { if (const char* e = getenv("PT_FRAME_GROUP")) { const uint32_t v = (uint32_t)atoi(e); if (v >= 16u && v <= 128u && v % 16u == 0u) kFrameGroups[0] = v; } } } g_frame_group_knob;
#else
constexpr uint32_t kFrameGroups[kFrameLevels] = {64u, 16u, 4u, 1u};
#endif
constexpr size_t kFrameSlabCap = (size_t)1 << 30;  // bytes a group's slabs may take

uint32_t count_local_rows(uint32_t height, const PtParams& p) {
  return pt_local_rows(height, p.band_rows, p.band_index, p.band_count);
}

// every tile exactly once, in order: what a tile order holds before any cost has sorted it (a blocking copy)
hipError_t fill_identity_order(DevBuf<uint32_t>& order, size_t tiles) {
  std::vector<uint32_t> ident(tiles);
  for (size_t i = 0; i < tiles; i++) ident[i] = (uint32_t)i;
  return hipMemcpy(order.get(), ident.data(), tiles * sizeof(uint32_t), hipMemcpyHostToDevice);
}

// what the context's buffers are sized for: the partition in place
ptbuf::Extent extent_of(const pt_ctx* c) { return {n_pixels(c), n_tiles(c), c->reserved_passes}; }

// a set's fit was refused (`what` names the set): above the planes' index cap nothing was freed, after a failed allocation the
// set is not in place until a later fit succeeds
int fit_refused(pt_ctx* c, const char* what, const ptbuf::Fit& f, const ptbuf::Extent& e) {
  if (f.capped) return fail(c, PT_ERR_CAPACITY, "%s: %zu local pixels exceed the kernels' 32-bit texel index", what, e.pix);
  return fail(c, PT_ERR_HIP, "%s: a device allocation for %zu local pixels failed: %s", what, e.pix, hipGetErrorString((hipError_t)f.err));
}

// The five sets fitted to the partition in place, in their order; what a fit reallocated is zeroed or filled here — also when a
// later buffer of the same set was refused: what is in place is defined.
int ensure_buffers(pt_ctx* c) {
  const ptbuf::Extent e = extent_of(c);
  auto zero = [c](auto& buf, size_t n) { return hipMemsetAsync(buf.get(), 0, n * sizeof(*buf.get()), c->stream); };
  {
    auto& s = c->frame;
    const ptbuf::Fit f = s.fit(e);
    if (f.fresh & s.ACCUM) {
      PT_HIP(c, zero(s.own_accum, e.pix));
      c->tally.own_fresh();
    }
    if (f.fresh & s.COST) PT_HIP(c, zero(s.tile_cost, e.tiles));
    if (f.fresh & s.ORDER) {
      // the identity order from the start: a launch that skips the order kernel (because an earlier one was only
      // CAPTURED into a caller's hipGraph and has not run yet) must still find every tile exactly once
      PT_HIP(c, fill_identity_order(s.tile_order, e.tiles));
      c->order.reseeded();
      changed(*c, ptstate::TILE_COUNT_CHANGED);
    }
    // create_texture x2 (src/webgl.rs:82-123), cleared: alpha 0 = "no data" (shader.frag:391)
    if (f.fresh & s.TEX0) PT_HIP(c, zero(s.tex[0], e.pix));
    if (f.fresh & s.TEX1) PT_HIP(c, zero(s.tex[1], e.pix));
    if (f.fresh & s.CANVAS) PT_HIP(c, zero(s.canvas, e.pix));
    if (!f.ok()) return fit_refused(c, "the context's buffers", f, e);
  }
  {
    // (the stage: pt_reproject_estimate gathers the state from other pixels' places: it cannot write in place, and it does not allocate)
    const ptbuf::Fit f = c->est.fit(e, c->hist.on);
    if (f.fresh & c->est.STATE) PT_HIP(c, zero(c->est.state, 2 * e.pix));
    if (!f.ok()) return fit_refused(c, "error estimate", f, e);
  }
  if (const ptbuf::Fit f = c->feat.fit(e); !f.ok()) return fit_refused(c, "feature planes", f, e);
  {
    if (c->query.on && !c->query.fits(e)) PT_HIP(c, hipStreamSynchronize(c->stream));  // (a query in flight uses what the fit frees)
    const ptbuf::Fit f = c->query.fit(e);
    if (f.fresh & c->query.ORDER) PT_HIP(c, fill_identity_order(c->query.order, e.tiles));
    if (!f.ok()) return fit_refused(c, "query planes", f, e);
  }
  if (const ptbuf::Fit f = c->hist.fit(e); !f.ok()) return fit_refused(c, "history planes", f, e);
  {
    // (fixed size: fresh once, when the option comes on — or again after a refused allocation; no tallies, no record yet)
    const ptbuf::Fit f = c->expo.fit();
    if (f.fresh & c->expo.STATE) PT_HIP(c, zero(c->expo.state, c->expo.kWords));
    if (!f.ok()) return fit_refused(c, "exposure state", f, e);
  }
  // (scratch: a fresh pyramid is not zeroed, every pt_glare writes what it reads)
  if (const ptbuf::Fit f = c->glare.fit(c->width, c->local_rows); !f.ok()) return fit_refused(c, "glare pyramid", f, e);
  return PT_OK;
}

// The contract of the frame set, as the planes have it: in place for the rows in place, or the call is refused.  Asked by every
// trace launch (prepare_launch) and by the entry points that hand the staging, the textures or the canvas to a copy or a kernel
// without one; with the estimate on its state belongs to every render and read-out, and is asked with them.  Host compares only.
int frame_buffers_ready(pt_ctx* c, const char* who) {
  const ptbuf::Extent e = extent_of(c);
  if (c->frame.in_place(e) && (!c->est.on || c->est.in_place(e, c->hist.on))) return PT_OK;
  return fail(c, PT_ERR_CAPACITY, "%s: the context's buffers are not allocated for the rows in place (an earlier allocation failed)", who);
}

// an entry point (`who`) of an opt-in set that is off
enum OptInSet { SET_ESTIMATE, SET_FEATURES, SET_QUERIES, SET_REPROJECT, SET_TONEMAP, SET_GLARE, SET_NEXT_EVENT };
int option_off(pt_ctx* c, const char* who, OptInSet set, int code = PT_ERR_NOT_READY) {
  static const char* const what[] = {"the error estimate is off (pt_set_option PT_OPT_ERROR_ESTIMATE)", "the feature planes are off (pt_set_option PT_OPT_FEATURES)",
                                     "ray queries are off (pt_set_option PT_OPT_RAY_QUERIES)", "reprojection is off (pt_set_option PT_OPT_REPROJECT)",
                                     "tone mapping is off (pt_set_option PT_OPT_TONEMAP)", "the glare is off (pt_set_option PT_OPT_GLARE)",
                                     "next-event estimation is off (pt_set_option PT_OPT_NEXT_EVENT)"};
  return fail(c, code, "%s: %s", who, what[set]);
}

// the error estimate speaks for the passes folded since its last clear: cleared wherever the accumulation is cleared or replaced
int clear_error(pt_ctx* c) {
  if (!c->est.on) return PT_OK;
  const size_t pix = n_pixels(c);
  if (pix) PT_HIP(c, hipMemsetAsync(c->est.state.get(), 0, 2 * pix * sizeof(float4), c->stream));
  c->est.spp = 0;
  return PT_OK;
}

// The accumulation emptied in place and the estimate with it: what pt_reset_accum, a repartition and an unbind share (a bound
// buffer and a checkpoint bring their own texels: pt_bind_accum and pt_load_accum clear the estimate alone).  The tallies'
// transition stays with each caller: some commit it before these fallible clears, others after their last synchronise.
int empty_accum(pt_ctx* c) {
  const size_t pix = n_pixels(c);
  if (c->frame.accum && pix) PT_HIP(c, hipMemsetAsync(c->frame.accum, 0, pix * sizeof(float4), c->stream));
  return clear_error(c);
}

int fold_events(pt_ctx* c) {
  // sum finished event pairs into kernel_ms (requires the stream to be idle)
  for (size_t i = 0; i < c->events_used; i++) {
    float ms = 0.f;
    PT_HIP(c, hipEventElapsedTime(&ms, c->events[i].first, c->events[i].second));
    c->kernel_ms += (double)ms;
  }
  c->events_used = 0;
  return PT_OK;
}

// the next pair of the timing event pool: a new pair while the pool holds fewer than 512, else the pool is drained first
// (this synchronises, but only once per 512 launches)
int next_events(pt_ctx* c, std::pair<hipEvent_t, hipEvent_t>** ev) {
  if (c->events_used == c->events.size()) {
    if (c->events.size() >= 512) {
      PT_HIP(c, hipStreamSynchronize(c->stream));
      int rc = fold_events(c);
      if (rc != PT_OK) return rc;
    } else {
      hipEvent_t a, b;
      PT_HIP(c, hipEventCreate(&a));
      PT_HIP(c, hipEventCreate(&b));
      c->events.emplace_back(a, b);
    }
  }
  *ev = &c->events[c->events_used++];
  return PT_OK;
}

// A timed span of stream work: the next pair of the pool, recorded before and after it.  take() comes before anything of the
// span is enqueued (it may drain the pool); a span that never took a pair — a launch being captured — records nothing.
struct TimedSpan {
  std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
  int take(pt_ctx* c) { return next_events(c, &ev); }
  int begin(pt_ctx* c) const {
    if (ev) PT_HIP(c, hipEventRecord(ev->first, c->stream));
    return PT_OK;
  }
  int end(pt_ctx* c) const {
    if (ev) PT_HIP(c, hipEventRecord(ev->second, c->stream));
    return PT_OK;
  }
};

// is the context's stream being captured into a hipGraph (its own or a caller's)?
bool is_capturing(const pt_ctx* c) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(c->stream, &cap);
  return cap != hipStreamCaptureStatusNone;
}
int not_capturing(pt_ctx* c, const char* who) {
  return is_capturing(c) ? fail(c, PT_ERR_INVALID, "%s: synchronises; not inside a stream capture", who) : PT_OK;
}

// every call that launches needs a scene and uniforms
int scene_and_uniforms(pt_ctx* c, const char* who) {
  if (c->state.have_spheres && c->state.have_params) return PT_OK;
  return fail(c, PT_ERR_NOT_READY, "%s: pt_set_spheres and pt_set_params must come first", who);
}

// the queue order of the tiles from their costs (the identity while every cost is zero)
int launch_tile_order(pt_ctx* c) {
  hipLaunchKernelGGL(pt_tile_order_kernel, dim3(1), dim3(1024), 0, c->stream, c->frame.tile_cost.get(), c->frame.tile_order.get(),
                     n_tiles(c));
  PT_HIP(c, hipGetLastError());
  return PT_OK;
}

// PT_GEOM_AUTO: once every trial launch has finished (non-blocking query), keep the path with
// the lowest time per camera sample.  Images do not depend on the choice.
void try_finish_tuning(pt_ctx* c) {
  if (!c->geom.awaiting_times()) return;
  for (int k = 0; k < c->geom.n_paths; k++)
    if (hipEventQuery(c->trial_ev[2 * k + 1]) != hipSuccess) return;
  double ms[4];
  for (int k = 0; k < c->geom.n_paths; k++) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, c->trial_ev[2 * k], c->trial_ev[2 * k + 1]) != hipSuccess) return;
    ms[k] = (double)t;
  }
  c->geom.settle(ms);
}

PathScene path_scene(const pt_ctx* c) {
  return {c->list.n, c->bvh.present, c->grid.present, c->grid.head.max_cell_entries, c->grid.head.n_always};
}

// the margin class the current uniforms need of the grid (pt_geom_plan.hpp); 0 = no grid / no uniforms / a camera that is not finite
double need_factor(const pt_ctx* c) {
  return c->grid.present && c->state.have_params ? view_need_factor(c->params, c->grid.head.c0, c->grid.head.s0) : 0.0;
}

// does the grid in place fit the view (PtStats.grid_fit_stale, pt_grid_fit)?
int fit_state(const pt_ctx* c) {
  return grid_fit_state(c->geom.grid_in_use(c->grid.present), need_factor(c), (double)c->grid.head.near_factor);
}

// the build of the grid kernel the next launch gets and the bytes it stages (with a grid)
Staging grid_build(const pt_ctx* c) {
  const ptgrid::Grid& g = c->grid.head;
  return grid_staging(ptscene::staged_cells(g), g.n_entries, walk_lds_room(), c->state.grid_cells_build, fit_state(c));
}

// The handle of a table cell's kernel (pt_trace_table.hpp), from its object's accessor.  The first use of a kernel of the five
// opt-in objects (roulette builds and twins, overlay, feature, query and radiance builds) loads that code object and lifts the
// kernel's dynamic-LDS limit, once per device and id; the main kernels' limit is lifted at pt_create, the small-list kernels need none.
const void* cell_kernel(int device, const TraceCell& k) {
#define PT_TRACE_ACCESSOR_OF(object, accessor, n_ids) accessor,
  // (... and behind the table's objects the side tables': the next-event builds, pt_nee_table.hpp, and the radiance-query builds
  // of that estimator, pt_rad_nee_table.hpp)
  static const void* (*const accessors[OBJ_COUNT + 2])(int) = {PT_TRACE_OBJECTS(PT_TRACE_ACCESSOR_OF) pt_nee_kernel, pt_rad_nee_kernel};
  static_assert(OBJ_NEE == OBJ_COUNT && OBJ_RAD_NEE == OBJ_COUNT + 1, "the next-event objects follow the trace table's");
  static std::once_flag once[64][OBJ_COUNT + 2][PT_EXTRA_COUNT];  // (function attributes belong to a device: the context's is current here)
  static_assert(PT_EXTRA_COUNT >= PT_VARIANT_COUNT, "the extra object has the most ids");
  const void* fn = accessors[k.object](k.id);
  if (fn && k.object >= OBJ_EXTRA)
    std::call_once(once[device & 63][k.object][k.id], [fn] {  // (every caller returns with the attribute set: no launch can overtake it)
      (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWalkLdsMax);
      (void)hipGetLastError();  // a refused attribute only limits that kernel to the default 64 KiB; the launch code checks sizes
    });
  return fn;
}

} // namespace

PT_API int pt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

PT_API const char* pt_last_error(pt_ctx* ctx) {
  return ctx ? ctx->error.c_str() : g_create_error.c_str();
}

// pt_create / pt_create_on_stream: `caller_stream` non-NULL = the context runs on the caller's stream from the start and creates
// none of its own (a stream is an HSA queue: 80-150 ms when it is the process's first)
static int create_common(pt_ctx** out, int device, uint32_t width, uint32_t height, void* caller_stream) {
  if (!out) return fail(nullptr, PT_ERR_INVALID, "pt_create: out is NULL");
  *out = nullptr;
  if (width == 0 || height == 0) return fail(nullptr, PT_ERR_INVALID, "pt_create: empty image");
  int n = 0;
  const double t_begin = host_ms();
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(nullptr, PT_ERR_NO_DEVICE,
                "pt_create: no HIP device (libptrace has no CPU backend by design)");
  const double t_runtime = host_ms();  // (the process's first HIP call brings the runtime up)
  if (device < 0 || device >= n)
    return fail(nullptr, PT_ERR_NO_DEVICE, "pt_create: device %d out of range (0..%d)", device, n - 1);
  pt_ctx* c = new (std::nothrow) pt_ctx();
  if (!c) return fail(nullptr, PT_ERR_INVALID, "pt_create: out of host memory");
  c->device = device;
  c->width = width;
  c->height = height;
  c->local_rows = height;
  auto bail = [&](hipError_t e, const char* what) {
    fail(nullptr, PT_ERR_HIP, "pt_create: %s: %s", what, hipGetErrorString(e));
    delete c;  // (frees whatever was made before the failure)
    return PT_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bail(e, "hipGetDeviceProperties");
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  const double t_device = host_ms();
  if (caller_stream) {
    c->stream = (hipStream_t)caller_stream;
  } else {
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess)
      return bail(e, "hipStreamCreateWithFlags");
    c->stream = c->own_stream;
  }
  const double t_stream = host_ms();
  if ((e = (hipError_t)c->d_counters.reserve(PT_CTR_ALLOC)) != hipSuccess) return bail(e, "hipMalloc(counters)");
  const double t_first_malloc = host_ms();
  if ((e = hipMemsetAsync(c->d_counters.get(), 0, PT_CTR_ALLOC * sizeof(unsigned long long), c->stream)) != hipSuccess)
    return bail(e, "hipMemsetAsync(counters)");
  const double t_first_memset = host_ms();
  if ((e = (hipError_t)c->d_frame_ctr.reserve(2)) != hipSuccess) return bail(e, "hipMalloc(frame counter)");
  if ((e = hipMemsetAsync(c->d_frame_ctr.get(), 0, 2 * sizeof(uint32_t), c->stream)) != hipSuccess)
    return bail(e, "hipMemsetAsync(frame counter)");
  const double t_small_allocs = host_ms();
  // allow the trace kernels to use the CU's whole 160 KiB LDS for big sphere lists
  // (the first hipFuncSetAttribute of a process also LOADS this translation unit's code object onto the device)
  for (int id = 0; id < PT_MAIN_COUNT; id++) (void)hipFuncSetAttribute(pt_main_kernel(id), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWalkLdsMax);
  (void)hipGetLastError(); // a refused attribute only limits that kernel to the default 64 KiB; the launch code checks sizes
  const double t_code = host_ms();
  int rc = ensure_buffers(c);
  if (rc != PT_OK) { g_create_error = c->error; delete c; return rc; }
  const double t_end = host_ms();
  c->setup_ms[PT_SETUP_CREATE_RUNTIME] = t_runtime - t_begin;
  c->setup_ms[PT_SETUP_CREATE_DEVICE] = t_device - t_runtime;
  c->setup_ms[PT_SETUP_CREATE_STREAM_ALLOCS] = t_small_allocs - t_device;
  c->setup_ms[PT_SETUP_CREATE_STREAM] = t_stream - t_device;
  c->setup_ms[PT_SETUP_CREATE_FIRST_MALLOC] = t_first_malloc - t_stream;
  c->setup_ms[PT_SETUP_CREATE_FIRST_MEMSET] = t_first_memset - t_first_malloc;
  c->setup_ms[PT_SETUP_CREATE_CODE_OBJECT] = t_code - t_small_allocs;
  c->setup_ms[PT_SETUP_CREATE_BUFFERS] = t_end - t_code;
  c->setup_ms[PT_SETUP_CREATE_TOTAL] = t_end - t_begin;
  *out = c;
  return PT_OK;
}

PT_API int pt_create(pt_ctx** out, int device, uint32_t width, uint32_t height) {
  return create_common(out, device, width, height, nullptr);
}
PT_API int pt_create_on_stream(pt_ctx** out, int device, uint32_t width, uint32_t height, void* hip_stream) {
  return create_common(out, device, width, height, hip_stream);
}

PT_API int pt_destroy(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c;
  return PT_OK;
}

PT_API int pt_set_stream(pt_ctx* c, void* hip_stream) {
  if (!c) return PT_ERR_INVALID;
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  int rc = fold_events(c);
  if (rc != PT_OK) return rc;
  if (!hip_stream && !c->own_stream)  // a context made by pt_create_on_stream that now wants a stream of its own
    PT_HIP(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return PT_OK;
}

namespace {

#define PT_TRY(call) do { if (int rc_ = (call); rc_ != PT_OK) return rc_; } while (0)

// `n` elements of `src` into `buf`, in front of padding up to `n_pad` elements of `pad_byte`: the buffer grows only when it is
// smaller, the padding is written, then the payload (the caller has made sure that nothing in flight reads the buffer)
template <class T>
int upload(pt_ctx* c, DevBuf<T>& buf, const T* src, size_t n, size_t n_pad, int pad_byte) {
  if (buf.capacity() < n_pad) PT_HIP(c, buf.reserve(n_pad));
  if (n_pad > n) PT_HIP(c, hipMemset(buf.get() + n, pad_byte, (n_pad - n) * sizeof(T)));
  if (n) PT_HIP(c, hipMemcpy(buf.get(), src, n * sizeof(T), hipMemcpyHostToDevice));
  return PT_OK;
}
template <class T>
int upload(pt_ctx* c, DevBuf<T>& buf, const std::vector<T>& src) { return upload(c, buf, src.data(), src.size(), src.size(), 0); }
template <class T>
void release(std::vector<T>& v) { std::vector<T>().swap(v); }

// no scene is in place (until an install has wholly succeeded: the render calls answer PT_ERR_NOT_READY meanwhile)
void drop_scene(pt_ctx* c) {
  c->bvh.present = c->grid.present = false;
  changed(*c, ptstate::SCENE_DROPPED);
}

// (list.n and list.host follow when the whole scene is in place: pt_set_spheres)
int install_list(pt_ctx* c, const ptscene::Split& sp, size_t n) {
  PT_TRY(upload(c, c->list.geom, sp.geom));
  PT_TRY(upload(c, c->list.mat, sp.mat.data(), n, n ? n : 1u, 0));
  return upload(c, c->list.r0, sp.r0.data(), 2 * n, n ? 2 * n : 2u, 0);
}

// a structure's index (padding: 0xff, no sphere) and per-slot materials (padding: 0); its uuids follow when the overlay is on (the
// caller has reported the change that ends the uuid arrays' validity: SCENE_DROPPED or GRID_REBUILT)
int install_slots(pt_ctx* c, SceneSlots& s, const std::vector<uint32_t>& index, size_t n, size_t n_pad, const ptscene::Split& sp) {
  s.present = false;  // (until the caller's install has succeeded: a failed allocation must not leave a structure that points nowhere)
  PT_TRY(upload(c, s.index, index.data(), n, n_pad, 0xff));
  s.index_n = n_pad;
  return upload(c, s.mat, ptscene::per_slot(index.data(), n, sp.mat.data(), sp.mat.size()).data(), n, n_pad, 0);
}

// upload a hierarchy / a grid (the caller has made sure that nothing in flight reads the previous one); empties the host arrays
int install_bvh(pt_ctx* c, ptbvh::Bvh& bvh, const ptscene::Split& sp) {
  PT_TRY(install_slots(c, c->bvh, bvh.slot_index, bvh.slot_index.size(), bvh.slot_index.size(), sp));
  PT_TRY(upload(c, c->bvh.nodes, bvh.nodes16));
  PT_TRY(upload(c, c->bvh.nodes32, bvh.nodes32));
  PT_TRY(upload(c, c->bvh.slots, bvh.slots));
  release(bvh.nodes); release(bvh.nodes16); release(bvh.nodes32); release(bvh.slots); release(bvh.slot_index);
  c->bvh.head = std::move(bvh);
  c->bvh.present = true;
  return PT_OK;
}
int install_grid(pt_ctx* c, ptgrid::Grid& grid, const ptscene::Split& sp) {
  // + four entries of slack: a leaf round reads four consecutive entries whatever the cell's
  // count (and lanes without a cell under test read, and discard, wherever their stale record points)
  const size_t n_ent = grid.n_entries, n_ent_pad = n_ent + 4u;
  PT_TRY(install_slots(c, c->grid, grid.entry_index, n_ent, n_ent_pad, sp));
  PT_TRY(upload(c, c->grid.entries, grid.entries.data(), n_ent * 4, n_ent_pad * 4, 0));
  // the device reads derived records (pt_grid_records.hpp): what a leaf round would decode from `first | count << 24`, made once
  std::vector<uint32_t> recs(grid.cells.size());
  for (size_t k = 0; k < recs.size(); k++) recs[k] = ptrec::from_host(grid.cells[k]);
  PT_TRY(upload(c, c->grid.cells, recs.data(), recs.size(), (recs.size() + 3u) & ~(size_t)3u, 0));  // (the kernels stage 16 B at a time)
  if (grid.n[1] == 1u) {  // ... and in the ring layout, for the two-axis walk
    recs.assign(((size_t)ptrec::ring_cells(grid.n[0], grid.n[2]) + 3u) & ~(size_t)3u, ptrec::kOutside);
    ptrec::ring_layout(grid.cells.data(), grid.n[0], grid.n[2], recs.data());
    PT_TRY(upload(c, c->grid.ring, recs));
  }
  release(grid.cells); release(grid.entries); release(grid.entry_index);
  c->grid.head = std::move(grid);
  c->grid.present = true;
  return PT_OK;
}

// The uuid arrays of the debug overlay, of the feature planes and of ray queries: PtSphere.uuid in list order and per slot of the structures in
// place (the walk kernels shade from a slot, like slot_mat).  Made when one of them is turned on and again whenever the scene or the
// grid changes while one is on (wants_uuids); a context that never enables one never allocates them.  Synchronises: a set-up call's work.
inline bool wants_uuids(const pt_ctx* c) { return c->dbg_enable || c->feat.on || c->query.on; }
int upload_uuids(pt_ctx* c, const std::vector<int32_t>& uuid) {
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));  // launches in flight may read the arrays in place
  PT_TRY(upload(c, c->list.uuid, uuid.data(), uuid.size(), uuid.empty() ? 1u : uuid.size(), 0));
  for (SceneSlots* s : std::initializer_list<SceneSlots*>{&c->bvh, &c->grid}) {
    if (!s->present || !s->index_n) continue;
    std::vector<uint32_t> index(s->index_n);  // (read back from the device: the structure's host arrays are gone by now)
    PT_HIP(c, hipMemcpy(index.data(), s->index.get(), index.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    PT_TRY(upload(c, s->uuid, ptscene::per_slot(index.data(), index.size(), uuid.data(), uuid.size())));  // (padding slots are never hit)
  }
  changed(*c, ptstate::UUIDS_UPLOADED);
  return PT_OK;
}

// The light table of PT_OPT_NEXT_EVENT for the list `sp` (pt_nee.hpp lights_of).  The caller has made sure that nothing in flight
// reads the table in place.  A refused allocation leaves the set not in place: render launches are refused until a later build
// succeeds (prepare_launch).
int upload_lights(pt_ctx* c, const ptscene::Split& sp, uint32_t n) {
  std::vector<ptnee::Light> table(n ? n : 1u);
  const uint32_t L = ptnee::lights_of(sp.geom.data(), sp.mat.data(), n, table.data());
  const ptbuf::Fit f = c->lights.fit(L);
  if (!f.ok()) return fail(c, PT_ERR_HIP, "PT_OPT_NEXT_EVENT: no room for the table of %u lights (%s)", L, hipGetErrorString((hipError_t)f.err));
  if (L) PT_HIP(c, hipMemcpy(c->lights.table.get(), table.data(), (size_t)L * sizeof(ptnee::Light), hipMemcpyHostToDevice));
  return PT_OK;
}

// the device half of pt_set_spheres: list, hierarchy, grid, the uuid arrays when the overlay or the feature planes are on, and the
// light table when next-event estimation is
int install_scene(pt_ctx* c, const ptscene::Split& sp, uint32_t n, ptbvh::Bvh* bvh, ptgrid::Grid* grid) {
  PT_TRY(install_list(c, sp, n));
  if (bvh) PT_TRY(install_bvh(c, *bvh, sp));
  if (grid) PT_TRY(install_grid(c, *grid, sp));
  if (c->lights.on) PT_TRY(upload_lights(c, sp, n));
  return wants_uuids(c) ? upload_uuids(c, sp.uuid) : PT_OK;
}

} // namespace

PT_API int pt_set_spheres(pt_ctx* c, const PtSphere* s, uint32_t n) {
  if (!c || (!s && n)) return fail(c, PT_ERR_INVALID, "pt_set_spheres: NULL argument");
  if (n > PT_MAX_SPHERES)
    return fail(c, PT_ERR_CAPACITY, "pt_set_spheres: %u spheres exceed the 16-bit candidate index range (%u)",
                n, PT_MAX_SPHERES);
  PT_HIP(c, hipSetDevice(c->device));
  const double t_begin = host_ms();
  ptscene::Split sp = ptscene::split(s, n);
  const double t_split = host_ms();
  // the culling hierarchy of PT_GEOM_BVH (regular scenes of at least 16 spheres)
  ptbvh::Bvh bvh;
  const bool have_bvh = sp.regular && ptbvh::build(sp.geom.data(), sp.radii.data(), n, &bvh);
  const double t_bvh = host_ms();
  // ... and the uniform grid of PT_GEOM_GRID (same precondition)
  ptgrid::Grid grid;
  const bool have_grid = sp.regular && ptscene::build_grid(sp.geom.data(), sp.radii.data(), n, 3.0, &grid);
  const double t_grid = host_ms();
  // the stream may still be reading the previous scene
  PT_HIP(c, hipStreamSynchronize(c->stream));
  // validate first, commit afterwards: from the first device write until everything is in place the context has no scene
  drop_scene(c);
  if (int rc = install_scene(c, sp, n, have_bvh ? &bvh : nullptr, have_grid ? &grid : nullptr); rc != PT_OK) return drop_scene(c), rc;
  c->list.n = n;
  c->list.host = std::move(sp);
  changed(*c, ptstate::SCENE_INSTALLED);
  c->geom.reset();  // a new scene: PT_GEOM_AUTO measures again
  c->geom.list_paths(path_scene(c));
  const double t_end = host_ms();
  c->setup_ms[PT_SETUP_SPHERES_SPLIT] = t_split - t_begin;
  c->setup_ms[PT_SETUP_SPHERES_BVH_BUILD] = t_bvh - t_split;
  c->setup_ms[PT_SETUP_SPHERES_GRID_BUILD] = t_grid - t_bvh;
  c->setup_ms[PT_SETUP_SPHERES_UPLOAD] = t_end - t_grid;
  c->setup_ms[PT_SETUP_SPHERES_TOTAL] = t_end - t_begin;
  return PT_OK;
}

PT_API int pt_set_params(pt_ctx* c, const PtParams* p) {
  if (!c || !p) return fail(c, PT_ERR_INVALID, "pt_set_params: NULL argument");
  if (p->width != c->width || p->height != c->height)
    return fail(c, PT_ERR_INVALID, "pt_set_params: %ux%u does not match the context's %ux%u (use pt_resize)",
                p->width, p->height, c->width, c->height);
  if (p->samples_per_pixel < 1 || p->max_depth < 1)
    return fail(c, PT_ERR_INVALID, "pt_set_params: samples_per_pixel and max_depth must be >= 1");
  if (p->band_count > 1 && (p->band_rows == 0 || p->band_index >= p->band_count))
    return fail(c, PT_ERR_INVALID, "pt_set_params: bad row partition (rows %u index %u count %u)",
                p->band_rows, p->band_index, p->band_count);
  PT_HIP(c, hipSetDevice(c->device));
  uint32_t rows = count_local_rows(c->height, *p);
  const bool repartition = rows != c->local_rows || ptstate::Partition(*p) != ptstate::Partition(c->params);
  // validate first, commit afterwards: a refused call leaves the context as it was
  if (repartition && c->frame.accum_bound && (size_t)rows * c->width > c->frame.accum_pixels)
    return fail(c, PT_ERR_CAPACITY, "pt_set_params: bound accumulation buffer too small for %u rows", rows);
  if (repartition) {
    changed(*c, ptstate::ROWS_ASKED);
    const uint32_t old_rows = c->local_rows;
    c->local_rows = rows;
    int rc = ensure_buffers(c);
    if (rc != PT_OK) {
      // allocation failed: the previous partition and uniforms stay the context's.  A buffer the failure freed is no longer in
      // place for them either: the render and read-out calls answer PT_ERR_CAPACITY until a sizing call succeeds
      c->local_rows = old_rows;
      return rc;
    }
    // From here on the new partition is in place (buffers sized for it), so the STATE is committed before the fallible
    // clears below: whatever they return, local_rows, params.band_* and the sample count agree with each other
    // (a refused clear leaves a self-consistent context whose old image is gone, never a new partition with old uniforms).
    c->params = *p;
    changed(*c, ptstate::UNIFORMS_OTHER_ROWS);
    c->tally.repartitioned();
    // a different set of rows: the accumulated image no longer applies, and neither do the frame textures
    if (int rc = empty_accum(c); rc != PT_OK) return rc;
    return pt_clear_textures(c);
  }
  c->params = *p;
  changed(*c, ptstate::UNIFORMS_SAME_ROWS);
  return PT_OK;
}

PT_API int pt_resize(pt_ctx* c, uint32_t width, uint32_t height) {
  if (!c || width == 0 || height == 0) return fail(c, PT_ERR_INVALID, "pt_resize: bad size");
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  c->width = width;
  c->height = height;
  changed(*c, ptstate::RESIZED);  // (uniforms must be re-uploaded for the new size)
  c->params.band_count = 0;
  c->local_rows = height;
  if (c->frame.accum_bound) { c->frame.accum_bound = false; c->frame.accum = nullptr; }
  int rc = ensure_buffers(c);
  if (rc != PT_OK) return rc;
  // update_render_dimensions_to_match_window re-specifies both textures as empty on EVERY resize
  // (src/state.rs:382-396), growing or not: alpha 0 = "no data" (static/shader.frag:391)
  rc = pt_clear_textures(c);
  if (rc != PT_OK) return rc;
  return pt_reset_accum(c);
}

PT_API int pt_reserve_passes(pt_ctx* c, uint32_t max_passes) {
  if (!c || max_passes == 0) return fail(c, PT_ERR_INVALID, "pt_reserve_passes: bad argument");
  PT_HIP(c, hipSetDevice(c->device));
  const double t_begin = host_ms();
  const uint32_t reserved = c->reserved_passes;
  if (max_passes > reserved) {
    PT_HIP(c, hipStreamSynchronize(c->stream));
    c->reserved_passes = max_passes;
  }
  const int rc = ensure_buffers(c);
  // a refused reservation leaves the count as it was.  The slab it freed comes back with the next sizing call that succeeds
  // (this one, a repartition, pt_resize); until then the render and read-out calls are refused (frame_buffers_ready).
  if (rc != PT_OK) c->reserved_passes = reserved;
  c->setup_ms[PT_SETUP_RESERVE_TOTAL] = host_ms() - t_begin;
  return rc;
}

PT_API int pt_reset_accum(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipMemsetAsync(c->d_counters.get(), 0, PT_CTR_COUNT * sizeof(unsigned long long), c->stream));
  if (int rc = empty_accum(c); rc != PT_OK) return rc;
  PT_HIP(c, hipStreamSynchronize(c->stream));
  c->events_used = 0;
  c->kernel_ms = 0.0;
  c->tally.emptied();
  return PT_OK;
}

PT_API int pt_bind_accum(pt_ctx* c, void* dev_ptr, size_t bytes) {
  if (!c) return PT_ERR_INVALID;
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  if (!dev_ptr) {
    c->frame.accum_bound = false;
    c->frame.accum = nullptr;
    c->tally.rebound();  // (whatever ensure_buffers answers)
    if (int rc = ensure_buffers(c); rc != PT_OK) return rc;
    // the own buffer comes back EMPTY: what it held when the caller's buffer took its place belongs to another frame — possibly to
    // another row partition, set while it was out of use — and the sample count above has just restarted
    return empty_accum(c);
  }
  size_t need = n_pixels(c) * sizeof(float4);
  if (bytes < need) return fail(c, PT_ERR_CAPACITY, "pt_bind_accum: %zu bytes < %zu needed", bytes, need);
  if (((uintptr_t)dev_ptr & 15u) != 0) return fail(c, PT_ERR_INVALID, "pt_bind_accum: pointer not 16-byte aligned");
  c->frame.accum = (float4*)dev_ptr;
  c->frame.accum_pixels = bytes / sizeof(float4);
  c->frame.accum_bound = true;
  c->tally.rebound();  // the caller owns the contents; spp counting restarts
  return clear_error(c);  // (and so does the estimate: it knows nothing of what the caller's buffer holds)
}

PT_API int pt_accum_ptr(pt_ctx* c, void** dev_ptr, size_t* bytes) {
  if (!c || !dev_ptr) return PT_ERR_INVALID;
  *dev_ptr = c->frame.accum;
  if (bytes) *bytes = n_pixels(c) * sizeof(float4);
  return PT_OK;
}

// Checkpoint / resume of the accumulation state (the reference's accumulation state is its
// ping-pong textures + render_count, src/state.rs:443-450; here: local_rows*width float4 of
// {sum r, sum g, sum b, spp}).  `dst` / `src` may be host or device pointers.
PT_API int pt_read_accum(pt_ctx* c, float* dst, size_t bytes) {
  if (!c || !dst) return fail(c, PT_ERR_INVALID, "pt_read_accum: NULL argument");
  const size_t need = n_pixels(c) * sizeof(float4);
  if (bytes < need) return fail(c, PT_ERR_CAPACITY, "pt_read_accum: %zu bytes < %zu needed", bytes, need);
  PT_HIP(c, hipSetDevice(c->device));
  if (need) PT_HIP(c, hipMemcpyAsync(dst, c->frame.accum, need, hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_load_accum(pt_ctx* c, const float* src, size_t bytes) {
  if (!c || !src) return fail(c, PT_ERR_INVALID, "pt_load_accum: NULL argument");
  const size_t need = n_pixels(c) * sizeof(float4);
  if (bytes != need)
    return fail(c, PT_ERR_INVALID, "pt_load_accum: %zu bytes, the current row partition holds %zu", bytes, need);
  if (int rc = frame_buffers_ready(c, "pt_load_accum"); rc != PT_OK) return rc;
  PT_HIP(c, hipSetDevice(c->device));
  if (need == 0) return PT_OK;
  // validate first, commit afterwards (like pt_set_params): the checkpoint is staged in the read-out
  // buffer, its sample count — the .w every pixel carries; a pass adds the same spp to all of them, so
  // the first and the last pixel must agree — is checked there, and only then does it replace the
  // accumulation.  A refused checkpoint leaves the context as it was.
  const size_t n_pix = n_pixels(c);
  PT_HIP(c, hipMemcpyAsync(c->frame.resolve.get(), src, need, hipMemcpyDefault, c->stream));
  float4 ends[2];
  PT_HIP(c, hipMemcpyAsync(&ends[0], c->frame.resolve.get(), sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipMemcpyAsync(&ends[1], c->frame.resolve.get() + (n_pix - 1), sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  const float w = ends[0].w;
  if (!(w >= 0.0f) || w >= 16777216.0f || w != std::floor(w))
    return fail(c, PT_ERR_INVALID, "pt_load_accum: sample count %g in the buffer is not a count", (double)w);
  if (ends[1].w != w)
    return fail(c, PT_ERR_INVALID, "pt_load_accum: sample counts differ across the buffer (%g ... %g): not an accumulation of whole passes",
                (double)w, (double)ends[1].w);
  PT_HIP(c, hipMemcpyAsync(c->frame.accum, c->frame.resolve.get(), need, hipMemcpyDeviceToDevice, c->stream));
  if (int rc = clear_error(c); rc != PT_OK) return rc;  // (a checkpoint carries sums, not the passes they came from)
  PT_HIP(c, hipStreamSynchronize(c->stream));
  c->tally.loaded((uint32_t)w, n_pix);  // the host-side mirrors follow the loaded state
  return PT_OK;
}

// the shader's uniforms (static/shader.frag:79-99) + this launch's share of the image, as the kernels read them
static int fill_uniforms(pt_ctx* c, uint32_t n_passes, PtKernelArgs& A) {
  const PtParams& p = c->params;
  memset(&A, 0, sizeof A);
  for (int k = 0; k < 3; k++) {
    A.origin[k] = p.camera_origin[k];
    A.horizontal[k] = p.horizontal[k];
    A.vertical[k] = p.vertical[k];
    A.llc[k] = p.lower_left_corner[k];
    A.cam_u[k] = p.u[k];
    A.cam_v[k] = p.v[k];
  }
  A.lens_radius = p.lens_radius;
  {
    // lens arithmetic may be skipped (pt_refill.hpp) when it provably adds +0 everywhere
    bool off = p.lens_radius == 0.0f;
    for (int k = 0; k < 3; k++) {
      off = off && std::isfinite(p.u[k]) && std::isfinite(p.v[k]);
      off = off && !(p.camera_origin[k] == 0.0f && std::signbit(p.camera_origin[k]));
    }
    A.lens_off = off ? 1u : 0u;
  }
  A.time0 = p.time;
  A.time_step = p.time_step != 0.0f ? p.time_step : 1.0f;
  A.first_pass = p.first_pass;
  A.spp = p.samples_per_pixel;
  A.max_depth = p.max_depth;
  A.rr_min_depth = c->rr_min_depth;
  A.background_mode = p.background_mode;
  A.width = c->width;
  A.height = c->height;
  A.local_rows = c->local_rows;
  A.band_rows = p.band_rows ? p.band_rows : 1;
  A.band_index = p.band_index;
  A.band_count = p.band_count;
  A.n_passes = n_passes;
  A.n_spheres = c->list.n;
  A.scene_regular = c->list.host.regular ? 1u : 0u;
  A.tiles_x = tiles_x(c);
  A.tiles_y = tiles_y(c);
  unsigned long long items = (unsigned long long)A.tiles_x * A.tiles_y * n_passes * 64ull;
  if (items > 0xfffffff0ull)
    return fail(c, PT_ERR_CAPACITY, "pt_render_passes: %llu work items exceed 2^32; render fewer passes per call", items);
  A.n_items = (uint32_t)items;
  A.fw = (float)c->width;
  A.fh = (float)c->height;
  A.div_per_tile = pt_div_make(64u * n_passes);
  A.div_tiles_x = pt_div_make(A.tiles_x);
  A.div_band_rows = pt_div_make(A.band_rows);
  A.geom = c->list.geom.get();
  A.mat = c->list.mat.get();
  A.mat_r0 = c->list.r0.get();
  A.slab = reinterpret_cast<float*>(c->frame.slab.get());
  A.counters = c->d_counters.get();
  A.tile_order = c->frame.tile_order.get();
  A.tile_cost = c->frame.tile_cost.get();
  A.carry_lanes = c->carry_lanes;
  A.refill_min = c->refill_min;
  A.frame_ctr = c->d_frame_ctr.get() + 1;  // the cell that stays 0 (pt_render_frames points at [0])
  if (c->dbg_enable) {  // (zero otherwise: an overlay-off launch's argument block is what it was before the overlay existed)
    A.uuid = c->list.uuid.get();
    A.dbg_selected = c->dbg_selected;
    for (int k = 0; k < 3; k++) A.dbg_cursor[k] = c->dbg_cursor[k];
  }
  return PT_OK;
}

// hierarchy walk: the tree's arrays and constants; returns what is staged in the LDS (hierarchy_staging)
static Staging bind_hierarchy(pt_ctx* c, PtKernelArgs& A) {
  const SceneBvh& b = c->bvh;
  A.bvh_nodes = b.nodes.get();
  A.bvh_nodes32 = b.nodes32.get();
  A.bvh_slots = b.slots.get();
  A.bvh_slot_index = b.index.get();
  A.slot_mat = b.mat.get();
  if (c->dbg_enable) A.slot_uuid = b.uuid.get();
  A.n_nodes = b.head.n_nodes;
  A.n_tree_slots = b.head.n_tree_slots;
  A.n_slots = b.head.n_slots;
  A.n_outliers = b.head.n_outliers;
  for (int k = 0; k < 3; k++) A.bvh_c0[k] = b.head.c0[k];
  A.bvh_s0 = b.head.s0;
  A.bvh_kinv = b.head.kinv;
  return hierarchy_staging(b.head.n_nodes, b.head.n_slots, walk_lds_room());
}

// grid walk: likewise (grid_staging)
static Staging bind_grid(pt_ctx* c, PtKernelArgs& A) {
  const ptgrid::Grid& g = c->grid.head;
  A.bvh_slots = c->grid.entries.get();
  A.bvh_slot_index = c->grid.index.get();
  A.slot_mat = c->grid.mat.get();
  if (c->dbg_enable) A.slot_uuid = c->grid.uuid.get();
  A.grid_cells = c->grid.cells.get();
  A.n_cells = g.n[0] * g.n[1] * g.n[2];
  A.n_tree_slots = g.n_cell_entries;
  A.n_slots = g.n_entries;
  A.n_outliers = g.n_always;
  for (int k = 0; k < 3; k++) {
    A.bvh_c0[k] = g.c0[k];
    A.grid_n[k] = g.n[k];
    A.grid_lo[k] = g.lo[k]; A.grid_hi[k] = g.hi[k];
    A.grid_h[k] = g.h[k]; A.grid_inv_h[k] = g.inv_h[k];
    A.grid_lo_n[k] = g.lo_n[k]; A.grid_hi_n[k] = g.hi_n[k];
  }
  A.bvh_s0 = g.s0;
  A.grid_r2_near = g.r2_near;
  return grid_build(c);
}

// Workgroups of `block` threads really RESIDENT on a CU at once: the occupancy query (LDS, VGPRs, and an SGPR rule
// that leaves out the trap handler's 16 per wave) capped by what the kernel is BUILT FOR (`built_for`: its entry's wave
// count, the kernel's amdgpu_waves_per_eu).  A launch of more workgroups than this is not wrong, but the extra ones start
// only when others end: for the shared queue that is an empty wave at the end, for a statically dealt launch a share
// of the frame that begins when everybody else is done (the reference's 25-spp paused frame x 4: 2.98 -> 2.44 ms).
static hipError_t resident_blocks(const void* kfn, uint32_t block, size_t lds, int built_for, int* out) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kfn, (int)block, lds);
  if (e != hipSuccess) return e;
  const int cap = built_for * 4 / (int)(block / 64u);  // four SIMDs per CU, block / 64 waves per workgroup
  *out = n < cap ? n : cap;
  return hipSuccess;
}

// walk kernels: whichever of 256 / 512 / 1024 threads puts the most waves on a CU (the staged scene is
// paid once per workgroup, the parked path state and the VGPRs per wave)
static uint32_t walk_block_threads(const void* kfn, int built_for, size_t scene, size_t lds_max, std::optional<uint32_t> knob) {
  uint32_t block = 0;
  int best_waves = -1;
  for (uint32_t b = 256; b <= 1024; b *= 2) {
    const size_t l = scene + (size_t)PT_PARK_STRIDE * 4 * b;
    if (l > lds_max) continue;
    int n = 0;
    if (resident_blocks(kfn, b, l, built_for, &n) != hipSuccess) {
      (void)hipGetLastError(); // a size this kernel cannot run at: not an error of this call
      continue;
    }
    const int waves = n * (int)(b / 64);
    if (waves > best_waves) { best_waves = waves; block = b; }
  }
  if (knob && *knob >= 64u && *knob <= 1024u && *knob % 64u == 0u) block = *knob;
  return block ? block : 1024u;
}

// The launch path's dev knobs (pt_launch_plan.hpp), read per launch: tools/sweep_knobs.py starts a process per point.
// libptrace.so as shipped reads no environment variable (the Python harness has two, both loader matters of
// ray_tracer_webgl_amd/_lib.py: PT_LIB and PT_NO_TORCH_HIP_PRELOAD)
static LaunchKnobs read_launch_knobs() {
  LaunchKnobs k;
#ifdef PT_DEV_KNOBS
  auto knob = [](const char* name, auto& field) { if (const char* e = getenv(name)) field = atoi(e); };
  knob("PT_CARRY_LANES", k.carry_lanes), knob("PT_BVH_BLOCK", k.bvh_block), knob("PT_COOP_MAX", k.coop_max);
  knob("PT_PER_CU", k.per_cu), knob("PT_QUEUE_CHUNK", k.queue_chunk), knob("PT_GRID_PERCENT", k.grid_percent);
  knob("PT_QUEUE_STATIC", k.queue_static), knob("PT_COST_FEEDBACK", k.cost_feedback), knob("PT_QUEUE_GROUPED", k.queue_grouped);
  knob("PT_FEWER_X10_1", k.fewer_x10_1), knob("PT_FEWER_X10_2", k.fewer_x10_2);
#endif
  return k;
}

// What a launch is for, as far as prepare_launch bakes it in.
struct LaunchUse {
  bool allow_trials = false;  // may be the autotune measurement of a geometry path (PT_GEOM_AUTO)
  // does the launch report per-tile costs: as plan_launch decides, or overridden AFTER the plan (the plan itself is the same)
  enum Feedback { PLANNED, OFF, ON } feedback = PLANNED;
  // n_first_tiles > 0: a partial round of pt_render_adaptive — the launch covers the first n_first_tiles positions of `table`, a
  // full permutation of the tiles, and is planned for that many items; tiles_x, tiles_y and div_per_tile stay the frame's
  uint32_t n_first_tiles = 0;
  const uint32_t* table = nullptr;
  // Which entry point's launch, where it is no render launch (pt_trace_table.hpp Door).  Every door takes its own column of the
  // row of the path forced or settled (the cold path while PT_GEOM_AUTO measures); it is no trial, settles nothing, reports no
  // tile costs and leaves `geom` as it finds it; the overlay and roulette do not act.
  //   DOOR_FEATURES  pt_render_features: one deterministic segment per pixel, one pass, into the feature planes
  //   DOOR_QUERY     pt_query_rays: the same estimator on the caller's rays (the first query_rays work items carry one), into the
  //                  query planes; c->last_build is not stored
  //   DOOR_RADIANCE  pt_query_radiance: the PLAIN estimator on the caller's query_rays rays — n_passes passes of the uniforms'
  //                  samples and depth into the pass slabs, frame_ctr at the zero cell; the staged rays travel in
  //                  PtKernelArgs::uuid and the batch's first pass is `first_pass`; c->last_build is not stored
  //   ... with next_event (set by pt_query_radiance_nee and the two _nee gather calls only, together with DOOR_RADIANCE): the
  //                  PT_OPT_NEXT_EVENT estimator on those rays — the row's cell of kRadNeeKernels, the light table beside the rays
  Door door = DOOR_NONE;
  bool next_event = false;
  uint32_t query_rays = 0;
  uint32_t first_pass = 0;
  // the entry point, for a refusal of prepare_launch's own (the frames' launches were asked under their names: frame_ready)
  const char* who = "pt_render";
};

// (what fill_uniforms zeroed and nothing here sets stays zero: wave_log and cell_hist, which only a measuring twin gets)
static int prepare_launch(pt_ctx* c, uint32_t n_passes, const LaunchUse& use, Launch* L) {
  PtKernelArgs& A = L->A;
  // no trace launch gets a pointer into a buffer that is not in place: after a failed allocation the call is refused
  if (int rc = frame_buffers_ready(c, use.who); rc != PT_OK) return rc;
  {
    int rc = fill_uniforms(c, n_passes, A);
    if (rc != PT_OK) return rc;
  }
  if (use.n_first_tiles) {
    A.n_items = use.n_first_tiles * 64u * n_passes;  // (below the frame's count, which fill_uniforms has checked)
    A.tile_order = use.table;
  }
  const LaunchKnobs knobs = read_launch_knobs();
  if (knobs.carry_lanes) A.carry_lanes = *knobs.carry_lanes;
  // all that follows reads of the door: is there one (no render launch: a variant row's build, no trial, nothing of the path or
  // the order moves), does it write first-hit records (`feat`), and which of the two query calls is it
  const bool door = use.door != DOOR_NONE, query = use.door == DOOR_QUERY, rad = use.door == DOOR_RADIANCE;
  const bool feat = use.door == DOOR_FEATURES || query;
  if (c->geom.policy == PT_GEOM_AUTO && !door) try_finish_tuning(c);
  const bool rr = !door && c->rr_min_depth > 0, dbg = !door && c->dbg_enable;
  // next-event estimation acts on render launches only; the doors stay the plain estimator
  const bool nee = !door && c->lights.on;
  // ... unless the entry point is one of the three that ask for the estimator by name (pt_rad_nee_table.hpp)
  const bool rad_nee = rad && use.next_event;
  if ((nee || rad_nee) && !c->lights.in_place()) return fail(c, PT_ERR_CAPACITY, "%s: PT_OPT_NEXT_EVENT's light table is not in place (a failed allocation: install the scene or turn the option on again)", use.who);
  if (rr && c->count_work) return fail(c, PT_ERR_INVALID, "PT_OPT_COUNT_WORK and PT_OPT_RUSSIAN_ROULETTE exclude each other");
  if (dbg && c->count_work) return fail(c, PT_ERR_INVALID, "PT_OPT_COUNT_WORK and the debug overlay exclude each other");
  if (dbg && !c->state.uuid_valid) return fail(c, PT_ERR_NOT_READY, "debug overlay: the uuid arrays are not in place (pt_set_debug_overlay after a failed upload?)");
  // (the overlay builds exist for the ways to read the list that have a roulette build: the same steering away from the LDS walk)
  if (feat && !c->state.uuid_valid) return fail(c, PT_ERR_NOT_READY, "%s: the uuid arrays are not in place (%s after a failed upload?)", query ? "ray queries" : "feature planes",
                                             query ? "PT_OPT_RAY_QUERIES" : "PT_OPT_FEATURES");
  const PathChoice choice = c->geom.choose(path_scene(c), use.allow_trials && !door, rr || dbg || door || nee);
  const int path = choice.path;
  if (!door) c->geom.last = path;

  // the kernel, its workgroup size and its dynamic LDS (staged scene + the parked path state of every
  // lane of a walk kernel's workgroup)
  const bool walk = path == PT_GEOM_BVH || path == PT_GEOM_GRID;
  size_t scene = 0;
  Staging st;
  if (walk) {
    st = path == PT_GEOM_BVH ? bind_hierarchy(c, A) : bind_grid(c, A);
    scene = st.bytes;
    A.lds_scene_bytes = (uint32_t)scene;
  } else {
    // the LDS copy exists whenever the list fits; the scalar and small-list walks only change how the
    // SCAN reads (their per-lane gathers — shading, tail mode — still come from the copy)
    scene = c->list.n <= PT_MAX_SPHERES_LDS ? (size_t)PT_LDS_ENTRIES(c->list.n) * 16 : 0;
  }
  const int row = trace_row(path, c->list.n, st.kind, c->grid.head.n[1]);
  const int build = door ? door_build(use.door) : trace_build(false, dbg, rr, c->count_work);
  if (feat) {  // one deterministic segment per pixel into the planes; the overlay and roulette do not act
    A.uuid = c->list.uuid.get();
    A.slot_uuid = path == PT_GEOM_BVH ? c->bvh.uuid.get() : (path == PT_GEOM_GRID ? c->grid.uuid.get() : nullptr);
    A.slab = reinterpret_cast<float*>(query ? c->query.planes.get() : c->feat.planes.get());
    A.spp = 1; A.max_depth = 1; A.rr_min_depth = 0;
    if (query) A.dbg_selected = (int32_t)use.query_rays;  // (the overlay's field: no build but the overlay's reads it as that)
  }
  if (rad) {  // the plain estimator on the caller's rays: the uniforms' samples and depth, the pass slabs fill_uniforms bound
    A.uuid = reinterpret_cast<const int32_t*>(c->query.planes.get());  // (the staged rays: pt_kernel_args.h says why there)
    A.slot_uuid = nullptr;
    A.dbg_selected = (int32_t)use.query_rays;
    A.first_pass = use.first_pass;
    A.rr_min_depth = 0;
  }
  // (the next-event builds: the side table's cell where the column would have been the plain build; their light table and its
  // length travel where the radiance builds find their rays — pt_kernel_args.h)
  const bool nee_cell = takes_nee_cell(nee, build);
  // the two-axis walk reads the ring layout; it is what `scene` was sized for (staged_cells).  The next-event build of that row
  // walks three axes, like the roulette build: the plain array
  if (!nee_cell && reads_ring_layout(row, build)) {
    A.grid_cells = c->grid.ring.get();
    A.n_cells = (uint32_t)ptrec::ring_cells(c->grid.head.n[0], c->grid.head.n[2]);
  }
  if (nee_cell) {
    A.uuid = reinterpret_cast<const int32_t*>(c->lights.table.get());
    A.slot_uuid = nullptr;
    A.dbg_selected = (int32_t)c->lights.n;
    A.rr_min_depth = 0;
  }
  // (the radiance-query builds of the estimator: their rays and the ray count stay where `rad` put them, so the light table travels
  // in slot_uuid, which both doors leave NULL, and its length as the bits of dbg_cursor[0], which neither reads — pt_kernel_args.h.
  // reads_ring_layout is false of BUILD_RAD: the build of the row `grid` walks three axes over the plain cell array)
  const bool rad_nee_cell = takes_rad_nee_cell(rad_nee, build);
  if (rad_nee_cell) {
    const uint32_t n_lights = c->lights.n;
    A.slot_uuid = reinterpret_cast<const int32_t*>(c->lights.table.get());
    memcpy(&A.dbg_cursor[0], &n_lights, sizeof n_lights);
  }
  const TraceCell& tk = rad_nee_cell ? kRadNeeKernels[row] : (nee_cell ? kNeeKernels[row] : kTraceKernels[row][build]);
  const void* kfn = cell_kernel(c->device, tk);
  if (!query && !rad) c->last_build = nee_cell ? (int)BUILD_NEXT_EVENT : build;  // (what pt_last_trace_build reports: a render or feature launch's column)
  const uint32_t block = walk ? walk_block_threads(kfn, tk.waves, scene, kWalkLdsMax, knobs.bvh_block) : list_block_threads(scene);
  const size_t lds = walk ? scene + (size_t)PT_PARK_STRIDE * 4 * block : scene;
  A.block_threads = block;
  int per_cu = 0;
  PT_HIP(c, resident_blocks(kfn, block, lds, tk.waves, &per_cu));

  const LaunchPlan P = plan_launch({A.n_items, feat ? 1 : c->params.samples_per_pixel, n_passes, block, per_cu, (uint32_t)c->num_cus, walk,
                                    c->list.n, knobs});
  A.queue_chunk = P.queue_chunk; A.queue_static = (uint32_t)P.deal; A.queue_groups = P.queue_groups;
  A.n_waves = P.n_waves; A.coop_max_live = P.coop_max_live; A.refill_ahead = P.refill_ahead;
  A.cost_feedback = use.feedback == LaunchUse::PLANNED ? P.cost_feedback : (use.feedback == LaunchUse::ON ? 1u : 0u);
  if (door) A.cost_feedback = 0u;
  L->kfn = kfn; L->grid = P.grid; L->block = block; L->lds = lds; L->path = path; L->trial = choice.trial;
  return PT_OK;
}

// THE launch of every kernel that lives in a unit of its own and is no trace kernel: `sig` is the kernel's parameter list
// (pt_sigs.h), `kernel` its handle (pt_extra.h), the arguments go by value and are checked against the list at compile time
// (pt_call.hpp has the rule) before they become the array of pointers.  Capture-safe: a launch only.
template <class... P, class... A>
static hipError_t call(ptcall::Sig<P...> sig, const void* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, A... args) {
  return ptcall::call([](const void* k, dim3 g, dim3 b, void** slots, size_t l, hipStream_t s) { return hipLaunchKernel(k, g, b, slots, l, s); },
                      sig, kernel, grid, block, lds, stream, args...);
}

// the trace kernel of a prepared launch (capture-safe: a launch only)
static int launch_trace(pt_ctx* c, const Launch& L) {
  void* kargs[] = {const_cast<PtKernelArgs*>(&L.A)};
  PT_HIP(c, hipLaunchKernel(L.kfn, dim3(L.grid), dim3(L.block), kargs, L.lds, c->stream));
  return PT_OK;
}

// A whole trace launch with nothing of the caller's between its steps: prepared, the queue's heads zeroed, enqueued; timed where
// the caller keeps a span (taken once the launch is prepared, around the kernel alone).
static int trace_once(pt_ctx* c, uint32_t n_passes, const LaunchUse& use, TimedSpan* span = nullptr) {
  Launch L;
  if (int rc = prepare_launch(c, n_passes, use, &L); rc != PT_OK) return rc;
  if (span)
    if (int rc = span->take(c); rc != PT_OK) return rc;
  PT_HIP(c, zero_queue_heads(c, L.A.queue_static));
  if (span)
    if (int rc = span->begin(c); rc != PT_OK) return rc;
  if (int rc = launch_trace(c, L); rc != PT_OK) return rc;
  return span ? span->end(c) : PT_OK;
}

PT_API int pt_render_passes(pt_ctx* c, uint32_t n_passes) {
  if (!c) return PT_ERR_INVALID;
  if (int rc = scene_and_uniforms(c, "pt_render"); rc != PT_OK) return rc;
  if (n_passes == 0) return fail(c, PT_ERR_INVALID, "pt_render_passes: n_passes == 0");
  if (n_passes > c->reserved_passes)
    return fail(c, PT_ERR_CAPACITY, "pt_render_passes: %u passes > %u reserved (pt_reserve_passes)",
                n_passes, c->reserved_passes);
  if (c->local_rows == 0) return PT_OK; // this band owns no rows
  const bool estimate = c->est.on && !c->est.paused;
  // the estimate folds pass SUMS: every pass since its last clear must hold the same number of samples
  if (estimate && c->est.spp != 0 && c->est.spp != c->params.samples_per_pixel)
    return fail(c, PT_ERR_INVALID, "pt_render_passes: %d samples per pixel while the error estimate holds passes of %d: clear first "
                                   "(pt_reset_accum)", c->params.samples_per_pixel, c->est.spp);
  PT_HIP(c, hipSetDevice(c->device));

  Launch L;
  {
    LaunchUse use;
    use.allow_trials = true;
    use.who = "pt_render_passes";
    int rc = prepare_launch(c, n_passes, use, &L);
    if (rc != PT_OK) return rc;
  }
  PtKernelArgs& A = L.A;
  const PtParams& p = c->params;
  const uint32_t grid = L.grid, block = L.block;
  const int path = L.path;
  int trial = L.trial;

  // inside a stream capture (hipGraph) nothing may synchronise or allocate and timing events are
  // meaningless: the launch sequence itself is capture-safe, the measuring twins' set-up is not
  const bool capturing = is_capturing(c);
  if (capturing && c->count_work)
    return fail(c, PT_ERR_INVALID, "pt_render_passes: PT_OPT_COUNT_WORK (measuring twin: allocates its wave log) cannot be captured into a hipGraph");
  if (c->count_work && (path == PT_GEOM_BVH || path == PT_GEOM_GRID || path == PT_GEOM_SMALL)) { // measuring twin: not a product launch, may allocate
    const size_t n_waves = (size_t)grid * (block / 64);
    if (c->d_wave_log.capacity() < n_waves * PT_WAVE_LOG_WORDS) PT_HIP(c, c->d_wave_log.reserve(n_waves * PT_WAVE_LOG_WORDS));
    PT_HIP(c, hipMemsetAsync(c->d_wave_log.get(), 0, n_waves * PT_WAVE_LOG_WORDS * sizeof(unsigned long long), c->stream));
    c->wave_log_n = n_waves;
    A.wave_log = c->d_wave_log.get();
    if (path == PT_GEOM_GRID && c->count_work >= 2) {  // which entry runs the leaf rounds gather (config 5's cache model, tools/config5_cache_model.py)
      const size_t n_hist = (size_t)A.n_slots + PT_COH_BINS;
      if (c->d_cell_hist.capacity() < n_hist) PT_HIP(c, c->d_cell_hist.reserve(n_hist));
      PT_HIP(c, hipMemsetAsync(c->d_cell_hist.get(), 0, n_hist * sizeof(uint32_t), c->stream));
      c->cell_hist_n = n_hist;
      A.cell_hist = c->d_cell_hist.get();
    }
  }
  TimedSpan span;  // (capturing: no timing event pair)
  if (!capturing)
    if (int rc = span.take(c); rc != PT_OK) return rc;

  PT_HIP(c, zero_queue_heads(c, A.queue_static));  // (a statically dealt launch takes no reservations from any head)
  // queue order from the previous launch's per-tile cost (identity when there is none yet); launches
  // that report no cost keep the order they find
  if (c->order.uniform_wants_order_kernel(A.cost_feedback != 0u)) {
    int rc = launch_tile_order(c);
    if (rc != PT_OK) return rc;
    c->order.uniform_order_kernel_enqueued(capturing);  // (a captured order kernel has not run: the next direct launch runs its own)
  }
  if (capturing) trial = -1;
  if (trial >= 0) {
    for (int k = 0; k < 2; k++)
      if (!c->trial_ev[2 * trial + k]) PT_HIP(c, hipEventCreate(&c->trial_ev[2 * trial + k]));
    PT_HIP(c, hipEventRecord(c->trial_ev[2 * trial], c->stream));
  }
  if (int rc = span.begin(c); rc != PT_OK) return rc;
  if (int rc = launch_trace(c, L); rc != PT_OK) return rc;
  c->order.uniform_traced(A.cost_feedback != 0u, capturing);
  if (int rc = span.end(c); rc != PT_OK) return rc;
  if (trial >= 0) {
    PT_HIP(c, hipEventRecord(c->trial_ev[2 * trial + 1], c->stream));
    c->geom.enqueued(trial, (double)n_pixels(c) * n_passes * (double)p.samples_per_pixel);
  }

  uint32_t n_pix = (uint32_t)n_pixels(c);
  if (estimate) {  // the same adds into accum, and the estimate's update beside them (pt_kernels_error.hip)
    PT_HIP(c, call(ptsig::FoldError{}, pt_error_kernel(PT_E_FOLD), dim3(pixel_grid(n_pix)), dim3(256), 0, c->stream,
                   c->frame.accum, c->est.state.get(), c->frame.slab.get(), n_pix, n_passes));
    c->est.spp = p.samples_per_pixel;
  } else {
    hipLaunchKernelGGL(pt_accumulate_kernel, dim3(pixel_grid(n_pix)), dim3(256), 0, c->stream,
                       c->frame.accum, c->frame.slab.get(), n_pix, n_passes);
    PT_HIP(c, hipGetLastError());
  }

  // Host-side tallies describe work enqueued directly.  A captured launch runs as often as its
  // graph is replayed, which the host cannot see: read-out takes its divisor from the device
  // (accum.w, see pixel_scale), and pt_get_stats reads the accumulated spp back from there.
  c->tally.uniform_launch(capturing, n_pix, n_passes, (uint32_t)p.samples_per_pixel);
  return PT_OK;
}

PT_API int pt_render(pt_ctx* c) { return pt_render_passes(c, 1); }

// ---- the reference's frame on device-resident textures ---------------------------------------------
// webgl::render (src/webgl.rs:180-205) as the rAF closure calls it (src/lib.rs:92-102): one pass of the
// hot path at the current uniforms, blended with the previous frame's texture by the shader's
// render() rule (static/shader.frag:387-404), drawn to the canvas and — when averaging — to the
// other texture.  Nothing crosses PCIe: the textures of src/webgl.rs:82-123 live in HBM.
namespace {

int plan_frame(pt_ctx* c, const uint32_t* ctr, uint32_t even_odd0, int max_render_count, uint32_t n_frames, float4* slab, FramePlan* F) {
  memset(static_cast<void*>(F), 0, sizeof *F);  // (padding too: plans are compared bytewise)
  // frames k .. k + n - 1 are the passes 0 .. n - 1 of ONE launch: pass p renders at u_time = time + float(first_pass + p + k) *
  // time_step (pt_refill.hpp), which IS frame k + p's time, into slab p
  // (a group of frames is dealt like any other launch of its shape — prepare_launch: statically for one- and two-sample
  // items, as the reference's frames are, through the shared queue from there on.  Round 4 dealt every group statically
  // "whatever its size"; measured in round 5 on the reference's scene and size: groups of 4- / 8- / 25-sample frames 0.126 /
  // 0.238 / 0.727 ms per frame dealt statically, 0.126 / 0.211 / 0.561 through the queue; profiles/r05_ab_runs.txt)
  LaunchUse use;
  use.feedback = LaunchUse::OFF;  // a frame is one short launch: it keeps the tile order it finds
  int rc = prepare_launch(c, n_frames, use, &F->L);
  if (rc != PT_OK) return rc;
  F->L.A.frame_ctr = ctr;
  F->ctr = ctr; F->even_odd0 = even_odd0; F->max_render_count = max_render_count;
  F->render_count0 = c->params.render_count; F->should_average = c->params.should_average;
  F->last_frame_weight = c->params.last_frame_weight;
  F->L.A.slab = reinterpret_cast<float*>(slab);
  F->stream = c->stream; F->slab = slab;
  F->tex0 = c->frame.tex[0].get(); F->tex1 = c->frame.tex[1].get(); F->canvas = c->frame.canvas.get();
  F->n_frames = n_frames;
  return PT_OK;
}

// enqueue one planned frame — or group of frames — (capture-safe: launches only)
int enqueue_frame(pt_ctx* c, FramePlan& F, bool advance) {
  if (int rc = launch_trace(c, F.L); rc != PT_OK) return rc;
  // a frame's one pass sits in its slab ({sum r, g, b, spp} per pixel): blend straight from there, frame after frame
  // (each blend reads the texture the one before it wrote)
  const uint32_t n_pix = (uint32_t)n_pixels(c);
  if (F.n_frames > 1u) {  // a group: its blends as one pass over the pixels
    hipLaunchKernelGGL(pt_frames_blend_kernel, dim3(pixel_grid(n_pix)), dim3(256), 0, c->stream, F.slab, F.n_frames,
                       c->frame.tex[0].get(), c->frame.tex[1].get(), c->frame.canvas.get(), n_pix, F.ctr, F.render_count0, F.even_odd0, F.max_render_count,
                       F.should_average, F.last_frame_weight);
    PT_HIP(c, hipGetLastError());
  }
  for (uint32_t f = 0; f < (F.n_frames > 1u ? 0u : 1u); f++) {
    hipLaunchKernelGGL(pt_frame_blend_kernel, dim3(pixel_grid(n_pix)), dim3(256), 0, c->stream, F.slab + (size_t)f * n_pix,
                       c->frame.tex[0].get(), c->frame.tex[1].get(), c->frame.canvas.get(), n_pix, F.ctr, f, F.render_count0, F.even_odd0, F.max_render_count,
                       F.should_average, F.last_frame_weight);
    PT_HIP(c, hipGetLastError());
  }
  if (advance) {
    hipLaunchKernelGGL(pt_frame_advance_kernel, dim3(1), dim3(PT_QUEUE_GROUPS_MAX), 0, c->stream, c->d_frame_ctr.get(), c->d_counters.get(), F.n_frames);
    PT_HIP(c, hipGetLastError());
  }
  return PT_OK;
}

// The tile order a frame finds must exist (frames report no costs and never run the order kernel themselves)
// ... and for frames of four samples or more it should be a COST-SORTED one.  A frame (group) is a statically dealt launch:
// wave w takes the reservations w, w + n_waves, ... of the tile-major item list, a fixed sample of the tiles.  In the IDENTITY
// order of a fresh context that sample is a few places of the image, and a wave's load follows what lies there (sky: one
// segment per path, glass: eight); in an order sorted by cost it is one tile from each cost stratum and the waves' loads come
// out nearly equal.  Frames report no costs themselves (plan_frame), so the order is PROBED: one extra pass at the current
// uniforms with the cost feedback on, into the scratch slab, then the order kernel — outside any capture, when there is no
// probed order yet, after a new scene or partition, and (at most every 64 frames) after the view has changed.  Measured on the
// reference's scene and size against the identity order (profiles/r05_ab_runs.txt): the paused mode's 25-spp frame 0.870 ->
// 0.768 ms, 8-spp frames 0.315 -> 0.275, groups of 4- / 8-spp frames 0.126 -> 0.119 / 0.212 -> 0.198 ms per frame; groups
// of 1- and 2-spp frames +-0, and the SINGLE 1-spp frame (which runs on three workgroups per CU, four or five tiles per
// wave) 0.083 -> 0.088-0.093: frames below four samples therefore keep — and, after a probed series, restore — the identity
// order.  (Dealing the rounds in serpentine order, the textbook companion of a sorted list, measured +2 ... +10 % on every
// statically dealt shape and is not used.)  Scheduling only: the probe's slab is scratch, its segment tally is taken back out
// of the statistics.
// (When which of it happens: TileOrder::frames, pt_tile_order.hpp.)
int ensure_cost_order(pt_ctx* c, uint32_t n_frames) {
  const TileOrder::FrameStep step = c->order.frames(c->params.samples_per_pixel, c->params, c->state.scene_gen, n_frames, [c] { return is_capturing(c); });
  if (step.zero_costs)  // back to the identity order: what the order kernel writes when every cost is zero
    PT_HIP(c, hipMemsetAsync(c->frame.tile_cost.get(), 0, c->frame.tile_cost.capacity() * sizeof(uint32_t), c->stream));
  if (step.order_kernel) {
    int rc = launch_tile_order(c);
    if (rc != PT_OK) return rc;
    c->order.order_kernel_ran();
  }
  if (!step.probe) return PT_OK;
  Launch L;
  LaunchUse use;
  use.feedback = LaunchUse::ON;
  int rc = prepare_launch(c, 1, use, &L);
  if (rc != PT_OK) return rc;
  L.A.slab = reinterpret_cast<float*>(c->frame.slab.get());  // scratch: a frame's own slab is written before it is read
  unsigned long long* seg = c->d_counters.get() + PT_CTR_SEGMENTS;
  PT_HIP(c, hipMemcpyAsync(c->d_counters.get() + PT_CTR_SCRATCH, seg, sizeof *seg, hipMemcpyDeviceToDevice, c->stream));
  PT_HIP(c, zero_queue_heads(c, L.A.queue_static));
  rc = launch_trace(c, L);
  if (rc != PT_OK) return rc;
  rc = launch_tile_order(c);
  if (rc != PT_OK) return rc;
  PT_HIP(c, hipMemcpyAsync(seg, c->d_counters.get() + PT_CTR_SCRATCH, sizeof *seg, hipMemcpyDeviceToDevice, c->stream));
  c->order.probed_for(c->params, c->state.scene_gen);
  return PT_OK;
}

int frame_ready(pt_ctx* c, const char* who) {
  if (!c) return PT_ERR_INVALID;
  if (int rc = scene_and_uniforms(c, who); rc != PT_OK) return rc;
  if (c->count_work) return fail(c, PT_ERR_INVALID, "%s: not with PT_OPT_COUNT_WORK (the measuring twins are not frame kernels)", who);
  return frame_buffers_ready(c, who);
}

} // namespace

PT_API int pt_clear_textures(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  if (int rc = frame_buffers_ready(c, "pt_clear_textures"); rc != PT_OK) return rc;
  PT_HIP(c, hipSetDevice(c->device));
  const size_t bytes = n_pixels(c) * sizeof(uint32_t);
  if (bytes == 0) return PT_OK;
  for (int k = 0; k < 2; k++) PT_HIP(c, hipMemsetAsync(c->frame.tex[k].get(), 0, bytes, c->stream));
  PT_HIP(c, hipMemsetAsync(c->frame.canvas.get(), 0, bytes, c->stream));
  return PT_OK;
}

PT_API int pt_render_frame(pt_ctx* c, uint32_t even_odd_count) {
  int rc = frame_ready(c, "pt_render_frame");
  if (rc != PT_OK) return rc;
  if (c->local_rows == 0) return PT_OK;
  PT_HIP(c, hipSetDevice(c->device));
  FramePlan F;
  rc = plan_frame(c, c->d_frame_ctr.get() + 1, even_odd_count, 0x7fffffff, 1, c->frame.slab.get(), &F);  // frame 0 of a series of one
  if (rc != PT_OK) return rc;
  rc = ensure_cost_order(c, 1);
  if (rc != PT_OK) return rc;
  PT_HIP(c, zero_queue_heads(c, F.L.A.queue_static));  // (the shared head, the groups' heads, or — statically dealt — none)
  rc = enqueue_frame(c, F, false);
  if (rc != PT_OK) return rc;
  c->tally.frames(1, n_pixels(c), (uint32_t)c->params.samples_per_pixel);
  return PT_OK;
}

PT_API int pt_render_frames(pt_ctx* c, uint32_t even_odd_count, uint32_t max_render_count, uint32_t n_frames) {
  int rc = frame_ready(c, "pt_render_frames");
  if (rc != PT_OK) return rc;
  if (n_frames == 0 || c->local_rows == 0) return PT_OK;
  if (max_render_count > 0x7fffffffu) max_render_count = 0x7fffffffu;
  PT_HIP(c, hipSetDevice(c->device));
  if (is_capturing(c))
    return fail(c, PT_ERR_INVALID, "pt_render_frames: the stream is being captured already (this call replays its own graph)");
  // hipStreamBeginCapture is refused on the legacy default stream (PT_STREAM_LEGACY, what a context bound to
  // torch's default stream runs on): say so instead of failing inside the capture
  if (c->stream == hipStreamLegacy || c->stream == nullptr)
    return fail(c, PT_ERR_INVALID, "pt_render_frames: the context runs on the legacy default stream (PT_STREAM_LEGACY), which cannot be "
                                   "captured into a hipGraph; give it a stream of its own (pt_set_stream(ctx, NULL) or a created stream) "
                                   "or issue the ticks with pt_render_frame");
  // Frames in GROUPS of 64, 16 and 4: ONE trace launch renders a group's frames as its passes (each pass has its own u_time: the
  // frame's), one kernel runs their blends in order.  A 1-spp frame of the reference's size is two items per resident lane,
  // and a wave ends when its slowest lane does: most of a single frame's 0.11 ms is that drain; a group shares one.  What is
  // left of the series is replayed frame by frame.  Same bits either way: a frame is a pass.
  uint32_t counts[kFrameLevels] = {0, 0, 0, 0};
  {
    uint32_t left = n_frames;
    for (int g = 0; g < kFrameLevels; g++) {
      if (kFrameGroups[g] > 16u && n_pixels(c) * kFrameGroups[g] * sizeof(float4) > kFrameSlabCap) continue;  // (too big a slab)
      counts[g] = left / kFrameGroups[g];
      left -= counts[g] * kFrameGroups[g];
    }
  }
  // the groups' own slabs (never the slab of pt_render_passes: a caller's captured launches keep theirs): the one allocation
  // this entry point ever makes, at the first use of a size.  16 x local_rows x width x 16 B is 230 MB at the reference's
  // 1280x702 and 2.1 GB at 4K; when it cannot be had the series falls back to groups of 4 (a quarter of it) and then to
  // single frames out of the slab every context owns — slower, never a failed call.
  for (int g = 0; g < kFrameLevels - 1; g++) {
    if (!counts[g]) continue;
    const size_t need = n_pixels(c) * kFrameGroups[g];
    if (c->d_frame_slab.capacity() >= need) break;
    PT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->d_frame_slab.reserve(need) == hipSuccess) break;
    (void)hipGetLastError();  // out of memory is not an error of this call: deal this group's frames to the next smaller one
    counts[g + 1] += counts[g] * (kFrameGroups[g] / kFrameGroups[g + 1]);
    counts[g] = 0;
  }
  rc = ensure_cost_order(c, n_frames);  // outside the capture: it runs once per series at most, not per frame
  if (rc != PT_OK) return rc;
  // everything a graph bakes in is decided outside the capture; a cached graph is reused while that is unchanged
  // (pt_set_params with the same values, as a frame loop issues before every series, does not re-capture)
  auto graph_for = [&](int g) -> int {
    const uint32_t frames = kFrameGroups[g];
    hipGraphExec_t* exec = &c->frame_exec[g];
    FramePlan* plan_store = &c->frame_plan[g];
    FramePlan F;
    int r = plan_frame(c, c->d_frame_ctr.get(), even_odd_count, (int)max_render_count, frames, frames > 1u ? c->d_frame_slab.get() : c->frame.slab.get(), &F);
    if (r != PT_OK) return r;
    if (*exec && memcmp(&F, plan_store, sizeof F) == 0) return PT_OK;  // (bytewise, padding included: plan_frame zeroed it)
    if (*exec) { (void)hipGraphExecDestroy(*exec); *exec = nullptr; }
    hipGraph_t graph = nullptr;
    PT_HIP(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    r = enqueue_frame(c, F, true);
    hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (r != PT_OK) { if (graph) (void)hipGraphDestroy(graph); return r; }
    if (e != hipSuccess) return fail(c, PT_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { *exec = nullptr; return fail(c, PT_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e)); }
    memcpy(static_cast<void*>(plan_store), &F, sizeof F);  // (not an assignment, which need not copy the padding)
    return PT_OK;
  };
  for (int g = 0; g < kFrameLevels; g++)
    if (counts[g]) { rc = graph_for(g); if (rc != PT_OK) return rc; }
  // the series starts at frame 0 with an empty queue; every replay leaves both ready for the next
  PT_HIP(c, hipMemsetAsync(c->d_frame_ctr.get(), 0, sizeof(uint32_t), c->stream));
  PT_HIP(c, hipMemsetAsync(c->d_counters.get() + PT_CTR_HEAD, 0, sizeof(unsigned long long), c->stream));
  PT_HIP(c, zero_queue_heads(c, 2u));
  TimedSpan span;
  if (rc = span.take(c); rc != PT_OK) return rc;
  if (rc = span.begin(c); rc != PT_OK) return rc;
  for (int g = 0; g < kFrameLevels; g++)
    for (uint32_t k = 0; k < counts[g]; k++) PT_HIP(c, hipGraphLaunch(c->frame_exec[g], c->stream));
  if (rc = span.end(c); rc != PT_OK) return rc;
  c->tally.frames(n_frames, n_pixels(c), (uint32_t)c->params.samples_per_pixel);
  return PT_OK;
}

static int read_rgba8(pt_ctx* c, const uint32_t* src, uint8_t* out, const char* who) {
  if (!c || !out) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  if (int rc = frame_buffers_ready(c, who); rc != PT_OK) return rc;
  PT_HIP(c, hipSetDevice(c->device));
  const size_t bytes = n_pixels(c) * 4;
  if (bytes) PT_HIP(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}
PT_API int pt_read_canvas(pt_ctx* c, uint8_t* rgba_out) { return read_rgba8(c, c ? c->frame.canvas.get() : nullptr, rgba_out, "pt_read_canvas"); }
PT_API int pt_read_texture(pt_ctx* c, int index, uint8_t* rgba_out) {
  if (c && (index < 0 || index > 1)) return fail(c, PT_ERR_INVALID, "pt_read_texture: index %d", index);
  return read_rgba8(c, c ? c->frame.tex[index].get() : nullptr, rgba_out, "pt_read_texture");
}
PT_API int pt_write_texture(pt_ctx* c, int index, const uint8_t* rgba_in) {
  if (!c || !rgba_in) return fail(c, PT_ERR_INVALID, "pt_write_texture: NULL argument");
  if (index < 0 || index > 1) return fail(c, PT_ERR_INVALID, "pt_write_texture: index %d", index);
  if (int rc = frame_buffers_ready(c, "pt_write_texture"); rc != PT_OK) return rc;
  PT_HIP(c, hipSetDevice(c->device));
  const size_t bytes = n_pixels(c) * 4;
  if (bytes) PT_HIP(c, hipMemcpyAsync(c->frame.tex[index].get(), rgba_in, bytes, hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}


// ---- include/ptrace_dev.h: developer diagnostics, not part of the versioned ABI ----------------
PT_API long pt_debug_counters(pt_ctx* c, unsigned long long* out, size_t cap) {
  if (!c || !out) return -1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -2;
  const size_t n = cap < (size_t)PT_CTR_COUNT ? cap : (size_t)PT_CTR_COUNT;
  if (hipMemcpy(out, c->d_counters.get(), n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  return (long)n;
}

// Dev diagnostics of the measuring twins: per wave {start, queue dry (0 = never saw it dry), end}
// of the last counted launch, in 100 MHz ticks, and where it ran (HW_ID | XCC_ID << 32): four u64 per wave.
// Returns the number of waves, or < 0.
PT_API long pt_debug_wave_log(pt_ctx* c, unsigned long long* out, size_t cap_waves) {
  if (!c || !c->d_wave_log.get() || !out) return -1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -2;
  const size_t n = c->wave_log_n < cap_waves ? c->wave_log_n : cap_waves;
  if (hipMemcpy(out, c->d_wave_log.get(), n * PT_WAVE_LOG_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  return (long)n;
}

PT_API long pt_debug_cell_hist(pt_ctx* c, uint32_t* out, size_t cap) {
  if (!c || !c->d_cell_hist.get() || !out) return -1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -2;
  const size_t n = c->cell_hist_n < cap ? c->cell_hist_n : cap;
  if (hipMemcpy(out, c->d_cell_hist.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  return (long)n;
}

PT_API long pt_debug_setup_times(pt_ctx* c, double* out_ms, size_t cap) {
  if (!c || !out_ms) return -1;
  const size_t n = cap < (size_t)PT_SETUP_COUNT ? cap : (size_t)PT_SETUP_COUNT;
  for (size_t k = 0; k < n; k++) out_ms[k] = c->setup_ms[k];
  return (long)n;
}

PT_API int pt_debug_wait(pt_ctx* c, unsigned timeout_ms) {
  if (!c) return -1;
  if (hipSetDevice(c->device) != hipSuccess) return -2;
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return -2;
  int rc = -2;
  if (hipEventRecord(ev, c->stream) == hipSuccess) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipEventQuery(ev);
      if (e == hipSuccess) { rc = 0; break; }
      if (e != hipErrorNotReady) { (void)hipGetLastError(); rc = -2; break; }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms)) { rc = 1; break; }
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
  }
  if (rc != 1) (void)hipEventDestroy(ev);  // (a pending event is left alone: destroying it could block like a synchronise)
  return rc;
}

// The two tile-table kernels on the caller's arrays, for tests/test_gpu_tile_tables.py: scratch buffers of the call's own (the
// context's order, costs, adaptive tables and TileOrder state are neither read nor written), the outputs filled with 0xFF bytes
// first, the launch the product makes — one workgroup of 1024 threads on the context's stream.
PT_API int pt_debug_tile_order(pt_ctx* c, const uint32_t* cost, uint32_t n, uint32_t* order_out, uint32_t* cost_out) {
  if (!c || !cost || !order_out || !cost_out || n == 0) return fail(c, PT_ERR_INVALID, "pt_debug_tile_order: NULL argument or no tiles");
  PT_TRY(not_capturing(c, "pt_debug_tile_order"));
  PT_HIP(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  DevBuf<uint32_t> d_cost, d_order;
  PT_HIP(c, d_cost.reserve(n));
  PT_HIP(c, d_order.reserve(n));
  PT_HIP(c, hipMemcpyAsync(d_cost.get(), cost, bytes, hipMemcpyHostToDevice, c->stream));
  PT_HIP(c, hipMemsetAsync(d_order.get(), 0xFF, bytes, c->stream));
  hipLaunchKernelGGL(pt_tile_order_kernel, dim3(1), dim3(1024), 0, c->stream, d_cost.get(), d_order.get(), n);
  PT_HIP(c, hipGetLastError());
  PT_HIP(c, hipMemcpyAsync(order_out, d_order.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipMemcpyAsync(cost_out, d_cost.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

// the partition kernel: `order` split by `flags` into part[0, n) — the flagged tiles first, both halves in order's order — and
// base; one workgroup; enqueued, not awaited
static int launch_partition(pt_ctx* c, const uint32_t* order, const uint32_t* flags, uint32_t* part, uint32_t* base, uint32_t n) {
  PT_HIP(c, call(ptsig::PartitionOrder{}, pt_error_kernel(PT_E_PARTITION), dim3(1), dim3(1024), 0, c->stream, order, flags, part, base, n));
  return PT_OK;
}

PT_API int pt_debug_partition_order(pt_ctx* c, const uint32_t* order, const uint32_t* flags, uint32_t n, uint32_t* part_out,
                                    uint32_t* base_out) {
  if (!c || !order || !flags || !part_out || !base_out || n == 0)
    return fail(c, PT_ERR_INVALID, "pt_debug_partition_order: NULL argument or no tiles");
  PT_TRY(not_capturing(c, "pt_debug_partition_order"));
  PT_HIP(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)n * sizeof(uint32_t);
  DevBuf<uint32_t> d_in, d_out;  // {order, flags} and {part, base}
  PT_HIP(c, d_in.reserve(2 * (size_t)n));
  PT_HIP(c, d_out.reserve(2 * (size_t)n));
  PT_HIP(c, hipMemcpyAsync(d_in.get(), order, bytes, hipMemcpyHostToDevice, c->stream));
  PT_HIP(c, hipMemcpyAsync(d_in.get() + n, flags, bytes, hipMemcpyHostToDevice, c->stream));
  PT_HIP(c, hipMemsetAsync(d_out.get(), 0xFF, 2 * bytes, c->stream));
  PT_TRY(launch_partition(c, d_in.get(), d_in.get() + n, d_out.get(), d_out.get() + n, n));
  PT_HIP(c, hipMemcpyAsync(part_out, d_out.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipMemcpyAsync(base_out, d_out.get() + n, bytes, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_synchronize(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

static int resolve_common(pt_ctx* c, void* out, int gamma, int mode, const uint8_t* prev) {
  if (!c || !out) return fail(c, PT_ERR_INVALID, "pt_resolve: NULL argument");
  if (c->tally.nothing_rendered()) return fail(c, PT_ERR_NOT_READY, "pt_resolve: nothing rendered yet");
  if (int rc = frame_buffers_ready(c, "pt_resolve"); rc != PT_OK) return rc;
  PT_HIP(c, hipSetDevice(c->device));
  uint32_t n_pix = (uint32_t)n_pixels(c);
  if (n_pix == 0) return PT_OK;
  // the 1/spp of static/shader.frag:376 is taken per pixel from accum.w on the device
  uint32_t grid = pixel_grid(n_pix);
  size_t bytes;
  if (mode == 0) {
    hipLaunchKernelGGL(pt_resolve_kernel, dim3(grid), dim3(256), 0, c->stream, c->frame.accum, c->frame.resolve.get(),
                       n_pix, gamma);
    bytes = (size_t)n_pix * sizeof(float4);
  } else if (mode == 1) {
    hipLaunchKernelGGL(pt_resolve_rgba8_kernel, dim3(grid), dim3(256), 0, c->stream, c->frame.accum,
                       reinterpret_cast<uint32_t*>(c->frame.resolve.get()), n_pix, gamma);
    bytes = (size_t)n_pix * 4;
  } else {
    // stage prev into the upper half of the resolve buffer (16 B/pixel holds 4 B in + 4 B out)
    uint32_t* d_out = reinterpret_cast<uint32_t*>(c->frame.resolve.get());
    uint32_t* d_prev = d_out + n_pix;
    PT_HIP(c, hipMemcpyAsync(d_prev, prev, (size_t)n_pix * 4, hipMemcpyDefault, c->stream));
    hipLaunchKernelGGL(pt_blend_rgba8_kernel, dim3(grid), dim3(256), 0, c->stream, c->frame.accum, d_prev, d_out,
                       n_pix, c->params.render_count, c->params.should_average,
                       c->params.last_frame_weight);
    bytes = (size_t)n_pix * 4;
  }
  PT_HIP(c, hipGetLastError());
  PT_HIP(c, hipMemcpyAsync(out, c->frame.resolve.get(), bytes, hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_resolve(pt_ctx* c, float* rgba_out, int gamma) { return resolve_common(c, rgba_out, gamma, 0, nullptr); }
PT_API int pt_resolve_rgba8(pt_ctx* c, uint8_t* rgba_out, int gamma) { return resolve_common(c, rgba_out, gamma, 1, nullptr); }
PT_API int pt_blend_rgba8(pt_ctx* c, const uint8_t* prev, uint8_t* out) {
  if (!prev) return fail(c, PT_ERR_INVALID, "pt_blend_rgba8: prev is NULL");
  return resolve_common(c, out, 1, 2, prev);
}

// ---- the error estimate's read-out (include/ptrace.h; kernels: pt_kernels_error.hip) ------------------------------------
PT_API int pt_error_ptr(pt_ctx* c, void** dev_ptr, size_t* bytes) {
  if (!c || !dev_ptr) return fail(c, PT_ERR_INVALID, "pt_error_ptr: NULL argument");
  if (!c->est.on) return option_off(c, "pt_error_ptr", SET_ESTIMATE);
  *dev_ptr = c->est.state.get();
  if (bytes) *bytes = n_pixels(c) * 2 * sizeof(float4);
  return PT_OK;
}

PT_API int pt_resolve_error(pt_ctx* c, float* rgba_out) {
  if (!c || !rgba_out) return fail(c, PT_ERR_INVALID, "pt_resolve_error: NULL argument");
  if (!c->est.on) return option_off(c, "pt_resolve_error", SET_ESTIMATE);
  PT_TRY(frame_buffers_ready(c, "pt_resolve_error"));
  PT_HIP(c, hipSetDevice(c->device));
  uint32_t n_pix = (uint32_t)n_pixels(c);
  if (n_pix == 0) return PT_OK;
  PT_HIP(c, call(ptsig::ResolveError{}, pt_error_kernel(PT_E_RESOLVE), dim3(pixel_grid(n_pix)), dim3(256), 0, c->stream,
                 c->est.state.get(), c->frame.resolve.get(), n_pix));
  PT_HIP(c, hipMemcpyAsync(rgba_out, c->frame.resolve.get(), (size_t)n_pix * sizeof(float4), hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

// the two filtered read-outs (include/ptrace.h): they read the estimate's state only.  `patch` NULL:
// pt_resolve_filtered and its kernel, else pt_resolve_filtered_patch and the patch-wise one; the checks and their order are shared
static int resolve_filtered(pt_ctx* c, const char* who, float* rgba_out, uint32_t radius, const uint32_t* patch, float kappa, int gamma) {
  if (!c || !rgba_out) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  if (radius > PT_FILTER_MAX_RADIUS) return fail(c, PT_ERR_INVALID, "%s: radius %u > PT_FILTER_MAX_RADIUS", who, radius);
  if (patch && *patch > PT_FILTER_MAX_PATCH) return fail(c, PT_ERR_INVALID, "%s: patch %u > PT_FILTER_MAX_PATCH", who, *patch);
  if (!std::isfinite(kappa) || kappa < 0.0f) return fail(c, PT_ERR_INVALID, "%s: kappa must be finite and >= 0", who);
  if (!c->est.on) return option_off(c, who, SET_ESTIMATE);
  PT_TRY(frame_buffers_ready(c, who));
  PT_HIP(c, hipSetDevice(c->device));
  uint32_t n_pix = (uint32_t)n_pixels(c);
  if (n_pix == 0) return PT_OK;
  const float4* est = c->est.state.get();
  float4* out = c->frame.resolve.get();
  const uint32_t width = c->width, rows = c->local_rows;
  const uint32_t band_rows = ptstate::Partition(c->params).rows;  // (0: no band, every local row is a neighbour)
  const dim3 grid((width + 31u) / 32u, (rows + 7u) / 8u);
  if (patch)
    PT_HIP(c, call(ptsig::FilterPatch{}, pt_error_kernel(PT_E_FILTER_PATCH), grid, dim3(256), 0, c->stream, est, out, width, rows, band_rows, radius, *patch, kappa, gamma));
  else
    PT_HIP(c, call(ptsig::Filter{}, pt_error_kernel(PT_E_FILTER), grid, dim3(256), 0, c->stream, est, out, width, rows, band_rows, radius, kappa, gamma));
  PT_HIP(c, hipMemcpyAsync(rgba_out, c->frame.resolve.get(), (size_t)n_pix * sizeof(float4), hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_resolve_filtered(pt_ctx* c, float* rgba_out, uint32_t radius, float kappa, int gamma) {
  return resolve_filtered(c, "pt_resolve_filtered", rgba_out, radius, nullptr, kappa, gamma);
}

PT_API int pt_resolve_filtered_patch(pt_ctx* c, float* rgba_out, uint32_t radius, uint32_t patch, float kappa, int gamma) {
  return resolve_filtered(c, "pt_resolve_filtered_patch", rgba_out, radius, &patch, kappa, gamma);
}

// the tile kernel over the current state: records into est.tiles[0, n), tallies into [n, 2 n); enqueued, not awaited
static int launch_error_tiles(pt_ctx* c) {
  uint32_t tiles_n = n_tiles(c);
  if (tiles_n == 0) return PT_OK;
  float4* tiles = c->est.tiles.get();
  PT_HIP(c, call(ptsig::ErrorTiles{}, pt_error_kernel(PT_E_TILES), dim3(tile_grid(tiles_n)), dim3(256), 0, c->stream,
                 c->est.state.get(), tiles, tiles + tiles_n, c->width, c->local_rows, tiles_x(c), tiles_n));
  return PT_OK;
}

PT_API int pt_error_tiles(pt_ctx* c, float* tiles_out, uint32_t* tx_out, uint32_t* ty_out) {
  if (!c) return PT_ERR_INVALID;
  if (!c->est.on) return option_off(c, "pt_error_tiles", SET_ESTIMATE);
  PT_TRY(frame_buffers_ready(c, "pt_error_tiles"));
  if (tx_out) *tx_out = tiles_x(c);
  if (ty_out) *ty_out = tiles_y(c);
  if (!tiles_out || n_tiles(c) == 0) return PT_OK;
  PT_HIP(c, hipSetDevice(c->device));
  if (int rc = launch_error_tiles(c); rc != PT_OK) return rc;
  PT_HIP(c, hipMemcpyAsync(tiles_out, c->est.tiles.get(), (size_t)tiles_x(c) * tiles_y(c) * sizeof(float4), hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

// (`h`: the records [0, tiles) and tallies [tiles, 2 tiles) as copied, four floats each, for a caller that goes on with them; the
// arithmetic on them: pt_error_plan.hpp)
static int error_stats(pt_ctx* c, PtErrorStats* out, std::vector<float>& h) {
  h.clear();
  if (!c || !out) return fail(c, PT_ERR_INVALID, "pt_error_stats: NULL argument");
  if (!c->est.on) return option_off(c, "pt_error_stats", SET_ESTIMATE);
  PT_TRY(frame_buffers_ready(c, "pt_error_stats"));
  memset(out, 0, sizeof *out);
  out->pixels = (uint64_t)n_pixels(c);
  PT_HIP(c, hipSetDevice(c->device));
  if (int rc = launch_error_tiles(c); rc != PT_OK) return rc;
  const size_t tiles = (size_t)tiles_x(c) * tiles_y(c);
  if (tiles == 0) return PT_OK;
  h.resize(8 * tiles);
  PT_HIP(c, hipMemcpyAsync(h.data(), c->est.tiles.get(), 2 * tiles * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  pterr::sum_tiles(h.data(), tiles, out->pixels, out);
  return PT_OK;
}

PT_API int pt_error_stats(pt_ctx* c, PtErrorStats* out) {
  std::vector<float> h;
  return error_stats(c, out, h);
}

// ---- rendering to a noise target: pt_render_until and, choosing tiles between the launches, pt_render_adaptive -------------------
namespace {

// what both entry points ask of their arguments (`who`: the entry point; `per`: what it calls the passes of one launch)
int noise_target_args(pt_ctx* c, const char* who, const char* per, float target, uint32_t passes_per, uint32_t max_passes, const PtErrorStats* out) {
  if (!c || !out) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  if (!c->est.on) return option_off(c, who, SET_ESTIMATE, PT_ERR_INVALID);
  if (!(target > 0.0f) || !std::isfinite(target)) return fail(c, PT_ERR_INVALID, "%s: the target must be finite and positive", who);
  if (passes_per == 0 || max_passes == 0) return fail(c, PT_ERR_INVALID, "%s: no passes to render", who);
  if (passes_per > c->reserved_passes)
    return fail(c, PT_ERR_CAPACITY, "%s: %u passes per %s > %u reserved (pt_reserve_passes)", who, passes_per, per, c->reserved_passes);
  return PT_OK;
}

// the frame is the frame one uninterrupted call would give: the next launch goes on where this one ended (pass indices are
// frame-wide: the step does not depend on how many tiles ran)
void advance_first_pass(pt_ctx* c, uint32_t k) { c->params.first_pass += k; }

// what a look at the estimate adds to its stats
void mark_look(PtErrorStats* out, uint32_t done, float target) {
  out->passes_rendered = done;
  out->reached = pterr::target_reached(*out, target) ? 1u : 0u;
}

} // namespace

PT_API int pt_render_until(pt_ctx* c, float target_rel_error, uint32_t passes_per_launch, uint32_t max_passes, PtErrorStats* out) {
  if (int rc = noise_target_args(c, "pt_render_until", "launch", target_rel_error, passes_per_launch, max_passes, out); rc != PT_OK) return rc;
  if (int rc = not_capturing(c, "pt_render_until"); rc != PT_OK) return rc;
  uint32_t done = 0;
  for (;;) {
    const uint32_t k = passes_per_launch < max_passes - done ? passes_per_launch : max_passes - done;
    if (int rc = pt_render_passes(c, k); rc != PT_OK) return rc;
    advance_first_pass(c, k);
    done += k;
    if (int rc = pt_error_stats(c, out); rc != PT_OK) return rc;
    mark_look(out, done, target_rel_error);
    if (out->reached || done >= max_passes) return PT_OK;
  }
}

// ---- adaptive sampling (include/ptrace.h pt_render_adaptive; kernels: pt_kernels_error.hip) -----------------------------------
namespace {

// One partial round: k passes over the tiles flagged in c->h_adapt_flags (n_active of `tiles`, 0 < n_active < tiles).
int partial_round(pt_ctx* c, uint32_t k, uint32_t tiles, uint32_t n_active, uint64_t pixels_active) {
  const PtParams& p = c->params;
  PT_TRY(scene_and_uniforms(c, "pt_render_adaptive"));
  PT_HIP(c, hipSetDevice(c->device));
  if (c->d_adapt.capacity() != 3 * (size_t)tiles) {
    PT_HIP(c, hipStreamSynchronize(c->stream));
    PT_HIP(c, c->d_adapt.reserve(3 * (size_t)tiles));
  }
  uint32_t* flags = c->d_adapt.get();
  uint32_t* part = flags + tiles;
  uint32_t* base = part + tiles;
  changed(*c, ptstate::PARTIAL_ROUND_BEGINS);
  // the cost order up to date, as the next pt_render_passes would bring it — and never from costs that are all zero: the order
  // kernel would write the identity over a sorted order
  if (c->order.partial_wants_order_kernel()) {
    if (int rc = launch_tile_order(c); rc != PT_OK) return rc;
    c->order.order_kernel_ran();
  }
  PT_HIP(c, hipMemcpyAsync(flags, c->h_adapt_flags.data(), (size_t)tiles * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  PT_TRY(launch_partition(c, c->frame.tile_order.get(), flags, part, base, tiles));
  LaunchUse use;
  use.feedback = LaunchUse::OFF;  // a partial launch keeps the order it finds, as a frame does
  use.n_first_tiles = n_active;
  use.table = part;
  use.who = "pt_render_adaptive";
  TimedSpan span;
  if (int rc = trace_once(c, k, use, &span); rc != PT_OK) return rc;
  PT_HIP(c, call(ptsig::FoldErrorTiles{}, pt_error_kernel(PT_E_FOLD_TILES), dim3(tile_grid(n_active)), dim3(256), 0, c->stream,
                 c->frame.accum, c->est.state.get(), c->frame.slab.get(), part, n_active, c->width, c->local_rows, tiles_x(c), k));
  c->est.spp = p.samples_per_pixel;
  changed(*c, ptstate::PARTIAL_ROUND_DONE);
  c->adapt_tiles = tiles;
  c->adapt_active = n_active;
  c->tally.partial_round(pixels_active, k, (uint32_t)p.samples_per_pixel);
  return PT_OK;
}

} // namespace

PT_API int pt_render_adaptive(pt_ctx* c, float target_rel_error, uint32_t passes_per_round, uint32_t max_passes, PtErrorStats* out,
                              PtAdaptiveStats* adaptive_out) {
  if (int rc = noise_target_args(c, "pt_render_adaptive", "round", target_rel_error, passes_per_round, max_passes, out); rc != PT_OK) return rc;
  if (c->count_work) return fail(c, PT_ERR_INVALID, "pt_render_adaptive: not with PT_OPT_COUNT_WORK (the measuring twins log whole launches)");
  if (int rc = not_capturing(c, "pt_render_adaptive"); rc != PT_OK) return rc;
  // (refused before the first look: a call must not answer for an estimate it could not continue)
  if (c->state.have_params && c->est.spp != 0 && c->est.spp != c->params.samples_per_pixel)
    return fail(c, PT_ERR_INVALID, "pt_render_adaptive: %d samples per pixel while the error estimate holds passes of %d: clear first "
                                   "(pt_reset_accum)", c->params.samples_per_pixel, c->est.spp);
  const uint32_t tiles = n_tiles(c);
  PtAdaptiveStats ad;
  memset(&ad, 0, sizeof ad);
  ad.tiles = tiles;
  uint32_t n_active = 0;
  uint64_t pixels_active = 0;
  std::vector<float> h;
  uint32_t done = 0;
  // `act` starts from a look at the state the call finds.  A fresh estimate has every pixel short: all tiles.  A frame under way
  // goes on with the selection its state gives, so two calls are the rounds of one call of their passes together.
  auto look = [&]() -> int {
    if (int rc = error_stats(c, out, h); rc != PT_OK) return rc;
    mark_look(out, done, target_rel_error);
    c->h_adapt_flags.assign(h.size() / 8, 0u);  // (a flag per tile record)
    n_active = pterr::select_tiles(*out, target_rel_error, h.data(), c->h_adapt_flags.size(), c->h_adapt_flags.data());
    pixels_active = 0;
    for (uint32_t t = 0; t < tiles; t++)
      if (c->h_adapt_flags[t]) pixels_active += pterr::tile_pixels(c->width, c->local_rows, tiles_x(c), t);
    ad.tiles_active = n_active;
    return PT_OK;
  };
  int rc = look();
  while (rc == PT_OK && !out->reached && done < max_passes && n_active != 0) {
    const uint32_t k = passes_per_round < max_passes - done ? passes_per_round : max_passes - done;
    if (n_active == tiles) {
      rc = pt_render_passes(c, k);
    } else {
      rc = partial_round(c, k, tiles, n_active, pixels_active);
    }
    if (rc != PT_OK) break;
    ad.rounds++;
    ad.partial_rounds += n_active != tiles ? 1u : 0u;
    ad.tile_passes += (uint64_t)n_active * k;
    ad.samples += pixels_active * k * (uint64_t)c->params.samples_per_pixel;
    advance_first_pass(c, k);
    done += k;
    rc = look();
  }
  if (adaptive_out) *adaptive_out = ad;
  return rc;
}

PT_API int pt_adaptive_tiles(pt_ctx* c, uint32_t* base_out, uint32_t* order_out, uint32_t* n_tiles, uint32_t* n_active) {
  if (!c) return PT_ERR_INVALID;
  if (!c->state.adapt_valid) return fail(c, PT_ERR_NOT_READY, "pt_adaptive_tiles: no partial round yet (pt_render_adaptive)");
  if (n_tiles) *n_tiles = c->adapt_tiles;
  if (n_active) *n_active = c->adapt_active;
  if (!base_out && !order_out) return PT_OK;
  PT_HIP(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)c->adapt_tiles * sizeof(uint32_t);
  const uint32_t* part = c->d_adapt.get() + c->adapt_tiles;
  if (order_out) PT_HIP(c, hipMemcpyAsync(order_out, part, bytes, hipMemcpyDeviceToHost, c->stream));
  if (base_out) PT_HIP(c, hipMemcpyAsync(base_out, part + c->adapt_tiles, bytes, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_get_stats(pt_ctx* c, PtStats* out) {
  if (!c || !out) return PT_ERR_INVALID;
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  int rc = fold_events(c);
  if (rc != PT_OK) return rc;
  unsigned long long ctr[PT_CTR_COUNT];
  PT_HIP(c, hipMemcpy(ctr, c->d_counters.get(), sizeof ctr, hipMemcpyDeviceToHost));
  memset(out, 0, sizeof *out);
  out->segments = ctr[PT_CTR_SEGMENTS];
  out->samples = c->tally.samples;
  out->sphere_tests = ctr[PT_CTR_SEGMENTS] * (uint64_t)c->list.n;
  out->render_kernel_ms = c->kernel_ms;
  out->render_launches = c->tally.launches;
  out->total_spp = c->tally.total_spp;
  if (c->frame.accum && c->local_rows) { // what the device has really accumulated (graph replays included)
    float4 px0;
    PT_HIP(c, hipMemcpy(&px0, c->frame.accum, sizeof px0, hipMemcpyDeviceToHost));
    if (px0.w >= 0.0f && px0.w < 4294967040.0f) out->total_spp = (uint32_t)px0.w;
  }
  out->n_spheres = c->list.n;
  try_finish_tuning(c);
  out->local_rows = c->local_rows;
  out->geometry_path = (uint32_t)c->geom.last;
  out->geometry_tuned = c->geom.tuned ? 1u : 0u;
  for (int k = 0; k < 8; k++) out->work[k] = ctr[PT_CTR_WORK + k];
  out->far_rays = ctr[PT_CTR_FAR_RAYS];
  if (c->grid.present) {
    for (int k = 0; k < 3; k++) out->grid_cells[k] = c->grid.head.n[k];
    out->grid_entries = c->grid.head.n_entries;
    out->grid_always = c->grid.head.n_always;
    out->grid_near_factor = c->grid.head.near_factor;
    out->grid_need_factor = (float)need_factor(c);
    out->grid_fit_stale = (uint32_t)fit_state(c);
    out->grid_kernel_build = (uint32_t)grid_build(c).kind;
    out->grid_walk_flat = grid_walk_flat((int)out->grid_kernel_build, c->grid.head.n[1]) ? 1u : 0u;
  }
  if (c->bvh.present) {
    out->bvh_nodes = c->bvh.head.n_nodes;
    out->bvh_slots = c->bvh.head.n_slots;
    out->bvh_outliers = c->bvh.head.n_outliers;
    out->bvh_depth = c->bvh.head.depth;
  }
  return PT_OK;
}

// An option that owns a set of buffers (`name`: the option's words in pt_set_option's messages).  The image does not depend on
// any of them; the set is allocated here and released when the option is turned off.  Drains the stream first: work in flight
// may use the set.  `off` releases the set and what hangs on it; `kernel` is one of the option's code object — asking for its
// attributes loads that object now: a set-up call's work, not a render call's —; `extra` is what the option needs beyond its
// buffers once they are in place.  Whatever fails, the option stays off with everything released.
template <class Set, class Off, class Extra>
static int set_buffer_option(pt_ctx* c, int value, const char* name, Set& set, Off off, const void* kernel, Extra extra) {
  if (value != 0 && value != 1) return fail(c, PT_ERR_INVALID, "pt_set_option: %s %d", name, value);
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  if (!value) { off(); return PT_OK; }
  if (set.on) return PT_OK;
  hipFuncAttributes attr;
  PT_HIP(c, hipFuncGetAttributes(&attr, kernel));
  set.on = true;
  int rc = ensure_buffers(c);
  if (rc == PT_OK) rc = extra();
  if (rc != PT_OK) off();
  return rc;
}

PT_API int pt_set_option(pt_ctx* c, int key, int value) {
  if (!c) return PT_ERR_INVALID;
  if (key == PT_OPT_GEOMETRY_PATH) {
    if (value != PT_GEOM_AUTO && value != PT_GEOM_LDS && value != PT_GEOM_SCALAR && value != PT_GEOM_BVH &&
        value != PT_GEOM_GRID && value != PT_GEOM_SMALL)
      return fail(c, PT_ERR_INVALID, "pt_set_option: bad geometry path %d", value);
    c->geom.policy = value;
    return PT_OK;
  }
  if (key == PT_OPT_COUNT_WORK) { // measuring twin of the walk kernels (PtStats.work); slower, never timed
    if (value > 0 && c->lights.on)
      return fail(c, PT_ERR_INVALID, "pt_set_option: PT_OPT_COUNT_WORK and PT_OPT_NEXT_EVENT exclude each other (turn next-event estimation off first: "
                                     "pt_set_option(ctx, PT_OPT_NEXT_EVENT, 0))");
    c->count_work = value < 0 ? 0 : (value > 2 ? 2 : value);  // 2 (dev tools only): the grid twins also fill the gather histogram (pt_debug_cell_hist)
    return PT_OK;
  }
  if (key == PT_OPT_REFILL_MIN) { // scheduling only, never results
    if (value < 1 || value > 64) return fail(c, PT_ERR_INVALID, "pt_set_option: refill min %d", value);
    c->refill_min = (uint32_t)value;
    return PT_OK;
  }
  if (key == PT_OPT_RUSSIAN_ROULETTE) { // changes sample values (not expectations): off unless asked for
    if (value < 0 || value > 1000000) return fail(c, PT_ERR_INVALID, "pt_set_option: roulette depth %d", value);
    if (value > 0 && c->dbg_enable)
      return fail(c, PT_ERR_INVALID, "pt_set_option: PT_OPT_RUSSIAN_ROULETTE and the debug overlay exclude each other (turn the overlay off first: "
                                     "pt_set_debug_overlay(ctx, 0, ...))");
    if (value > 0 && c->lights.on)
      return fail(c, PT_ERR_INVALID, "pt_set_option: PT_OPT_RUSSIAN_ROULETTE and PT_OPT_NEXT_EVENT exclude each other (turn next-event estimation off first: "
                                     "pt_set_option(ctx, PT_OPT_NEXT_EVENT, 0))");
    c->rr_min_depth = value;
    return PT_OK;
  }
  if (key == PT_OPT_NEXT_EVENT) { // changes sample values (not expectations): off unless asked for
    if (value != 0 && value != 1) return fail(c, PT_ERR_INVALID, "pt_set_option: next-event estimation %d", value);
    if (value && c->rr_min_depth > 0)
      return fail(c, PT_ERR_INVALID, "pt_set_option: PT_OPT_NEXT_EVENT and PT_OPT_RUSSIAN_ROULETTE exclude each other (turn roulette off first: "
                                     "pt_set_option(ctx, PT_OPT_RUSSIAN_ROULETTE, 0))");
    if (value && c->dbg_enable)
      return fail(c, PT_ERR_INVALID, "pt_set_option: PT_OPT_NEXT_EVENT and the debug overlay exclude each other (turn the overlay off first: "
                                     "pt_set_debug_overlay(ctx, 0, ...))");
    if (value && c->count_work)
      return fail(c, PT_ERR_INVALID, "pt_set_option: PT_OPT_NEXT_EVENT and PT_OPT_COUNT_WORK exclude each other (turn the measuring twins off first: "
                                     "pt_set_option(ctx, PT_OPT_COUNT_WORK, 0))");
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipStreamSynchronize(c->stream));  // launches in flight may read the table in place
    if (!value) { c->lights.release(); return PT_OK; }
    if (c->lights.on) return PT_OK;
    hipFuncAttributes attr;  // (loads the next-event builds' code object now: a set-up call's work, not a render call's)
    PT_HIP(c, hipFuncGetAttributes(&attr, pt_nee_kernel(PT_VARIANT_ID(pt_trace_kernel_scalar))));
    c->lights.on = true;
    if (c->state.have_spheres) {  // over an installed scene: its table, now
      int rc = upload_lights(c, c->list.host, c->list.n);
      if (rc != PT_OK) { c->lights.release(); return rc; }
    }
    return PT_OK;
  }
  if (key == PT_OPT_CARRY_LANES) { // 0 = lockstep to the last lane; scheduling only, never results
    if (value < 0 || value > 64) return fail(c, PT_ERR_INVALID, "pt_set_option: carry lanes %d", value);
    c->carry_lanes = (uint32_t)value;
    return PT_OK;
  }
  if (key == PT_OPT_GRID_FIT) { // how pt_tune chooses the grid's margin class; speed only, never results
    if (value != 0 && value != 1) return fail(c, PT_ERR_INVALID, "pt_set_option: grid fit mode %d", value);
    c->grid_fit_mode = value;
    return PT_OK;
  }
  // (reprojection reads the feature planes and stages the estimate's state: off with the former, and the stage with it)
  auto reproject_off = [c] { c->hist.release(); c->est.stage.release(); };
  auto uuids = [c] { return !c->state.uuid_valid && c->state.have_spheres ? upload_uuids(c, c->list.host.uuid) : PT_OK; };  // the scene in place
  if (key == PT_OPT_ERROR_ESTIMATE)
    return set_buffer_option(c, value, "error estimate", c->est, [c] { c->est.release(); }, pt_error_kernel(PT_E_FOLD), [c] { return clear_error(c); });
  if (key == PT_OPT_FEATURES)
    return set_buffer_option(c, value, "feature planes", c->feat, [&] { c->feat.release(); c->probe.release_stage(); reproject_off(); },
                             pt_feature_kernel(PT_VARIANT_ID(pt_trace_kernel_scalar)), uuids);
  if (key == PT_OPT_RAY_QUERIES)
    return set_buffer_option(c, value, "ray queries", c->query, [c] { c->query.release(); c->gather.release(); c->probe.release_points(); }, pt_query_kernel(PT_VARIANT_ID(pt_trace_kernel_scalar)), uuids);
  if (key == PT_OPT_REPROJECT) {
    if (value == 1 && !c->feat.on) return fail(c, PT_ERR_INVALID, "pt_set_option: PT_OPT_REPROJECT needs PT_OPT_FEATURES on (it reads the feature planes)");
    return set_buffer_option(c, value, "reprojection", c->hist, reproject_off, pt_reproject_kernel_handle(), [] { return PT_OK; });
  }
  if (key == PT_OPT_TONEMAP)
    return set_buffer_option(c, value, "tone mapping", c->expo, [c] { c->expo.release(); }, pt_display_kernel(PT_D_METER), [] { return PT_OK; });
  if (key == PT_OPT_GLARE)
    return set_buffer_option(c, value, "glare", c->glare, [c] { c->glare.release(); }, pt_glare_kernel(PT_G_DOWN), [] { return PT_OK; });
  return fail(c, PT_ERR_INVALID, "pt_set_option: unknown key %d", key);
}

// u_enable_debugging / u_selected_object / u_cursor_point (static/shader.frag:100-102; the reference uploads them every frame,
// src/webgl.rs:554-587).  Copies; takes effect from the next render call (a captured frame bakes the values in: the plans of
// pt_render_frames differ and their graphs are captured again).
PT_API int pt_set_debug_overlay(pt_ctx* c, int enable, int32_t selected_object, const float cursor_point[3]) {
  if (!c) return PT_ERR_INVALID;
  if (enable && !cursor_point) return fail(c, PT_ERR_INVALID, "pt_set_debug_overlay: cursor_point is NULL");
  if (enable && c->rr_min_depth > 0)
    return fail(c, PT_ERR_INVALID, "pt_set_debug_overlay: the debug overlay and PT_OPT_RUSSIAN_ROULETTE exclude each other (turn roulette off first: "
                                   "pt_set_option(ctx, PT_OPT_RUSSIAN_ROULETTE, 0))");
  if (enable && c->lights.on)
    return fail(c, PT_ERR_INVALID, "pt_set_debug_overlay: the debug overlay and PT_OPT_NEXT_EVENT exclude each other (turn next-event estimation off first: "
                                   "pt_set_option(ctx, PT_OPT_NEXT_EVENT, 0))");
  if (!enable) {
    c->dbg_enable = false;
    return PT_OK;
  }
  if (!c->state.uuid_valid && c->state.have_spheres) {
    int rc = upload_uuids(c, c->list.host.uuid);
    if (rc != PT_OK) return rc;
  }
  c->dbg_enable = true;
  c->dbg_selected = selected_object;
  for (int k = 0; k < 3; k++) c->dbg_cursor[k] = cursor_point[k];
  return PT_OK;
}

// which build of the trace kernel the most recent launch was: 0 plain, 1 Russian roulette, 2 measuring twin, 3 debug overlay,
// 4 first-hit features, 16 next-event estimation (no column of the trace table: pt_nee_table.hpp)
PT_API int pt_last_trace_build(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  return c->last_build;
}

// ---- first-hit feature planes (PT_OPT_FEATURES; include/ptrace.h has the record) ---------------------------------------------
// (the planes are in place for the local rows unless an allocation failed: ensure_buffers sizes them wherever the rows change)
// ONE launch of the feature build of whichever kernel the context renders with, into the planes.  Nothing else of the context
// moves: no fold, no timing events, no tile costs, no order kernel, no trial of PT_GEOM_AUTO (prepare_launch, DOOR_FEATURES);
// the kernel adds its segments to the device counter like every trace launch.
PT_API int pt_render_features(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  if (c->count_work) return fail(c, PT_ERR_INVALID, "pt_render_features: not with PT_OPT_COUNT_WORK (the measuring twins have no feature build)");
  PT_TRY(scene_and_uniforms(c, "pt_render_features"));
  if (!c->feat.on) return option_off(c, "pt_render_features", SET_FEATURES);
  PT_HIP(c, hipSetDevice(c->device));
  if (is_capturing(c)) return fail(c, PT_ERR_INVALID, "pt_render_features: not inside a stream capture");
  if (!c->feat.in_place(extent_of(c))) return fail(c, PT_ERR_CAPACITY, "pt_render_features: the planes are not allocated for the rows in place (an earlier allocation failed)");
  if (c->local_rows == 0) { c->feat.valid = true; return PT_OK; }  // this band owns no rows: nothing to do, and its (empty) planes speak
  LaunchUse use;
  use.door = DOOR_FEATURES;
  use.who = "pt_render_features";
  if (int rc = trace_once(c, 1, use); rc != PT_OK) return rc;
  c->feat.valid = true;
  return PT_OK;
}

PT_API int pt_features_ptr(pt_ctx* c, int plane, void** dev_ptr, size_t* bytes) {
  if (!c || !dev_ptr) return fail(c, PT_ERR_INVALID, "pt_features_ptr: NULL argument");
  if (plane < 0 || plane >= PT_FEAT_PLANES) return fail(c, PT_ERR_INVALID, "pt_features_ptr: plane %d out of range", plane);
  if (!c->feat.on) return option_off(c, "pt_features_ptr", SET_FEATURES);
  if (!c->feat.in_place(extent_of(c))) return fail(c, PT_ERR_CAPACITY, "pt_features_ptr: the planes are not allocated for the rows in place (an earlier allocation failed)");
  *dev_ptr = c->feat.planes.get() + (size_t)plane * n_pixels(c);
  if (bytes) *bytes = n_pixels(c) * sizeof(float4);
  return PT_OK;
}

PT_API int pt_read_features(pt_ctx* c, int plane, void* out) {
  if (!c || !out) return fail(c, PT_ERR_INVALID, "pt_read_features: NULL argument");
  if (plane < 0 || plane >= PT_FEAT_PLANES) return fail(c, PT_ERR_INVALID, "pt_read_features: plane %d out of range", plane);
  if (c->count_work) return fail(c, PT_ERR_INVALID, "pt_read_features: not with PT_OPT_COUNT_WORK");
  if (!c->feat.on) return option_off(c, "pt_read_features", SET_FEATURES);
  if (!c->feat.valid)
    return fail(c, PT_ERR_NOT_READY, "pt_read_features: no pt_render_features since the scene, the uniforms or the size last changed");
  PT_HIP(c, hipSetDevice(c->device));
  if (is_capturing(c)) return fail(c, PT_ERR_INVALID, "pt_read_features: not inside a stream capture (a read-out synchronises)");
  const size_t need = n_pixels(c) * sizeof(float4);
  if (need) PT_HIP(c, hipMemcpyAsync(out, c->feat.planes.get() + (size_t)plane * n_pixels(c), need, hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

// ---- ray queries (PT_OPT_RAY_QUERIES; include/ptrace.h has the contract) --------------------------------------
// can the device read (and write) this pointer of the caller's?  A pointer the runtime does not know is the host's.
static bool device_pointer(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

PT_API uint32_t pt_query_batch(pt_ctx* c) {
  if (!c || !c->query.on || !c->state.have_spheres || !c->state.have_params || c->local_rows == 0 || !c->query.in_place(extent_of(c))) return 0u;
  return (uint32_t)n_pixels(c);
}

// What pt_query_rays and pt_query_radiance (`who`; `build`: its word for the kernels the measuring twins lack) both ask of their
// arguments and the context before anything is enqueued.
static int query_ready(pt_ctx* c, const char* who, const char* build, const void* rays, const void* out) {
  if (!rays || !out) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  if (c->count_work) return fail(c, PT_ERR_INVALID, "%s: not with PT_OPT_COUNT_WORK (the measuring twins have no %s build)", who, build);
  if (!c->query.on) return option_off(c, who, SET_QUERIES);
  PT_TRY(scene_and_uniforms(c, who));
  PT_HIP(c, hipSetDevice(c->device));
  PT_TRY(not_capturing(c, who));
  if (c->local_rows == 0) return fail(c, PT_ERR_NOT_READY, "%s: this band owns no rows, so it has no work items to decode rays against", who);
  if (!c->query.in_place(extent_of(c))) return fail(c, PT_ERR_CAPACITY, "%s: the planes are not allocated for the rows in place (an earlier allocation failed)", who);
  return frame_buffers_ready(c, who);  // (before the first ray is staged, not only at the launch)
}

// One batch of m rays into the point and normal planes of the query planes: a device array through the pack kernel, a host array
// packed into h_in (the caller's, so that nothing is allocated per batch) and copied plane by plane.
static int stage_rays(pt_ctx* c, const PtRay* rays, bool on_device, uint32_t m, std::vector<ptq::F4>& h_in) {
  ptq::F4* planes = reinterpret_cast<ptq::F4*>(c->query.planes.get());
  const uint32_t plane = (uint32_t)n_pixels(c);
  if (on_device) {
    PT_HIP(c, call(ptsig::QueryPack{}, pt_query_pack_kernel_handle(), dim3((m + 255u) / 256u), dim3(256), 0, c->stream, rays, m, planes, plane));
    return PT_OK;
  }
  h_in.resize(2 * (size_t)m);
  for (uint32_t i = 0; i < m; i++) ptq::pack_ray(rays[i], &h_in[i], &h_in[(size_t)m + i]);
  PT_HIP(c, hipMemcpyAsync(planes + (size_t)PT_FEAT_POINT * plane, h_in.data(), (size_t)m * sizeof(ptq::F4), hipMemcpyHostToDevice, c->stream));
  PT_HIP(c, hipMemcpyAsync(planes + (size_t)PT_FEAT_NORMAL * plane, h_in.data() + m, (size_t)m * sizeof(ptq::F4), hipMemcpyHostToDevice, c->stream));
  return PT_OK;
}

// What the three _nee entry points ask beyond their namesakes, after the namesake's own checks: the option on — refused the way
// an off PT_OPT_RAY_QUERIES is — and its light table in place (prepare_launch's sentence, before anything is staged).  With the
// option on the context has no roulette, overlay or twins (pt_set_option's exclusions): nothing else to exclude.
static int estimator_ready(pt_ctx* c, const char* who, bool next_event) {
  if (!next_event) return PT_OK;
  if (!c->lights.on) return option_off(c, who, SET_NEXT_EVENT);
  if (!c->lights.in_place()) return fail(c, PT_ERR_CAPACITY, "%s: PT_OPT_NEXT_EVENT's light table is not in place (a failed allocation: install the scene or turn the option on again)", who);
  return PT_OK;
}

// The launch of a batch of m staged rays through `door`: over the tile rows the rays occupy, in the query planes' own tile order.
static LaunchUse batch_use(const pt_ctx* c, Door door, uint32_t m) {
  LaunchUse use;
  use.door = door;
  use.who = door == DOOR_QUERY ? "pt_query_rays" : "pt_query_radiance";
  use.query_rays = m;
  use.n_first_tiles = ptq::tiles_covered(m, c->width);
  use.table = c->query.order.get();
  return use;
}

// n rays in batches of the local pixel count; a batch: stage the rays into the point and normal planes (stage_rays), ONE launch
// of the query build over the tile rows the rays occupy, the records out of the four planes (the unpack kernel, or four copies
// and the host's unpack).  Nothing else of the context moves (prepare_launch, DOOR_QUERY).
PT_API int pt_query_rays(pt_ctx* c, const PtRay* rays, uint32_t n, PtRayHit* hits) {
  if (!c) return PT_ERR_INVALID;
  if (n == 0) return PT_OK;
  if (int rc = query_ready(c, "pt_query_rays", "query", rays, hits); rc != PT_OK) return rc;
  const uint32_t plane = (uint32_t)n_pixels(c);
  const bool rays_on_device = device_pointer(rays), hits_on_device = device_pointer(hits);
  const ptq::F4* planes = reinterpret_cast<const ptq::F4*>(c->query.planes.get());
  std::vector<ptq::F4> h_in, h_out;  // host arrays only: the two planes going up, the four coming down
  const uint32_t batches = ptq::n_batches(n, plane);
  for (uint32_t k = 0; k < batches; k++) {
    const size_t first = (size_t)k * plane;
    const uint32_t m = ptq::batch_rays(n, plane, k);
    if (int rc = stage_rays(c, rays + first, rays_on_device, m, h_in); rc != PT_OK) return rc;
    if (int rc = trace_once(c, 1, batch_use(c, DOOR_QUERY, m)); rc != PT_OK) return rc;
    if (hits_on_device) {
      PT_HIP(c, call(ptsig::QueryUnpack{}, pt_query_unpack_kernel_handle(), dim3((m + 255u) / 256u), dim3(256), 0, c->stream, planes, plane, m, hits + first));
    } else {
      h_out.resize(PT_FEAT_PLANES * (size_t)m);
      for (int q = 0; q < PT_FEAT_PLANES; q++)
        PT_HIP(c, hipMemcpyAsync(h_out.data() + (size_t)q * m, planes + (size_t)q * plane, (size_t)m * sizeof(ptq::F4), hipMemcpyDeviceToHost, c->stream));
    }
    // (the next batch stages into the planes this one reads out of, and a host batch is unpacked from h_out)
    PT_HIP(c, hipStreamSynchronize(c->stream));
    if (!hits_on_device) {
      const ptq::I4* ids = reinterpret_cast<const ptq::I4*>(h_out.data() + (size_t)PT_FEAT_IDS * m);
      for (uint32_t i = 0; i < m; i++)
        hits[first + i] = ptq::unpack_hit(h_out[(size_t)PT_FEAT_ALBEDO * m + i], h_out[(size_t)PT_FEAT_NORMAL * m + i], h_out[(size_t)PT_FEAT_POINT * m + i], ids[i]);
    }
  }
  return PT_OK;
}

// ---- radiance queries (needs PT_OPT_RAY_QUERIES; include/ptrace.h has the contract) ---------------------------
// n_passes of a radiance or gather call: not zero, and no more than the pass slabs hold
static int passes_ready(pt_ctx* c, const char* who, uint32_t n_passes) {
  if (n_passes == 0) return fail(c, PT_ERR_INVALID, "%s: n_passes == 0", who);
  if (n_passes > c->reserved_passes)
    return fail(c, PT_ERR_CAPACITY, "%s: %u passes > %u reserved (pt_reserve_passes)", who, n_passes, c->reserved_passes);
  return PT_OK;
}

// THE RADIANCE BATCH of pt_query_radiance and the gather calls: batch k's m rays, which the caller has staged in the query
// planes, through ONE launch of the row's radiance build and ONE fold of its pass slabs into `dst`, m records on the device.
// Enqueued, not awaited.
static int radiance_batch(pt_ctx* c, const char* who, bool next_event, uint32_t k, uint32_t m, uint32_t n_passes, PtRayRadiance* dst) {
  LaunchUse use = batch_use(c, DOOR_RADIANCE, m);
  use.who = who;
  use.next_event = next_event;
  use.first_pass = ptr::batch_first_pass(c->params.first_pass, k, n_passes);
  if (int rc = trace_once(c, n_passes, use); rc != PT_OK) return rc;
  PT_HIP(c, call(ptsig::RadianceFold{}, pt_radiance_fold_kernel_handle(), dim3((m + 255u) / 256u), dim3(256), 0, c->stream,
                 c->frame.slab.get(), (uint32_t)n_pixels(c), n_passes, c->query.planes.get(), m, dst));
  return PT_OK;
}

// n rays in batches of the local pixel count, as pt_query_rays deals them; a batch: stage the rays into the point and normal
// planes of the query planes (pt_query_rays' own staging), ONE launch of the row's radiance build over the tile rows the rays
// occupy — n_passes passes of the batch's own into the pass slabs — and ONE fold of those slabs into the records
// (radiance_batch): straight into a device `out`, or into the query planes' first plane (a record is a texel) and
// copied from there.  Nothing is allocated per call but the host vector of a host batch's staging.
// Both estimators share the body: `next_event` is pt_query_radiance_nee's (its own precondition after the namesake's checks, its
// own side table's cell at the launch: LaunchUse::next_event), and nothing else differs.
static int query_radiance(pt_ctx* c, const char* who, bool next_event, const PtRay* rays, uint32_t n, uint32_t n_passes, PtRayRadiance* out) {
  if (!c) return PT_ERR_INVALID;
  if (n == 0) return PT_OK;
  if (int rc = query_ready(c, who, "radiance", rays, out); rc != PT_OK) return rc;
  if (int rc = passes_ready(c, who, n_passes); rc != PT_OK) return rc;
  if (int rc = estimator_ready(c, who, next_event); rc != PT_OK) return rc;
  static_assert(sizeof(PtRayRadiance) == sizeof(ptq::F4), "a record is a texel: the fold's scratch is a plane");
  const uint32_t plane = (uint32_t)n_pixels(c);
  const bool rays_on_device = device_pointer(rays), out_on_device = device_pointer(out);
  PtRayRadiance* scratch = reinterpret_cast<PtRayRadiance*>(c->query.planes.get() + (size_t)PT_FEAT_ALBEDO * plane);
  std::vector<ptq::F4> h_in;  // host rays only: the two planes going up
  const uint32_t batches = ptq::n_batches(n, plane);
  for (uint32_t k = 0; k < batches; k++) {
    const size_t first = (size_t)k * plane;
    const uint32_t m = ptq::batch_rays(n, plane, k);
    if (int rc = stage_rays(c, rays + first, rays_on_device, m, h_in); rc != PT_OK) return rc;
    PtRayRadiance* dst = out_on_device ? out + first : scratch;
    if (int rc = radiance_batch(c, who, next_event, k, m, n_passes, dst); rc != PT_OK) return rc;
    if (!out_on_device) PT_HIP(c, hipMemcpyAsync(out + first, dst, (size_t)m * sizeof(PtRayRadiance), hipMemcpyDeviceToHost, c->stream));
    // (the next batch stages into the planes this one's fold reads, and a host batch's vector is packed again)
    PT_HIP(c, hipStreamSynchronize(c->stream));
  }
  return PT_OK;
}

PT_API int pt_query_radiance(pt_ctx* c, const PtRay* rays, uint32_t n, uint32_t n_passes, PtRayRadiance* out) {
  return query_radiance(c, "pt_query_radiance", false, rays, n, n_passes, out);
}
PT_API int pt_query_radiance_nee(pt_ctx* c, const PtRay* rays, uint32_t n, uint32_t n_passes, PtRayRadiance* out) {
  return query_radiance(c, "pt_query_radiance_nee", true, rays, n, n_passes, out);
}

// ---- gather queries (needs PT_OPT_RAY_QUERIES; include/ptrace.h has the contract) ------------------------------
// What every gather call asks before anything is enqueued: pt_query_radiance's checks in its order, with the direction count
// and the ray total between the passes and the estimator.  `in` is the caller's array of items (pt_bake_lattice: its lattice).
static int gather_ready(pt_ctx* c, const char* who, bool next_event, const void* in, uint32_t n, uint32_t D, uint32_t n_passes, const void* out) {
  if (int rc = query_ready(c, who, "radiance", in, out); rc != PT_OK) return rc;
  if (int rc = passes_ready(c, who, n_passes); rc != PT_OK) return rc;
  if (!ptgather::directions_valid(D))
    return fail(c, PT_ERR_INVALID, "%s: %u directions (a multiple of 64 in [%d, %d])", who, D, (int)ptgather::kMinDirections, (int)ptgather::kMaxDirections);
  if (ptgather::total_rays(n, D) == 0) return fail(c, PT_ERR_INVALID, "%s: %u items of %u directions are more than 2^32 - 1 rays", who, n, D);
  return estimator_ready(c, who, next_event);
}

// The batches of a gather call that gather_ready has passed (n > 0), behind pt_gather_irradiance, pt_bake_probes and
// pt_bake_lattice: the workspace in place, then the n * D rays of the defining sentence in pt_query_radiance's batches.  A batch:
// the items it touches into the workspace (a host array's; a device array is read in place), the generator in stage_rays' place,
// pt_query_radiance's launch and fold as they are (radiance_batch) — the folded records wait in the query planes' first plane,
// where a host call's wait for their copy — and the reduce over the items the batch touches: an item that ends in the batch is
// written (straight into a device `out`, or into the workspace and copied from there), the one that goes on leaves its lanes'
// partial sums in the workspace for the next batch.
static int gather_batches(pt_ctx* c, const char* who, int kind, bool next_event, const PtGatherPoint* points, uint32_t n, uint32_t D, uint32_t n_passes, void* out) {
  const ptbuf::Extent e = extent_of(c);
  if (!c->gather.in_place(e)) {
    if (const ptbuf::Fit f = c->gather.fit(e); !f.ok())
      return fail(c, PT_ERR_CAPACITY, "%s: the workspace's allocation for %zu local pixels failed: %s", who, e.pix, hipGetErrorString((hipError_t)f.err));
  }
  const uint32_t plane = (uint32_t)n_pixels(c), total = (uint32_t)ptgather::total_rays(n, D);
  const size_t record = kind == ptgather::PROBE ? sizeof(PtProbeSH) : sizeof(PtIrradiance);
  const bool points_on_device = device_pointer(points), out_on_device = device_pointer(out);
  PtRayRadiance* folded = reinterpret_cast<PtRayRadiance*>(c->query.planes.get() + (size_t)PT_FEAT_ALBEDO * plane);
  PtGatherPoint* staged_points = reinterpret_cast<PtGatherPoint*>(c->gather.points());
  void* staged_out = c->gather.records(e);
  const uint32_t batches = ptq::n_batches(total, plane);
  for (uint32_t k = 0; k < batches; k++) {
    const uint32_t first = (uint32_t)((uint64_t)k * plane), m = ptq::batch_rays(total, plane, k);
    // the items the batch touches — no more than the workspace holds (ptgather::items_per_batch: m <= plane) — and those of
    // them that end in it
    const ptgather::ItemSpan s = ptgather::item_span(first, m, D);
    const PtGatherPoint* pts = points + s.item0;
    if (!points_on_device) {
      PT_HIP(c, hipMemcpyAsync(staged_points, pts, (size_t)s.items * sizeof(PtGatherPoint), hipMemcpyHostToDevice, c->stream));
      pts = staged_points;
    }
    PT_HIP(c, call(ptsig::GatherRays{}, pt_gather_kernel(PT_GATHER_RAYS), dim3((m + 255u) / 256u), dim3(256), 0, c->stream,
                   pts, s.item0, first, m, D, kind, c->query.planes.get(), plane));
    if (int rc = radiance_batch(c, who, next_event, k, m, n_passes, folded); rc != PT_OK) return rc;
    // (batch k writes the carry slot of its parity and reads the other, which batch k - 1 wrote: never one slot in one launch)
    PT_HIP(c, call(ptsig::GatherReduce{}, pt_gather_kernel(PT_GATHER_REDUCE), dim3((s.items + 3u) / 4u), dim3(256), 0, c->stream,
                   folded, pts, s.item0, s.items, first, m, D, kind, c->gather.carry(k + 1u), c->gather.carry(k),
                   out_on_device ? out : staged_out, out_on_device ? 0u : s.done0));
    if (!out_on_device && s.done1 > s.done0)
      PT_HIP(c, hipMemcpyAsync(static_cast<char*>(out) + (size_t)s.done0 * record, staged_out, (size_t)(s.done1 - s.done0) * record, hipMemcpyDeviceToHost, c->stream));
    // (the next batch stages into the planes and the workspace this one reads)
    PT_HIP(c, hipStreamSynchronize(c->stream));
  }
  return PT_OK;
}

static int gather(pt_ctx* c, const char* who, int kind, bool next_event, const PtGatherPoint* points, uint32_t n, uint32_t D, uint32_t n_passes, void* out) {
  if (!c) return PT_ERR_INVALID;
  if (n == 0) return PT_OK;
  if (int rc = gather_ready(c, who, next_event, points, n, D, n_passes, out); rc != PT_OK) return rc;
  return gather_batches(c, who, kind, next_event, points, n, D, n_passes, out);
}

PT_API int pt_gather_irradiance(pt_ctx* c, const PtGatherPoint* points, uint32_t n, uint32_t directions, uint32_t n_passes, PtIrradiance* out) {
  return gather(c, "pt_gather_irradiance", ptgather::IRRADIANCE, false, points, n, directions, n_passes, out);
}
PT_API int pt_bake_probes(pt_ctx* c, const PtGatherPoint* probes, uint32_t n, uint32_t directions, uint32_t n_passes, PtProbeSH* out) {
  return gather(c, "pt_bake_probes", ptgather::PROBE, false, probes, n, directions, n_passes, out);
}
PT_API int pt_gather_irradiance_nee(pt_ctx* c, const PtGatherPoint* points, uint32_t n, uint32_t directions, uint32_t n_passes, PtIrradiance* out) {
  return gather(c, "pt_gather_irradiance_nee", ptgather::IRRADIANCE, true, points, n, directions, n_passes, out);
}
PT_API int pt_bake_probes_nee(pt_ctx* c, const PtGatherPoint* probes, uint32_t n, uint32_t directions, uint32_t n_passes, PtProbeSH* out) {
  return gather(c, "pt_bake_probes_nee", ptgather::PROBE, true, probes, n, directions, n_passes, out);
}

// ---- probe lattices (no option of their own; include/ptrace.h has the contract) ------------------------------
// pt_bake_lattice: the lattice's own checks, the gather calls' (gather_ready, once: no generator runs for a call that is
// refused), the generator into the ProbeSet's point buffer, then the gather calls' batches on that DEVICE pointer: the defining
// sentence by construction, and no second copy of the bake loop.
PT_API int pt_bake_lattice(pt_ctx* c, const PtProbeLattice* lattice, uint32_t first, uint32_t count, uint32_t directions, uint32_t n_passes, int estimator,
                           PtProbeSH* out) {
  if (!c) return PT_ERR_INVALID;
  const char* who = "pt_bake_lattice";
  if (!lattice) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  if (const char* why = ptprobe::lattice_error(*lattice)) return fail(c, PT_ERR_INVALID, "%s: %s", who, why);
  if (estimator != 0 && estimator != 1) return fail(c, PT_ERR_INVALID, "%s: estimator %d (0: pt_bake_probes, 1: pt_bake_probes_nee)", who, estimator);
  if (!ptprobe::slice_valid(*lattice, first, count))
    return fail(c, PT_ERR_INVALID, "%s: nodes %u .. %u + %u of a lattice of %u", who, first, first, count, ptprobe::node_count(*lattice));
  if (count == 0) return PT_OK;
  const bool next_event = estimator == 1;
  if (int rc = gather_ready(c, who, next_event, lattice, count, directions, n_passes, out); rc != PT_OK) return rc;
  if (!c->probe.points_in_place(count)) {
    PT_HIP(c, hipStreamSynchronize(c->stream));  // (nothing in flight reads what the fit frees)
    if (const ptbuf::Fit f = c->probe.fit_points(count); !f.ok())
      return fail(c, PT_ERR_CAPACITY, "%s: the point buffer's allocation for %u nodes failed: %s", who, count, hipGetErrorString((hipError_t)f.err));
  }
  PtGatherPoint* points = reinterpret_cast<PtGatherPoint*>(c->probe.points.get());
  PT_HIP(c, call(ptsig::ProbePoints{}, pt_lattice_kernel(PT_PROBE_POINTS), dim3((count + 255u) / 256u), dim3(256), 0, c->stream,
                 *lattice, first, count, c->list.geom.get(), c->list.mat.get(), c->list.n, points));
  return gather_batches(c, who, ptgather::PROBE, next_event, points, count, directions, n_passes, out);
}

PT_API int pt_debug_probe_form(pt_ctx* c, int form, uint32_t* paths_dev) {
  if (!c) return PT_ERR_INVALID;
  if (form == -1) form = kProbeFormDefault;
  if (form != 0 && form != 1) return fail(c, PT_ERR_INVALID, "pt_debug_probe_form: form %d", form);
  if (form == 0 && paths_dev) return fail(c, PT_ERR_INVALID, "pt_debug_probe_form: only form 1 reports its paths");
  c->probe_form = form;
  c->probe_paths = paths_dev;
  return PT_OK;
}

// pt_shade_probes: one launch of the shading kernel over the feature planes in place.  Host records go through the ProbeSet's
// staging, a host frame comes back through the read-outs' staging (scratch between calls, as pt_glare uses it); device pointers
// are used in place and the call is then asynchronous.  No event pair, no counter, no flag of the context moves.
PT_API int pt_shade_probes(pt_ctx* c, const PtProbeLattice* lattice, const PtProbeSH* probes, const PtProbeShadeOptions* options, float* rgba_out) {
  if (!c) return PT_ERR_INVALID;
  const char* who = "pt_shade_probes";
  if (!lattice || !probes || !rgba_out) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  if (const char* why = ptprobe::lattice_error(*lattice)) return fail(c, PT_ERR_INVALID, "%s: %s", who, why);
  uint32_t flags = options ? options->flags : (uint32_t)PT_PROBE_HALFSPACE;
  float bias = options ? options->normal_bias : 0.0f;
  if (const char* why = ptprobe::options_error(flags, bias)) return fail(c, PT_ERR_INVALID, "%s: %s", who, why);
  if (c->count_work) return fail(c, PT_ERR_INVALID, "%s: not with PT_OPT_COUNT_WORK", who);
  if (!c->feat.on) return option_off(c, who, SET_FEATURES);
  if (!c->feat.valid)
    return fail(c, PT_ERR_NOT_READY, "%s: no pt_render_features since the scene, the uniforms or the size last changed", who);
  PT_HIP(c, hipSetDevice(c->device));
  if (is_capturing(c)) return fail(c, PT_ERR_INVALID, "%s: not inside a stream capture", who);
  if (c->local_rows == 0) return PT_OK;  // this band owns no rows
  if (!c->feat.in_place(extent_of(c))) return fail(c, PT_ERR_CAPACITY, "%s: the planes are not allocated for the rows in place (an earlier allocation failed)", who);
  const uint32_t nodes = ptprobe::node_count(*lattice);
  const bool probes_on_device = device_pointer(probes), out_on_device = device_pointer(rgba_out);
  if (!out_on_device) PT_TRY(frame_buffers_ready(c, who));  // (the read-outs' staging holds a host caller's frame)
  const float* records = reinterpret_cast<const float*>(probes);
  if (!probes_on_device) {
    if (!c->probe.stage_in_place(nodes)) {
      PT_HIP(c, hipStreamSynchronize(c->stream));  // (nothing in flight reads what the fit frees)
      if (const ptbuf::Fit f = c->probe.fit_stage(nodes); !f.ok())
        return fail(c, PT_ERR_CAPACITY, "%s: the staging's allocation for %u records failed: %s", who, nodes, hipGetErrorString((hipError_t)f.err));
    }
    PT_HIP(c, hipMemcpyAsync(c->probe.stage.get(), probes, (size_t)nodes * sizeof(PtProbeSH), hipMemcpyHostToDevice, c->stream));
    records = c->probe.stage.get();
  }
  {
    const float4* planes = c->feat.planes.get();
    const uint32_t plane = (uint32_t)n_pixels(c);
    const float* cam = c->params.camera_origin;
    float* dst = out_on_device ? rgba_out : reinterpret_cast<float*>(c->frame.resolve.get());
    const dim3 grid((n_tiles(c) + 3u) / 4u);
    if (c->probe_form == 1)
      PT_HIP(c, call(ptsig::ProbeShadeShared{}, pt_lattice_kernel(PT_PROBE_SHADE_SHARED), grid, dim3(256), 0, c->stream,
                     planes, plane, c->width, c->local_rows, *lattice, flags, bias, cam[0], cam[1], cam[2], records, dst, c->probe_paths));
    else
      PT_HIP(c, call(ptsig::ProbeShade{}, pt_lattice_kernel(PT_PROBE_SHADE), grid, dim3(256), 0, c->stream,
                     planes, plane, c->width, c->local_rows, *lattice, flags, bias, cam[0], cam[1], cam[2], records, dst));
    if (!out_on_device) PT_HIP(c, hipMemcpyAsync(rgba_out, dst, n_pixels(c) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  }
  if (!probes_on_device || !out_on_device) PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

// ---- exposure metering and the toned read-out (PT_OPT_TONEMAP; include/ptrace.h has the contract) -------------
// The source image of pt_meter and the toned read-outs, ready for a kernel: the accumulation (src NULL: what pt_resolve asks of
// the context is asked here), the caller's device texels in place, or the caller's host texels copied into the pass slabs (free
// between calls, as pt_query_radiance uses them: the read-outs' own staging holds the result).
struct ToneSource {
  const pttone::F4* texels = nullptr;
  int from_accum = 0;
  bool staged = false;  // a host source: the call synchronises before it returns
};
static int tone_source(pt_ctx* c, const char* who, const float* src, ToneSource& s) {
  if (!src && c->tally.nothing_rendered()) return fail(c, PT_ERR_NOT_READY, "%s: nothing rendered yet", who);
  PT_TRY(frame_buffers_ready(c, who));
  const size_t n_pix = n_pixels(c);
  if (!src) {
    s.texels = reinterpret_cast<const pttone::F4*>(c->frame.accum);
    s.from_accum = 1;
  } else if (device_pointer(src)) {
    s.texels = reinterpret_cast<const pttone::F4*>(src);
  } else {
    if (n_pix) PT_HIP(c, hipMemcpyAsync(c->frame.slab.get(), src, n_pix * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    s.texels = reinterpret_cast<const pttone::F4*>(c->frame.slab.get());
    s.staged = true;
  }
  return PT_OK;
}

PT_API int pt_meter(pt_ctx* c, const float* src, const PtMeterOptions* opt) {
  if (!c || !opt) return fail(c, PT_ERR_INVALID, "pt_meter: NULL argument");
  if (!pttone::meter_options_valid(*opt))
    return fail(c, PT_ERR_INVALID, "pt_meter: key, e_min <= e_max and white_min must be finite and positive, key_permille <= high_permille <= 1000, rate no NaN");
  if (!c->expo.on) return option_off(c, "pt_meter", SET_TONEMAP);
  PT_HIP(c, hipSetDevice(c->device));
  if (is_capturing(c)) return fail(c, PT_ERR_INVALID, "pt_meter: not inside a stream capture");
  ToneSource s;
  PT_TRY(tone_source(c, "pt_meter", src, s));
  if (!c->expo.in_place()) return fail(c, PT_ERR_CAPACITY, "pt_meter: the exposure state is not allocated (an earlier allocation failed)");
  uint32_t* state = c->expo.state.get();
  const uint32_t n_pix = (uint32_t)n_pixels(c);
  const ptstate::Partition part(c->params);
  const pttone::Window win = {opt->x0, opt->y0, opt->w, opt->h, part.rows, part.index, part.count};
  PT_HIP(c, hipMemsetAsync(state, 0, pttone::kTallies * sizeof(uint32_t), c->stream));
  if (n_pix) {  // (a band without rows: N == 0 on the device)
    PT_HIP(c, call(ptsig::Meter{}, pt_display_kernel(PT_D_METER), dim3(pixel_grid(n_pix)), dim3(256), 0, c->stream, s.texels, s.from_accum, n_pix, c->width, win, state));
  }
  PT_HIP(c, call(ptsig::Exposure{}, pt_display_kernel(PT_D_EXPOSURE), dim3(1), dim3(256), 0, c->stream, state, *opt, c->expo.valid ? 1 : 0));
  c->expo.valid = true;
  if (s.staged) PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_meter_read(pt_ctx* c, PtExposure* out, uint32_t hist256[256]) {
  if (!c) return PT_ERR_INVALID;
  if (!c->expo.on) return option_off(c, "pt_meter_read", SET_TONEMAP);
  if (!c->expo.valid || !c->expo.in_place()) return fail(c, PT_ERR_NOT_READY, "pt_meter_read: no exposure yet (pt_meter or pt_meter_set come first)");
  PT_HIP(c, hipSetDevice(c->device));
  PT_TRY(not_capturing(c, "pt_meter_read"));
  const uint32_t* state = c->expo.state.get();
  if (hist256) PT_HIP(c, hipMemcpyAsync(hist256, state, pttone::kBins * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (out) PT_HIP(c, hipMemcpyAsync(out, state + pttone::kTallies, sizeof(PtExposure), hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_meter_set(pt_ctx* c, const PtExposure* rec) {
  if (!c || !rec) return fail(c, PT_ERR_INVALID, "pt_meter_set: NULL argument");
  if (!pttone::finite_positive(rec->exposure) || !pttone::finite_positive(rec->white))
    return fail(c, PT_ERR_INVALID, "pt_meter_set: exposure and white must be finite and positive");
  if (!c->expo.on) return option_off(c, "pt_meter_set", SET_TONEMAP);
  PT_HIP(c, hipSetDevice(c->device));
  PT_TRY(not_capturing(c, "pt_meter_set"));
  if (!c->expo.in_place()) return fail(c, PT_ERR_CAPACITY, "pt_meter_set: the exposure state is not allocated (an earlier allocation failed)");
  PT_HIP(c, hipMemcpyAsync(c->expo.state.get() + pttone::kTallies, rec, sizeof(PtExposure), hipMemcpyHostToDevice, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  c->expo.valid = true;
  return PT_OK;
}

PT_API int pt_exposure_solve(const uint32_t hist256[256], uint32_t below, const PtMeterOptions* opt, const PtExposure* prev, PtExposure* out) {
  if (!hist256 || !opt || !out || !pttone::meter_options_valid(*opt)) return PT_ERR_INVALID;
  const PtExposure none{};
  *out = pttone::solve(hist256, below, *opt, prev != nullptr, prev ? *prev : none);
  return PT_OK;
}

// the two toned read-outs: `bytes` 0 float texels, 1 RGBA8
static int resolve_toned(pt_ctx* c, const char* who, const float* src, const PtToneOptions* opt, void* rgba_out, int bytes) {
  if (!c || !opt || !rgba_out) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  if (opt->curve != PT_TONE_CLAMP && opt->curve != PT_TONE_REINHARD && opt->curve != PT_TONE_FILMIC)
    return fail(c, PT_ERR_INVALID, "%s: curve %d is none of PT_TONE_CLAMP, PT_TONE_REINHARD, PT_TONE_FILMIC", who, (int)opt->curve);
  const bool from_record = opt->exposure == 0.0f;
  if (!from_record && !pttone::finite_positive(opt->exposure))
    return fail(c, PT_ERR_INVALID, "%s: exposure must be 0 (the device record's) or finite and positive", who);
  if (!from_record && opt->curve == PT_TONE_REINHARD && !(opt->white > 0.0f))
    return fail(c, PT_ERR_INVALID, "%s: PT_TONE_REINHARD needs a white above 0", who);
  if (from_record) {
    if (!c->expo.on) return option_off(c, who, SET_TONEMAP);
    if (!c->expo.valid || !c->expo.in_place()) return fail(c, PT_ERR_NOT_READY, "%s: no exposure yet (pt_meter or pt_meter_set come first)", who);
  }
  PT_HIP(c, hipSetDevice(c->device));
  PT_TRY(not_capturing(c, who));
  ToneSource s;
  PT_TRY(tone_source(c, who, src, s));
  uint32_t n_pix = (uint32_t)n_pixels(c);
  if (n_pix == 0) return PT_OK;
  void* out = c->frame.resolve.get();
  const PtExposure* record = from_record ? reinterpret_cast<const PtExposure*>(c->expo.state.get() + pttone::kTallies) : nullptr;
  PT_HIP(c, call(ptsig::Tone{}, pt_display_kernel(PT_D_TONE), dim3(pixel_grid(n_pix)), dim3(256), 0, c->stream,
                 s.texels, s.from_accum, out, bytes, n_pix, opt->curve, opt->gamma, opt->exposure, opt->white, record));
  PT_HIP(c, hipMemcpyAsync(rgba_out, out, (size_t)n_pix * (bytes ? 4 : sizeof(float4)), hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

PT_API int pt_resolve_toned(pt_ctx* c, const float* src, const PtToneOptions* opt, float* rgba_out) {
  return resolve_toned(c, "pt_resolve_toned", src, opt, rgba_out, 0);
}
PT_API int pt_resolve_toned_rgba8(pt_ctx* c, const float* src, const PtToneOptions* opt, uint8_t* rgba_out) {
  return resolve_toned(c, "pt_resolve_toned_rgba8", src, opt, rgba_out, 1);
}

// ---- glare: the bloom pyramid ahead of the toned read-out (PT_OPT_GLARE; include/ptrace.h has the contract) ----
// `levels` downs, `levels` gathers, one composite into the read-outs' staging and one copy to the caller: rgba_out may be a
// device src, which the composite still reads.
// the down kernel's grid: a 256-thread workgroup per 16x16 tile of the level, capped — the kernel strides over the tiles
inline uint32_t glare_tile_grid(uint32_t w, uint32_t h) { return grid_for(((w + 15u) / 16u) * ((h + 15u) / 16u), 1, 2048); }

PT_API int pt_glare(pt_ctx* c, const float* src, const PtGlareOptions* opt, float* rgba_out) {
  if (!c || !opt || !rgba_out) return fail(c, PT_ERR_INVALID, "pt_glare: NULL argument");
  if (!ptglare::options_valid(*opt))
    return fail(c, PT_ERR_INVALID, "pt_glare: strength must be finite and in [0, 1], threshold finite and >= 0, levels 1 .. %d, the weights of the levels in use finite and >= 0",
                (int)PT_GLARE_MAX_LEVELS);
  if (!c->glare.on) return option_off(c, "pt_glare", SET_GLARE);
  if (!ptstate::Partition(c->params).every_row())
    return fail(c, PT_ERR_INVALID, "pt_glare: a band context holds interleaved rows whose neighbours live on other ranks: glare the gathered frame on a context of "
                                   "the whole frame, through src");
  PT_HIP(c, hipSetDevice(c->device));
  if (is_capturing(c)) return fail(c, PT_ERR_INVALID, "pt_glare: synchronises; not inside a stream capture");
  ToneSource s;
  PT_TRY(tone_source(c, "pt_glare", src, s));
  if (!c->glare.in_place(c->width, c->local_rows))
    return fail(c, PT_ERR_CAPACITY, "pt_glare: the pyramid is not allocated for the rows in place (an earlier allocation failed)");
  uint32_t w = c->width, h = c->local_rows;
  if ((size_t)w * h == 0) return PT_OK;
  // level k of the pyramid (k = 1 .. levels) behind level k - 1
  pttone::F4* level[PT_GLARE_MAX_LEVELS + 1] = {nullptr};
  uint32_t lw[PT_GLARE_MAX_LEVELS + 1], lh[PT_GLARE_MAX_LEVELS + 1];
  lw[0] = w; lh[0] = h;
  pttone::F4* next = reinterpret_cast<pttone::F4*>(c->glare.pyramid.get());
  for (uint32_t k = 1; k <= opt->levels; k++) {
    lw[k] = ptglare::half_up(lw[k - 1]); lh[k] = ptglare::half_up(lh[k - 1]);
    level[k] = next;
    next += (size_t)lw[k] * lh[k];
  }
  for (uint32_t k = 1; k <= opt->levels; k++) {
    const pttone::F4* from = k == 1 ? s.texels : level[k - 1];
    const int mode = k == 1 ? (s.from_accum ? 2 : 1) : 0;
    PT_HIP(c, call(ptsig::GlareDown{}, pt_glare_kernel(PT_G_DOWN), dim3(glare_tile_grid(lw[k], lh[k])), dim3(256), 0, c->stream,
                   from, mode, opt->threshold, lw[k - 1], lh[k - 1], level[k], lw[k], lh[k]));
  }
  for (uint32_t k = opt->levels; k >= 1; k--) {
    const bool top = k == opt->levels;
    const pttone::F4* above = top ? nullptr : level[k + 1];
    const uint32_t W = top ? 0u : lw[k + 1], H = top ? 0u : lh[k + 1];
    PT_HIP(c, call(ptsig::GlareGather{}, pt_glare_kernel(PT_G_GATHER), dim3(pixel_grid(lw[k] * lh[k])), dim3(256), 0, c->stream,
                   level[k], lw[k], lh[k], opt->weight[k - 1], above, W, H));
  }
  float4* out = c->frame.resolve.get();
  PT_HIP(c, call(ptsig::GlareComposite{}, pt_glare_kernel(PT_G_COMPOSITE), dim3(pixel_grid(w * h)), dim3(256), 0, c->stream,
                 s.texels, s.from_accum, opt->threshold, opt->strength, level[1], lw[1], lh[1], out, w, h));
  PT_HIP(c, hipMemcpyAsync(rgba_out, out, (size_t)w * h * sizeof(float4), hipMemcpyDefault, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  return PT_OK;
}

// ---- temporal reprojection (PT_OPT_REPROJECT; include/ptrace.h has the contract) ------------------------------
static int reproject_ready(pt_ctx* c, const char* who) {
  if (!c->hist.on) return option_off(c, who, SET_REPROJECT);
  if (!c->hist.in_place(extent_of(c))) return fail(c, PT_ERR_CAPACITY, "%s: the history planes are not allocated for the rows in place (an earlier allocation failed)", who);
  return PT_OK;
}

PT_API int pt_keep_history(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  if (int rc = reproject_ready(c, "pt_keep_history"); rc != PT_OK) return rc;
  if (!c->feat.on || !c->feat.valid || !c->feat.in_place(extent_of(c)))
    return fail(c, PT_ERR_NOT_READY, "pt_keep_history: no pt_render_features since the scene, the uniforms or the size last changed");
  PT_HIP(c, hipSetDevice(c->device));
  if (const size_t pix = n_pixels(c)) {
    const size_t bytes = pix * sizeof(float4);
    PT_HIP(c, hipMemcpyAsync(c->hist.planes.get(), c->feat.planes.get() + (size_t)PT_FEAT_IDS * pix, bytes, hipMemcpyDeviceToDevice, c->stream));
    PT_HIP(c, hipMemcpyAsync(c->hist.planes.get() + pix, c->feat.planes.get() + (size_t)PT_FEAT_POINT * pix, bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  c->hist.params = c->params;
  c->hist.valid = true;
  return PT_OK;
}

PT_API int pt_load_history(pt_ctx* c, const PtParams* prev, const void* ids, const void* point) {
  if (!c || !prev || !ids || !point) return fail(c, PT_ERR_INVALID, "pt_load_history: NULL argument");
  if (int rc = reproject_ready(c, "pt_load_history"); rc != PT_OK) return rc;
  if (prev->width != c->width || prev->height != c->height || ptstate::Partition(*prev) != ptstate::Partition(c->params))
    return fail(c, PT_ERR_INVALID, "pt_load_history: the history view's size or row partition is not the context's");
  PT_HIP(c, hipSetDevice(c->device));
  PT_TRY(not_capturing(c, "pt_load_history"));
  if (const size_t pix = n_pixels(c)) {
    const size_t bytes = pix * sizeof(float4);
    PT_HIP(c, hipMemcpyAsync(c->hist.planes.get(), ids, bytes, hipMemcpyDefault, c->stream));
    PT_HIP(c, hipMemcpyAsync(c->hist.planes.get() + pix, point, bytes, hipMemcpyDefault, c->stream));
  }
  PT_HIP(c, hipStreamSynchronize(c->stream));
  c->hist.params = *prev;
  c->hist.valid = true;
  return PT_OK;
}

PT_API int pt_reproject_constants(const PtParams* prev, float tolerance_px, float out16[16]) {
  if (!prev || !out16 || prev->width == 0) return PT_ERR_INVALID;
  if (!std::isfinite(tolerance_px) || tolerance_px < 0.0f) return PT_ERR_INVALID;
  return ptrep::constants(prev->camera_origin, prev->horizontal, prev->vertical, prev->lower_left_corner, prev->width, tolerance_px, out16)
             ? PT_OK : PT_ERR_INVALID;
}

// pt_reproject and pt_reproject_estimate (`carry`): the same checks in the same order, the same history, accumulation and tallies;
// they differ in what becomes of the error estimate's state — cleared, or gathered by the same kernel pass
static int reproject_call(pt_ctx* c, const PtReprojectOptions* opt, const char* who, bool carry) {
  if (!c || !opt) return fail(c, PT_ERR_INVALID, "%s: NULL argument", who);
  for (const float cap : {opt->cap_diffuse, opt->cap_other})
    if (!(cap >= 0.0f) || !(cap < 16777216.0f) || cap != std::floor(cap))
      return fail(c, PT_ERR_INVALID, "%s: a cap of %g is not a whole number in [0, 2^24)", who, (double)cap);
  if (!std::isfinite(opt->tolerance_px) || opt->tolerance_px < 0.0f)
    return fail(c, PT_ERR_INVALID, "%s: tolerance_px must be finite and >= 0", who);
  if (int rc = reproject_ready(c, who); rc != PT_OK) return rc;
  if (carry && !c->est.on) return option_off(c, who, SET_ESTIMATE);
  PT_TRY(frame_buffers_ready(c, who));  // (the gather goes through the read-out staging)
  PT_HIP(c, hipSetDevice(c->device));
  if (is_capturing(c)) return fail(c, PT_ERR_INVALID, "%s: not inside a stream capture", who);
  if (!c->hist.valid) return fail(c, PT_ERR_NOT_READY, "%s: no history (pt_keep_history / pt_load_history; one pt_reproject uses it up)", who);
  if (!c->feat.on || !c->feat.valid || !c->feat.in_place(extent_of(c)))
    return fail(c, PT_ERR_NOT_READY, "%s: no pt_render_features since the uniforms of the new view went up", who);
  // (nothing folded since the last clear: the state is zero and there is nothing to carry — the call is pt_reproject)
  carry = carry && c->est.spp != 0;
  const size_t pix = n_pixels(c);  // (the state's staging buffer is in place with the estimate: frame_buffers_ready above)
  float k16[ptrep::K_COUNT];
  if (pt_reproject_constants(&c->hist.params, opt->tolerance_px, k16) != PT_OK)
    return fail(c, PT_ERR_INVALID, "%s: the history view's camera is degenerate", who);
  changed(*c, ptstate::REPROJECTED);  // one-shot: from here on the accumulation belongs to the new view
  c->hist.ran = true;
  PT_HIP(c, hipMemsetAsync(c->hist.tally.get(), 0, 3 * sizeof(unsigned long long), c->stream));
  if (pix == 0) return PT_OK;  // this band owns no rows
  ptrep::Consts K;
  for (int k = 0; k < 3; k++) {
    K.O[k] = k16[ptrep::K_O + k];
    K.N[k] = k16[ptrep::K_N + k];
    K.A[k] = k16[ptrep::K_A + k];
    K.B[k] = k16[ptrep::K_B + k];
  }
  K.ea = k16[ptrep::K_EA];
  K.eb = k16[ptrep::K_EB];
  K.k = k16[ptrep::K_K];
  K.cap_diffuse = opt->cap_diffuse;
  K.cap_other = opt->cap_other;
  const ptstate::Partition part(c->params);
  const ptrep::Frame F = {c->width, c->height, c->local_rows, part.rows, part.index, part.count};
  const float4* cur_ids = c->feat.planes.get() + (size_t)PT_FEAT_IDS * pix;
  const float4* cur_pnt = c->feat.planes.get() + (size_t)PT_FEAT_POINT * pix;
  const float4* hist_ids = c->hist.planes.get();
  const float4* hist_pnt = c->hist.planes.get() + pix;
  const float4* accum = c->frame.accum;
  float4* out = c->frame.resolve.get();  // (the staging buffer pt_load_accum uses: the gather reads accum at other pixels' places)
  unsigned long long* tally = c->hist.tally.get();
  const dim3 grid((c->width + 31u) / 32u, (c->local_rows + 7u) / 8u);
  if (!carry) {
    PT_HIP(c, call(ptsig::Reproject{}, pt_reproject_kernel_handle(), grid, dim3(256), 0, c->stream, cur_ids, cur_pnt, hist_ids, hist_pnt, accum, out, K, F, tally));
    PT_HIP(c, hipMemcpyAsync(c->frame.accum, out, pix * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    return clear_error(c);  // (history is sums, not the passes they came from: as pt_load_accum)
  }
  // the estimate's constants: the caps in passes of err_spp samples; err_spp stays, so the next fold must use the same value
  const ptrep::EstConsts E = ptrep::est_consts(c->est.spp, opt->cap_diffuse, opt->cap_other);
  const float4* err = c->est.state.get();
  float4* out_err = c->est.stage.get();
  PT_HIP(c, call(ptsig::ReprojectEstimate{}, pt_reproject_estimate_kernel_handle(), grid, dim3(256), 0, c->stream,
                 cur_ids, cur_pnt, hist_ids, hist_pnt, accum, err, out, out_err, K, E, F, tally));
  PT_HIP(c, hipMemcpyAsync(c->frame.accum, out, pix * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
  PT_HIP(c, hipMemcpyAsync(c->est.state.get(), out_err, 2 * pix * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
  return PT_OK;
}

PT_API int pt_reproject(pt_ctx* c, const PtReprojectOptions* opt) { return reproject_call(c, opt, "pt_reproject", false); }

PT_API int pt_reproject_estimate(pt_ctx* c, const PtReprojectOptions* opt) { return reproject_call(c, opt, "pt_reproject_estimate", true); }

PT_API int pt_reproject_stats(pt_ctx* c, PtReprojectStats* out) {
  if (!c || !out) return fail(c, PT_ERR_INVALID, "pt_reproject_stats: NULL argument");
  if (!c->hist.on) return option_off(c, "pt_reproject_stats", SET_REPROJECT);
  if (!c->hist.ran) return fail(c, PT_ERR_NOT_READY, "pt_reproject_stats: no pt_reproject yet");
  PT_HIP(c, hipSetDevice(c->device));
  PT_TRY(not_capturing(c, "pt_reproject_stats"));
  unsigned long long h[3] = {0, 0, 0};
  PT_HIP(c, hipMemcpyAsync(h, c->hist.tally.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  out->pixels = (uint64_t)n_pixels(c);
  out->pixels_hit = h[0];
  out->pixels_kept = h[1];
  out->samples_kept = h[2];
  return PT_OK;
}

namespace {

// FIT THE GRID TO THE VIEW.  pt_set_spheres builds the grid for rays that start within 2 s0 of the scene's middle (d_near =
// 3 s0): it does not know where the camera will stand.  The margin every sphere is registered with grows with d_near^2 (the
// cancellation in the shader's own `c` term: pt_grid.hpp), so a scene whose rays all start close by pays for rays that never
// come, and a camera beyond 2 s0 turns every primary ray into a far ray (exact, but tested against the whole list).  Two
// entry points rebuild the grid for another of the classes kNearFactors: pt_tune — the synchronous set-up call that fits the
// context to scene AND uniforms, and may launch: it MEASURES the candidates (tune_grid_to_view) — and pt_refit_grid — what a
// frame loop calls when its camera has moved: host arithmetic only, the class the camera needs but never below the default.
// A matter of speed only: the image bits do not depend on d_near.  Not after a launch has been captured into a caller's
// hipGraph (its arguments hold the old grid's numbers).  Whether the grid in place still fits is host arithmetic on the
// uniforms (grid_fit_state: PtStats.grid_fit_stale, pt_grid_fit): pt_set_params never rebuilds — a rebuild synchronises the
// stream and moves device buffers.
// (the decisions: pt_geom_plan.hpp)
// May the grid be rebuilt for the view at all: there is one (and with it the host copies it is built from), with uniforms, no launch
// captured into a caller's hipGraph holds its numbers, and no A/B build fixes its factor (PT_GRID_DNEAR, PT_DEV_KNOBS builds only:
// pt_grid.hpp builds every grid for it)?
bool grid_refittable(const pt_ctx* c) {
  if (!c->grid.present || !c->state.have_params || c->tally.captured) return false;
#ifdef PT_DEV_KNOBS
  if (getenv("PT_GRID_DNEAR")) return false;  // (the A/B build's own factor stands)
#endif
  return true;
}

// replace the grid in place by one built for d_near = factor * s0 (the caller has decided that it should be)
int rebuild_grid(pt_ctx* c, double factor, bool keep_tuned) {
  ptgrid::Grid grid;
  const ptscene::Split& sp = c->list.host;
  if (!ptscene::build_grid(sp.geom.data(), sp.radii.data(), c->list.n, factor, &grid)) return PT_OK;  // (no grid for that factor: the one in place stays)
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));  // launches in flight read the grid in place
  const int tuned = c->geom.tuned;
  changed(*c, ptstate::GRID_REBUILT);
  int rc = install_grid(c, grid, sp);
  if (rc == PT_OK && wants_uuids(c)) rc = upload_uuids(c, sp.uuid);
  c->geom.list_paths(path_scene(c));  // (which kernels the grid can feed, and whether PT_GEOM_AUTO has anything to measure, follow its size — or its absence, had the upload failed)
  if (keep_tuned && rc == PT_OK && tuned == PT_GEOM_GRID && c->grid.present) c->geom.tuned = tuned;  // a refit keeps the settled choice
  return rc;
}

// policy: 0 = rebuild whenever another class fits better, 1 = only when the class in place is too SMALL (refit_factor)
int fit_grid_to_view(pt_ctx* c, int policy) {
  if (!grid_refittable(c)) return PT_OK;
  const double factor = refit_factor(policy, fit_state(c), need_factor(c));
  return factor > 0.0 ? rebuild_grid(c, factor, true) : PT_OK;
}

// pt_tune's part (i): the grid's margin class (GridClassSearch) and build
int tune_grid_to_view(pt_ctx* c, uint32_t n_passes, bool* launched) {
  *launched = false;
  if (!grid_refittable(c) || !c->geom.grid_tried()) return PT_OK;
  const double need = need_factor(c);
  if (need <= 0.0) return PT_OK;
  auto at = [&](double f) { return same_class(f, (double)c->grid.head.near_factor); };
  if (grid_class_unmeasured(c->grid_fit_mode, n_passes, c->reserved_passes)) {  // the class the camera needs
    return at(need) ? PT_OK : rebuild_grid(c, need, false);
  }
  // one timed launch of n_timed passes through the grid walk on the grid built for `f`, after a cold one of one pass (the
  // `yardstick` of timed_passes): kernel time from the launch's events, far share from its tallies.  `*probe` stays empty when no
  // grid could be built for f.
  const int policy_kept = c->geom.policy;
  uint32_t n_timed = timed_passes(-1.0, n_passes);
  auto measure = [&](double f, bool cold, bool yardstick, std::optional<ClassProbe>* probe) -> int {
    if (!at(f)) { int rc = rebuild_grid(c, f, false); if (rc != PT_OK) return rc; }
    if (!c->grid.present || !at(f)) return PT_OK;  // (no grid for that class: not a candidate)
    c->geom.policy = PT_GEOM_GRID;
    int rc = PT_OK;
    for (int k = cold ? 0 : 1; k < 2 && rc == PT_OK; k++) {
      unsigned long long before[PT_CTR_SCRATCH], after[PT_CTR_SCRATCH];
      rc = hipStreamSynchronize(c->stream) == hipSuccess ? fold_events(c) : PT_ERR_HIP;
      if (rc != PT_OK) break;
      const double ms0 = c->kernel_ms;
      if (hipMemcpy(before, c->d_counters.get(), sizeof before, hipMemcpyDeviceToHost) != hipSuccess) { rc = PT_ERR_HIP; break; }
      rc = pt_render_passes(c, k == 0 ? 1u : n_timed);
      if (rc != PT_OK) break;
      rc = hipStreamSynchronize(c->stream) == hipSuccess ? fold_events(c) : PT_ERR_HIP;
      if (rc != PT_OK) break;
      if (hipMemcpy(after, c->d_counters.get(), sizeof after, hipMemcpyDeviceToHost) != hipSuccess) { rc = PT_ERR_HIP; break; }
      const double ms = c->kernel_ms - ms0;
      if (k == 0 && yardstick) {
        n_timed = timed_passes(ms, n_passes);
      } else if (k == 1) {
        const double seg = (double)(after[PT_CTR_SEGMENTS] - before[PT_CTR_SEGMENTS]);
        *probe = ClassProbe{f, ms, seg > 0 ? (double)(after[PT_CTR_FAR_RAYS] - before[PT_CTR_FAR_RAYS]) / seg : 0.0};
      }
    }
    c->geom.policy = policy_kept;
    *launched = true;
    return rc == PT_ERR_HIP ? fail(c, PT_ERR_HIP, "pt_tune: a HIP call failed while timing a grid class") : rc;
  };
  GridClassSearch search(need);
  for (GridClassSearch::Step step = search.next(); step.factor != 0.0; step = search.next()) {
    std::optional<ClassProbe> probe;
    if (int rc = measure(step.factor, step.cold, step.cold, &probe); rc != PT_OK) return rc;
    search.report(probe);
  }
  if (!search.kept()) return PT_OK;
  const double keep = search.keep();
  if (!at(keep)) { int rc = rebuild_grid(c, keep, false); if (rc != PT_OK) return rc; }
  changed(*c, ptstate::CELLS_BUILD_UNMEASURED);
  if (c->grid.present && at(keep) && cells_build_worth_timing(c->grid.head.n_entries, grid_build(c).kind)) {
    changed(*c, ptstate::CELLS_BUILD_CHOSEN);  // (on trial: the launch below is the build's)
    std::optional<ClassProbe> probe;
    const int rc = measure(keep, true, false, &probe);
    if (rc != PT_OK || !keep_cells_build(probe, search.keep_ms())) changed(*c, ptstate::CELLS_BUILD_UNMEASURED);
    return rc;
  }
  return PT_OK;
}

} // namespace

PT_API int pt_refit_grid(pt_ctx* c, int only_if_stale) {
  if (!c) return PT_ERR_INVALID;
  if (!c->state.have_spheres || !c->state.have_params) return PT_OK;
  return fit_grid_to_view(c, only_if_stale ? 1 : 0);
}

PT_API int pt_grid_fit(pt_ctx* c) {
  if (!c) return PT_ERR_INVALID;
  return fit_state(c);
}

PT_API int pt_tune(pt_ctx* c, uint32_t n_passes) {
  if (!c || n_passes == 0) return fail(c, PT_ERR_INVALID, "pt_tune: bad argument");
  // measuring launches are not part of any frame: they fold the plain way, and whatever they launched is cleared below
  struct Pause { pt_ctx* c; ~Pause() { c->est.paused = false; } } pause{c};
  c->est.paused = true;
  bool launched = false;
  if (c->state.have_spheres) {
    int rc = tune_grid_to_view(c, n_passes, &launched);
    if (rc != PT_OK) return rc;
  }
  if (!c->state.have_spheres || !c->geom.has_path_to_decide())
    return launched ? pt_reset_accum(c) : PT_OK;
  c->geom.reset();
  for (int k = 0; k < 1 + c->geom.n_paths; k++) {
    int rc = pt_render_passes(c, n_passes);
    if (rc != PT_OK) return rc;
  }
  PT_HIP(c, hipSetDevice(c->device));
  PT_HIP(c, hipStreamSynchronize(c->stream));
  try_finish_tuning(c);
  return pt_reset_accum(c);
}

// Device-side evaluation of single PT-SPEC functions (parity tests; see pt_kernel_args.h).
// `in`/`out` are HOST pointers; counts are in floats.
PT_API int pt_probe(pt_ctx* c, int kind, const float* in, size_t n_in, float* out, size_t n_out,
                    uint32_t n) {
  if (!c || !in || !out || n == 0) return fail(c, PT_ERR_INVALID, "pt_probe: bad argument");
  PT_HIP(c, hipSetDevice(c->device));
  DevBuf<float> d_in, d_out;  // (freed on every return)
  PT_HIP(c, d_in.reserve(n_in));
  PT_HIP(c, d_out.reserve(n_out));
  PT_HIP(c, hipMemcpy(d_in.get(), in, n_in * sizeof(float), hipMemcpyHostToDevice));
  PT_HIP(c, hipMemsetAsync(d_out.get(), 0, n_out * sizeof(float), c->stream));
  hipLaunchKernelGGL(pt_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, kind, d_in.get(), d_out.get(), n);
  PT_HIP(c, hipGetLastError());
  PT_HIP(c, hipStreamSynchronize(c->stream));
  PT_HIP(c, hipMemcpy(out, d_out.get(), n_out * sizeof(float), hipMemcpyDeviceToHost));
  return PT_OK;
}
