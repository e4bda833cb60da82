/*
 * ptrace.h — C ABI of libptrace.so, the MI355X-native replacement for the GPU boundary of
 * austintheriot/ray-tracer-webgl (the WebGL2 surface used by src/webgl.rs + static/shader.frag).
 *
 * Everything here is plain C: POD structs, plain pointers, sizes, int error codes.  No torch /
 * C++ types cross this boundary, nothing throws or aborts across it.  A Rust `extern "C"` block
 *  binds these symbols unchanged.
 *
 * Reference citations are `path:line` relative to the reference repository root.
 *
 * Threading contract (same as the reference, src/lib.rs:66-69): one host thread drives a
 * pt_ctx at a time; separate contexts (one per GPU) are independent.
 *
 * There is NO CPU backend: pt_create fails with PT_ERR_NO_DEVICE when no HIP device exists.
 */
#ifndef PTRACE_H
#define PTRACE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 5 /* 5: PtStats grew (grid_fit_stale, grid_near_factor, far_rays); pt_refit_grid, pt_create_on_stream;
                            pt_tune refits the grid; the dev header's pt_debug_wave_log writes four words per wave */

/* ---- error codes (returned by every int function; 0 = success) ------------------------------ */
enum {
  PT_OK = 0,
  PT_ERR_INVALID = -1,    /* bad argument (NULL, zero size, spp < 1, max_depth < 1 ...)        */
  PT_ERR_NO_DEVICE = -2,  /* no HIP device / device index out of range                         */
  PT_ERR_HIP = -3,        /* a HIP runtime call failed; pt_last_error() has the text           */
  PT_ERR_NOT_READY = -4,  /* render before pt_set_spheres / pt_set_params                      */
  PT_ERR_CAPACITY = -5,   /* scene or pass count exceeds what was reserved                     */
};

/* ---- material types: static/shader.frag:45-47, src/glsl.rs:10-24 ---------------------------- */
enum {
  PT_DIFFUSE = 0,
  PT_METAL = 1,
  PT_GLASS = 2,
  PT_EMISSIVE = 3, /* build extension (BASELINE config 4): emits `albedo`, absorbs the path     */
};

/* ---- how the intersection loop looks at the sphere list (pt_set_option PT_OPT_GEOMETRY_PATH) --
 * All of them run the same fp32 arithmetic on every sphere that can possibly be hit and give
 * bit-identical images.
 *   LDS    the whole list, staged into LDS once per workgroup, ds_read_b128 broadcasts
 *          (n <= 10 232)
 *   SCALAR the whole list through wave-uniform scalar loads (s_load_dwordx16) via the scalar
 *          cache / L2; sphere data reaches the VALU as SGPR operands (any n up to 65 528)
 *   BVH    a bounding-box hierarchy built by pt_set_spheres decides which spheres a ray looks
 *          at: boxes are inflated by a per-ray margin that covers the rounding of the literal
 *          test, so only spheres that cannot pass it are skipped (regular scenes of >= 16
 *          spheres; a scene without a hierarchy falls back to SCALAR)
 *   GRID   a uniform grid built by pt_set_spheres (cells of about two spheres each, 3D-DDA walk,
 *          entries registered with a margin that covers the rounding of the literal test and of
 *          the walk): a ray looks at the entries of the cells it passes through, in order, and
 *          stops once its closest root lies before the current cell's exit.  The better
 *          structure when most rays start inside the scene (bounce rays): a hierarchy spends two
 *          box tests per level just locating the ray's origin.  Same preconditions as BVH; a
 *          scene without a grid falls back to BVH, then SCALAR
 *   AUTO   (default) after pt_set_spheres the first launch runs cold (unmeasured), the next
 *          ones measure one usable path each, and the fastest (time per camera sample) is
 *          used from then on.  Paths whose outcome is not open are not measured: the list
 *          walks beside a structure on more than 64 spheres, the hierarchy beside an even
 *          grid (no cell with more than 16 entries, at most 8 always-tested spheres)       */
enum {
  PT_GEOM_AUTO = 0,
  PT_GEOM_LDS = 1,
  PT_GEOM_SCALAR = 2,
  PT_GEOM_BVH = 3,
  PT_GEOM_GRID = 4,
  PT_GEOM_SMALL = 5, /* lists of at most 16 spheres (the reference's `uniform Sphere[15] u_sphere_list`,
                        static/shader.frag:103): no LDS traffic in the scan, no candidate queue — four spheres per
                        s_load_dwordx16 reach the VALU as SGPR operands, candidates are finished group by
                        group in list order with the shader's own sequential acceptance.  A longer list
                        falls back to SCALAR.  PT_GEOM_AUTO tries it first on such scenes. */
};
enum {
  PT_OPT_GEOMETRY_PATH = 1,
  PT_OPT_COUNT_WORK = 2,  /* 1: the walk kernels' measuring twins fill PtStats.work (slower; never time them) */
  PT_OPT_CARRY_LANES = 3, /* walk kernels: move on to shading when fewer lanes than this (and less than half
                             of the wave) are still walking; the stragglers continue in the next wave step.
                             The grid walk raises the threshold by 4 per iteration a step's walk has already
                             run (scenes of long walks).  Scheduling only — images do not depend on it.
                             0 = lockstep.  Default 12. */
  PT_OPT_REFILL_MIN = 4,  /* lanes of a busy wave that wait for a new work item before the (wave-wide) item
                             decode runs for them.  Scheduling only.  1 = refill at once.  Default 4.
                             Builds with the look-ahead refill (every lane holds one decoded next item and
                             takes it the moment its item ends: csrc/pt_deal.hpp) do not consult it: no lane
                             waits.  The option is still accepted, stored and read back. */
  PT_OPT_RUSSIAN_ROULETTE = 5, /* value k > 0: after k bounces a path survives each further bounce with
                             probability q = min(max(throughput), 1) and carries throughput / q (unbiased:
                             every pixel's EXPECTATION is the reference's, depth-exhaustion term included).
                             NOT the reference's estimator sample for sample — static/shader.frag:297-339
                             never ends a path early — so images of this mode match the oracle only
                             statistically; it exists for deep-bounce scenes (BASELINE config 4: mean path
                             length 40 segments).  0 = off (default): bit-exact against the oracle. */
  PT_OPT_GRID_FIT = 6,    /* how pt_tune chooses the grid's margin class.  0 (default): it measures the candidates (see
                             pt_tune).  1: the smallest class that covers the camera, no launches.  Speed only. */
  PT_OPT_ERROR_ESTIMATE = 7, /* 1: keep a per-pixel error estimate beside the accumulation (see pt_error_ptr below); allocates
                             and zeroes two float4 per local pixel.  0 (default): off, releases them.  The image bits of a
                             context are the same either way. */
  PT_OPT_FEATURES = 8,    /* 1: allocate the four first-hit feature planes (see pt_render_features below; 64 bytes per local
                             pixel) and keep the uuid arrays on the device.  0 (default): release them.  The image bits of a
                             context are the same either way. */
  PT_OPT_REPROJECT = 9,   /* 1: allocate the history planes of temporal reprojection (see pt_reproject below; ids + point, 32 bytes
                             per local pixel).  Needs PT_OPT_FEATURES on (PT_ERR_INVALID otherwise).  0 (default): release them.
                             Turning PT_OPT_FEATURES off turns this off too.  The image bits of a context that never calls
                             pt_reproject are the same either way.  While PT_OPT_ERROR_ESTIMATE is on as well, 32 more bytes
                             per local pixel: the staging buffer of pt_reproject_estimate. */
  PT_OPT_RAY_QUERIES = 10, /* 1: allocate the query planes of pt_query_rays (see below; 64 bytes per local pixel), keep the uuid
                             arrays on the device and load the query builds' code object.  0 (default): release the planes.
                             The image bits of a context are the same either way. */
  PT_OPT_TONEMAP = 11,     /* 1: put the exposure state in place (see pt_meter below; 258 tallies and one PtExposure record, about
                             1 KB whatever the size of the frame) and load the display kernels' code object.  0 (default): release
                             it; the exposure is forgotten.  The image bits of a context are the same either way. */
  PT_OPT_GLARE = 12,       /* 1: allocate the glare pyramid of pt_glare (see below; one float4 per texel of the eight levels, about a
                             third of the frame: 5.4 bytes per local pixel; scratch only, no state) and load the glare kernels' code
                             object.  0 (default): release it.  The image bits of a context are the same either way. */
  PT_OPT_NEXT_EVENT = 13,  /* 1: NEXT-EVENT ESTIMATION — the render launches (pt_render_passes, _frame(s), _until, _adaptive) sample
                             the emissive spheres at DIFFUSE hits.  NOT the reference's estimator sample for sample: every pixel's
                             EXPECTATION is the plain estimator's, the samples differ.  0 (default): off, the table is released;
                             bit-exact against the oracle.  Excludes PT_OPT_RUSSIAN_ROULETTE, the debug overlay and
                             PT_OPT_COUNT_WORK (PT_ERR_INVALID, whichever comes second).  pt_render_features, pt_query_rays and
                             pt_query_radiance stay the plain estimator (this estimator along the caller's rays has entry points
                             of its own, which need the option on: pt_query_radiance_nee, pt_gather_irradiance_nee and
                             pt_bake_probes_nee, below).  The statements (csrc/pt_nee.hpp has each as one fp32
                             operation; the order below is the contract):
                               LIGHTS  the spheres of the installed list with type == PT_EMISSIVE, a finite centre, a finite
                                       non-zero radius and a finite albedo, in list order; L of them.  The device table holds
                                       {centre, r * r, albedo, list index} per light; it is built when the option is turned on
                                       over an installed scene and by pt_set_spheres while the option is on, never otherwise.
                               AT A DIFFUSE HIT x with face-forward normal n:
                                1. the shader's scatter draw, unchanged;  2. depth++ and the depth test, unchanged (a path that
                                   has used up its depth adds its throughput and ends);
                                3. if the path goes on and L > 0: ONE hash3 -> (u0, u1, u2);
                                4. k = min((int)(u0 * float(L)), L - 1);
                                5. w = c_k - x (per component), d2 = fma(w.z, w.z, fma(w.y, w.y, w.x * w.x)), r2 = r_k * r_k;
                                6. P(x, k) := d2 > r2 — the light can be sampled from x;
                                7. if P: q = r2 / d2; cosmax = sqrt(max(0, 1 - q)); om = 1 - cosmax; cos_t = 1 - u1 * om;
                                   sin_t = sqrt(max(0, fma(-cos_t, cos_t, 1))); (s, c) = sincos2pi(u2);
                                8. z = w * (1 / sqrt(d2)); sg = copysign(1, z.z); a = -1 / (sg + z.z); b = (z.x * z.y) * a;
                                   t = (fma(sg * (z.x * z.x), a, 1), sg * b, -sg * z.x); bt = (b, fma(z.y * z.y, a, sg), -z.y)
                                   (branch-free, finite for every unit z, (0, 0, -1) included: |sg + z.z| >= 1);
                                   omega = fma(z, cos_t, fma(bt, sin_t * s, t * (sin_t * c))) per component;
                                9. cos_s = fma(n.z, omega.z, fma(n.y, omega.y, n.x * omega.x));
                               10. if cos_s > 0: the next segment is the SHADOW RAY (x, omega) through the unchanged
                                   intersection (MIN_T, MAX_T, ties as hit_world);
                               11. if its closest hit is list index k:
                                   sum.c = sum.c + (throughput.c * albedo_k.c) * ((float(L) * (2 * om)) * cos_s),
                                   throughput after the hit's albedo;
                               12. the path goes on along the scattered ray of step 1.
                             A shadow segment is no bounce; it is one segment in PtStats.segments and in the tile cost.
                             NO DOUBLE COUNTING: a path that reaches a light j straight from a vertex where steps 3 onward ran
                             adds j's emission only if !P(o, j), o the segment's origin; every other arrival (from the camera,
                             after METAL or GLASS, with L == 0, on an emissive sphere that is no light) adds it as always.  With
                             L == 0 no draw is made and nothing is skipped: the output is the plain build's, bit for bit. */
};

/* ---- background modes ----------------------------------------------------------------------- */
enum {
  PT_BG_SKY = 0,   /* static/shader.frag:289-294 white→(0.5,0.7,1.0) gradient                   */
  PT_BG_BLACK = 1, /* build extension for enclosed scenes                                      */
};

/*
 * One sphere, exactly the fields webgl::set_geometry uploads per element of `u_sphere_list`
 * (src/webgl.rs:225-274; struct Sphere static/shader.frag:55-61).  `is_active` is implied by
 * the count passed to pt_set_spheres.  `radius` may be negative (src/state.rs:200,213): the
 * outward normal flips, r*r is unchanged.  48 bytes.
 */
typedef struct PtSphere {
  float center[3];
  float radius;
  int32_t type; /* PT_DIFFUSE / PT_METAL / PT_GLASS / PT_EMISSIVE; anything else absorbs      */
  float albedo[3];
  float fuzz;
  float refraction_index;
  int32_t uuid;
  int32_t _pad;
} PtSphere;

/*
 * The per-frame uniform block: what Uniforms::run_setters uploads (src/webgl.rs:279-593,
 * :629-633; declarations static/shader.frag:79-102), minus the uniforms no code path reads
 * (u_aspect_ratio, u_viewport_*, u_focal_length, u_w) and the debug overlay (:100-102, opt-in:
 * enable_debugging is 0 by default, src/state.rs:259; they go up through pt_set_debug_overlay).
 */
typedef struct PtParams {
  uint32_t width;  /* u_width  */
  uint32_t height; /* u_height */
  float time;      /* u_time: per-pass seed offset (static/shader.frag:356)                    */
  int32_t samples_per_pixel; /* u_samples_per_pixel (per pass)                                 */
  int32_t max_depth;         /* u_max_depth                                                    */
  float camera_origin[3];     /* u_camera_origin     */
  float horizontal[3];        /* u_horizontal        */
  float vertical[3];          /* u_vertical          */
  float lower_left_corner[3]; /* u_lower_left_corner */
  float u[3];                 /* u_u                 */
  float v[3];                 /* u_v                 */
  float lens_radius;          /* u_lens_radius       */
  int32_t render_count;       /* u_render_count      (temporal blend only) */
  int32_t should_average;     /* u_should_average    (temporal blend only) */
  float last_frame_weight;    /* u_last_frame_weight (temporal blend only) */
  /* ---- build extensions ---- */
  int32_t background_mode; /* PT_BG_* */
  /*
   * Row partition for multi-GPU rendering.  This context owns the image rows y (0 = bottom,
   * static/shader.frag:410) with (y / band_rows) % band_count == band_index; its buffers hold
   * only those rows, compacted in increasing y.  band_count <= 1 means "all rows".
   */
  uint32_t band_rows;
  uint32_t band_index;
  uint32_t band_count;
  /*
   * pt_render_passes: pass p of the call renders with
   *     u_time = time + float(first_pass + p) * time_step      (fp32 multiply, then add; step 0 means 1)
   * so a frame rendered as several calls (first_pass = passes done so far) has the bits of one
   * call, whatever the step.  Whole-number steps make consecutive passes REUSE each other's random
   * numbers (the seed advances by .1 per draw, static/shader.frag:22, so pass p + 1 walks the
   * seeds pass p reaches ten draws later): measured +27 % variance of the accumulated frame.
   * The reference's own u_time is performance.now(), which never lines up like that; a step such
   * as PT_TIME_STEP_DECORRELATED keeps the passes independent (tests/test_reference_pins.py).
   */
  float time_step;
  uint32_t first_pass;
} PtParams;
#define PT_TIME_STEP_DECORRELATED 0.3618034f /* 0.1 x (3 + 1/golden ratio): multiples never near a multiple of .1 */

/*
 * Inputs of State::update_pipeline (src/state.rs:319-347) / State::default (:98-125): the
 * camera-derived members of `State`.  All double, like the reference's Vec3 (src/math.rs:17).
 */
typedef struct PtCameraIn {
  uint32_t width, height;
  double camera_origin[3];
  double yaw_degrees;   /* State.yaw   */
  double pitch_degrees; /* State.pitch */
  double vup[3];
  double fov_radians;    /* State.camera_field_of_view */
  double focus_distance; /* State.focus_distance       */
  double aperture;       /* State.aperture; lens_radius = aperture / 2 (src/state.rs:102)      */
} PtCameraIn;

/* Look-at form (Shirley-style), for scenes the yaw/pitch form cannot express conveniently. */
typedef struct PtLookAtIn {
  uint32_t width, height;
  double look_from[3], look_at[3], vup[3];
  double vfov_radians;
  double focus_distance;
  double aperture;
} PtLookAtIn;

typedef struct PtStats {
  uint64_t segments;        /* ray segments (hit_world invocations) since the last reset        */
  uint64_t samples;         /* camera paths started                                             */
  uint64_t sphere_tests;    /* segments * n_spheres                                             */
  double render_kernel_ms;  /* sum of the path-tracing kernel's durations (HIP events)          */
  uint32_t render_launches; /* number of path-tracing kernel launches in that sum               */
  uint32_t total_spp;       /* samples per pixel accumulated                                    */
  uint32_t n_spheres;
  uint32_t local_rows;      /* rows held by this context (row partition)                        */
  uint32_t geometry_path;   /* PT_GEOM_LDS / _SCALAR / _BVH used by the most recent launch          */
  uint32_t geometry_tuned;  /* 1 once PT_GEOM_AUTO has measured the usable paths for this scene     */
  uint32_t bvh_nodes;       /* hierarchy of the current scene: nodes (0 = none), slots (4 per leaf   */
  uint32_t bvh_slots;       /* + the spheres tested for every ray), how many of those, depth        */
  uint32_t bvh_outliers;
  uint32_t bvh_depth;
  uint32_t grid_cells[3];   /* uniform grid of the current scene (0 = none): cells per axis,          */
  uint32_t grid_entries;    /* entries (copies of a sphere, one per cell it is registered in + padding) */
  uint32_t grid_always;     /* spheres tested for every ray                                            */
  uint32_t grid_fit_stale;  /* does the grid still fit the camera of the last pt_set_params?  0: yes (or no grid / not the
                               path in use).  1: NO — the camera stands outside the region whose rays walk the cells, so every
                               primary ray takes the far path (exact, but tested against the WHOLE list): call pt_refit_grid
                               (or pt_tune).  2: looser than needed — a smaller margin class (not below the default, 3) would
                               cover the camera (a few per cent of speed, never a cliff).  The reference moves its camera every tick
                               (src/state.rs:411-441); pt_set_params only sets this flag, it never rebuilds.       */
  /* executed work of the walk kernels since the last reset, filled when PT_OPT_COUNT_WORK is on:
   * [0] walk iterations (node steps / cell steps, wave-level)   [1] lanes active in them (sum)
   * [2] leaf rounds (four literal tests per lane)               [3] lanes active in them
   * [4] exact evaluations (sqrt + division), wave-level         [5] lanes active in them
   * [6] wave steps                                              [7] lanes carried over (sum)   */
  uint64_t work[8];
  float grid_near_factor;   /* d_near / s0 the grid in place was built for (3 from pt_set_spheres; pt_tune / pt_refit_grid
                               choose among 2.5 / 3 / 4 / 5.5 / 8 / 12 / 16); 0 = no grid                              */
  float grid_need_factor;   /* the smallest of those classes that covers the current camera and its lens           */
  uint64_t far_rays;        /* ray segments since the last reset that reached the grid from OUTSIDE its near region and
                               were therefore tested against the whole list (grid walk only; ~0 on a fitted grid)     */
  uint32_t grid_kernel_build; /* which build of the grid kernel the next launch gets: 1 cell records AND entries staged in the LDS
                               (pt_trace_kernel_grid), 2 the cell records staged, the entries gathered from L2 (…_grid_cells),
                               3 nothing staged (…_grid_gmem), 0 no grid.  What fits is staged — except while grid_fit_stale is 1
                               (the builds that gather hand a far ray to the whole wave: a stale view costs 4 x, not 16 x) and
                               where pt_tune timed the gathering build faster.  Scheduling only.                       */
  uint32_t grid_walk_flat;  /* 1: that launch is build 1 on a grid of ONE layer of cells along y (grid_cells[1] == 1) and runs the
                               two-axis walk, pt_trace_kernel_grid; 0 with build 1: pt_trace_kernel_grid_layers, three axes.  (Took
                               the place of a padding word: the struct's size and the other offsets are unchanged.)  */
} PtStats;

typedef struct pt_ctx pt_ctx;

/* ---- lifetime: replaces setup_program + create_texture x2 + create_framebuffer x2 ------------
 * (src/webgl.rs:66-80, :82-123, :153-167).  Allocates the fp32 linear accumulation buffer for
 * a w*h image on HIP device `device` and a stream.  Caller frees with pt_destroy. */
int pt_create(pt_ctx** out, int device, uint32_t width, uint32_t height);
/* Same, for a host that brings its own hipStream_t (a torch stream, an engine's render queue): the context runs on it
 * from the start and never creates a stream — hence an HSA queue, ~80-150 ms when it is the process's first — of its own.
 * `hip_stream` as in pt_set_stream (PT_STREAM_LEGACY names the default stream); NULL behaves like pt_create.  A later
 * pt_set_stream(ctx, NULL) on such a context creates the own stream then. */
int pt_create_on_stream(pt_ctx** out, int device, uint32_t width, uint32_t height, void* hip_stream);
int pt_destroy(pt_ctx* ctx);
/* resize path, src/state.rs:364-398: reallocates buffers and clears the accumulation.  Everything that belongs to the old size goes
 * with it: accumulation, sample count, error estimate, both textures, the canvas and the statistics are cleared, the row partition
 * is dropped ("all rows"), a caller-bound accumulation buffer is given back (as pt_bind_accum(ctx, NULL) does), and the uniforms are
 * forgotten: the render calls return PT_ERR_NOT_READY until pt_set_params has brought uniforms of the new size. */
int pt_resize(pt_ctx* ctx, uint32_t width, uint32_t height);

/* ---- scene + uniforms ------------------------------------------------------------------------
 * pt_set_spheres replaces webgl::set_geometry (src/webgl.rs:225-274); n is not capped at 15:
 * up to 10 232 spheres are walked from LDS, up to 65 528 from global memory (PT_ERR_CAPACITY beyond).
 * pt_set_params replaces Uniforms::run_setters (src/webgl.rs:629-633). Both copy.  pt_set_spheres replaces the scene and nothing
 * else: accumulation, error estimate, textures and statistics stay, passes of the new scene add to what is there.  pt_set_params
 * replaces ALL uniforms, first_pass included (it overwrites what pt_render_until / pt_render_adaptive have advanced).  A
 * pt_set_params that CHANGES THE ROW PARTITION — band_* name another set of rows; band_count <= 1 is "all rows" whatever band_rows
 * and band_index hold — clears the accumulation, its sample count, the error estimate, both textures and the canvas (they held
 * other rows) and ends the validity of pt_adaptive_tiles; the statistics (PtStats.segments, samples, render_launches) keep counting.
 * It is refused with PT_ERR_CAPACITY, nothing changed, when a caller-bound accumulation buffer cannot hold the new rows.  A
 * pt_set_spheres that fails after its
 * first device write leaves the context without a scene: the render calls return PT_ERR_NOT_READY until a call succeeds. */
int pt_set_spheres(pt_ctx* ctx, const PtSphere* spheres, uint32_t n);
int pt_set_params(pt_ctx* ctx, const PtParams* params);

/* ---- rendering: replaces webgl::render -> draw (src/webgl.rs:180-205, :169-178) ---------------
 * pt_render enqueues ONE pass (`samples_per_pixel` samples at seed offset `time`) that adds each
 * pixel's linear radiance sum into the accumulation buffer.  Asynchronous on the context's
 * stream; no host synchronisation, no allocation (after pt_reserve_passes).
 * pt_render_passes enqueues n_passes passes in one launch; pass p uses u_time = time + p. The
 * result is bit-identical to n_passes pt_render calls with those times. */
int pt_render(pt_ctx* ctx);
int pt_render_passes(pt_ctx* ctx, uint32_t n_passes);
/* Pre-sizes the per-pass workspace so pt_render_passes(n <= max_passes) never allocates.  The reservation only grows: a smaller
 * max_passes leaves it as it is.  pt_render_passes with more passes than the largest reservation so far returns PT_ERR_CAPACITY
 * and enqueues nothing.  A refused reservation (PT_ERR_HIP) leaves the count as it was; the context's buffers are then not in place
 * after a failed allocation: the render and read-out calls return PT_ERR_CAPACITY until a sizing call (pt_reserve_passes, a
 * repartitioning pt_set_params, pt_resize) succeeds. */
int pt_reserve_passes(pt_ctx* ctx, uint32_t max_passes);
/* render_count = 0 (src/state.rs:343-346): clears accumulation, spp counter and statistics */
int pt_reset_accum(pt_ctx* ctx);
int pt_synchronize(pt_ctx* ctx);

/* ---- read-out: replaces the canvas read (src/dom.rs:126-143) -----------------------------------
 * Writes local_rows*width RGBA fp32 texels (row 0 = lowest owned row): rgb = accum / total_spp,
 * then sqrt when gamma != 0 (static/shader.frag:376-380); a = 1.  `out` may be a host or a
 * device pointer.  Synchronises the stream.  The divisor is read per pixel from the device-side
 * sample count (the buffer's .a), so it is also right after hipGraph replays of a captured
 * pt_render_passes, which the host-side counters cannot see. */
int pt_resolve(pt_ctx* ctx, float* rgba_out, int gamma);
/* Same, clamped and quantised to RGBA8 like the reference framebuffer (src/webgl.rs:109-119). */
int pt_resolve_rgba8(pt_ctx* ctx, uint8_t* rgba_out, int gamma);
/* Raw accumulation buffer (local_rows*width float4: r,g,b sums, a = spp): device pointer. */
int pt_accum_ptr(pt_ctx* ctx, void** dev_ptr, size_t* bytes);
/* Checkpoint / resume (the reference's accumulation state is its ping-pong textures +
 * render_count, src/state.rs:443-450): copy the accumulation buffer out / back in.  The sample
 * count travels inside the buffer (the .a of every pixel), so rendering k passes, pt_read_accum,
 * a new context with the same scene / uniforms / row partition, pt_load_accum and k more passes
 * give the bits of 2k uninterrupted passes.  `dst` / `src`: host or device pointers to
 * local_rows*width*16 bytes.  Both synchronise the stream.  pt_load_accum returns PT_ERR_INVALID, nothing changed, when `bytes` is not
 * exactly that size, and when the buffer is not an accumulation of whole passes: the sample counts of its first and last pixel
 * differ (a frame after a partial round of pt_render_adaptive is no checkpoint) or are not counts.  PtStats.segments keeps counting;
 * total_spp and samples follow the loaded count. */
int pt_read_accum(pt_ctx* ctx, float* dst, size_t bytes);
int pt_load_accum(pt_ctx* ctx, const float* src, size_t bytes);
/* Render into caller-owned device memory (e.g. a torch tensor) instead.  The caller owns the contents: passes add to what the
 * buffer holds, and the .a of its pixels is the sample count from then on.  NULL restores the context's own buffer, CLEARED (what
 * it held when the caller's buffer took its place is another frame's, possibly another row partition's).  Either way the error
 * estimate is cleared and the statistics keep counting.  PT_ERR_CAPACITY when `bytes` is below local_rows*width*16. */
int pt_bind_accum(pt_ctx* ctx, void* dev_ptr, size_t bytes);
/* Use a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the own stream.  The
 * device's default stream IS the NULL handle: name it as hipStreamLegacy, PT_STREAM_LEGACY. */
int pt_set_stream(pt_ctx* ctx, void* hip_stream);
#define PT_STREAM_LEGACY ((void*)1) /* = hipStreamLegacy */

/* ---- per-pixel error estimate: how noisy is the frame still? (build extension, opt-in: PT_OPT_ERROR_ESTIMATE) ----------
 * pt_render_passes writes every pass into a slab of its own and then folds the slabs into the accumulation in pass order.
 * While the estimate is on, the fold also keeps, per local pixel i, the running mean and sum of squared deviations of the
 * PASS SUMS (batch means; Welford's update) in two float4:
 *     A = {mean.r, mean.g, mean.b, n}      B = {M2.r, M2.g, M2.b, k}          n passes folded, k = their samples
 * For each pass p in order, with s = slab[p][i] = {sum r, sum g, sum b, spp}, in fp32, ONE IEEE operation per statement,
 * nothing fused, `/` correctly rounded:
 *     accum.c = accum.c + s.c  (c = r, g, b, w: the adds of a context without the estimate, in their order)
 *     n = n + 1.0f;   k = k + s.w;
 *     per channel c:  d = s.c - mean.c;  mean.c = mean.c + d / n;  e = s.c - mean.c;  M2.c = M2.c + d * e;
 * s.c is the pass SUM, not its mean, so all passes of an estimate must have the same samples_per_pixel: the first fold
 * after a clear decides, and pt_render / pt_render_passes with another value return PT_ERR_INVALID (clear first).  n and k
 * live in the buffer, like accum.w: the estimate stays right when a captured pt_render_passes is replayed from a hipGraph.
 * THE ESTIMATE SPEAKS FOR THE PASSES FOLDED SINCE ITS LAST CLEAR.  It is cleared wherever the accumulation is cleared or
 * replaced: pt_reset_accum, pt_tune when it launched anything, pt_resize, a pt_set_params that changes the row partition,
 * pt_load_accum, pt_bind_accum — after pt_load_accum the image holds more passes than the estimate knows of.
 * pt_render_frame(s) are not involved.
 * ASSUMPTION: the passes are independent, i.e. time_step is a step such as PT_TIME_STEP_DECORRELATED.  With whole-number
 * steps consecutive passes share random numbers (PtParams.time_step: the +27 % finding) and the estimate reads low.
 *
 * pt_error_ptr: the raw state, device pointer to local_rows*width pairs A, B (32 bytes per pixel, row 0 = lowest owned
 * row); PT_ERR_NOT_READY while the estimate is off — like the three read-outs below.
 * pt_resolve_error: the standard error of each pixel's mean as linear radiance, local_rows*width RGBA fp32 texels to a host
 * or device pointer; synchronises like pt_resolve.  Per pixel:
 *     if (!(n >= 2.0f) || !(k > 0.0f))  se = {0, 0, 0};
 *     else { q = n / k;  v.c = M2.c / (n * (n - 1.0f));  se.c = sqrtf(v.c) * q; }
 *     out = {se.r, se.g, se.b, n}                      and the estimate's own mean is  m.c = mean.c * q
 * pt_error_tiles: one record of four floats per 8x8 tile of the LOCAL rows (the work queue's tiles), ceil(width / 8) x
 * ceil(local_rows / 8) of them in row-major order; tiles_out (host or device) may be NULL to query the sizes only.  One
 * wave64 handles a tile, lane l owns local pixel (8 tx + l % 8, 8 ty + l / 8).  A lane is COUNTED when its pixel lies inside
 * the image, has n >= 2, k > 0 and finite se and m; it contributes e = (se.r*se.r + se.g*se.g) + se.b*se.b and
 * m2 = (m.r*m.r + m.g*m.g) + m.b*m.b, every other lane +0 to both, and the wave adds them with the fixed tree
 *     for off in 32, 16, 8, 4, 2, 1:  v[l] = v[l] + v[l + off]   (l < off)
 * record = {sum e, sum m2, counted lanes, min n over counted lanes (0 if none)}.  The same state gives the same bits on every
 * run and launch shape.
 * pt_error_stats: runs the tile kernel, copies the records (and a second float4 of tallies per tile: 1 MB in all at
 * 1920x1080) to the host and adds them in tile index order in double. */
typedef struct PtErrorStats {
  double sum_e2;    /* E: sum of the records' sum e  (squared standard errors over counted pixels and channels) */
  double sum_m2;    /* M: sum of the records' sum m2 (squared means, likewise)                                  */
  double rel_error; /* M > 0 ? sqrt(E / M) : 0     the frame's noise relative to its signal                   */
  double rms_error; /* counted ? sqrt(E / (3 counted)) : 0                                                    */
  uint64_t pixels;           /* local_rows * width                                                             */
  uint64_t pixels_counted;   /* the counted lanes of all tiles                                                 */
  uint64_t pixels_short;     /* pixels with !(n >= 2): too few passes for a variance                           */
  uint64_t pixels_nonfinite; /* pixels with n >= 2 that are not counted: se or m not finite (NaN / inf radiance), or !(k > 0) */
  uint32_t passes_min, passes_max; /* min / max n over the counted pixels (0 if none)                            */
  uint32_t passes_rendered;  /* pt_render_until: passes this call rendered (0 from pt_error_stats)             */
  uint32_t reached;          /* pt_render_until: 1 when it stopped because the target was met                  */
} PtErrorStats;
/* Multi-GPU: sum_e2, sum_m2 and the pixel counts of the ranks' row bands ADD (passes_min / passes_max: min / max), so the frame
 * figure of an N-rank render is the ranks' sums combined: rel_error = sqrt(sum of sum_e2 / sum of sum_m2). */
int pt_error_ptr(pt_ctx* ctx, void** dev_ptr, size_t* bytes);
int pt_resolve_error(pt_ctx* ctx, float* rgba_out);
int pt_error_tiles(pt_ctx* ctx, float* tiles_out, uint32_t* tiles_x, uint32_t* tiles_y);
int pt_error_stats(pt_ctx* ctx, PtErrorStats* out);
/* Render to a noise target.  Synchronous, a set-up-style call (not inside a stream capture): needs the estimate on
 * (PT_ERR_INVALID otherwise), passes_per_launch <= the reserved passes (PT_ERR_CAPACITY) and a finite positive target.  Loop:
 * render min(passes_per_launch, max_passes - done) passes, advance the context's params.first_pass by that many (so the frame
 * is the frame one uninterrupted pt_render_passes would give), take pt_error_stats; stop with reached = 1 when
 * rel_error <= target and pixels_short == 0, with reached = 0 (still PT_OK) when max_passes are spent.  first_pass stays
 * advanced: a second call continues the same frame.  Relies on the ASSUMPTION above (independent passes). */
int pt_render_until(pt_ctx* ctx, float target_rel_error, uint32_t passes_per_launch, uint32_t max_passes, PtErrorStats* out);

/* ---- adaptive sampling: render only the tiles that still miss the noise target (build extension, opt-in) ----------------
 * pt_render_adaptive is pt_render_until with a choice of tiles between the launches.  Preconditions and error codes are
 * pt_render_until's (estimate on, finite positive target, passes_per_round <= the reserved passes, not inside a stream
 * capture, one samples_per_pixel per estimate); PT_OPT_COUNT_WORK must be off (PT_ERR_INVALID).  The tiles are the 8x8 tiles
 * of pt_error_tiles: the work queue's.  `act` starts from a look (steps 4 to 6 with done = 0) at the state the call finds: in
 * a fresh estimate every pixel is short, so `act` starts as "all tiles"; in a frame under way it is the selection that state
 * gives, so two calls are exactly the rounds of one call of their passes together — and a call that finds the target met, or
 * no tile active, renders nothing.  Each round:
 *   1. k = min(passes_per_round, max_passes - done).
 *   2. Every tile active: the round IS pt_render_passes(k).  Otherwise a PARTIAL round: the trace launch runs over the work
 *      items of the active tiles only (the same kernel, reading a tile table that is a stable partition of the queue's cost
 *      order, active tiles first, and n_active x 64 x k items; it reports no costs), and the fold runs over their pixels only,
 *      statement for statement the fold above.  Pixels of idle tiles are neither read nor written.
 *   3. params.first_pass += k, done += k — k does not depend on how many tiles ran, so a pass index is frame-wide: A PIXEL HOLDS
 *      EXACTLY THOSE PASSES OF THE UNINTERRUPTED FRAME DURING WHICH ITS TILE WAS ACTIVE, FOLDED IN ORDER.
 *   4. pt_error_stats -> out; passes_rendered = done; reached = rel_error <= target && pixels_short == 0.
 *   5. `act` for the next round, THE SELECTION RULE, on the host in double, one IEEE operation per statement, from the records
 *      and tallies pt_error_stats has just copied — E, M, C = sum_e2, sum_m2, pixels_counted; per tile t: e_t = the record's
 *      sum e, c_t its counted lanes, short_t its pixels with !(n >= 2):
 *          tau = (double)target;  t2 = tau * tau;  b = t2 * M;  Cd = (double)C;
 *          per tile t:  lhs = (double)e_t * Cd;  rhs = b * (double)c_t;  active_t = short_t > 0 || lhs > rhs;
 *      A tile is active while its mean squared standard error per counted pixel is above the per-pixel share that meets the
 *      frame target, if every tile meets it.  A tile with no counted and no short pixel is never active: sampling cannot help
 *      it (it lies outside the image or holds non-finite radiance).
 *   6. Stop when the target is reached, when done >= max_passes, when no tile is active.
 * first_pass stays advanced: a second call continues the frame.  After a partial
 * round the pixels of one frame hold different numbers of passes; every read-out divides by the pixel's own count,
 * PtErrorStats.passes_min / passes_max show the spread, and PtStats.total_spp is pixel (0, 0)'s count.  PtStats.samples,
 * render_launches and render_kernel_ms count a partial round like any launch (samples: the camera paths really started).
 * Multi-GPU: a band context selects on its own band's E, M and C; the ranks' choices are then not the single-GPU frame's. */
typedef struct PtAdaptiveStats {
  uint32_t rounds;         /* launches this call made                                              */
  uint32_t partial_rounds; /* of them, launches over fewer than all tiles                          */
  uint32_t tiles;          /* 8x8 tiles of the local rows                                          */
  uint32_t tiles_active;   /* tiles the rule selects after the last look                           */
  uint64_t tile_passes;    /* sum over the rounds of (active tiles x passes of the round)          */
  uint64_t samples;        /* camera paths this call started: in-image pixels of active tiles x passes x spp */
} PtAdaptiveStats;
int pt_render_adaptive(pt_ctx* ctx, float target_rel_error, uint32_t passes_per_round, uint32_t max_passes, PtErrorStats* out,
                       PtAdaptiveStats* adaptive_out /* may be NULL */);
/* The tables of the most recent partial round.  base = the cost order it partitioned.  order = the table the trace launch read.
 * n_tiles entries each (host pointers; capacity: the tile count of pt_error_tiles).  Pointers may be NULL (sizes only).
 * PT_ERR_NOT_READY before the first partial round, and again after pt_set_spheres, pt_resize and any repartition. */
int pt_adaptive_tiles(pt_ctx* ctx, uint32_t* base_out, uint32_t* order_out, uint32_t* n_tiles, uint32_t* n_active);

/* ---- variance-guided filtered read-out of the estimate (build extension, opt-in: PT_OPT_ERROR_ESTIMATE) ------------------
 * pt_resolve_filtered: the estimate's own mean of each pixel, averaged with those neighbours within `radius` whose means differ
 * from it by no more than their standard errors explain (kappa standard errors of the difference, all three channels
 * together).  rgba_out: host or device pointer to local_rows*width RGBA fp32 texels, row 0 = lowest owned row.  Synchronises
 * like pt_resolve: a read-out, not for use inside a stream capture.
 * PT_ERR_INVALID for a NULL ctx or rgba_out, for radius > PT_FILTER_MAX_RADIUS, for a kappa that is not finite or is below 0;
 * PT_ERR_NOT_READY while the estimate is off, like pt_resolve_error.
 * THE CALL READS THE ESTIMATE'S STATE ONLY.  It never reads accum: it speaks for the passes the estimate knows of.
 * fp32, ONE IEEE operation per statement, nothing fused, `/` and sqrtf correctly rounded (the error kernels' discipline):
 *     (the read-out of DESIGN.md §4.8b is pt_resolve_error's above: se, and m.c = mean.c * q; both 0 where !known)
 *     per pixel: (se, m, known) = the read-out of §4.8b (pixel_error)
 *                counted = known && finite se && finite m     (the tile kernel's "counted")
 *                v.c = se.c * se.c
 *     once:      k2 = kappa * kappa
 *     rows p may look at: band_count <= 1: all local rows
 *                         otherwise: the local rows ly with ly / band_rows == y_p / band_rows
 *                         (p's own chunk of consecutive image rows; local rows of different chunks
 *                         are not neighbours in the image)
 *     centre p = (x, y) not counted:
 *         f = m                                   (0 where unknown, non-finite stays non-finite)
 *         cnt = 0
 *     centre p counted:
 *         sum = {+0, +0, +0}
 *         cnt = +0
 *         for dy = -R .. R ascending, for dx = -R .. R ascending:
 *             q = (x + dx, y + dy)
 *             skip unless 0 <= q.x < width, q.y is a row p may look at, and q is counted
 *             if (dx, dy) != (0, 0):
 *                 d.c = m_p.c - m_q.c
 *                 d2.c = d.c * d.c
 *                 t = (d2.r + d2.g) + d2.b
 *                 s.c = v_p.c + v_q.c
 *                 u = (s.r + s.g) + s.b
 *                 rhs = k2 * u
 *                 skip unless t <= rhs            (a NaN on either side skips)
 *             sum.c = sum.c + m_q.c
 *             cnt = cnt + 1.0f
 *         f.c = sum.c / cnt
 *     gamma != 0: f.c = sqrtf(f.c)                (every pixel)
 *     out = {f.r, f.g, f.b, cnt}                  (.a = accepted taps, 0 for an uncounted centre)
 * Radius 0 is the estimate's own mean with cnt 1: the centre is always accepted.  The test is symmetric in p and q.
 * Multi-GPU: a band context filters inside its own row chunks, so its gathered frame differs from the single-GPU filtered
 * frame near chunk borders.  A host that wants exactly that frame gathers the ranks' raw states (pt_error_ptr), loads them
 * into one full-height context and filters there: the state is the only input, so this works.
 * There is no standard error of the filtered frame (the propagated variance reads far too low). */
#define PT_FILTER_MAX_RADIUS 4
#define PT_FILTER_KAPPA_DEFAULT 2.0f
int pt_resolve_filtered(pt_ctx* ctx, float* rgba_out, uint32_t radius, float kappa, int gamma);

/* ---- patch-wise filtered read-out: neighbourhoods, not pixels, pass the test (build extension, opt-in: PT_OPT_ERROR_ESTIMATE) --
 * pt_resolve_filtered_patch: pt_resolve_filtered with another acceptance test.  A neighbour q is averaged into p when the
 * (2 patch + 1)^2 neighbourhoods around p and q, compared texel by texel, differ by no more than their standard errors explain:
 * the squared differences and the variances are summed over the patch before they are compared.  One noisy pixel no longer
 * decides; the same error in a whole neighbourhood (a shadow's or a reflection's edge on a diffuse surface) does.  Only m_q
 * enters the average: the patch decides, it is not averaged.  rgba_out, the synchronisation and what the call reads and leaves
 * alone are pt_resolve_filtered's: the estimate's state only, never accum, never the feature planes.
 * PT_ERR_INVALID for a NULL ctx or rgba_out, for radius > PT_FILTER_MAX_RADIUS, for patch > PT_FILTER_MAX_PATCH, for a kappa
 * that is not finite or is below 0, in this order; PT_ERR_NOT_READY while the estimate is off.  A context with no pixels: PT_OK.
 * fp32, ONE IEEE operation per statement, nothing fused, `/` and sqrtf correctly rounded, P = patch:
 *     patch-wise test: (se, m, known), counted, v.c, k2 and the rows p may look at are pt_resolve_filtered's (§4.8d)
 *     centre p = (x, y) not counted:
 *         f = m                                   (0 where unknown, non-finite stays non-finite)
 *         cnt = 0
 *     centre p counted:
 *         sum = {+0, +0, +0}
 *         cnt = +0
 *         for dy = -R .. R ascending, for dx = -R .. R ascending:
 *             q = (x + dx, y + dy)
 *             skip unless 0 <= q.x < width, q.y is a row p may look at, and q is counted
 *             if (dx, dy) != (0, 0):
 *                 T = +0
 *                 U = +0
 *                 for oy = -P .. P ascending, for ox = -P .. P ascending:
 *                     a = (x + ox, y + oy), b = (q.x + ox, q.y + oy)
 *                     skip unless 0 <= a.x < width, 0 <= b.x < width, a.y and b.y are rows p may look at, a and b are counted
 *                     d.c = m_a.c - m_b.c
 *                     d2.c = d.c * d.c
 *                     t = (d2.r + d2.g) + d2.b
 *                     s.c = v_a.c + v_b.c
 *                     u = (s.r + s.g) + s.b
 *                     T = T + t
 *                     U = U + u
 *                 rhs = k2 * U
 *                 skip unless T <= rhs            (a NaN on either side skips)
 *             sum.c = sum.c + m_q.c
 *             cnt = cnt + 1.0f
 *         f.c = sum.c / cnt
 *     gamma != 0: f.c = sqrtf(f.c)                (every pixel)
 *     out = {f.r, f.g, f.b, cnt}                  (.a = accepted taps of the patch-wise test, 0 for an uncounted centre)
 * The term (ox, oy) = (0, 0) is always present for such a tap (a = p and b = q are counted rows p may look at), and +0 + t and
 * +0 + u are exact: patch = 0 IS pt_resolve_filtered's test, the two calls give the same bits.  An uncounted a or b drops its
 * term, never the tap.  The test is symmetric in p and q inside one chunk and in a context that is no band; at a chunk border
 * "rows p may look at" is p's chunk, and p and q of one chunk still see the same terms.  Multi-GPU: the gathered frame of a band
 * differs from the single-GPU frame within radius + patch rows of a chunk border (gather the raw states and filter in one
 * full-height context, as with pt_resolve_filtered).  There is no standard error of the filtered frame. */
#define PT_FILTER_MAX_PATCH 1
#define PT_FILTER_PATCH_KAPPA_DEFAULT 1.5f
int pt_resolve_filtered_patch(pt_ctx* ctx, float* rgba_out, uint32_t radius, uint32_t patch, float kappa, int gamma);

/* ---- first-hit feature planes: albedo, normal, hit point and ids per pixel (build extension, opt-in: PT_OPT_FEATURES) ----
 * What a denoiser, a picker or a compositor wants beside the colour: for every local pixel the first surface ONE deterministic
 * ray through the pixel centre meets.  pt_render_features is one launch of the trace kernels' feature builds (a code object of
 * their own, loaded when the option is turned on), asynchronous on the context's stream, no allocation; it goes through the
 * geometry path forced or settled (an unsettled PT_GEOM_AUTO: its cold path; PT_GEOM_LDS: the scalar walk, as with roulette),
 * is never one of PT_GEOM_AUTO's measuring launches, and leaves the accumulation, the estimate, the textures, the canvas,
 * first_pass, the tile order and the tile costs alone.  Of PtStats it moves only `segments`, by one per in-image local pixel
 * (and `far_rays`, which counts segments of the grid walk's far path, by those of them that take it);
 * pt_last_trace_build returns 4 after it.  The debug overlay and Russian roulette do not act on it.
 * THE RAY, fp32, for local pixel (px, ly), row 0 the lowest owned row, image row y = pt_band_row(..., ly):
 *     vx = float(2 px + 1) / float(width) - 1          vy = float(2 y + 1) / float(height) - 1     (the pixel centre)
 *     s = (vx + 1) * 0.5                               t = (vy + 1) * 0.5
 *     dd.c = fma(t, vertical.c, fma(s, horizontal.c, lower_left_corner.c))
 *     o = camera_origin                                d.c = dd.c - camera_origin.c
 * No jitter, no lens, no seed: lens_radius, time, time_step, samples_per_pixel, max_depth and first_pass do not enter.
 * hit_world(o, d, t_min, t_max) is the trace kernels' own: ties go to the later sphere, a negative radius flips the normal.
 * THE RECORD: four planes of local_rows*width 16-byte texels, row 0 = lowest owned row:
 *     plane              texel on a hit                                             texel on a miss
 *     PT_FEAT_ALBEDO 0   {albedo.r, albedo.g, albedo.b, t}: PtSphere.albedo as      {bg.r, bg.g, bg.b, +0}: what the path tracer
 *                        uploaded; t the accepted root, in units of unnormalised d  returns for this ray (sky gradient / zeros)
 *     PT_FEAT_NORMAL 1   {n.x, n.y, n.z, +0}: the face-forward normal               all +0
 *     PT_FEAT_POINT  2   {hp.x, hp.y, hp.z, +0}: hp.c = fma(d.c, t, o.c)            all +0
 *     PT_FEAT_IDS    3   int32 x4 {list index, PtSphere.uuid, PtSphere.type as      {-1, -1, -1, 0}
 *                        uploaded (any value), front_face}
 * The floats of a hit are the bits the path tracer's own hit record holds for that segment.  A device pick is IDS[y][x].
 * The planes are one allocation: pt_features_ptr(plane) is its device pointer (and bytes = local_rows*width*16) while the
 * option is on; pt_resize and a repartition reallocate them.  They speak for the scene and uniforms of the last
 * pt_render_features: pt_set_spheres, pt_set_params, pt_resize, a pt_refit_grid or pt_tune that rebuilds the grid, and turning
 * the option off end that, and pt_read_features (host or device pointer; synchronises like pt_resolve) returns PT_ERR_NOT_READY
 * until the next pt_render_features.  Per band, like every buffer.
 * PT_ERR_INVALID: NULL ctx (or out pointer), a plane out of range, pt_render_features / pt_read_features under PT_OPT_COUNT_WORK
 * or inside a stream capture.  PT_ERR_NOT_READY: no scene or no uniforms yet, or the option is off.  A band that owns no rows:
 * PT_OK, nothing to do. */
enum { PT_FEAT_ALBEDO = 0, PT_FEAT_NORMAL = 1, PT_FEAT_POINT = 2, PT_FEAT_IDS = 3, PT_FEAT_PLANES = 4 };
int pt_render_features(pt_ctx* ctx);
int pt_features_ptr(pt_ctx* ctx, int plane, void** dev_ptr, size_t* bytes);
int pt_read_features(pt_ctx* ctx, int plane, void* out);

/* ---- temporal reprojection: carry the accumulation across a camera move (build extension, opt-in: PT_OPT_REPROJECT) ---------
 * The reference restarts its image whenever the camera moves (render_count = 0, src/state.rs:343-346), and so does a host that
 * calls pt_reset_accum.  pt_reproject instead moves the accumulated radiance to where the same surface lies in the NEW view: for
 * each pixel of the new view its first-hit point (the feature planes) is projected into the camera of an earlier view, the
 * HISTORY; where the history planes show the same sphere and side at that place, within a distance of tolerance_px pixel
 * footprints, the accumulation is fetched from there, bilinearly, and its sample count capped, so that fresh samples soon
 * outweigh what no longer holds (reflections and refractions move with the camera: they get the smaller cap).
 * A host's tick while the camera moves:
 *     pt_keep_history(ctx);  pt_set_params(ctx, next);  pt_render_features(ctx);  pt_reproject(ctx, &opt);  pt_render_passes(ctx, n);
 * with `time` advanced from tick to tick, so that the fresh samples are new ones.
 * pt_keep_history: needs the option on and valid feature planes (PT_ERR_NOT_READY otherwise: pt_read_features' rule); copies the
 * PT_FEAT_IDS and PT_FEAT_POINT planes device-to-device into the history planes and remembers the PtParams they were rendered
 * with.  Asynchronous on the context's stream, no synchronisation, no allocation.
 * pt_load_history: the same from caller memory (host or device pointers to local_rows*width*16 bytes each) and an explicit
 * `prev`, which must have the context's width, height and row partition (PT_ERR_INVALID otherwise).  Synchronises.
 * THE HISTORY ENDS — pt_reproject returns PT_ERR_NOT_READY afterwards — at pt_set_spheres (its indices would name other spheres),
 * at pt_resize, at a pt_set_params that changes the row partition, when the option is turned off, and at pt_reproject itself:
 * the call is one-shot, afterwards the accumulation belongs to the new view.  An ordinary pt_set_params does NOT end it.
 * pt_reproject: needs the option on, a valid history and valid CURRENT planes, i.e. a pt_render_features after the
 * pt_set_params of the new view (PT_ERR_NOT_READY otherwise).  PT_ERR_INVALID: NULL arguments, a cap that is not a whole number
 * in [0, 2^24), a tolerance_px that is not finite or is below 0, a history camera pt_reproject_constants refuses, a call inside
 * a stream capture.  A context with no local pixels: PT_OK.  Asynchronous, no synchronisation, no allocation: one kernel writes
 * the staging buffer pt_load_accum uses, one device-to-device copy brings it into the accumulation — pt_accum_ptr and a
 * caller-bound buffer keep their addresses.  The error estimate is cleared, as pt_load_accum clears it (history is sums, not
 * passes).  first_pass, the textures, the canvas, the tile order, the tile costs and PtStats.segments do not move.  Afterwards
 * the pixels of the frame hold DIFFERENT sample counts: every read-out divides by the pixel's own count and a zero count reads
 * 0, PtStats.total_spp is pixel (0, 0)'s count as after a partial round of pt_render_adaptive (0 where that pixel kept
 * nothing), and the buffer is no checkpoint for pt_load_accum.  PtStats.samples counts camera paths started and does not move.
 * HOST CONSTANTS (pt_reproject_constants: pure host arithmetic, no device; csrc/pt_reproject_plan.hpp), computed in double from
 * the float fields of `prev`, one IEEE operation per statement, each result narrowed ONCE:
 *     O = camera_origin;  Hh = horizontal;  V = vertical;  L = lower_left_corner
 *     e = L - O;  n = Hh x V;  N = n / (e.n)
 *     A = (V x n) / (Hh.(V x n));  B = (n x Hh) / (V.(n x Hh))
 *     ea = e.A;  eb = e.B                                        (A and B as doubles)
 *     k = tolerance_px^2 * (Hh.Hh) / width^2
 *     out16 = {O.xyz, N.xyz, A.xyz, B.xyz, ea, eb, k, 0}
 * (a x b = {a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x};  a.b = (a.x*b.x + a.y*b.y) + a.z*b.z.)  PT_ERR_INVALID when
 * e.n or either denominator is 0, or when any result is not finite.  The lens does not enter: the planes are pinhole.
 * PER LOCAL PIXEL p = (px, ly), fp32, ONE IEEE operation per statement, nothing fused, `/` correctly rounded.  ids and Pn come
 * from the CURRENT planes (PT_FEAT_IDS, PT_FEAT_POINT), HIDS, HPNT and ACC from the history planes and the accumulation as the
 * call finds them; out starts as {+0, +0, +0, +0}:
 *     done if ids.x < 0                                            (a miss: sky needs no history)
 *     w.c = Pn.c - O.c
 *     lam = (w.x*N.x + w.y*N.y) + w.z*N.z ;  done unless lam > 0
 *     ws, wt likewise with A, B
 *     s = ws / lam ;  s = s - ea ;  t = wt / lam ;  t = t - eb
 *     fx = s * float(width) ;  fx = fx - 0.5f ;  fy = t * float(height) ;  fy = fy - 0.5f     (fy is an IMAGE row, 0 = bottom)
 *     done unless fx > -1 && fx < float(width) && fy > -1 && fy < float(height)              (NaN: done; only now convert to int)
 *     x0f = floorf(fx); ax = fx - x0f; y0f = floorf(fy); ay = fy - y0f;  x0 = (int)x0f, y0 = (int)y0f
 *     lam2 = lam*lam ;  rhs = k * lam2
 *     cap = ids.z == PT_DIFFUSE ? cap_diffuse : cap_other
 *     sum = {+0,+0,+0}; cnt = +0; wsum = +0
 *     for dy in 0,1 (outer), dx in 0,1:
 *         q = (x0+dx, y0+dy); skip unless 0 <= q.x < width, 0 <= q.y < height and q.y is a row this context owns (the inverse of
 *             pt_band_row; band_count <= 1: every row); lq = its local row
 *         skip unless HIDS[q].x == ids.x && HIDS[q].w == ids.w
 *         d.c = HPNT[q].c - Pn.c ;  d2 = (d.x*d.x + d.y*d.y) + d.z*d.z ;  skip unless d2 <= rhs
 *         a = ACC[q] ;  skip unless a.w > 0
 *         wx = dx ? ax : 1.0f - ax ;  wy = dy ? ay : 1.0f - ay ;  g = wx*wy ;  skip unless g > 0
 *         m.c = a.c / a.w ;  sum.c = sum.c + g*m.c (two statements) ;  cnt = cnt + g*a.w (two) ;  wsum = wsum + g
 *     done unless wsum > 0
 *     nq = cnt / wsum ;  nq = floorf(nq) ;  if (nq > cap) nq = cap ;  done unless nq >= 1
 *     col.c = sum.c / wsum ;  out = {col.r*nq, col.g*nq, col.b*nq, nq}
 * Counts stay whole numbers; non-finite colour stays non-finite.  The distance test is in pixel footprints at the history
 * camera's depth: it catches the far side of the same sphere and the horizon.  A band context gathers from its own rows only: a
 * tap on a row another band owns is skipped (no history rows are exchanged between ranks).
 * pt_reproject_stats: synchronises; the tallies of the last pt_reproject (PT_ERR_NOT_READY before the first): pixels =
 * local_rows*width, pixels_hit those with ids.x >= 0, pixels_kept those with out.w > 0, samples_kept the sum of nq.  Integers,
 * summed per workgroup and added with one integer atomic each: exact, whatever the order. */
#define PT_REPROJECT_TOLERANCE_DEFAULT 2.0f
#define PT_REPROJECT_CAP_DIFFUSE_DEFAULT 32.0f
#define PT_REPROJECT_CAP_OTHER_DEFAULT 8.0f
typedef struct PtReprojectOptions {
  float cap_diffuse;  /* the most samples a kept PT_DIFFUSE pixel carries over */
  float cap_other;    /* ... and a pixel of any other material (0: diffuse surfaces only) */
  float tolerance_px;
  uint32_t _pad;
} PtReprojectOptions;
typedef struct PtReprojectStats {
  uint64_t pixels, pixels_hit, pixels_kept, samples_kept;
} PtReprojectStats;
int pt_keep_history(pt_ctx* ctx);
int pt_load_history(pt_ctx* ctx, const PtParams* prev, const void* ids, const void* point);
int pt_reproject(pt_ctx* ctx, const PtReprojectOptions* options);
int pt_reproject_stats(pt_ctx* ctx, PtReprojectStats* out);
int pt_reproject_constants(const PtParams* prev, float tolerance_px, float out16[16]);

/* ---- temporal reprojection WITH the error estimate (build extension, opt-in: PT_OPT_REPROJECT and PT_OPT_ERROR_ESTIMATE) -------
 * pt_reproject clears the estimate's state, so while the camera moves nothing that reads the state (pt_resolve_filtered,
 * pt_resolve_filtered_patch, pt_error_tiles, pt_error_stats) knows of the history.  pt_reproject_estimate is pt_reproject in
 * every respect — the same preconditions and errors in the same order, the history used up, the SAME BITS in the accumulation,
 * the same three tallies, the same things that do not move, asynchronous, no synchronisation, no allocation, refused inside a
 * stream capture, PT_OK for a context with no local pixels — but for the state (pt_error_ptr: A = {mean.rgb, n}, B = {M2.rgb, k}
 * per local pixel), which is gathered from the history's places by the same kernel pass instead of being cleared.  In the tick
 * above it takes pt_reproject's place.  Additionally: PT_ERR_NOT_READY while PT_OPT_ERROR_ESTIMATE is off (checked after
 * PT_OPT_REPROJECT, before the capture, the history and the planes).  The state's staging buffer (2 texels per local pixel: the
 * gather reads the state at other pixels' places) is allocated wherever the context sizes its buffers while both options are on.
 * The remembered samples_per_pixel of the folded passes stays as it is, so the next fold with another value is refused until a
 * clear, as ever.  With nothing folded since the last clear the call IS pt_reproject and the state stays zero.
 * THE STATE'S STATEMENTS, fp32, ONE IEEE operation per statement, nothing fused, `/` correctly rounded.  Up to and including the
 * per-tap tests on range, row ownership, HIDS == ids, d2 <= rhs, and g = wx*wy, g > 0 they are pt_reproject's; the accumulation's
 * sums are pt_reproject's own (under their `a.w > 0`), the estimate's sums are separate and do NOT depend on a.w > 0:
 *     host, once: S = err_spp ;  Sf = float(S) ;  S2 = Sf*Sf ;  capP_x = floorf(cap_x / Sf) for the two caps
 *     per pixel: mu = W = {+0,+0,+0} ;  cntE = wsumE = +0 ;  capP = ids.z == PT_DIFFUSE ? capP_diffuse : capP_other
 *     per tap that passed the common tests, Aq = A[q], Bq = B[q]:
 *         skip (estimate only) unless Aq.w >= 2 && Bq.w > 0
 *         qq = Aq.w / Bq.w ;  qq2 = qq*qq ;  n1 = Aq.w - 1.0f
 *         per channel: m = Aq.c*qq ; gm = g*m ; mu.c = mu.c + gm ;
 *                      pv = Bq.c / n1 ; pv = pv*qq2 ; gp = g*pv ; W.c = W.c + gp
 *         gn = g*Aq.w ; cntE = cntE + gn ; wsumE = wsumE + g
 *     after the taps: A' = B' = all +0 unless wsumE > 0
 *         nE = cntE / wsumE ; nE = floorf(nE) ; if (nE > capP) nE = capP ; all +0 unless nE >= 2
 *         n1 = nE - 1.0f ; kE = nE*Sf
 *         per channel: a = mu.c / wsumE ; mean'.c = a*Sf ; b = W.c / wsumE ; b = b*n1 ; M2'.c = b*S2
 *         A' = {mean', nE} ;  B' = {M2', kE}
 *     (a pixel that is `done` before the taps leaves A' = B' = all +0)
 * The per-sample mean is blended bilinearly; the per-pass variance of a sample is blended the same way (as SVGF blends moments:
 * conservative against the variance of the blended mean); the pass count is the floor of the blended count, capped in PASSES.
 * The read-out of the carried state gives se'^2 = W / nE: a cap that bites widens the standard error.  A class whose cap is below
 * 2 passes carries no estimate.  Non-finite operands stay non-finite (the read-outs' "counted" rule deals with them).
 * The carried estimate steers a filter; it is NO stopping criterion: what lags behind the camera (reflections) is bias the
 * standard error does not know of (DESIGN.md §4.8h has the measured calibration). */
int pt_reproject_estimate(pt_ctx* ctx, const PtReprojectOptions* options);

/* ---- ray queries: the closest hit of the CALLER's rays (build extension, opt-in: PT_OPT_RAY_QUERIES) ---------------------------
 * pt_render_features answers "what does the ray through this pixel centre meet"; pt_query_rays answers it for any ray: an
 * autofocus or selection ray, a pick under a cursor while the uniforms are already the next tick's, a visibility probe between
 * two points, a probe that starts on a surface, a batch from a baking tool.  Ray i is hit_world(origin, direction, t_min, t_max)
 * of the trace kernels themselves, through the geometry path forced or settled exactly as pt_render_features chooses it (the
 * query builds: the feature builds with the ray read from memory, a code object of their own): the direction is NOT normalised
 * (t is in its units, and t_min = 0.001 and t_max = 1e5 are too: a short direction sees less far), ties go to the later sphere, a negative radius flips the normal.  There is no camera, no jitter, no lens
 * and no seed: of PtParams the camera, time, time_step, samples_per_pixel, max_depth and first_pass do not enter; width, height
 * and the row partition only shape the work items (which is why pt_set_params must have come first), background_mode gives a
 * miss its colour.
 * THE RECORD of ray i, hits[i], is the feature record of pt_render_features above, field for field: {albedo, t}, {normal,
 * _pad0}, {point, _pad1} and {index, uuid, type, front_face} are the texels of PT_FEAT_ALBEDO, PT_FEAT_NORMAL, PT_FEAT_POINT
 * and PT_FEAT_IDS on a hit and on a miss as the table there states them (a miss: the background for THIS ray, ids -1, -1, -1, 0);
 * the pads are +0.
 * INVALID RAYS: a ray with a non-finite component (NaN, +inf, -inf) in origin or direction, or whose three direction components
 * are all +0 or -0, is invalid.  That is decided on the device before any walk; its record is all +0 with the ids
 * {PT_RAY_INVALID, PT_RAY_INVALID, PT_RAY_INVALID, 0}, and it is not counted in PtStats.segments.  Every other ray is valid and
 * is answered, however long, short or far away (|d|^2 outside (1e-12, 1e6), an origin component at or beyond 1e15: the trace
 * kernels' literal loop, as for such a bounce ray).  The pads of PtRay are not read.
 * `rays` and `hits` are host or device pointers (n of each), as pt_resolve takes them.  The call is synchronous on the context's
 * stream: it returns when hits[0..n) are written, and writes nothing else.  It works through n in batches of pt_query_batch(ctx)
 * rays, one launch each (ray i of a batch is work item "local pixel i"; a launch covers only the tile rows its rays occupy, so
 * one ray costs one tile row, not a frame); n == 0 is PT_OK with nothing done.
 * What it leaves alone: the accumulation, the estimate, the feature and history planes and their validity, the textures and the
 * canvas, first_pass, the tile order and costs, the geometry path (never a measuring launch of PT_GEOM_AUTO, nothing settles)
 * and pt_last_trace_build.  Of PtStats it moves `segments` by one per valid ray and `far_rays` by those of them that take the
 * grid walk's far path; nothing else.
 * PT_ERR_INVALID: NULL ctx, rays or hits (n > 0), PT_OPT_COUNT_WORK on, or inside a stream capture (refused before anything is
 * enqueued).  PT_ERR_NOT_READY: the option is off, no scene or no uniforms yet, or a band that owns no rows (it has no work
 * items to decode rays against: ask another rank; the answer does not depend on the rows a context owns).  PT_ERR_CAPACITY: the
 * planes are not in place after a failed allocation.
 * pt_query_batch: the rays one launch takes, i.e. the local pixel count; 0 for a NULL ctx or while pt_query_rays would return
 * PT_ERR_NOT_READY or PT_ERR_CAPACITY. */
#define PT_RAY_INVALID (-2)
typedef struct PtRay {
  float origin[3];
  float _pad0;
  float direction[3];
  float _pad1;
} PtRay; /* 32 bytes */
typedef struct PtRayHit {
  float albedo[3], t;
  float normal[3], _pad0;
  float point[3], _pad1;
  int32_t index, uuid, type, front_face;
} PtRayHit; /* 64 bytes */
int pt_query_rays(pt_ctx* ctx, const PtRay* rays, uint32_t n, PtRayHit* hits);
uint32_t pt_query_batch(pt_ctx* ctx);

/* ---- radiance queries: the path-traced radiance along the CALLER's rays (needs PT_OPT_RAY_QUERIES on; no option of its own) ----
 * pt_query_rays says what a ray meets; pt_query_radiance says how much light arrives along it: an irradiance or reflection
 * probe, a baking tool's batch, a second view (a mirror, a minimap), auto-exposure from a point in the scene — without moving
 * the camera and without touching the accumulation.  Ray i is walked n_passes * samples_per_pixel times by the plain estimator
 * of pt_render_passes (static/shader.frag:297-339 with the emissive and background extensions), through the geometry path
 * forced or settled exactly as pt_query_rays chooses it (the radiance builds: the plain builds with the ray read from memory, a
 * code object of their own, loaded at the first call); PT_OPT_RUSSIAN_ROULETTE and the debug overlay do not act, as with
 * pt_render_features.
 * THE RAY: hit_world of the trace kernels themselves, as pt_query_rays states it: the direction is NOT normalised, t_min = 0.001
 * and t_max = 1e5 are in its units, ties go to the later sphere, a negative radius flips the normal.
 * WHAT ENTERS of PtParams: time, time_step (0 means 1), first_pass, samples_per_pixel, max_depth and background_mode; width,
 * height and the row partition shape the work items and therefore the SEEDS.  The camera, the lens and render_count do not
 * enter.  first_pass is NOT advanced: the same call again gives the same bits.
 * THE RECORD of ray i, out[i], fp32, one IEEE operation per statement.  B = pt_query_batch(ctx); ray i lies in batch b = i / B
 * at place j = i % B:
 *   px = j % width;  ly = j / width;  y = pt_band_row(band_rows, band_index, band_count, ly)   (band_count <= 1: y = ly)
 *   vx = float(2 px + 1) / float(width) - 1;   vy = float(2 y + 1) / float(height) - 1
 *   out = {+0, +0, +0, +0}
 *   for p = 0 .. n_passes - 1:
 *       u_time = time + float(first_pass + b * n_passes + p) * step        (multiply, then add: the render calls' rule)
 *       seed = init_global_seed(vx, vy, u_time)                            (static/shader.frag:354-357)
 *       s = {+0, +0, +0}
 *       for k = 0 .. samples_per_pixel - 1:
 *           c = ray_color(origin_i, direction_i, seed)     (shader.frag:297-339; the seed is carried from sample to sample;
 *                                                           NO jitter draw and NO lens draws precede it)
 *           s.c = s.c + c.c
 *       out.sum.c = out.sum.c + s.c ;  out.samples = out.samples + float(samples_per_pixel)
 * The estimate of the radiance is sum / samples.
 * PASSES PER BATCH: a batch takes passes of its own (b * n_passes): rays at the same place of different batches share no random
 * numbers.  The record of a ray therefore depends on its INDEX in the call and on the context's SIZE (width, height, the row
 * partition), not on the ray alone: two rays with the same origin and direction at different indices get different samples of
 * the same expectation.  The second batch of a call is the first batch of a call at first_pass + n_passes.
 * INVALID RAYS: invalid as pt_query_rays states it (a non-finite component, or a direction of three zeros), decided on the
 * device before any walk; the record is {+0, +0, +0, +0}, and samples == 0 is the mark.  Every other ray has samples ==
 * n_passes * samples_per_pixel.
 * `rays` and `out` are host or device pointers (n of each).  The call is synchronous on the context's stream: it returns when
 * out[0..n) are written, and writes nothing else.  One launch plus one fold per batch, over the tile rows the batch's rays
 * occupy; n == 0 is PT_OK with nothing done.  n_passes is at least 1 and at most the passes reserved with pt_reserve_passes:
 * the context's pass slabs are the workspace (they are free between calls: every render call folds them before it returns).
 * What it moves: PtStats.segments by exactly the segments traced (invalid rays add none) and far_rays as a render would.  What
 * it leaves alone: everything pt_query_rays leaves alone — the accumulation, the estimate, the feature and history planes and
 * their validity, the textures and the canvas, first_pass, the tile order and costs (no cost feedback), the geometry path
 * (never a measuring launch) and pt_last_trace_build — and PtStats.samples, total_spp, render_launches and render_kernel_ms.
 * PT_ERR_INVALID: NULL ctx, rays or out (n > 0), PT_OPT_COUNT_WORK on, inside a stream capture, n_passes == 0.
 * PT_ERR_NOT_READY: PT_OPT_RAY_QUERIES is off, no scene or no uniforms yet, or a band that owns no rows.  PT_ERR_CAPACITY: the
 * query planes are not in place after a failed allocation, or n_passes exceeds the reservation.  (Checked in pt_query_rays'
 * order, then n_passes.) */
typedef struct PtRayRadiance {
  float sum[3];
  float samples;
} PtRayRadiance; /* 16 bytes: an accumulation texel */
int pt_query_radiance(pt_ctx* ctx, const PtRay* rays, uint32_t n, uint32_t n_passes, PtRayRadiance* out);

/* ---- gather queries: the irradiance at points and SH probes, made on the device (needs PT_OPT_RAY_QUERIES on; no option of its own) ----
 * pt_query_radiance answers a ray; these two answer "how much light arrives HERE": the rays of an item are made on the device,
 * walked by pt_query_radiance's own launches and folds, and reduced on the device — 32 bytes up and 16 or 112 bytes down per
 * item instead of 32 up and 16 down per ray.  The kernels are a code object of their own (csrc/pt_kernels_gather.hip, loaded at
 * the first call); the arithmetic is csrc/pt_gather.hpp, shared with the host.
 * THE DEFINING SENTENCE: item i of a call with D = directions is exactly what a caller gets who (1) makes the n * D rays below
 * on the host, ray j of item i at index i * D + j, (2) calls pt_query_radiance(ctx, rays, n * D, n_passes, rec) ONCE — the batch,
 * place, pass and seed rules above apply unchanged to those indices — and (3) reduces rec[i * D .. i * D + D) by the statement
 * list below.  What pt_query_radiance leaves alone these calls leave alone; PtStats moves exactly as that one call moves it.
 * D is a multiple of 64 in [64, 4096], and n * D is at most 2^32 - 1.
 * THE DIRECTION SET, the same for every item; fp32, one IEEE operation per statement, `/` and sqrt correctly rounded, for j < D:
 *   a = float(2 j + 1) / float(D)
 *   u = float(((j * 0x9E3779B97F4A7C15) mod 2^64) >> 40) * 2^-24      (frac(j * 0.61803398875) cut to 24 bits, in integers:
 *                                                            the constant is 2^64 / the golden ratio, j * 0.618... to 2^-52)
 *   (s, c) = sincos2pi(u)                                    (sin and cos of 2 pi u: the arithmetic contract's)
 * pt_bake_probes — the sphere, +y the stratified axis (the axis the sky varies along); `normal` is not read:
 *   y = 1 - a;  r2 = fma(-y, y, 1);  r = sqrt(r2);  omega = (r * c, y, r * s)
 * pt_gather_irradiance — the hemisphere about the normal, cosine-weighted:
 *   h = a * 0.5;  sh = sqrt(h);  lx = sh * c;  ly = sh * s;  m = 1 - h;  lz = sqrt(m)
 *   g = max(|n.x|, |n.y|, |n.z|);  p = n / g (per component);  d2 = fma(p.z, p.z, fma(p.y, p.y, p.x * p.x));  i = 1 / sqrt(d2);
 *   z = p * i                                                (the unit normal of ANY finite non-zero normal, however short or long)
 *   sg = copysign(1, z.z);  q = -1 / (sg + z.z);  b = (z.x * z.y) * q
 *   t = (fma(sg * (z.x * z.x), q, 1), sg * b, -sg * z.x);  bt = (b, fma(z.y * z.y, q, sg), -z.y)     (csrc/pt_nee.hpp's frame)
 *   omega.k = fma(z.k, lz, fma(bt.k, ly, t.k * lx))
 * The ray is {position, omega}; nothing is offset (t_min = 0.001 along a unit direction is the bounce ray's own guard).
 * THE REDUCTION of an item's records r_j = rec[i * D + j], and ITS ORDER, which is part of the contract: 64 lanes; lane l starts
 * from accumulators of +0 and takes j = l, l + 64, l + 128, ... in ascending order:
 *   mean.c = r_j.sum.c / r_j.samples
 *   irradiance: acc.c = acc.c + mean.c                 probe: acc[k].c = fma(mean.c, Y_k(omega_j), acc[k].c), k = 0 .. 8
 *   acc.samples = acc.samples + r_j.samples
 * then the tree: for o = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l xor o] for every lane at once, per accumulator; the item's sums
 * are v[0].  Neither the launch shape nor a batch boundary enters (an item that straddles batches carries its lanes' partial
 * sums from one to the next: the same adds in the same order), and no floating-point atomic is used.
 *   irradiance: e.c = v.c * (3.14159265f / float(D))          probe: sh[k].c = v[k].c * (12.5663706f / float(D))
 *   samples = v.samples                                       (D * n_passes * samples_per_pixel, exact below 2^24)
 * THE BASIS, with (x, y, z) = omega, in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2):
 *   Y0 = 0.282095f;  Y1 = 0.488603f * y;  Y2 = 0.488603f * z;  Y3 = 0.488603f * x;  Y4 = 1.092548f * (x * y);
 *   Y5 = 1.092548f * (y * z);  Y6 = 0.315392f * fma(3, z * z, -1);  Y7 = 1.092548f * (x * z);  Y8 = 0.546274f * fma(x, x, -(y * y))
 * INVALID ITEMS: an item with a non-finite position component — for pt_gather_irradiance also with a non-finite normal
 * component or a normal of three zeros — is invalid.  That is decided on the device; its D rays are null rays (invalid rays of
 * pt_query_radiance: nothing is traced, PtStats.segments does not move), and its record is all +0: samples == 0 is the mark.
 * `points` / `probes` and `out` are host or device pointers (n of each), as pt_query_radiance takes them; the pads are not read.
 * The calls are synchronous on the context's stream; n == 0 is PT_OK with nothing done.  Per batch of pt_query_batch(ctx) rays:
 * the generator, pt_query_radiance's launch and fold, the reduce.  The first call puts a small buffer of the context's in place
 * (the lanes' carried sums and the staging of a batch's items: 14 336 + 144 * (pt_query_batch / 64 + 2) bytes), kept until
 * PT_OPT_RAY_QUERIES is turned off.
 * ERRORS: pt_query_radiance's, checked in its order, then `directions`: PT_ERR_INVALID for a D outside the set above or
 * n * D beyond 2^32 - 1.  PT_ERR_CAPACITY also where that buffer's allocation is refused (nothing is launched). */
typedef struct PtGatherPoint {
  float position[3];
  float _pad0;
  float normal[3];
  float _pad1;
} PtGatherPoint; /* 32 bytes */
typedef struct PtIrradiance {
  float e[3];
  float samples;
} PtIrradiance; /* 16 bytes */
typedef struct PtProbeSH {
  float sh[9][3];
  float samples;
} PtProbeSH; /* 112 bytes */
int pt_gather_irradiance(pt_ctx* ctx, const PtGatherPoint* points, uint32_t n, uint32_t directions, uint32_t n_passes, PtIrradiance* out);
int pt_bake_probes(pt_ctx* ctx, const PtGatherPoint* probes, uint32_t n, uint32_t directions, uint32_t n_passes, PtProbeSH* out);

/* ---- the same three calls by the NEXT-EVENT estimator (need PT_OPT_RAY_QUERIES and PT_OPT_NEXT_EVENT on; no option of their own) ----
 * pt_query_radiance, pt_gather_irradiance and pt_bake_probes stay the plain estimator whatever the options say: they find the
 * lamp of a closed room by chance only.  These three take the same arguments and walk the same rays by the estimator of
 * PT_OPT_NEXT_EVENT: the same expectation per record, different samples, far less noise where a lamp is small.  The kernels are a
 * code object of their own (csrc/pt_kernels_radiance_nee.hip: the radiance builds with the next-event shade, loaded at the first
 * of these calls).
 * pt_query_radiance_nee, THE RECORD of ray i:
 *   - the batch b, the place j, the pixel centre (vx, vy) and the seed of pt_query_radiance's statement list: the seed of pass p
 *     depends on first_pass + b * n_passes + p; NO jitter draw and NO lens draws are made;
 *   - from that seed, samples_per_pixel CHAINED paths (the seed is carried from sample to sample) of the PT_OPT_NEXT_EVENT
 *     estimator exactly as stated at the option above and in csrc/pt_nee.hpp, along the caller's ray;
 *   - the caller's ray is a path's FIRST segment: no light sample precedes it, so an emissive sphere it hits adds its emission;
 *   - from the first DIFFUSE hit on, the option's rules hold: the draw order (steps 1 to 4), the shadow segment (10 to 12), and
 *     nothing added for a light that could have been sampled from the segment's origin (NO DOUBLE COUNTING);
 *   - a sample's terms are added to the PASS's running sum s in the order they arise — s is carried across the samples of a
 *     pass, as a render launch's per-item sum receives them (not c = ray_color(...); s = s + c);
 *   - out.sum.c = out.sum.c + s.c per pass, in pass order;  out.samples = out.samples + float(samples_per_pixel).
 * Records, the samples == 0 mark of an invalid ray, the batch size (pt_query_batch) and the host or device pointers are
 * pt_query_radiance's.  PtStats.segments moves by the path segments PLUS the shadow segments, as a next-event render launch
 * counts them.  Everything pt_query_radiance leaves alone stays alone (the accumulation, the estimate, the feature and history
 * planes, first_pass, pt_last_trace_build, the geometry path, the tile orders).  With no light in the scene (L == 0) the records
 * are pt_query_radiance's, bit for bit.
 * pt_gather_irradiance_nee / pt_bake_probes_nee, THE DEFINING SENTENCE: item i is exactly what a caller gets who makes the n * D
 * rays of the direction set above, calls pt_query_radiance_nee(ctx, rays, n * D, n_passes, rec) ONCE and reduces by the
 * statement list above: the generator, the reduce and the workspace are pt_gather_irradiance's.  NO light sample is drawn AT
 * the gather point itself: its D rays are first segments.
 * ERRORS: the namesake's, in the namesake's order and words (for the gather calls through `directions`); then PT_ERR_NOT_READY
 * while PT_OPT_NEXT_EVENT is off, and PT_ERR_CAPACITY where its light table is not in place after a failed allocation. */
int pt_query_radiance_nee(pt_ctx* ctx, const PtRay* rays, uint32_t n, uint32_t n_passes, PtRayRadiance* out);
int pt_gather_irradiance_nee(pt_ctx* ctx, const PtGatherPoint* points, uint32_t n, uint32_t directions, uint32_t n_passes, PtIrradiance* out);
int pt_bake_probes_nee(pt_ctx* ctx, const PtGatherPoint* probes, uint32_t n, uint32_t directions, uint32_t n_passes, PtProbeSH* out);

/* ---- probe lattices: bake a regular lattice of SH probes, shade the feature planes from it (no option of their own) ----
 * pt_bake_probes ends at the host; these two keep the chain on the device.  pt_bake_lattice makes the points of a regular
 * lattice on the device and bakes them (needs PT_OPT_RAY_QUERIES, and PT_OPT_NEXT_EVENT for estimator 1); pt_shade_probes
 * blends the eight records around every first hit of the feature planes into a linear RGBA frame (needs PT_OPT_FEATURES and
 * a pt_render_features of the view): one feature launch plus one streaming kernel give a noise-free picture of the diffuse
 * light transport at any camera.  The kernels are a code object of their own (csrc/pt_kernels_probe.hip, loaded at the first
 * of these calls); the arithmetic is csrc/pt_probe.hpp, shared with the host.
 * THE LATTICE: nx, ny, nz lie in [2, 256] and nx * ny * nz is at most 2^20; every step is finite and > 0; every origin
 * component is finite; flags holds PT_LATTICE_SKIP_BURIED or nothing.  Anything else is PT_ERR_INVALID.
 *   node i = (iz * ny + iy) * nx + ix
 *   position.c = fma(float(i_c), step.c, origin.c)
 * PT_LATTICE_SKIP_BURIED (off by default: a scene inside a dome sphere is legitimately inside a sphere): a node is BURIED if
 * for some sphere of the installed list with type != PT_GLASS
 *   w = position - centre;  d2 = fma(w.z, w.z, fma(w.y, w.y, w.x * w.x));  d2 < r * r
 * with r * r the bits the kernels intersect.  The comparison is strict (a node on the surface is not buried), and
 * a NaN centre never buries.  A buried node's position is written as NaN: by pt_bake_probes' own rule it is an invalid item,
 * nothing is traced for it and its record is all +0 with samples == 0.
 * pt_bake_lattice, THE DEFINING SENTENCE: out[k] is, bit for bit, item k of pt_bake_probes (estimator == 0) or
 * pt_bake_probes_nee (estimator == 1) called ONCE on the `count` points made above for nodes first .. first + count - 1.
 * AN ITEM'S INDEX, AND WITH IT ITS SEEDS, IS ITS INDEX IN THE CALL, NOT IN THE LATTICE:
 * a sliced bake draws other samples than a whole one.  Errors (after the lattice's own), batches, PtStats and everything left alone are that call's.  first + count
 * beyond nx * ny * nz, or an estimator other than 0 and 1: PT_ERR_INVALID; count == 0: PT_OK with nothing done.  `out` is a
 * host or device pointer, as pt_bake_probes takes it.  The points are made by a generator kernel into a buffer of the
 * context's (32 bytes per node of the slice, kept until PT_OPT_RAY_QUERIES is turned off; a refused allocation is
 * PT_ERR_CAPACITY and nothing is launched).
 * pt_shade_probes: `probes` are the records of all nx * ny * nz nodes in node order, on the host or the device; `rgba_out`
 * holds local_rows * width linear RGBA fp32 texels on the host or the device, row 0 the lowest owned row — the layout
 * pt_read_features uses and pt_meter, pt_glare and pt_resolve_toned accept as `src`.  options NULL: flags =
 * PT_PROBE_HALFSPACE, normal_bias 0.  It needs valid feature planes, by pt_read_features' rule and errors (PT_ERR_NOT_READY
 * while PT_OPT_FEATURES is off or the planes are stale; PT_ERR_INVALID under PT_OPT_COUNT_WORK or inside a capture), and it
 * moves nothing of the context: not the accumulation, PtStats, first_pass, pt_last_trace_build or the planes.  A band that
 * owns no rows: PT_OK.  Host records are staged in a buffer of the context's (112 bytes per node, kept until PT_OPT_FEATURES
 * is turned off; a refused allocation is PT_ERR_CAPACITY and nothing is launched).  Synchronous where `probes` or `rgba_out`
 * is a host pointer, asynchronous on the context's stream otherwise.
 * PER PIXEL, fp32, one IEEE operation per statement; dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), unit() is the
 * gather section's unit normal (g, p, d2, i, z) and Y_j its basis; albedo, n, hp and ids are the feature planes' texels:
 *   miss (ids.x < 0): {albedo-plane rgb, 1} — the background the path tracer returns
 *   PT_EMISSIVE: {albedo, 1}
 *   a type outside the four: {0, 0, 0, 1} — it absorbs
 *   otherwise the look-up point and direction:
 *   q.c = fma(normal_bias, n.c, hp.c)
 *   g.c = (q.c - origin.c) / step.c
 *   i.c = clamp(int(floor(g.c)), 0, n_c - 2)                 (outside the lattice the border cell answers; a NaN takes cell 0)
 *   f.c = min(max(g.c - float(i.c), 0), 1)
 *   DIFFUSE: omega = n; b = (3.14159265f, 2.09439510f x3, 0.785398163f x5)              (pi, 2 pi / 3, pi / 4)
 *   METAL: v.c = hp.c - camera_origin.c; d = dot(v, n); k = 2 * d; m.c = k * n.c; r.c = v.c - m.c; omega = unit(r); b = 1
 *   GLASS: omega = unit(v); b = 1                            (fuzz and refraction do not enter)
 *   B_j = b_j * Y_j(omega)
 *   corners k = 0 .. 7 in ascending order (bit 0 = x, bit 1 = y, bit 2 = z): wx = bit ? f.x : 1 - f.x, likewise wy, wz;
 *   w_k = (wx * wy) * wz
 *   a corner is KEPT iff w_k > 0, its record has samples > 0 and, under PT_PROBE_HALFSPACE, dot(pos_k - hp, n) > 0 (this
 *   drops probes at or behind the tangent plane, every probe inside the convex ball the pixel lies on among them); then
 *   E_k.c = fma(B_8, sh[8].c, ... fma(B_0, sh[0].c, +0))     (j ascending)
 *   W = W + w_k
 *   S.c = fma(w_k, E_k.c, S.c)
 *   W > 0: v.c = max(S.c / W, 0); DIFFUSE: out.c = albedo.c * (v.c * 0.318309886f); METAL: out.c = albedo.c * v.c;
 *          GLASS: out.c = v.c; alpha 1
 *   W == 0: {0, 0, 0, 0} — alpha 0 is the mark of "no usable probe"
 * OUT OF SCOPE: visibility-weighted or octahedral-depth probes (light leaks through thin walls); specular chains behind METAL
 * and GLASS (one look-up along the mirror or the view direction stands for them); probes that follow a moving scene (bake
 * again); a FrameLoop mode (the calls compose with it from outside); multi-rank baking beyond the first / count slice. */
#define PT_LATTICE_SKIP_BURIED 1u
#define PT_PROBE_HALFSPACE 1u
typedef struct PtProbeLattice {
  float origin[3];
  uint32_t nx;
  float step[3];
  uint32_t ny;
  uint32_t nz;
  uint32_t flags; /* PT_LATTICE_SKIP_BURIED */
  uint32_t _pad[2];
} PtProbeLattice; /* 48 bytes */
typedef struct PtProbeShadeOptions {
  uint32_t flags; /* PT_PROBE_HALFSPACE */
  float normal_bias;
  uint32_t _pad[2];
} PtProbeShadeOptions; /* 16 bytes */
int pt_bake_lattice(pt_ctx* ctx, const PtProbeLattice* lattice, uint32_t first, uint32_t count, uint32_t directions, uint32_t n_passes,
                    int estimator, PtProbeSH* out);
int pt_shade_probes(pt_ctx* ctx, const PtProbeLattice* lattice, const PtProbeSH* probes, const PtProbeShadeOptions* options, float* rgba_out);

/* ---- exposure metering and tone-mapped read-out (build extension, opt-in: PT_OPT_TONEMAP) --------------------------------------
 * Every other read-out ends in sqrt and a clamp at 1: the reference's framebuffer.  A frame lit by PT_EMISSIVE spheres holds far
 * more range than that; these calls meter the frame on the device, keep an EXPOSURE there and read the frame out through a tone
 * curve.  No existing read-out changes.  The kernels are a code object of their own (loaded when the option is turned on, or at
 * the first toned read-out with an explicit exposure); the arithmetic is csrc/pt_tone.hpp, shared with pt_exposure_solve.
 * THE OPTION puts one fixed-size device buffer in place: 256 + 2 uint32 tallies and one PtExposure record.  The record is VALID
 * once it was metered or set since the option came on.  An exposure is the viewer's adaptation, not a product of the scene: it
 * survives pt_set_spheres, pt_set_params, pt_resize and pt_reset_accum and ends only when the option is turned off.
 * THE SOURCE IMAGE, `src`: NULL is the context's accumulation, per pixel x.c = v.c * scale with scale = v.w > 0 ? 1 / v.w : 0 —
 * pt_resolve with gamma = 0, bit for bit.  Otherwise a host or device pointer to local_rows*width linear RGBA fp32 texels (what
 * pt_resolve_filtered_patch(..., gamma = 0) wrote, for instance): x = src.rgb, its .a is not read.  A device src is read in place;
 * a host src is copied into the pass slabs first (free between calls, as pt_query_radiance uses them).
 * pt_meter: asynchronous on the context's stream, no allocation, and no synchronisation for a NULL or device src (a call with a
 * host src synchronises).  Two kernels behind a clear of the tallies.
 * KERNEL 1, per local pixel inside the window, fp32, ONE IEEE operation per statement, nothing fused:
 *     Y = 0.2126f*x.r ;  t = 0.7152f*x.g ;  Y = Y + t ;  t = 0.0722f*x.b ;  Y = Y + t
 *     if !(Y >= 2^-16): below += 1                     (zero, negative, NaN, subnormal, too dark)
 *     else: k = (bits(Y) >> 20) - 888 ;  if k > 255: k = 255 ;  hist[k] += 1
 * 888 is bits(2^-16) >> 20: the 256 bins are eight per octave over [2^-16, 2^16), everything at or above 2^16, +inf included,
 * lands in bin 255, and the lower edge of bin k is the float whose bits are (k + 888) << 20.  The counts are integers, summed per
 * workgroup in the LDS and added with integer atomics: exact in any order.
 * THE WINDOW {x0, y0, w, h} is in IMAGE coordinates, row 0 at the bottom; w == 0 or h == 0 means the whole frame.  Local pixel
 * (px, ly) is metered when x0 <= px < x0 + w and its image row y = pt_band_row(band_rows, band_index, band_count, ly) lies in
 * [y0, y0 + h); the sums cannot wrap: a window that reaches past the frame ends at the frame.  A band context meters its rows.
 * KERNEL 2, one workgroup, from the tallies and the record before (`/` correctly rounded; N, rank and the cumulative counts uint64):
 *     N = sum hist
 *     if N == 0: the record keeps exposure, white, y_key and y_high (1, white_min, 0, 0 when it was never valid);
 *                lit = 0, below is stored, meterings += 1; done
 *     rank(p) = min(N - 1, (N * p) / 1000)
 *     bin(p)  = the smallest k whose cumulative count exceeds rank(p)
 *     y_key = edge(bin(key_permille)) ;  y_high = edge(bin(high_permille))
 *     e_t = key / y_key
 *     if (e_t < e_min) e_t = e_min ;  if (e_t > e_max) e_t = e_max
 *     if the record was valid and rate < 1:
 *         if !(rate > 0): e = e_prev
 *         else: d = e_t - e_prev ;  d = d * rate ;  e = e_prev + d
 *     else: e = e_t
 *     white = y_high * e ;  if !(white >= white_min) white = white_min
 *     record = {exposure e, white, y_key, y_high, lit = N, below, meterings + 1}
 * pt_meter: PT_ERR_INVALID for a NULL ctx or options, a key, e_min, e_max or white_min that is not finite and positive,
 * e_min > e_max, a permille above 1000, key_permille > high_permille, a rate that is NaN; then PT_ERR_NOT_READY while the option
 * is off; then PT_ERR_INVALID inside a stream capture; then, for src == NULL, what pt_resolve would answer (PT_ERR_NOT_READY
 * before anything was rendered), and PT_ERR_CAPACITY while the buffers are not in place.
 * pt_meter_read: synchronises; the record and the tallies of the last metering (all zero while a pt_meter_set is all there was);
 * either out pointer may be NULL.  PT_ERR_NOT_READY while the option is off or the record is not valid.
 * pt_meter_set: loads a record as it is (meterings included) and makes the state valid; exposure and white must be finite and
 * positive (PT_ERR_INVALID); PT_ERR_NOT_READY while the option is off; synchronises, not inside a stream capture.
 * pt_exposure_solve: kernel 2's statements on the host, no device and no context: the same header, the same bits.  The window of
 * `options` is not read; prev NULL means "never valid".  PT_ERR_INVALID for a NULL hist256, options or out and for the option
 * values pt_meter refuses.  It is what makes an N-rank frame equal the single-GPU one: the ranks add their histograms and their
 * `below` (integers, any order), each solves with the same prev, each calls pt_meter_set.
 * THE TONED READ-OUTS follow pt_resolve: rgba_out is a host or device pointer to local_rows*width texels, the call synchronises.
 * PtToneOptions.exposure == 0 reads exposure and white from the device record, with no host round trip — a pt_meter enqueued just
 * before is enough — and answers PT_ERR_NOT_READY while the option is off or the record is not valid.  exposure > 0 (finite) uses
 * the caller's exposure and white and needs neither record nor option.  Per channel, fp32, one operation per statement:
 *     x = x * e
 *     PT_TONE_CLAMP     y = x
 *     PT_TONE_REINHARD  w2 = white*white  (once)
 *                       a = x / w2 ;  a = a + 1 ;  n = x * a ;  d = x + 1 ;  y = n / d
 *     PT_TONE_FILMIC    a = 2.51f*x ;  a = a + 0.03f ;  n = x * a ;
 *                       b = 2.43f*x ;  b = b + 0.59f ;  d = x * b ;  d = d + 0.14f ;  y = n / d
 *     gamma != 0:       y = sqrtf(y)
 * The float form writes {y.rgb, 1}; the byte form writes unorm8(y) with alpha 255, unorm8 as pt_resolve_rgba8 has it
 * (!(y > 0) -> 0; y >= 1 -> 255; else truncate (y * 255 + 0.5), two statements).  Non-finite and negative operands go through the
 * statements as they are.  PT_TONE_CLAMP with exposure 1 IS pt_resolve / pt_resolve_rgba8, bit for bit.
 * PT_ERR_INVALID: NULL ctx, options or rgba_out, a curve that is none of the three, an exposure that is neither 0 nor finite and
 * positive, PT_TONE_REINHARD with a caller's white that is not above 0 (+inf is allowed: plain x / (1 + x)); then, for
 * exposure == 0, PT_ERR_NOT_READY as above; then PT_ERR_INVALID inside a stream capture; then, for src == NULL, what pt_resolve
 * would answer.
 * WHAT THESE CALLS LEAVE ALONE is what pt_resolve leaves alone: the accumulation, the estimate, the planes and their validity, the
 * textures and the canvas, first_pass, the tile order, PtStats and pt_last_trace_build. */
enum { PT_TONE_CLAMP = 0, PT_TONE_REINHARD = 1, PT_TONE_FILMIC = 2 };
typedef struct PtMeterOptions {
  float key;              /* the luminance the key percentile is exposed to          default 0.18  */
  uint32_t key_permille;  /* the percentile of the lit pixels that is the key        default 500   */
  uint32_t high_permille; /* ... and the one that becomes `white`                    default 990   */
  float e_min, e_max;     /* the range of the exposure                               default 2^-8, 2^8 */
  float white_min;        /* the least `white`                                       default 1     */
  float rate;             /* the share of the way to the target one metering goes    default 1     */
  uint32_t x0, y0, w, h;  /* the window, image coordinates; w == 0 or h == 0: the whole frame */
  uint32_t _pad;
} PtMeterOptions; /* 48 bytes */
#define PT_METER_OPTIONS_DEFAULT {0.18f, 500u, 990u, 0.00390625f, 256.0f, 1.0f, 1.0f, 0u, 0u, 0u, 0u, 0u}
typedef struct PtExposure {
  float exposure, white; /* what the toned read-outs multiply by, and Reinhard's white point (exposed luminance) */
  float y_key, y_high;   /* the lower edges of the bins the two percentiles fell in (linear luminance)          */
  uint64_t lit;          /* N: the metered pixels that fell in a bin                                            */
  uint32_t below;        /* ... and those that did not                                                          */
  uint32_t meterings;    /* meterings since the record became valid                                             */
} PtExposure; /* 32 bytes */
typedef struct PtToneOptions {
  int32_t curve;  /* PT_TONE_*                                             */
  int32_t gamma;  /* != 0: the square root after the curve                 */
  float exposure; /* 0: the device record's exposure and white; > 0: these */
  float white;
} PtToneOptions; /* 16 bytes */
int pt_meter(pt_ctx* ctx, const float* src, const PtMeterOptions* options);
int pt_meter_read(pt_ctx* ctx, PtExposure* out, uint32_t hist256[256]);
int pt_meter_set(pt_ctx* ctx, const PtExposure* record);
int pt_exposure_solve(const uint32_t hist256[256], uint32_t below, const PtMeterOptions* options, const PtExposure* prev_or_NULL,
                      PtExposure* out);
int pt_resolve_toned(pt_ctx* ctx, const float* src, const PtToneOptions* options, float* rgba_out);
int pt_resolve_toned_rgba8(pt_ctx* ctx, const float* src, const PtToneOptions* options, uint8_t* rgba_out);

/* ---- glare: an energy-conserving bloom pyramid ahead of the toned read-out (build extension, opt-in: PT_OPT_GLARE) -------------
 * After any tone curve a light is a flat disc at the byte 255; what says "this is fifteen times brighter than the wall" on a
 * display is the veil a lens or an eye puts around it.  pt_glare spreads a share of the frame's light over a pyramid of levels
 * and adds it back: accumulation -> [filter] -> GLARE -> meter -> tone.  It touches no existing read-out and composes through
 * `src`, as pt_meter and pt_resolve_toned do.  Three kernels in a code object of their own (loaded when the option is turned on);
 * the arithmetic is csrc/pt_glare.hpp, shared with the CPU checks.
 * THE OPTION puts one float4 buffer in place, the pyramid: levels 1 .. PT_GLARE_MAX_LEVELS of the local frame, refitted by
 * pt_resize and by a repartition.  It is scratch: nothing in it outlives a call, it has no validity.
 * `src` and `rgba_out` are pt_resolve_toned's: src NULL is the accumulation (x.c = v.c * scale, scale = v.w > 0 ? 1 / v.w : 0),
 * otherwise width*local_rows linear RGBA fp32 texels on the host or the device (.a not read; a host src is copied into the pass
 * slabs first); rgba_out is a host or device pointer and may equal a device src; the call synchronises.  The output is LINEAR
 * radiance {r, g, b, 1}: what pt_meter(ctx, out, ...) and pt_resolve_toned(ctx, out, ...) take next.
 * THE STATEMENTS, fp32, ONE IEEE operation per statement, nothing fused.  (w_0, h_0) is the frame, w_k = (w_{k-1} + 1) / 2,
 * h_k likewise; weight[k] below is the weight of level k, PtGlareOptions.weight[k - 1].  Per channel c:
 *   bright, per pixel:   x = source colour ;  Y = luminance(x)           (pt_meter's five statements)
 *                        if !(Y - Y == 0):         b.c = 0               (NaN or infinite: one bad pixel must not veil the frame)
 *                        else if threshold == 0:   b.c = x.c
 *                        else: t = Y - threshold ; if !(t > 0) b.c = 0 else { m = t / Y ;  b.c = x.c * m }
 *   down, D_0 = b, D_k from D_{k-1}, k = 1 .. levels.  First along x, then along y; the x pass's result is rounded to fp32:
 *                        taps t0..t3 at 2X-1, 2X, 2X+1, 2X+2, each index clamped to [0, w_{k-1} - 1]
 *                        o = t0 + t3 ;  i = t1 + t2 ;  i = 3 * i ;  s = o + i ;  v = s * 0.125
 *   up(A) to a (w, h) level from a (W, H) level.  First along x, then along y:
 *                        p = X >> 1 ;  q = (X odd) ? p + 1 : p - 1 ;  both clamped to [0, W - 1]
 *                        t = 3 * A[p] ;  t = t + A[q] ;  v = t * 0.25
 *   gather:              U_levels = weight[levels] * D_levels
 *                        k = levels - 1 .. 1:  a = weight[k] * D_k ;  U_k = a + up(U_{k+1})
 *   composite, per pixel: G = up(U_1) at frame size ;  d = G.c - b.c ;  d = d * strength ;  out.c = x.c + d ;  out.w = 1
 * down's taps are 1 3 3 1 over 8 and up's 3 1 over 4: both sum to one and both are exact on a constant, so with weights that add up
 * to 1 the glare CONSERVES ENERGY — a constant frame comes back bit for bit, and what the veil gains the light's own pixels
 * lose (d is negative there).  The bits do not depend on how the kernels tile a level.
 * REFUSALS, in this order: PT_ERR_INVALID for a NULL ctx, options or rgba_out, a strength that is not finite or outside [0, 1], a
 * threshold that is not finite or negative, levels outside 1 .. PT_GLARE_MAX_LEVELS, a weight of a used level that is not finite or
 * negative (the weights past `levels` are not read); PT_ERR_NOT_READY while the option is off; PT_ERR_INVALID on a band context
 * (a row partition of more than one rank: its rows are interleaved and its neighbours live on other ranks — an N-rank frame is
 * glared after the gather, on a context of the whole frame, through a non-NULL src); PT_ERR_INVALID inside a stream capture;
 * for src == NULL what pt_resolve would answer; PT_ERR_CAPACITY while the pyramid is not in place.  A context without rows
 * launches nothing.
 * WHAT THE CALL LEAVES ALONE is what pt_resolve_toned leaves alone, and the exposure record. */
#define PT_GLARE_MAX_LEVELS 8
typedef struct PtGlareOptions {
  float strength;    /* share of the spread light that is added back, finite, 0 .. 1          */
  float threshold;   /* linear luminance above which a pixel spills; 0: every pixel, whole    */
  uint32_t levels;   /* 1 .. PT_GLARE_MAX_LEVELS                                              */
  uint32_t _pad;
  float weight[PT_GLARE_MAX_LEVELS]; /* weight of level 1 .. levels; used as they are; each finite and >= 0;
                                        the glare conserves energy when they add up to 1      */
} PtGlareOptions; /* 48 bytes */
#define PT_GLARE_OPTIONS_DEFAULT {0.15f, 0.0f, 6u, 0u, {0.35f, 0.25f, 0.18f, 0.12f, 0.06f, 0.04f, 0.0f, 0.0f}}
int pt_glare(pt_ctx* ctx, const float* src, const PtGlareOptions* options, float* rgba_out);

/* ---- temporal blend of the reference, static/shader.frag:387-404 + src/webgl.rs:186-204 --------
 * Blends the current resolved, gamma-encoded frame with `prev_rgba8` (the ping-pong texture)
 * using params.render_count / should_average / last_frame_weight, writes RGBA8 to `out_rgba8`.
 * Both are device or host pointers to local_rows*width*4 bytes. */
int pt_blend_rgba8(pt_ctx* ctx, const uint8_t* prev_rgba8, uint8_t* out_rgba8);

/* ---- the reference's FRAME on device-resident textures: webgl::render (src/webgl.rs:180-205) ------
 * The context owns the two RGBA8 ping-pong textures of src/webgl.rs:82-123 (local_rows*width texels
 * each, cleared to 0: alpha 0 = "no data", static/shader.frag:391) and a canvas, all in HBM.
 * pt_render_frame is ONE animation tick of src/lib.rs:92-102 with the current uniforms: trace one
 * pass (samples_per_pixel samples at u_time = time + float(first_pass) * time_step), blend it with
 * texture[(even_odd_count + 1) % 2] by the shader's render() rule using params.render_count /
 * should_average / last_frame_weight, draw the result to the canvas and, when should_average, to
 * texture[even_odd_count % 2].  Asynchronous on the context's stream; nothing crosses PCIe.
 * Neither frame call advances params.first_pass or touches the accumulation; their segments count in PtStats.segments.
 * pt_render_frames replays n_frames ticks at a constant frame interval from captured hipGraphs —
 * groups of 64 (while their slabs stay below 1 GiB), 16 and 4 frames (ONE trace launch renders a group's frames as its passes into slabs of
 * their own, allocated by the first call that needs them; their blends follow in order; advance) and
 * single frames for the remainder (trace + blend + advance) — with the per-frame
 * state of State::update_render_globals (src/state.rs:443-450) kept on the device: frame k of the
 * call renders at u_time = time + float(first_pass + k) * time_step with
 * render_count = min(params.render_count + k, max_render_count) and even_odd_count + k — the bits
 * of n_frames pt_render_frame calls made with those uniforms (u_time is fp32(time) + float(k) * fp32(time_step),
 * computed in fp32 on the device: it equals fp32(time + k * time_step) rounded from the host's f64 — what a tick-by-tick
 * host uploads — for every k only when time, time_step and their products are exact in fp32, e.g. whole or half
 * milliseconds; otherwise some frames get a neighbouring seed: equally valid samples, not the same bits).  That equals n_frames ticks of the
 * reference's loop only while nothing but the clock changes between them: with should_average off
 * just the first tick draws (update_render_globals clears should_render, src/state.rs:443-447), with a
 * movement key held every tick has its own camera — issue such ticks one by one (pt_render_frame).
 * The graph is re-captured only when something it bakes in has changed (uniforms, scene size, launch
 * shape, stream).  NOT on a context bound to the legacy default stream (PT_STREAM_LEGACY): HIP does not
 * capture that stream, the call returns PT_ERR_INVALID there.  The accumulation buffer of
 * pt_render / pt_resolve is not involved.  pt_read_canvas / pt_read_texture copy RGBA8 texels out
 * (host or device pointer; they synchronise), pt_write_texture copies a texture in. */
int pt_clear_textures(pt_ctx* ctx);
int pt_render_frame(pt_ctx* ctx, uint32_t even_odd_count);
int pt_render_frames(pt_ctx* ctx, uint32_t even_odd_count, uint32_t max_render_count, uint32_t n_frames);
int pt_read_canvas(pt_ctx* ctx, uint8_t* rgba_out);
int pt_read_texture(pt_ctx* ctx, int index, uint8_t* rgba_out);
int pt_write_texture(pt_ctx* ctx, int index, const uint8_t* rgba_in);

/* ---- diagnostics ------------------------------------------------------------------------------ */
int pt_get_stats(pt_ctx* ctx, PtStats* out);
int pt_set_option(pt_ctx* ctx, int key, int value);
/* The shader's DEBUG OVERLAY (static/shader.frag:307-318; uniforms u_enable_debugging, u_selected_object, u_cursor_point
 * :100-102, uploaded every frame by src/webgl.rs:554-587).  With enable != 0 every hit is tested right after its hit record
 * is complete — before the PT_EMISSIVE test and before any scatter draw:
 *   cursor dot   sqrt(dot(v, v)) < 0.1 with v = hit_point - cursor_point  ->  the sample's value is (0, 0, 1)
 *   outline      otherwise, PtSphere.uuid == selected_object && dot(normal, direction) > -0.05  ->  (1, 0, 0)
 * (face-forward normal, unnormalised direction; the value is the shader's `return`: not multiplied by the path's
 * throughput, also when the hit is seen through a mirror) and the path ends; the segment is counted in PtStats.segments.
 * selected_object is compared as it is: the reference's "nothing selected" is 1000 (NO_SELECTED_OBJECT_ID, src/state.rs:12),
 * and a sphere whose uuid is that value is outlined, as in the shader.  Copies its arguments (cursor_point may be NULL with
 * enable == 0); takes effect from the next pt_render / pt_render_passes / pt_render_frame / pt_render_frames, whose graphs
 * are captured again when the values change, as for any uniform.  enable == 0 restores the kernels and the bits of a context
 * that never enabled it.  The overlay runs in builds of the trace kernels of its own (loaded at first use) and excludes
 * PT_OPT_RUSSIAN_ROULETTE and PT_OPT_COUNT_WORK.  Overlay and roulette: turning one on while the other is on returns
 * PT_ERR_INVALID and changes nothing.  PT_OPT_COUNT_WORK beside the overlay or beside roulette: the option calls succeed in either
 * order, and every render call (pt_render*, pt_tune's launches) returns PT_ERR_INVALID and enqueues nothing while both are on;
 * pt_render_frame(s), pt_render_adaptive and a pt_render_passes inside a stream capture return PT_ERR_INVALID under
 * PT_OPT_COUNT_WORK alone.  A context
 * set to PT_GEOM_LDS renders through the scalar walk meanwhile, as with roulette. */
int pt_set_debug_overlay(pt_ctx* ctx, int enable, int32_t selected_object, const float cursor_point[3]);
/* Which build of the trace kernel the most recent launch was: 0 plain, 1 Russian roulette, 2 measuring twin, 3 debug overlay,
 * 4 first-hit features (pt_render_features). */
int pt_last_trace_build(pt_ctx* ctx);
/* Fits the context to scene AND uniforms.  (i) The uniform grid pt_set_spheres built for rays that start within twice the
 * scene's radius of its middle is rebuilt for the margin class that renders THIS view fastest: the smallest class that
 * covers the camera set by pt_set_params is a lower bound (a camera outside it sends every primary ray down the far path), and
 * whether a class at or above it wins depends on where bounce rays start, so the candidates are measured — one timed launch of
 * a few passes each (as many as make ~4 ms, at most four and at most n_passes): the class the camera needs, the default class when that is smaller, and up to two classes wider while
 * the launch's far-ray tally says such rays matter and the wider class keeps winning; then, on scenes whose staged entries
 * take more than 16 KB of the LDS, the build that gathers its entries from L2 against the LDS-staged one (PtStats.grid_kernel_build)
 * (pt_set_option PT_OPT_GRID_FIT 1: no launches, the class the camera needs).  Speed only, the image does not depend on it; skipped once a launch has been captured
 * into a caller's hipGraph.  (ii) Settles PT_GEOM_AUTO now
 * instead of lazily: renders n_passes passes with the current scene
 * and uniforms once cold and once per usable path, keeps the fastest path.  Whenever it has launched anything it clears the
 * accumulation and statistics again.  Synchronous; a set-up call like pt_reserve_passes (which must have reserved n_passes).
 * Call it before capturing pt_render* into a hipGraph: a captured launch keeps the path it was
 * captured with (no measuring happens while a stream is capturing). */
int pt_tune(pt_ctx* ctx, uint32_t n_passes);
/* The frame loop's half of (i): rebuild the grid when the CURRENT camera has left the region it serves — for the smallest
 * margin class that covers the camera, never below the default class (3 scene radii: whether a tighter class pays is a
 * measurement, pt_tune's) — or, with only_if_stale == 0, also when the grid is looser than that.  Nothing else: no launches,
 * accumulation, textures and statistics untouched.  What a frame loop calls when PtStats.grid_fit_stale (or pt_grid_fit(ctx))
 * says so: the reference's camera moves every tick (State::update_position, src/state.rs:411-441), and a camera that has left
 * the region the grid was fitted to sends every primary ray down the far path.  Synchronises the stream when it rebuilds
 * (~2 ms of host work for 10 000 spheres); a no-op (PT_OK) when the grid fits, when there is none, when another geometry path
 * is forced or settled, and once a launch has been captured into a caller's hipGraph (its arguments hold the old grid's
 * numbers; pt_render_frames' own graphs are re-captured by themselves). */
int pt_refit_grid(pt_ctx* ctx, int only_if_stale);
/* PtStats.grid_fit_stale without the synchronisation pt_get_stats implies: 0 / 1 / 2 as there, < 0 on error.  Host arithmetic only. */
int pt_grid_fit(pt_ctx* ctx);
/* The hierarchy pt_set_spheres builds for PT_GEOM_BVH, on the host (no device needed; tests
 * check its invariants): nodes = 8 floats each {lo.xyz, bits(skip), hi.xyz, bits(first slot of
 * the leaf | 0xffffffff)}, slots = 4 floats each {cx, cy, cz, r*r}, slot_index = original sphere
 * index per slot (0xffffffff = padding), margin4 = {c0.xyz, s0}, counts5 = {n_nodes, n_slots,
 * n_tree_slots, n_outliers, depth}; nodes16 = the packed form the kernels read, 4 words per node
 * for n_nodes + 1 nodes {lo.x|lo.y, lo.z|hi.x, hi.y|hi.z as binary16 of (x - c0) * kscale rounded
 * outward, skip | leaf_number << 16}; nodes32 = the fp32 form small scenes use, 8 floats per
 * node for n_nodes + 1 nodes {lo - c0, bits(32 * skip), hi - c0, bits(leaf_number)}.  Array pointers
 * may be NULL (sizes only); capacities are in elements.  Returns PT_ERR_NOT_READY when the scene gets no hierarchy (fewer than 16
 * spheres, non-finite values), PT_ERR_CAPACITY when an array is too small. */
int pt_build_bvh(const PtSphere* spheres, uint32_t n, float* nodes, size_t node_floats, float* slots,
                 size_t slot_floats, uint32_t* slot_index, size_t n_index, float* margin4,
                 uint32_t* counts5, uint32_t* nodes16, size_t n_words16, float* kscale,
                 float* nodes32, size_t n_floats32);
/* The grid pt_set_spheres builds for PT_GEOM_GRID, on the host (no device needed; tests check the
 * registration invariant): dims9 = {n[3] as floats' bit patterns are NOT used: see counts}, i.e.
 * counts8 = {n.x, n.y, n.z, n_cell_entries, n_always, n_entries, max entries per cell, non-empty
 * cells}; geom12 = {lo.xyz, h.xyz, hi.xyz, c0.xyz}; margin4 = {s0, rmin, rmax, d_near};
 * delta_g = registration inflation; cells = n.x*n.y*n.z records (first entry | entries << 24),
 * entries = 4 floats each {cx, cy, cz, r*r}, entry_index = original sphere
 * index per entry (0xffffffff = padding).  Array pointers may be NULL (sizes only); capacities in
 * elements.  PT_ERR_NOT_READY when the scene gets no grid, PT_ERR_CAPACITY when an array is too small. */
int pt_build_grid(const PtSphere* spheres, uint32_t n, uint32_t* counts8, float* geom12, float* margin4,
                  float* delta_g, uint32_t* cells, size_t n_cells, float* entries, size_t entry_floats,
                  uint32_t* entry_index, size_t n_index);
/* What the grid kernels' entry test and cell look-up read beside geom12 / margin4 (tests emulate the
 * kernel's walk on the host with exactly these): out10 = {r2_near: rays with |o - c0|^2 <= it walk the
 * cells; lo_n.xyz, hi_n.xyz: the grid's box widened for the rounding of the slab test; inv_h.xyz}. */
int pt_grid_walk_constants(const PtSphere* spheres, uint32_t n, float* out10);
const char* pt_last_error(pt_ctx* ctx); /* ctx may be NULL: last create-time error */
int pt_abi_version(void);
int pt_device_count(void);
/* Device-side evaluation of single arithmetic building blocks (hash, sin/cos, cbrt, ...) for
 * parity tests; kinds are listed in ray_tracer_webgl_amd/csrc/pt_kernel_args.h.  in/out are
 * host pointers, n_in/n_out their lengths in floats, n the number of work items. */
int pt_probe(pt_ctx* ctx, int kind, const float* in, size_t n_in, float* out, size_t n_out,
             uint32_t n);
uint32_t pt_local_rows(uint32_t height, uint32_t band_rows, uint32_t band_index, uint32_t band_count);
/* The image row (0 = bottom) that local row `local_row` of band `band_index` is: rank r of n owns the rows y with
 * (y / band_rows) % n == r, in ascending order (PtParams.band_*).  What a host needs to put gathered per-rank buffers
 * back into image order (examples/render_bands.c): row l of rank r goes to image row
 * pt_band_row(band_rows, r, n, l), for l < pt_local_rows(height, band_rows, r, n).  Pure arithmetic, no device. */
uint32_t pt_band_row(uint32_t band_rows, uint32_t band_index, uint32_t band_count, uint32_t local_row);

/* ---- host-side camera derivation: State::update_pipeline (src/state.rs:319-347) ----------------
 * Double precision throughout, narrowed to float at the end like Vec3::to_array
 * (src/math.rs:107-109).  Fills the camera members + width/height + lens_radius of *out and
 * leaves the rest of *out untouched. */
int pt_camera_from_state(const PtCameraIn* in, PtParams* out);
int pt_camera_look_at(const PtLookAtIn* in, PtParams* out);

/* ---- host-side scene types: src/glsl.rs:27-40 ---------------------------------------------------
 * The reference keeps spheres in f64 on the host (Vec3 is 3 x f64, src/math.rs:17; radius f64;
 * fuzz / refraction_index f32) and narrows to f32 only at upload (src/webgl.rs:232-262). */
typedef struct PtHostSphere {
  double center[3];
  double radius;
  int32_t type;
  int32_t uuid;
  double albedo[3];
  float fuzz;
  float refraction_index;
} PtHostSphere;

/* The narrowing webgl::set_geometry performs (src/webgl.rs:225-274, Vec3::to_array
 * src/math.rs:107-109, `sphere.radius as f32`). */
int pt_narrow_spheres(const PtHostSphere* in, uint32_t n, PtSphere* out);
/* glsl::set_sphere_uuids (src/glsl.rs:84-88): uuid = index. */
int pt_set_sphere_uuids(PtHostSphere* spheres, uint32_t n);

/* ---- the reference's built-in scene: State::default sphere_list (src/state.rs:148-257) ---------
 * Writes up to cap spheres, returns the scene's sphere count (9). */
int pt_default_scene(PtHostSphere* out, uint32_t cap);
/* State::default camera block (src/state.rs:98-125) for a w*h canvas. */
int pt_default_camera(uint32_t width, uint32_t height, PtCameraIn* out);

/* ---- CPU pick ray: glsl::get_center_hit (src/glsl.rs:213-239) + Sphere::hit (:42-82), f64,
 * t_min = 0, t_max = inf.  Returns 1 on hit (fills t, hit point, normal, front_face, uuid),
 * 0 on miss, <0 on error. */
typedef struct PtCenterHit {
  double t;
  double hit_point[3];
  double normal[3];
  int32_t front_face;
  int32_t uuid;
} PtCenterHit;
int pt_center_hit(const PtHostSphere* spheres, uint32_t n, const PtCameraIn* cam,
                  PtCenterHit* out);

/* ---- the reference's State object (src/state.rs:31-94) behind an opaque handle -------------------
 * The caller side of the boundary: camera + render bookkeeping exactly as src/state.rs keeps
 * them (f64), so an interactive / turntable harness can drive the tracer the way src/lib.rs:65-104
 * drives WebGL.  Pure host code, no GPU needed. */
typedef struct pt_state pt_state;

typedef struct PtStateView {
  uint32_t width, height;
  uint32_t samples_per_pixel, max_depth;
  double aspect_ratio;
  double camera_origin[3], camera_front[3], vup[3];
  double yaw, pitch, camera_field_of_view;
  double u[3], v[3], w[3];
  double aperture, lens_radius, focus_distance;
  double viewport_height, viewport_width;
  double horizontal[3], vertical[3], lower_left_corner[3];
  double cursor_point[3];
  int32_t selected_object;
  int32_t is_paused, should_average, should_render;
  uint32_t even_odd_count, render_count, max_render_count;
  float last_frame_weight;
  uint32_t n_spheres;
} PtStateView;

int pt_state_create(pt_state** out, uint32_t width, uint32_t height); /* State::default :96-315 */
int pt_state_destroy(pt_state* s);
int pt_state_get(const pt_state* s, PtStateView* out);
int pt_state_set_fov(pt_state* s, double fov_radians);                 /* :349-352 */
int pt_state_set_camera_angles(pt_state* s, double yaw, double pitch); /* :354-358 */
int pt_state_set_camera_origin(pt_state* s, const double origin[3]);
int pt_state_set_lens(pt_state* s, double aperture, double focus_distance); /* lens_radius = aperture/2 */
int pt_state_set_quality(pt_state* s, uint32_t samples_per_pixel, uint32_t max_depth);
int pt_state_set_flags(pt_state* s, int is_paused, int should_average, float last_frame_weight);
/* KeydownMap :14-28 as a bit mask: 1 w, 2 a, 4 s, 8 d, 16 space, 32 shift */
int pt_state_set_keys(pt_state* s, uint32_t key_mask);
/* State.enable_debugging (src/state.rs:87), and the three overlay uniforms as run_setters uploads them (src/webgl.rs:554-587:
 * the cursor narrowed like Vec3::to_array) — what a frame loop hands to pt_set_debug_overlay every tick.  Out pointers may be NULL. */
int pt_state_set_debugging(pt_state* s, int enable);
int pt_state_debug_overlay(const pt_state* s, int32_t* enable, int32_t* selected_object, float cursor_point[3]);
int pt_state_update_position(pt_state* s, double dt_ms);      /* :411-441 (+ autofocus :453-471) */
int pt_state_update_render_globals(pt_state* s);              /* :443-450 */
int pt_state_resize(pt_state* s, uint32_t width, uint32_t height); /* :364-398, State half */
int pt_state_should_render(const pt_state* s, int should_save);    /* src/lib.rs:77-82 */
int pt_state_set_spheres(pt_state* s, const PtHostSphere* spheres, uint32_t n); /* uuids reassigned */
int pt_state_spheres(const pt_state* s, PtSphere* out, uint32_t cap);  /* set_geometry narrowing */
int pt_state_to_params(const pt_state* s, double now_ms, PtParams* out); /* run_setters :279-593 */
/* dom::get_adjusted_screen_dimensions (src/dom.rs:277-291) */
int pt_adjusted_screen_dimensions(double raw_width, double raw_height, uint32_t* w, uint32_t* h);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_H */
