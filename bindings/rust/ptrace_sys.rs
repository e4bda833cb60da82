// bindings/rust/ptrace_sys.rs — SOURCE-ONLY Rust FFI for libptrace.so (include/ptrace.h).
//
// The reference's host code is Rust (src/*.rs); this file is what replaces its `mod webgl`.
// The build image has no Rust toolchain (no cargo/rustc, no network), so this file has never
// been compiled here; the same ABI is exercised by the ctypes binding
// (ray_tracer_webgl_amd/_lib.py) and by every `-m gpu` test.  Keep in sync with the header:
// tests/test_abi.py::test_rust_binding_lists_the_render_abi checks the symbol list.
// src/ptrace_sys.rs — FFI for libptrace.so (include/ptrace.h).  Replaces `mod webgl`.
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtSphere {            // == u_sphere_list[i], static/shader.frag:55-61
    pub center: [f32; 3], pub radius: f32,
    pub type_: i32, pub albedo: [f32; 3],
    pub fuzz: f32, pub refraction_index: f32,
    pub uuid: i32, pub _pad: i32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtParams {            // == uniform block, static/shader.frag:79-99
    pub width: u32, pub height: u32,
    pub time: f32, pub samples_per_pixel: i32, pub max_depth: i32,
    pub camera_origin: [f32; 3], pub horizontal: [f32; 3], pub vertical: [f32; 3],
    pub lower_left_corner: [f32; 3], pub u: [f32; 3], pub v: [f32; 3],
    pub lens_radius: f32,
    pub render_count: i32, pub should_average: i32, pub last_frame_weight: f32,
    pub background_mode: i32,
    pub band_rows: u32, pub band_index: u32, pub band_count: u32,
    pub time_step: f32, pub first_pass: u32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtErrorStats {        // the frame's noise figures, summed from the error estimate's tile records
    pub sum_e2: f64, pub sum_m2: f64, pub rel_error: f64, pub rms_error: f64,
    pub pixels: u64, pub pixels_counted: u64, pub pixels_short: u64, pub pixels_nonfinite: u64,
    pub passes_min: u32, pub passes_max: u32, pub passes_rendered: u32, pub reached: u32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtAdaptiveStats {     // what one pt_render_adaptive call did
    pub rounds: u32, pub partial_rounds: u32, pub tiles: u32, pub tiles_active: u32,
    pub tile_passes: u64, pub samples: u64,
}

#[repr(C)] #[derive(Clone, Copy)]
pub struct PtReprojectOptions {  // one pt_reproject: the caps are whole numbers in [0, 2^24), the tolerance is in pixel footprints
    pub cap_diffuse: f32, pub cap_other: f32, pub tolerance_px: f32, pub _pad: u32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtReprojectStats {    // the tallies of the last pt_reproject
    pub pixels: u64, pub pixels_hit: u64, pub pixels_kept: u64, pub samples_kept: u64,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtRay {               // one ray of pt_query_rays, 32 bytes; the direction is not normalised, the pads are not read
    pub origin: [f32; 3], pub _pad0: f32, pub direction: [f32; 3], pub _pad1: f32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtRayHit {            // its record, 64 bytes: the four feature texels; index -1 a miss, PT_RAY_INVALID an invalid ray
    pub albedo: [f32; 3], pub t: f32, pub normal: [f32; 3], pub _pad0: f32, pub point: [f32; 3], pub _pad1: f32,
    pub index: i32, pub uuid: i32, pub type_: i32, pub front_face: i32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtRayRadiance {       // the record of one ray of pt_query_radiance, 16 bytes: an accumulation texel; samples 0 marks an invalid ray
    pub sum: [f32; 3], pub samples: f32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtGatherPoint {       // one item of pt_gather_irradiance / pt_bake_probes, 32 bytes; a probe's normal and the pads are not read
    pub position: [f32; 3], pub _pad0: f32, pub normal: [f32; 3], pub _pad1: f32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtIrradiance {        // the record of one point of pt_gather_irradiance, 16 bytes; samples 0 marks an invalid item
    pub e: [f32; 3], pub samples: f32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtProbeSH {           // the record of one probe of pt_bake_probes, 112 bytes: nine real SH coefficients of bands 0 to 2 per channel
    pub sh: [[f32; 3]; 9], pub samples: f32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtProbeLattice {      // a regular lattice of probes, 48 bytes: node (iz * ny + iy) * nx + ix at fma(i_c, step.c, origin.c)
    pub origin: [f32; 3], pub nx: u32, pub step: [f32; 3], pub ny: u32, pub nz: u32, pub flags: u32, pub _pad: [u32; 2],
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtProbeShadeOptions { // the rule of one pt_shade_probes, 16 bytes; NULL stands for {PT_PROBE_HALFSPACE, 0.0}
    pub flags: u32, pub normal_bias: f32, pub _pad: [u32; 2],
}

#[repr(C)] #[derive(Clone, Copy)]
pub struct PtMeterOptions {      // the rule of one pt_meter, 48 bytes; the window is in image coordinates, w == 0 or h == 0: the whole frame
    pub key: f32, pub key_permille: u32, pub high_permille: u32, pub e_min: f32, pub e_max: f32, pub white_min: f32, pub rate: f32,
    pub x0: u32, pub y0: u32, pub w: u32, pub h: u32, pub _pad: u32,
}
impl Default for PtMeterOptions {  // PT_METER_OPTIONS_DEFAULT
    fn default() -> Self {
        PtMeterOptions { key: 0.18, key_permille: 500, high_permille: 990, e_min: 0.00390625, e_max: 256.0, white_min: 1.0, rate: 1.0,
                         x0: 0, y0: 0, w: 0, h: 0, _pad: 0 }
    }
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtExposure {          // the exposure record pt_meter keeps on the device, 32 bytes
    pub exposure: f32, pub white: f32, pub y_key: f32, pub y_high: f32, pub lit: u64, pub below: u32, pub meterings: u32,
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct PtToneOptions {       // curve PT_TONE_*, gamma, exposure (0: the device record's exposure and white), white; 16 bytes
    pub curve: i32, pub gamma: i32, pub exposure: f32, pub white: f32,
}

pub const PT_GLARE_MAX_LEVELS: usize = 8;
#[repr(C)] #[derive(Clone, Copy)]
pub struct PtGlareOptions {      // the rule of one pt_glare, 48 bytes; weight[k - 1] is the weight of level k, the first `levels` are read
    pub strength: f32, pub threshold: f32, pub levels: u32, pub _pad: u32, pub weight: [f32; PT_GLARE_MAX_LEVELS],
}
impl Default for PtGlareOptions {  // PT_GLARE_OPTIONS_DEFAULT
    fn default() -> Self {
        PtGlareOptions { strength: 0.15, threshold: 0.0, levels: 6, _pad: 0, weight: [0.35, 0.25, 0.18, 0.12, 0.06, 0.04, 0.0, 0.0] }
    }
}

#[repr(C)] pub struct PtCtx { _private: [u8; 0] }

#[link(name = "ptrace")]
extern "C" {
    pub fn pt_create(out: *mut *mut PtCtx, device: c_int, width: u32, height: u32) -> c_int;
    // for a host that brings its own hipStream_t: the context never creates a stream (an HSA queue) of its own
    pub fn pt_create_on_stream(out: *mut *mut PtCtx, device: c_int, width: u32, height: u32, hip_stream: *mut c_void) -> c_int;
    pub fn pt_destroy(ctx: *mut PtCtx) -> c_int;
    pub fn pt_resize(ctx: *mut PtCtx, width: u32, height: u32) -> c_int;
    pub fn pt_set_spheres(ctx: *mut PtCtx, spheres: *const PtSphere, n: u32) -> c_int;
    pub fn pt_set_params(ctx: *mut PtCtx, params: *const PtParams) -> c_int;
    pub fn pt_render(ctx: *mut PtCtx) -> c_int;
    pub fn pt_render_passes(ctx: *mut PtCtx, n_passes: u32) -> c_int;
    pub fn pt_reserve_passes(ctx: *mut PtCtx, max_passes: u32) -> c_int;
    pub fn pt_reset_accum(ctx: *mut PtCtx) -> c_int;
    pub fn pt_synchronize(ctx: *mut PtCtx) -> c_int;
    pub fn pt_resolve(ctx: *mut PtCtx, rgba_out: *mut f32, gamma: c_int) -> c_int;
    pub fn pt_resolve_rgba8(ctx: *mut PtCtx, rgba_out: *mut u8, gamma: c_int) -> c_int;
    pub fn pt_blend_rgba8(ctx: *mut PtCtx, prev: *const u8, out: *mut u8) -> c_int;
    pub fn pt_accum_ptr(ctx: *mut PtCtx, dev_ptr: *mut *mut c_void, bytes: *mut usize) -> c_int;
    pub fn pt_bind_accum(ctx: *mut PtCtx, dev_ptr: *mut c_void, bytes: usize) -> c_int;
    pub fn pt_read_accum(ctx: *mut PtCtx, dst: *mut f32, bytes: usize) -> c_int;
    pub fn pt_load_accum(ctx: *mut PtCtx, src: *const f32, bytes: usize) -> c_int;
    pub fn pt_set_stream(ctx: *mut PtCtx, hip_stream: *mut c_void) -> c_int;
    pub fn pt_set_option(ctx: *mut PtCtx, key: c_int, value: c_int) -> c_int;
    pub fn pt_tune(ctx: *mut PtCtx, n_passes: u32) -> c_int;
    // the shader's debug overlay (static/shader.frag:307-318): the three uniforms of src/webgl.rs:554-587, copied
    pub fn pt_set_debug_overlay(ctx: *mut PtCtx, enable: c_int, selected_object: i32, cursor_point: *const f32) -> c_int;
    pub fn pt_last_trace_build(ctx: *mut PtCtx) -> c_int;
    // the per-pixel error estimate (pt_set_option PT_OPT_ERROR_ESTIMATE 1): raw state, standard-error image, 8x8-tile
    // records {sum se^2, sum mean^2, counted pixels, min passes}, the frame's figures, and rendering to a noise target
    pub fn pt_error_ptr(ctx: *mut PtCtx, dev_ptr: *mut *mut c_void, bytes: *mut usize) -> c_int;
    pub fn pt_resolve_error(ctx: *mut PtCtx, rgba_out: *mut f32) -> c_int;
    pub fn pt_error_tiles(ctx: *mut PtCtx, tiles_out: *mut f32, tiles_x: *mut u32, tiles_y: *mut u32) -> c_int;
    pub fn pt_error_stats(ctx: *mut PtCtx, out: *mut PtErrorStats) -> c_int;
    pub fn pt_render_until(ctx: *mut PtCtx, target_rel_error: f32, passes_per_launch: u32, max_passes: u32, out: *mut PtErrorStats) -> c_int;
    pub fn pt_render_adaptive(ctx: *mut PtCtx, target_rel_error: f32, passes_per_round: u32, max_passes: u32, out: *mut PtErrorStats, adaptive_out: *mut PtAdaptiveStats) -> c_int;
    pub fn pt_adaptive_tiles(ctx: *mut PtCtx, base_out: *mut u32, order_out: *mut u32, n_tiles: *mut u32, n_active: *mut u32) -> c_int;
    // the variance-guided filtered read-out of the estimate: each pixel's mean averaged with the neighbours within `radius` whose
    // means differ by no more than kappa standard errors of the difference; out.a = accepted taps
    pub fn pt_resolve_filtered(ctx: *mut PtCtx, rgba_out: *mut f32, radius: u32, kappa: f32, gamma: c_int) -> c_int;
    // the same read-out with the test summed over the (2 patch + 1)^2 neighbourhoods around the two pixels; patch 0 gives
    // pt_resolve_filtered's bits
    pub fn pt_resolve_filtered_patch(ctx: *mut PtCtx, rgba_out: *mut f32, radius: u32, patch: u32, kappa: f32, gamma: c_int) -> c_int;
    // the first-hit feature planes (pt_set_option PT_OPT_FEATURES 1): one pinhole ray per pixel, four planes of 16-byte texels —
    // {albedo.rgb, t}, {normal, 0}, {hit point, 0}, int32 {list index, uuid, type, front_face}; a device pick is IDS[y][x]
    pub fn pt_render_features(ctx: *mut PtCtx) -> c_int;
    pub fn pt_features_ptr(ctx: *mut PtCtx, plane: c_int, dev_ptr: *mut *mut c_void, bytes: *mut usize) -> c_int;
    pub fn pt_read_features(ctx: *mut PtCtx, plane: c_int, out: *mut c_void) -> c_int;
    // temporal reprojection (pt_set_option PT_OPT_REPROJECT 1, beside PT_OPT_FEATURES): carry the accumulation across a camera
    // move.  A tick: pt_keep_history, pt_set_params(next), pt_render_features, pt_reproject, pt_render_passes
    pub fn pt_keep_history(ctx: *mut PtCtx) -> c_int;
    pub fn pt_load_history(ctx: *mut PtCtx, prev: *const PtParams, ids: *const c_void, point: *const c_void) -> c_int;
    pub fn pt_reproject(ctx: *mut PtCtx, options: *const PtReprojectOptions) -> c_int;
    pub fn pt_reproject_stats(ctx: *mut PtCtx, out: *mut PtReprojectStats) -> c_int;
    pub fn pt_reproject_constants(prev: *const PtParams, tolerance_px: f32, out16: *mut f32) -> c_int;
    // pt_reproject that also carries the error estimate's state (needs PT_OPT_ERROR_ESTIMATE too): the same accumulation bits
    pub fn pt_reproject_estimate(ctx: *mut PtCtx, options: *const PtReprojectOptions) -> c_int;
    // ray queries (pt_set_option PT_OPT_RAY_QUERIES 1): the closest hit of the caller's rays through the trace kernels' own
    // intersection — the autofocus and selection ray (src/state.rs get_center_hit), picks, visibility probes; host or device
    // pointers, synchronous; pt_query_batch: the rays one launch takes
    pub fn pt_query_rays(ctx: *mut PtCtx, rays: *const PtRay, n: u32, hits: *mut PtRayHit) -> c_int;
    pub fn pt_query_batch(ctx: *mut PtCtx) -> u32;
    // radiance queries (PT_OPT_RAY_QUERIES on): the path-traced radiance along the caller's rays — probes, a baker's batch, a second
    // view — by the plain estimator, n_passes passes (at most those reserved) of samples_per_pixel samples per ray; host or device
    // pointers, synchronous; the camera, the accumulation and first_pass do not move
    pub fn pt_query_radiance(ctx: *mut PtCtx, rays: *const PtRay, n: u32, n_passes: u32, out: *mut PtRayRadiance) -> c_int;
    pub fn pt_gather_irradiance(ctx: *mut PtCtx, points: *const PtGatherPoint, n: u32, directions: u32, n_passes: u32, out: *mut PtIrradiance) -> c_int;
    pub fn pt_bake_probes(ctx: *mut PtCtx, probes: *const PtGatherPoint, n: u32, directions: u32, n_passes: u32, out: *mut PtProbeSH) -> c_int;
    // the same three by the next-event estimator (PT_OPT_RAY_QUERIES and PT_OPT_NEXT_EVENT on): the caller's ray is a path's first
    // segment, the light samples start at its first DIFFUSE hit; same arguments, records and batches as the namesakes
    pub fn pt_query_radiance_nee(ctx: *mut PtCtx, rays: *const PtRay, n: u32, n_passes: u32, out: *mut PtRayRadiance) -> c_int;
    pub fn pt_gather_irradiance_nee(ctx: *mut PtCtx, points: *const PtGatherPoint, n: u32, directions: u32, n_passes: u32, out: *mut PtIrradiance) -> c_int;
    pub fn pt_bake_probes_nee(ctx: *mut PtCtx, probes: *const PtGatherPoint, n: u32, directions: u32, n_passes: u32, out: *mut PtProbeSH) -> c_int;
    // probe lattices: bake the nodes first .. first + count - 1 of a lattice as pt_bake_probes (estimator 0) or pt_bake_probes_nee
    // (estimator 1) bakes the same points, made on the device; shade the feature planes in place from a lattice's records into
    // linear RGBA f32 texels (host or device pointers; alpha 0 marks a pixel without a usable probe)
    pub fn pt_bake_lattice(ctx: *mut PtCtx, lattice: *const PtProbeLattice, first: u32, count: u32, directions: u32, n_passes: u32, estimator: c_int, out: *mut PtProbeSH) -> c_int;
    pub fn pt_shade_probes(ctx: *mut PtCtx, lattice: *const PtProbeLattice, probes: *const PtProbeSH, options: *const PtProbeShadeOptions, rgba_out: *mut f32) -> c_int;
    // exposure metering and the toned read-outs (pt_set_option PT_OPT_TONEMAP 1): meter the frame on the device (src NULL: the
    // accumulation; else host or device linear RGBA f32 texels), keep the exposure record there, read the frame out through a tone
    // curve; pt_exposure_solve is the metering's second kernel on the host (ranks add their histograms, solve, pt_meter_set)
    pub fn pt_meter(ctx: *mut PtCtx, src: *const f32, options: *const PtMeterOptions) -> c_int;
    pub fn pt_meter_read(ctx: *mut PtCtx, out: *mut PtExposure, hist256: *mut u32) -> c_int;
    pub fn pt_meter_set(ctx: *mut PtCtx, record: *const PtExposure) -> c_int;
    pub fn pt_exposure_solve(hist256: *const u32, below: u32, options: *const PtMeterOptions, prev_or_null: *const PtExposure, out: *mut PtExposure) -> c_int;
    pub fn pt_resolve_toned(ctx: *mut PtCtx, src: *const f32, options: *const PtToneOptions, rgba_out: *mut f32) -> c_int;
    pub fn pt_resolve_toned_rgba8(ctx: *mut PtCtx, src: *const f32, options: *const PtToneOptions, rgba_out: *mut u8) -> c_int;
    // glare (pt_set_option PT_OPT_GLARE 1): a share of the frame's light spread over a bloom pyramid and added back, energy
    // conserved; src as above, rgba_out linear RGBA f32 on the host or the device (may be a device src): what pt_meter and
    // pt_resolve_toned take next; synchronous
    pub fn pt_glare(ctx: *mut PtCtx, src: *const f32, options: *const PtGlareOptions, rgba_out: *mut f32) -> c_int;
    // the camera moves every tick (State::update_position, src/state.rs:411-441): does the grid of a large scene still fit
    // it (0 yes / 1 no: refit now / 2 looser than needed), and the rebuild for the margin class the camera needs
    pub fn pt_grid_fit(ctx: *mut PtCtx) -> c_int;
    pub fn pt_refit_grid(ctx: *mut PtCtx, only_if_stale: c_int) -> c_int;
    // the reference's frame on device-resident textures: webgl::render, src/webgl.rs:180-205
    pub fn pt_clear_textures(ctx: *mut PtCtx) -> c_int;
    pub fn pt_render_frame(ctx: *mut PtCtx, even_odd_count: u32) -> c_int;
    pub fn pt_render_frames(ctx: *mut PtCtx, even_odd_count: u32, max_render_count: u32, n_frames: u32) -> c_int;
    pub fn pt_read_canvas(ctx: *mut PtCtx, rgba_out: *mut u8) -> c_int;
    pub fn pt_read_texture(ctx: *mut PtCtx, index: c_int, rgba_out: *mut u8) -> c_int;
    pub fn pt_write_texture(ctx: *mut PtCtx, index: c_int, rgba_in: *const u8) -> c_int;
    pub fn pt_last_error(ctx: *mut PtCtx) -> *const c_char;
    pub fn pt_abi_version() -> c_int;
    pub fn pt_device_count() -> c_int;
    // multi-GPU from one host process: the row arithmetic of the band partition
    pub fn pt_local_rows(height: u32, band_rows: u32, band_index: u32, band_count: u32) -> u32;
    pub fn pt_band_row(band_rows: u32, band_index: u32, band_count: u32, local_row: u32) -> u32;
}

pub const PT_OPT_GEOMETRY_PATH: c_int = 1;      // PT_GEOM_AUTO 0 / LDS 1 / SCALAR 2 / BVH 3 / GRID 4 / SMALL 5
pub const PT_OPT_ERROR_ESTIMATE: c_int = 7;     // opt-in, 0 = off; the image bits do not depend on it
pub const PT_OPT_FEATURES: c_int = 8;           // opt-in, 0 = off; the image bits do not depend on it
pub const PT_OPT_REPROJECT: c_int = 9;          // opt-in, 0 = off; needs PT_OPT_FEATURES on
pub const PT_OPT_RAY_QUERIES: c_int = 10;       // opt-in, 0 = off; the image bits do not depend on it
pub const PT_OPT_TONEMAP: c_int = 11;           // opt-in, 0 = off; the image bits do not depend on it
pub const PT_OPT_GLARE: c_int = 12;             // opt-in, 0 = off; scratch only, the image bits do not depend on it
pub const PT_TONE_CLAMP: i32 = 0;
pub const PT_TONE_REINHARD: i32 = 1;
pub const PT_TONE_FILMIC: i32 = 2;
pub const PT_LATTICE_SKIP_BURIED: u32 = 1;       // PtProbeLattice.flags: a node inside a sphere that is not GLASS is an invalid item
pub const PT_PROBE_HALFSPACE: u32 = 1;           // PtProbeShadeOptions.flags: drop the probes at or behind the pixel's tangent plane
pub const PT_RAY_INVALID: i32 = -2;             // PtRayHit.index / uuid / type of an invalid ray
pub const PT_REPROJECT_TOLERANCE_DEFAULT: f32 = 2.0;
pub const PT_REPROJECT_CAP_DIFFUSE_DEFAULT: f32 = 32.0;
pub const PT_REPROJECT_CAP_OTHER_DEFAULT: f32 = 8.0;
pub const PT_FEAT_ALBEDO: c_int = 0;
pub const PT_FEAT_NORMAL: c_int = 1;
pub const PT_FEAT_POINT: c_int = 2;
pub const PT_FEAT_IDS: c_int = 3;
pub const PT_FEAT_PLANES: c_int = 4;
pub const PT_FILTER_MAX_RADIUS: u32 = 4;        // pt_resolve_filtered: the largest radius
pub const PT_FILTER_KAPPA_DEFAULT: f32 = 2.0;   // ... and the kappa its callers start from
pub const PT_FILTER_MAX_PATCH: u32 = 1;               // pt_resolve_filtered_patch: the largest patch radius
pub const PT_FILTER_PATCH_KAPPA_DEFAULT: f32 = 1.5;   // ... and the kappa its callers start from
pub const PT_OPT_RUSSIAN_ROULETTE: c_int = 5;   // opt-in, 0 = off: the reference's estimator has none (shader.frag:297-339)
pub const PT_OPT_NEXT_EVENT: c_int = 13;        // opt-in, 0 = off: the render launches sample the emissive spheres at diffuse hits (same
                                                // expectation, other samples); excludes roulette, the debug overlay and PT_OPT_COUNT_WORK
pub const PT_BUILD_NEXT_EVENT: c_int = 16;      // pt_last_trace_build after a next-event launch

// The rAF closure of src/lib.rs:65-104 with webgl::render replaced (one tick):
//     state::update_render_globals(&mut state);
//     let p = PtParams::from_state(&state, now);            // uniforms.run_setters(now)
//     pt_set_params(ctx, &p);
//     if pt_grid_fit(ctx) == 1 { pt_refit_grid(ctx, 0); }   // scenes of hundreds of spheres: the camera has left the region the
//                                                           // grid was fitted to (host arithmetic; 0 for the reference's 9 spheres)
//     pt_render_frame(ctx, state.even_odd_count);           // webgl::render: trace + blend into the ping-pong textures
//     if should_save { pt_read_canvas(ctx, pixels.as_mut_ptr()); }
// A run of ticks with nothing else happening (no input: no key held; should_average on — without it only the
// first tick draws, src/state.rs:443-447) is one call:
//     p.time_step = frame_interval_ms; pt_set_params(ctx, &p);
//     pt_render_frames(ctx, state.even_odd_count, state.max_render_count, n);   // one hipGraph replayed n times
//     for _ in 1..n { state::update_render_globals(&mut state); }

// State -> uniforms: what Uniforms::run_setters uploads (src/webgl.rs:279-593)
impl PtParams {
    pub fn from_state(s: &crate::state::State, now_ms: f64) -> Self {
        let spp = if s.is_paused { s.samples_per_pixel.max(25) } else { s.samples_per_pixel };
        PtParams {
            width: s.width, height: s.height, time: now_ms as f32,
            samples_per_pixel: spp as i32, max_depth: s.max_depth as i32,
            camera_origin: s.camera_origin.to_array(), horizontal: s.horizontal.to_array(),
            vertical: s.vertical.to_array(), lower_left_corner: s.lower_left_corner.to_array(),
            u: s.u.to_array(), v: s.v.to_array(), lens_radius: s.lens_radius as f32,
            render_count: s.render_count as i32, should_average: s.should_average as i32,
            last_frame_weight: s.last_frame_weight, background_mode: 0,
            band_rows: 8, band_index: 0, band_count: 1,
            time_step: 0.0, first_pass: 0,   // one pass per frame at u_time = now, as the reference renders
        }
    }
}

// Sphere -> u_sphere_list[i]: what webgl::set_geometry uploads (src/webgl.rs:225-274)
impl From<&crate::glsl::Sphere> for PtSphere {
    fn from(s: &crate::glsl::Sphere) -> Self {
        PtSphere {
            center: s.center.to_array(), radius: s.radius as f32,
            type_: s.material.material_type.value(), albedo: s.material.albedo.to_array(),
            fuzz: s.material.fuzz, refraction_index: s.material.refraction_index,
            uuid: s.uuid, _pad: 0,
        }
    }
}
