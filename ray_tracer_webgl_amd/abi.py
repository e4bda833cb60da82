"""ctypes mirrors of the POD structs in include/ptrace.h.

Field order, types and sizes must match the header exactly (tests/test_abi.py checks the sizes
against a C program compiled from the header).  Reference citations: PtSphere mirrors the fields
webgl::set_geometry uploads (src/webgl.rs:225-274); PtParams mirrors the uniform block
(static/shader.frag:79-102) as uploaded by Uniforms::run_setters (src/webgl.rs:629-633);
PtCameraIn mirrors the camera members of State (src/state.rs:31-57).
"""
import ctypes as C

import numpy as np

PT_ABI_VERSION = 5

PT_OK = 0
PT_ERR_INVALID = -1
PT_ERR_NO_DEVICE = -2
PT_ERR_HIP = -3
PT_ERR_NOT_READY = -4
PT_ERR_CAPACITY = -5

# static/shader.frag:45-47, src/glsl.rs:10-24 (+ build extension 3)
PT_DIFFUSE = 0
PT_METAL = 1
PT_GLASS = 2
PT_EMISSIVE = 3

PT_BG_SKY = 0
PT_BG_BLACK = 1

PT_GEOM_AUTO, PT_GEOM_LDS, PT_GEOM_SCALAR, PT_GEOM_BVH, PT_GEOM_GRID, PT_GEOM_SMALL = 0, 1, 2, 3, 4, 5
PT_OPT_GEOMETRY_PATH, PT_OPT_COUNT_WORK, PT_OPT_CARRY_LANES, PT_OPT_REFILL_MIN, PT_OPT_RUSSIAN_ROULETTE, PT_OPT_GRID_FIT = 1, 2, 3, 4, 5, 6
PT_OPT_FEATURES = 8  # the first-hit feature planes (pt_render_features, pt_features_ptr, pt_read_features)
PT_FEAT_ALBEDO, PT_FEAT_NORMAL, PT_FEAT_POINT, PT_FEAT_IDS, PT_FEAT_PLANES = 0, 1, 2, 3, 4
PT_OPT_ERROR_ESTIMATE = 7  # the per-pixel error estimate (pt_error_ptr, pt_resolve_error, pt_error_tiles, pt_error_stats, pt_render_until)
PT_OPT_REPROJECT = 9  # temporal reprojection's history planes (pt_keep_history, pt_load_history, pt_reproject, pt_reproject_estimate, pt_reproject_stats)
PT_OPT_RAY_QUERIES = 10  # the query planes of pt_query_rays (closest hits for the caller's rays), pt_query_batch
PT_OPT_TONEMAP = 11  # the exposure state of pt_meter and the toned read-outs (pt_meter_read, pt_meter_set, pt_resolve_toned, pt_resolve_toned_rgba8)
PT_TONE_CLAMP, PT_TONE_REINHARD, PT_TONE_FILMIC = 0, 1, 2  # PtToneOptions.curve
PT_OPT_GLARE = 12  # the pyramid of pt_glare (scratch only, no state)
PT_GLARE_MAX_LEVELS = 8
PT_OPT_NEXT_EVENT = 13  # next-event estimation: the render launches sample the emissive spheres at DIFFUSE hits (same expectation, other samples)
PT_GLARE_STRENGTH_DEFAULT = 0.15    # PtGlareOptions: the share of the spread light that is added back
PT_GLARE_LEVELS_DEFAULT = 6         # ... the levels in use
PT_GLARE_WEIGHTS_DEFAULT = (0.35, 0.25, 0.18, 0.12, 0.06, 0.04, 0.0, 0.0)  # ... and their weights (they add up to 1)
PT_METER_KEY_DEFAULT = 0.18            # PtMeterOptions: the luminance the key percentile is exposed to
PT_METER_KEY_PERMILLE_DEFAULT = 500    # ... the percentile that is the key
PT_METER_HIGH_PERMILLE_DEFAULT = 990   # ... and the one that becomes white
PT_METER_E_MIN_DEFAULT = 2.0 ** -8     # ... the exposure's range
PT_METER_E_MAX_DEFAULT = 2.0 ** 8
PT_RAY_INVALID = -2  # PtRayHit.index, .uuid and .type of an invalid ray (a non-finite component, or a direction of three zeros)
PT_REPROJECT_TOLERANCE_DEFAULT = 2.0     # pt_reproject: the distance test, in pixel footprints at the history camera's depth
PT_REPROJECT_CAP_DIFFUSE_DEFAULT = 32.0   # ... the most samples a kept diffuse pixel carries over
PT_REPROJECT_CAP_OTHER_DEFAULT = 8.0      # ... and a pixel of any other material
PT_TIME_STEP_DECORRELATED = 0.3618034  # include/ptrace.h
PT_FILTER_MAX_RADIUS = 4        # pt_resolve_filtered: the largest radius
PT_FILTER_KAPPA_DEFAULT = 2.0   # ... and the kappa its callers start from
PT_FILTER_MAX_PATCH = 1               # pt_resolve_filtered_patch: the largest patch radius (3x3 neighbourhoods)
PT_FILTER_PATCH_KAPPA_DEFAULT = 1.5   # ... and the kappa its callers start from
NO_SELECTED_OBJECT_ID = 1000  # src/state.rs:12: State.selected_object while the crosshair is on nothing
BUILD_PLAIN, BUILD_ROULETTE, BUILD_TWIN, BUILD_DEBUG_OVERLAY, BUILD_FEATURES = 0, 1, 2, 3, 4  # pt_last_trace_build
BUILD_NEXT_EVENT = 16  # ... and the next-event builds, which are no column of the trace table (csrc/pt_nee_table.hpp)
PT_STREAM_LEGACY = 1  # include/ptrace.h: hipStreamLegacy, the default (NULL) stream by name
GEOM_NAMES = {0: "auto", 1: "lds", 2: "scalar", 3: "bvh", 4: "grid", 5: "small"}

f3 = C.c_float * 3
d3 = C.c_double * 3


class PtSphere(C.Structure):
    _fields_ = [
        ("center", f3),
        ("radius", C.c_float),
        ("type", C.c_int32),
        ("albedo", f3),
        ("fuzz", C.c_float),
        ("refraction_index", C.c_float),
        ("uuid", C.c_int32),
        ("_pad", C.c_int32),
    ]


# numpy view of the same 48-byte record, for bulk scene generation
SPHERE_DTYPE = np.dtype(
    [
        ("center", "<f4", 3),
        ("radius", "<f4"),
        ("type", "<i4"),
        ("albedo", "<f4", 3),
        ("fuzz", "<f4"),
        ("refraction_index", "<f4"),
        ("uuid", "<i4"),
        ("_pad", "<i4"),
    ]
)
assert SPHERE_DTYPE.itemsize == C.sizeof(PtSphere) == 48


class PtParams(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("time", C.c_float),
        ("samples_per_pixel", C.c_int32),
        ("max_depth", C.c_int32),
        ("camera_origin", f3),
        ("horizontal", f3),
        ("vertical", f3),
        ("lower_left_corner", f3),
        ("u", f3),
        ("v", f3),
        ("lens_radius", C.c_float),
        ("render_count", C.c_int32),
        ("should_average", C.c_int32),
        ("last_frame_weight", C.c_float),
        ("background_mode", C.c_int32),
        ("band_rows", C.c_uint32),
        ("band_index", C.c_uint32),
        ("band_count", C.c_uint32),
        ("time_step", C.c_float),
        ("first_pass", C.c_uint32),
    ]

    def copy(self):
        out = PtParams()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(PtParams))
        return out


class PtCameraIn(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("camera_origin", d3),
        ("yaw_degrees", C.c_double),
        ("pitch_degrees", C.c_double),
        ("vup", d3),
        ("fov_radians", C.c_double),
        ("focus_distance", C.c_double),
        ("aperture", C.c_double),
    ]


class PtLookAtIn(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("look_from", d3),
        ("look_at", d3),
        ("vup", d3),
        ("vfov_radians", C.c_double),
        ("focus_distance", C.c_double),
        ("aperture", C.c_double),
    ]


class PtStats(C.Structure):
    _fields_ = [
        ("segments", C.c_uint64),
        ("samples", C.c_uint64),
        ("sphere_tests", C.c_uint64),
        ("render_kernel_ms", C.c_double),
        ("render_launches", C.c_uint32),
        ("total_spp", C.c_uint32),
        ("n_spheres", C.c_uint32),
        ("local_rows", C.c_uint32),
        ("geometry_path", C.c_uint32),
        ("geometry_tuned", C.c_uint32),
        ("bvh_nodes", C.c_uint32),
        ("bvh_slots", C.c_uint32),
        ("bvh_outliers", C.c_uint32),
        ("bvh_depth", C.c_uint32),
        ("grid_cells", C.c_uint32 * 3),
        ("grid_entries", C.c_uint32),
        ("grid_always", C.c_uint32),
        ("grid_fit_stale", C.c_uint32),  # 0 fits / 1 camera outside the near region (far path: refit) / 2 looser than needed
        ("work", C.c_uint64 * 8),
        ("grid_near_factor", C.c_float),
        ("grid_need_factor", C.c_float),
        ("far_rays", C.c_uint64),
        ("grid_kernel_build", C.c_uint32),  # 1 pt_trace_kernel_grid (all staged in the LDS) / 2 _grid_cells / 3 _grid_gmem / 0 no grid
        ("grid_walk_flat", C.c_uint32),  # 1: build 1 on a one-layer grid, the two-axis walk (pt_trace_kernel_grid); 0 with build 1: _grid_layers
    ]


class PtErrorStats(C.Structure):
    """include/ptrace.h PtErrorStats: the frame's noise figures, summed from the error estimate's tile records."""

    _fields_ = [
        ("sum_e2", C.c_double),
        ("sum_m2", C.c_double),
        ("rel_error", C.c_double),
        ("rms_error", C.c_double),
        ("pixels", C.c_uint64),
        ("pixels_counted", C.c_uint64),
        ("pixels_short", C.c_uint64),
        ("pixels_nonfinite", C.c_uint64),
        ("passes_min", C.c_uint32),
        ("passes_max", C.c_uint32),
        ("passes_rendered", C.c_uint32),
        ("reached", C.c_uint32),
    ]


class PtAdaptiveStats(C.Structure):
    """include/ptrace.h PtAdaptiveStats: what one pt_render_adaptive call did."""

    _fields_ = [
        ("rounds", C.c_uint32),
        ("partial_rounds", C.c_uint32),
        ("tiles", C.c_uint32),
        ("tiles_active", C.c_uint32),
        ("tile_passes", C.c_uint64),
        ("samples", C.c_uint64),
    ]


class PtReprojectOptions(C.Structure):
    """include/ptrace.h PtReprojectOptions: the caps (whole numbers below 2^24) and the distance tolerance of one pt_reproject."""

    _fields_ = [
        ("cap_diffuse", C.c_float),
        ("cap_other", C.c_float),
        ("tolerance_px", C.c_float),
        ("_pad", C.c_uint32),
    ]

    def __init__(self, cap_diffuse=PT_REPROJECT_CAP_DIFFUSE_DEFAULT, cap_other=PT_REPROJECT_CAP_OTHER_DEFAULT,
                 tolerance_px=PT_REPROJECT_TOLERANCE_DEFAULT):
        super().__init__(cap_diffuse, cap_other, tolerance_px, 0)


class PtReprojectStats(C.Structure):
    """include/ptrace.h PtReprojectStats: the tallies of the last pt_reproject."""

    _fields_ = [
        ("pixels", C.c_uint64),
        ("pixels_hit", C.c_uint64),
        ("pixels_kept", C.c_uint64),
        ("samples_kept", C.c_uint64),
    ]


class PtRay(C.Structure):
    """include/ptrace.h PtRay: one ray of pt_query_rays, 32 bytes; the direction is not normalised, the pads are not read."""

    _fields_ = [
        ("origin", C.c_float * 3),
        ("_pad0", C.c_float),
        ("direction", C.c_float * 3),
        ("_pad1", C.c_float),
    ]


class PtRayHit(C.Structure):
    """include/ptrace.h PtRayHit: the record of one ray, 64 bytes — the four feature texels of pt_render_features in order."""

    _fields_ = [
        ("albedo", C.c_float * 3),
        ("t", C.c_float),
        ("normal", C.c_float * 3),
        ("_pad0", C.c_float),
        ("point", C.c_float * 3),
        ("_pad1", C.c_float),
        ("index", C.c_int32),
        ("uuid", C.c_int32),
        ("type", C.c_int32),
        ("front_face", C.c_int32),
    ]


class PtRayRadiance(C.Structure):
    """include/ptrace.h PtRayRadiance: the record of one ray of pt_query_radiance, 16 bytes — an accumulation texel; samples 0 marks an invalid ray."""

    _fields_ = [
        ("sum", C.c_float * 3),
        ("samples", C.c_float),
    ]


class PtGatherPoint(C.Structure):
    """include/ptrace.h PtGatherPoint: one item of pt_gather_irradiance / pt_bake_probes, 32 bytes; a probe's normal and the pads are not read."""

    _fields_ = [
        ("position", C.c_float * 3),
        ("_pad0", C.c_float),
        ("normal", C.c_float * 3),
        ("_pad1", C.c_float),
    ]


class PtIrradiance(C.Structure):
    """include/ptrace.h PtIrradiance: the record of one point of pt_gather_irradiance, 16 bytes; samples 0 marks an invalid item."""

    _fields_ = [
        ("e", C.c_float * 3),
        ("samples", C.c_float),
    ]


class PtProbeSH(C.Structure):
    """include/ptrace.h PtProbeSH: the record of one probe of pt_bake_probes, 112 bytes — nine real SH coefficients of bands 0 to 2
    per channel, in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2); samples 0 marks an invalid item."""

    _fields_ = [
        ("sh", (C.c_float * 3) * 9),
        ("samples", C.c_float),
    ]


PT_GATHER_MIN_DIRECTIONS, PT_GATHER_MAX_DIRECTIONS = 64, 4096  # a multiple of 64 in between


def sh_irradiance(sh, normals):
    """The irradiance a probe's SH record gives a surface with unit normal n: the cosine convolution, band factors pi, 2 pi / 3
    and pi / 4 on the nine coefficients in PtProbeSH's order.  `sh`: (..., 9, 3), `normals`: (..., 3), broadcast against each
    other; (..., 3) float64 out.  Exact for light without a band above 2 (up to the probe's quadrature)."""
    import numpy as np

    sh = np.asarray(sh, np.float64)
    n = np.asarray(normals, np.float64)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    basis = np.stack([0.282095 * np.ones_like(x), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                      0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], axis=-1)
    band = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return np.einsum("...k,...kc->...c", basis * band, sh)


PT_LATTICE_SKIP_BURIED = 1  # PtProbeLattice.flags: a node inside a sphere that is not GLASS is an invalid item (NaN position)
PT_PROBE_HALFSPACE = 1      # PtProbeShadeOptions.flags: drop the probes at or behind the pixel's tangent plane
PT_LATTICE_MIN_NODES, PT_LATTICE_MAX_NODES, PT_LATTICE_MAX_TOTAL = 2, 256, 1 << 20  # per axis; nx * ny * nz


class PtProbeLattice(C.Structure):
    """include/ptrace.h PtProbeLattice: a regular lattice of probes, 48 bytes.  Node (iz * ny + iy) * nx + ix stands at
    fma(float(i_c), step.c, origin.c); nx, ny, nz in [2, 256], their product at most 2^20, every step finite and > 0."""

    _fields_ = [
        ("origin", C.c_float * 3),
        ("nx", C.c_uint32),
        ("step", C.c_float * 3),
        ("ny", C.c_uint32),
        ("nz", C.c_uint32),
        ("flags", C.c_uint32),
        ("_pad", C.c_uint32 * 2),
    ]

    def __init__(self, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), n=(2, 2, 2), flags=0):
        super().__init__((C.c_float * 3)(*origin), n[0], (C.c_float * 3)(*step), n[1], n[2], flags, (C.c_uint32 * 2)(0, 0))

    @property
    def nodes(self):
        return int(self.nx) * int(self.ny) * int(self.nz)

    def copy(self):
        out = PtProbeLattice()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(self))
        return out


class PtProbeShadeOptions(C.Structure):
    """include/ptrace.h PtProbeShadeOptions: the rule of one pt_shade_probes, 16 bytes.  The default is the call's NULL."""

    _fields_ = [
        ("flags", C.c_uint32),
        ("normal_bias", C.c_float),
        ("_pad", C.c_uint32 * 2),
    ]

    def __init__(self, flags=PT_PROBE_HALFSPACE, normal_bias=0.0):
        super().__init__(flags, normal_bias, (C.c_uint32 * 2)(0, 0))


def probe_lattice_positions(lattice):
    """(nx * ny * nz, 3) float32: the node positions of a lattice in node order, position.c = fma(float(i_c), step.c, origin.c)
    with the device's bits.  The fp32 fma in numpy: the product of an index below 2^8 and a float32 is exact in float64; the sum
    is rounded to odd there (two-sum finds the lost part, an inexact even result moves to its odd neighbour on that side), and a
    53-bit round-to-odd value rounds to float32 as the exact sum does."""
    import numpy as np

    axes = []
    for c, n in enumerate((lattice.nx, lattice.ny, lattice.nz)):
        p = np.arange(int(n), dtype=np.float64) * np.float64(lattice.step[c])
        o = np.full_like(p, np.float64(lattice.origin[c]))
        s = p + o
        t = s - p
        lost = (p - (s - t)) + (o - t)
        even = (s.view(np.int64) & 1) == 0
        s = np.where((lost != 0) & even, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)), s)
        axes.append(s.astype(np.float32))
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3))


class PtMeterOptions(C.Structure):
    """include/ptrace.h PtMeterOptions: the rule of one pt_meter (and of pt_exposure_solve, which does not read the window),
    48 bytes.  The window {x0, y0, w, h} is in image coordinates, row 0 at the bottom; w == 0 or h == 0 is the whole frame."""

    _fields_ = [
        ("key", C.c_float),
        ("key_permille", C.c_uint32),
        ("high_permille", C.c_uint32),
        ("e_min", C.c_float),
        ("e_max", C.c_float),
        ("white_min", C.c_float),
        ("rate", C.c_float),
        ("x0", C.c_uint32),
        ("y0", C.c_uint32),
        ("w", C.c_uint32),
        ("h", C.c_uint32),
        ("_pad", C.c_uint32),
    ]

    def __init__(self, key=PT_METER_KEY_DEFAULT, key_permille=PT_METER_KEY_PERMILLE_DEFAULT, high_permille=PT_METER_HIGH_PERMILLE_DEFAULT,
                 e_min=PT_METER_E_MIN_DEFAULT, e_max=PT_METER_E_MAX_DEFAULT, white_min=1.0, rate=1.0, window=(0, 0, 0, 0)):
        super().__init__(key, key_permille, high_permille, e_min, e_max, white_min, rate, window[0], window[1], window[2], window[3], 0)

    def copy(self):
        out = PtMeterOptions()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(self))
        return out


class PtExposure(C.Structure):
    """include/ptrace.h PtExposure: the exposure record pt_meter keeps on the device, 32 bytes."""

    _fields_ = [
        ("exposure", C.c_float),
        ("white", C.c_float),
        ("y_key", C.c_float),
        ("y_high", C.c_float),
        ("lit", C.c_uint64),
        ("below", C.c_uint32),
        ("meterings", C.c_uint32),
    ]

    def copy(self):
        out = PtExposure()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(self))
        return out


class PtToneOptions(C.Structure):
    """include/ptrace.h PtToneOptions: curve (PT_TONE_*), gamma, and the exposure — 0 reads exposure and white from the device
    record, a positive value uses these —, 16 bytes."""

    _fields_ = [
        ("curve", C.c_int32),
        ("gamma", C.c_int32),
        ("exposure", C.c_float),
        ("white", C.c_float),
    ]

    def __init__(self, curve=PT_TONE_REINHARD, gamma=1, exposure=0.0, white=1.0):
        super().__init__(curve, gamma, exposure, white)


class PtGlareOptions(C.Structure):
    """include/ptrace.h PtGlareOptions: the rule of one pt_glare, 48 bytes.  `weights`: the weights of level 1 .. levels (at most
    PT_GLARE_MAX_LEVELS; the rest are 0); the glare conserves energy when they add up to 1."""

    _fields_ = [
        ("strength", C.c_float),
        ("threshold", C.c_float),
        ("levels", C.c_uint32),
        ("_pad", C.c_uint32),
        ("weight", C.c_float * PT_GLARE_MAX_LEVELS),
    ]

    def __init__(self, strength=PT_GLARE_STRENGTH_DEFAULT, threshold=0.0, levels=PT_GLARE_LEVELS_DEFAULT, weights=PT_GLARE_WEIGHTS_DEFAULT):
        w = tuple(weights) + (0.0,) * (PT_GLARE_MAX_LEVELS - len(tuple(weights)))
        super().__init__(strength, threshold, levels, 0, (C.c_float * PT_GLARE_MAX_LEVELS)(*w))

    def copy(self):
        out = PtGlareOptions()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(self))
        return out


class PtHostSphere(C.Structure):
    """src/glsl.rs:27-40: f64 centre/radius/albedo, f32 fuzz/refraction_index."""

    _fields_ = [
        ("center", d3),
        ("radius", C.c_double),
        ("type", C.c_int32),
        ("uuid", C.c_int32),
        ("albedo", d3),
        ("fuzz", C.c_float),
        ("refraction_index", C.c_float),
    ]


class PtCenterHit(C.Structure):
    _fields_ = [
        ("t", C.c_double),
        ("hit_point", d3),
        ("normal", d3),
        ("front_face", C.c_int32),
        ("uuid", C.c_int32),
    ]


class PtStateView(C.Structure):
    """Snapshot of the reference's State (src/state.rs:31-94), f64 like the original."""

    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("samples_per_pixel", C.c_uint32), ("max_depth", C.c_uint32),
        ("aspect_ratio", C.c_double),
        ("camera_origin", d3), ("camera_front", d3), ("vup", d3),
        ("yaw", C.c_double), ("pitch", C.c_double), ("camera_field_of_view", C.c_double),
        ("u", d3), ("v", d3), ("w", d3),
        ("aperture", C.c_double), ("lens_radius", C.c_double), ("focus_distance", C.c_double),
        ("viewport_height", C.c_double), ("viewport_width", C.c_double),
        ("horizontal", d3), ("vertical", d3), ("lower_left_corner", d3),
        ("cursor_point", d3),
        ("selected_object", C.c_int32),
        ("is_paused", C.c_int32), ("should_average", C.c_int32), ("should_render", C.c_int32),
        ("even_odd_count", C.c_uint32), ("render_count", C.c_uint32), ("max_render_count", C.c_uint32),
        ("last_frame_weight", C.c_float),
        ("n_spheres", C.c_uint32),
    ]


KEY_W, KEY_A, KEY_S, KEY_D, KEY_SPACE, KEY_SHIFT = 1, 2, 4, 8, 16, 32


def spheres_as_ctypes(spheres):
    """numpy SPHERE_DTYPE array (or PtSphere ctypes array) -> (PtSphere pointer, n, keepalive)."""
    if isinstance(spheres, np.ndarray):
        arr = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        return arr.ctypes.data_as(C.POINTER(PtSphere)), int(arr.shape[0]), arr
    n = len(spheres)
    return C.cast(spheres, C.POINTER(PtSphere)), n, spheres


def local_rows(height, band_rows, band_index, band_count):
    """Rows y in [0,height) with (y // band_rows) % band_count == band_index (include/ptrace.h)."""
    if band_count <= 1 or band_rows == 0:
        return int(height)
    full, rem = divmod(int(height), band_rows * band_count)
    n = full * band_rows
    lo = band_index * band_rows
    n += max(0, min(rem - lo, band_rows))
    return n


def owned_rows(height, band_rows, band_index, band_count):
    """Ascending global row indices owned by band_index."""
    ys = np.arange(height, dtype=np.int64)
    if band_count <= 1 or band_rows == 0:
        return ys
    return ys[(ys // band_rows) % band_count == band_index]
