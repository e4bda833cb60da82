"""The first-hit feature planes (PT_OPT_FEATURES, pt_render_features; include/ptrace.h has the record) on the device, bit
for bit.

Every comparison is equal uint32 views of all four planes against tests/feature_ref.py — the contract restated from the
oracle's exported pieces, itself pinned to ora_first_hit_map by tests/test_feature_ref.py — or, where a frame is too large
for a per-pixel Python loop, of the ids plane against ora_first_hit_map and of all four planes against the scalar walk's
on the same context.  Tolerance: none.

  (a) every row      each of the twelve kernels of csrc/pt_kernels_features.hip, reached the way the overlay tests reach
                     their namesakes, at 37x21 (edge tiles, out-of-image lanes); a forced PT_GEOM_LDS goes through the
                     scalar walk; the walk kernels once more at 200x120 against the scalar walk
  (b) corners        one 16-sphere scene: a later twin wins, a negative radius, the camera inside glass, an emissive
                     sphere, a type of 7, uuids that are not indices, misses under both backgrounds
  (c) far, irregular a grid seen from outside its near region; a camera outside the regular range
  (d) bands          three bands of four rows put back with pt_band_row; a band without rows
  (e) pinhole        lens, time, samples per pixel and depth do not enter
  (f) undisturbed    accumulation, estimate, textures, canvas, first_pass, statistics; overlay and roulette do not act
  (g) validity       every PT_ERR_* case of the header, every invalidating call, reallocation on resize
  (h) full size      1280x702 (the refill runs), 960x540, config 5 at 1920x1080 on the grid pt_tune kept
"""
import ctypes as C

import numpy as np
import pytest

import feature_ref as F
import overlay_ref as R
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer, PtError
from test_gpu_fuzz import random_scene
from trace_builds import build_of

pytestmark = pytest.mark.gpu

PLANES = ("albedo", "normal", "point", "ids")
KERNELS = ["small_t0_feat", "small_t1_feat", "small_t2_feat", "small_t3_feat", "scalar_feat", "scalar_nolds_feat", "bvh_feat",
           "bvh_nodes_feat", "bvh_gmem_feat", "grid_feat", "grid_cells_feat", "grid_gmem_feat"]
REACHED = {}
W, H = 37, 21


def assert_planes_equal(got, ref, what):
    for k in PLANES:
        g, r = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
        assert got[k].dtype == (np.int32 if k == "ids" else np.float32), (what, k, got[k].dtype)
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        if not np.array_equal(g, r):
            bad = np.argwhere(g != r)
            raise AssertionError("%s, plane %s: %d of %d values differ, first at %s: %r vs %r" % (
                what, k, len(bad), g.size, tuple(bad[0]), got[k][tuple(bad[0])], ref[k][tuple(bad[0])]))


def kernel_of(t, path):
    """the feature kernel a launch through the forced `path` is (kTraceKernels of csrc/pt_trace_table.hpp, by row)"""
    assert t.last_trace_build() == abi.BUILD_FEATURES
    st = t.stats()
    if path == abi.PT_GEOM_AUTO:
        raise AssertionError("features through geometry path %d" % path)
    # (a feature launch leaves PtStats.geometry_path as it finds it; PT_GEOM_LDS is steered to the scalar row)
    return build_of(st, "_feat", path=abi.PT_GEOM_SCALAR if path == abi.PT_GEOM_LDS else path)


def context(sph, p, path=None, features=True):
    t = PathTracer(p.width, p.height)
    if path is not None:
        t.set_geometry_path(path)
    t.set_spheres(sph)
    if features:
        t.feature_planes(True)
    t.set_params(p)
    return t


def render(t):
    """one feature launch and its read-out; the segments it added"""
    before = t.stats().segments
    t.render_features()
    out = t.features()
    return out, t.stats().segments - before


def resized(p, w, h):
    q = p.copy()
    q.width, q.height = w, h
    return q


# ---------------------------------------------------------------------------------------------- the scenes, made once
_SCENES = {}


def scene(name):
    """(spheres, params at 37x21): small<n> — a random list of n spheres; cover — 484 spheres, a one-layer grid; field<n> — a
    random field on a ground, several layers of cells, uuids that are not indices"""
    if name not in _SCENES:
        if name.startswith("small"):
            n = int(name[5:])
            # (seeds whose frames show five or more different spheres and misses, found by looking at the restatement's planes)
            sc = random_scene(np.random.default_rng(91000 + 100 * n + {9: 36, 10: 21, 11: 34, 12: 16}[n]), n, W, H, 2, 8, 1)
            sc.spheres["uuid"] = (50 + 11 * np.arange(n)).astype(np.int32)
            _SCENES[name] = (sc.spheres, sc.params)
        elif name == "cover":
            sc = scenes.config2(W, H, 1, 1, 8)
            _SCENES[name] = (sc.spheres, sc.params)
        else:
            c = R.field_case(int(name[5:]), W, H, True)
            _SCENES[name] = (c.spheres, c.params)
    return _SCENES[name]


_REFS = {}


def reference(name):
    if name not in _REFS:
        sph, p = scene(name)
        _REFS[name] = F.planes(sph, p)
    return _REFS[name]


# ------------------------------------------------------------------------------------------------ (a) every row
ROWS = [
    ("small_t1_feat", "small9", abi.PT_GEOM_SMALL), ("small_t2_feat", "small10", abi.PT_GEOM_SMALL),
    ("small_t3_feat", "small11", abi.PT_GEOM_SMALL), ("small_t0_feat", "small12", abi.PT_GEOM_SMALL),
    ("scalar_feat", "cover", abi.PT_GEOM_SCALAR), ("scalar_nolds_feat", "field12000", abi.PT_GEOM_SCALAR),
    ("scalar_feat", "cover", abi.PT_GEOM_LDS),  # forced to the LDS list walk: through the scalar walk, as with roulette
    ("bvh_feat", "cover", abi.PT_GEOM_BVH), ("bvh_nodes_feat", "field3000", abi.PT_GEOM_BVH), ("bvh_gmem_feat", "field20000", abi.PT_GEOM_BVH),
    ("grid_feat", "cover", abi.PT_GEOM_GRID),      # a one-layer grid, walked along three axes
    ("grid_feat", "field1500", abi.PT_GEOM_GRID),  # several layers
    ("grid_cells_feat", "field10000", abi.PT_GEOM_GRID), ("grid_gmem_feat", "field60000", abi.PT_GEOM_GRID),
]
ROW_IDS = ["%s-%s-%s" % (k, s, abi.GEOM_NAMES[p]) for k, s, p in ROWS]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_every_row_of_the_kernel_table(row):
    kernel, name, path = row
    sph, p = scene(name)
    ref = reference(name)
    t = context(sph, p, path)
    try:
        got, seg = render(t)
        st = t.stats()
        assert kernel_of(t, path) == kernel, (kernel, kernel_of(t, path), st.n_spheres, st.bvh_nodes, st.bvh_slots, st.grid_kernel_build)
        if path == abi.PT_GEOM_GRID:
            assert (st.grid_cells[1] == 1) == (name == "cover"), (name, list(st.grid_cells))
        assert_planes_equal(got, ref, "%s through %s" % (name, kernel))
        assert seg == W * H, (kernel, seg)
        hit = ref["ids"][..., 0] >= 0
        assert hit.any() and len(np.unique(ref["ids"][..., 0])) >= 5, "the case shows hits on several spheres"
        REACHED.setdefault(kernel, []).append("%s/%s" % (name, abi.GEOM_NAMES[path]))
    finally:
        t.close()


def test_every_feature_kernel_was_reached():
    """(runs after the test above) each of the twelve kernels of csrc/pt_kernels_features.hip was launched and compared"""
    print("feature kernels reached\n" + "\n".join("  %-18s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in KERNELS))
    assert sorted(REACHED) == sorted(KERNELS), sorted(set(KERNELS) - set(REACHED))


WALKS = [r for r in ROWS if r[2] in (abi.PT_GEOM_BVH, abi.PT_GEOM_GRID)]


@pytest.mark.parametrize("row", WALKS, ids=["%s-%s" % (k, s) for k, s, _ in WALKS])
def test_walk_kernels_equal_the_scalar_walk_at_200x120(row):
    """more than one workgroup's worth of tiles, carried stragglers: GPU against GPU on one context"""
    kernel, name, path = row
    sph, p37 = scene(name)
    p = (scenes.config2(200, 120, 1, 1, 8) if name == "cover" else R.field_case(int(name[5:]), 200, 120, True)).params
    t = context(sph, p, path)
    try:
        got, seg = render(t)
        assert kernel_of(t, path) == kernel and seg == 200 * 120
        t.set_geometry_path(abi.PT_GEOM_SCALAR)
        want, seg = render(t)
        assert kernel_of(t, abi.PT_GEOM_SCALAR).startswith("scalar") and seg == 200 * 120
        assert_planes_equal(got, want, "%s against the scalar walk" % kernel)
        idx = want["ids"][..., 0]
        assert (idx >= 0).any() and len(np.unique(idx)) >= 8
        assert np.array_equal(want["ids"][..., 1][idx >= 0], sph["uuid"][idx[idx >= 0]])
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (b) corners
def corner_scene():
    D, M, G, E = abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS, abi.PT_EMISSIVE
    items = [
        ((0.0, -100.5, -1.0), 100.0, D, (0.8, 0.8, 0.0)),
        ((0.0, 0.0, -1.0), 0.5, D, (0.7, 0.3, 0.3)),
        ((-1.2, 0.0, -1.2), 0.4, M, (0.8, 0.8, 0.8)),    # 2, 3: the same sphere twice — the later one wins every tie
        ((-1.2, 0.0, -1.2), 0.4, G, (0.25, 0.5, 0.75)),
        ((1.2, 0.0, -1.2), -0.4, G, (1.0, 1.0, 1.0)),    # 4: a negative radius flips the normal: front_face 0 from outside
        ((0.0, 1.1, -1.5), 0.3, E, (4.0, 5.0, 6.0)),     # 5: emissive, albedo above 1
        ((0.45, -0.3, -0.3), 0.15, 7, (0.1, 0.2, 0.3)),  # 6: a type nothing recognises
        ((3.0, 0.5, 2.0), 0.8, G, (0.9, 0.95, 1.0)),     # 7: the glass sphere the second camera sits in
    ]
    rng = np.random.default_rng(92016)
    for k in range(8):
        items.append(((float(rng.uniform(-1.6, 1.6)), float(rng.uniform(-0.4, 0.9)), float(rng.uniform(-2.5, -0.2))), float(rng.uniform(0.08, 0.2)),
                      [D, M, G][k % 3], tuple(float(x) for x in rng.uniform(0.1, 1.0, 3))))
    sph = np.zeros(len(items), dtype=abi.SPHERE_DTYPE)
    for i, (c, r, ty, a) in enumerate(items):
        sph[i]["center"], sph[i]["radius"], sph[i]["type"], sph[i]["albedo"] = c, r, ty, a
        sph[i]["fuzz"], sph[i]["refraction_index"] = 0.1, 1.5
    sph["uuid"] = (1000 - 13 * np.arange(len(items))).astype(np.int32)  # not indices, not ascending
    assert len(sph) == 16
    return sph


_CORNER = {}


def corner_case(camera, background):
    key = (camera, background)
    if key not in _CORNER:
        sph = corner_scene()
        if camera == "outside":
            p = R.look_at(W, H, 1, 8, (0.1, 0.35, 1.6), (0.0, 0.1, -1.0), 62.0, 1.0, background)
        else:
            p = R.look_at(W, H, 1, 8, (3.1, 0.45, 2.05), (0.0, 0.2, -1.0), 50.0, 1.0, background)
        _CORNER[key] = (sph, p, F.planes(sph, p))
    return _CORNER[key]


def test_the_corner_scene_shows_its_corners():
    """(CPU arithmetic only, but it says what the GPU comparison below is worth)"""
    sph, p, ref = corner_case("outside", abi.PT_BG_SKY)
    ids = ref["ids"]
    idx = ids[..., 0]
    assert (idx == 3).any() and not (idx == 2).any()                     # the later twin
    assert (idx == 4).any() and (ids[..., 3][idx == 4] == 0).all()        # the negative radius
    assert (ids[..., 3][idx == 1] == 1).all() and (idx == 1).any()
    assert (ids[..., 2] == 7).any() and (ids[..., 2] == abi.PT_EMISSIVE).any()
    assert (ref["albedo"][..., :3][idx == 5] == np.float32([4, 5, 6])).all()
    assert (idx < 0).any() and (ref["albedo"][..., 2][idx < 0] > 0.9).all()  # sky
    assert np.array_equal(ids[..., 1][idx >= 0], sph["uuid"][idx[idx >= 0]])
    _, _, black = corner_case("outside", abi.PT_BG_BLACK)
    assert not black["albedo"][idx < 0].view(np.uint32).any() and np.array_equal(black["ids"], ids)
    _, _, inside = corner_case("inside", abi.PT_BG_SKY)
    assert (inside["ids"][..., 0] == 7).all() and (inside["ids"][..., 3] == 0).all()  # the camera inside glass


@pytest.mark.parametrize("path", [abi.PT_GEOM_SMALL, abi.PT_GEOM_SCALAR, abi.PT_GEOM_BVH, abi.PT_GEOM_GRID], ids=lambda v: abi.GEOM_NAMES[v])
def test_the_hit_records_corners(path):
    t = None
    try:
        for camera, background in (("outside", abi.PT_BG_SKY), ("outside", abi.PT_BG_BLACK), ("inside", abi.PT_BG_SKY)):
            sph, p, ref = corner_case(camera, background)
            if t is None:
                t = context(sph, p, path)
            else:
                t.set_params(p)
            got, seg = render(t)
            assert_planes_equal(got, ref, "corner scene, camera %s, background %d, path %s" % (camera, background, abi.GEOM_NAMES[path]))
            assert seg == W * H
        st = t.stats()
        assert st.n_spheres == 16 and (path not in (abi.PT_GEOM_BVH, abi.PT_GEOM_GRID) or (st.bvh_nodes > 0 and st.grid_entries > 0))
    finally:
        if t is not None:
            t.close()


# ------------------------------------------------------------------------------------------------ (c) far and irregular rays
@pytest.mark.parametrize("name", ["field1500", "field10000"])
def test_far_rays_of_a_grid_seen_from_outside_its_near_region(name):
    """no refit: every primary ray that reaches the grid is handed over whole, to the wave-wide look of the build that gathers
    its entries — which is what a stale fit launches, also where the entries would fit the LDS (csrc/pt_geom_plan.hpp
    grid_staging)"""
    sph, _ = scene(name)
    c = sph["center"].astype(np.float64)
    mid, ext = c[1:].mean(axis=0), float(np.abs(c[1:] - c[1:].mean(axis=0)).max())
    p = R.look_at(W, H, 1, 8, mid + np.array([60.0, 15.0, 60.0]) * ext / 4.0, mid, 8.0, 100.0)
    ref = F.planes(sph, p)
    assert (ref["ids"][..., 0] >= 0).mean() > 0.5
    t = context(sph, p, abi.PT_GEOM_GRID)
    try:
        far0 = t.stats().far_rays
        got, seg = render(t)
        st = t.stats()
        # (PtStats.far_rays counts the rays handed over: those that reach the grid's box — most of this frame sees the ground,
        # which is tested for every ray and lies outside it)
        assert st.grid_fit_stale == 1 and st.far_rays - far0 > 0, (st.grid_fit_stale, st.far_rays - far0)
        assert kernel_of(t, abi.PT_GEOM_GRID) == "grid_cells_feat"
        assert_planes_equal(got, ref, "%s from far outside" % name)
    finally:
        t.close()


@pytest.mark.parametrize("path", [abi.PT_GEOM_SMALL, abi.PT_GEOM_SCALAR, abi.PT_GEOM_BVH, abi.PT_GEOM_GRID], ids=lambda v: abi.GEOM_NAMES[v])
def test_irregular_rays_take_the_literal_loop(path):
    """every ray irregular (csrc/pt_list.hpp regular_ray): directions 2 000 long (|d|^2 >= 1e6, the scene's own view, so the
    rays hit what they always hit), and tests/test_gpu_parity.py's camera outside the regular range (they all miss)"""
    if path == abi.PT_GEOM_SMALL:
        sph = scenes.default_scene(W, H, spp=1, max_depth=8).spheres
        long_d = R.look_at(W, H, 1, 8, (0.1, 0.2, 1.0), (-0.3, 0.0, -1.0), 60.0, 2000.0)
    else:
        sph = scene("cover")[0]
        long_d = R.look_at(W, H, 1, 8, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 2000.0)
    outside = scene("cover")[1].copy()
    outside.camera_origin[0] = 3e15
    t = None
    try:
        for what, p in (("long directions", long_d), ("a camera at 3e15", outside)):
            ref = F.planes(sph, p)
            hits = (ref["ids"][..., 0] >= 0).mean()
            assert (hits > 0.5 and len(np.unique(ref["ids"][..., 0])) >= 5) if p is long_d else hits == 0
            if t is None:
                t = context(sph, p, path)
            else:
                t.set_params(p)
            got, seg = render(t)
            assert_planes_equal(got, ref, "%s through %s" % (what, abi.GEOM_NAMES[path]))
            assert seg == W * H
    finally:
        if t is not None:
            t.close()


# ------------------------------------------------------------------------------------------------ (d) bands
def test_three_bands_put_back_with_pt_band_row(lib):
    sph, p = scene("cover")
    whole = reference("cover")
    full = context(sph, p, abi.PT_GEOM_GRID)
    try:
        got_whole, _ = render(full)
        assert_planes_equal(got_whole, whole, "the full-height context")
    finally:
        full.close()
    back = {k: np.zeros_like(whole[k]) for k in PLANES}
    total = 0
    for r in range(3):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, r, 3
        t = context(sph, q, abi.PT_GEOM_GRID)
        try:
            got, seg = render(t)
            n = lib.pt_local_rows(H, 4, r, 3)
            assert got["ids"].shape == (n, W, 4) and seg == n * W
            assert_planes_equal(got, F.planes(sph, q), "band %d of 3 against the banded restatement" % r)
            for l in range(n):
                y = lib.pt_band_row(4, r, 3, l)
                for k in PLANES:
                    back[k][y] = got[k][l]
            total += n
        finally:
            t.close()
    assert total == H
    assert_planes_equal(back, got_whole, "three bands put back against the full-height context")


def test_a_band_without_rows_has_nothing_to_do():
    sph, p = scene("cover")
    q = p.copy()
    q.band_rows, q.band_index, q.band_count = 4, 7, 8  # 21 rows are six chunks of four: ranks 6 and 7 own none
    t = context(sph, q, abi.PT_GEOM_GRID)
    try:
        assert t.local_rows == 0
        got, seg = render(t)
        assert seg == 0 and all(got[k].shape == (0, W, 4) for k in PLANES)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (e) pinhole by definition
def test_lens_time_samples_and_depth_do_not_enter():
    sph, p = scene("cover")
    ref = reference("cover")
    q = p.copy()
    q.lens_radius, q.time, q.time_step, q.first_pass, q.samples_per_pixel, q.max_depth = 0.3, 117.0, 0.5, 9, 7, 3
    for path in (abi.PT_GEOM_SCALAR, abi.PT_GEOM_GRID):
        t = context(sph, q, path)
        try:
            got, seg = render(t)
            assert_planes_equal(got, ref, "lens 0.3, time 117, 7 spp, depth 3 through %s" % abi.GEOM_NAMES[path])
            assert seg == W * H
        finally:
            t.close()


# ------------------------------------------------------------------------------------------------ (f) nothing is disturbed
def test_the_accumulation_and_the_estimate_do_not_notice():
    sc = scenes.default_scene(96, 54, spp=2, max_depth=8)
    p = sc.params.copy()
    p.time_step, p.first_pass = abi.PT_TIME_STEP_DECORRELATED, 3
    k = 2
    out = []
    for with_features in (True, False):
        t = context(sc.spheres, p, abi.PT_GEOM_SMALL, features=with_features)
        try:
            t.error_estimate(True)
            t.reserve_passes(k)
            t.reset()
            t.render_passes(k)
            if with_features:
                before = t.stats()
                t.render_features()
                after = t.stats()
                assert t.last_trace_build() == abi.BUILD_FEATURES
                assert after.segments - before.segments == 96 * 54
                assert (after.samples, after.total_spp, after.render_launches) == (before.samples, before.total_spp, before.render_launches)
                assert after.geometry_path == before.geometry_path and after.geometry_tuned == before.geometry_tuned
            t.render_passes(k)  # (the same first_pass: had the feature launch moved it, these passes would differ)
            assert t.last_trace_build() == abi.BUILD_PLAIN
            st = t.stats()
            out.append((t.accum(), t.error_state(), st.samples, st.total_spp, st.render_launches, st.segments))
            if with_features:
                assert_planes_equal(t.features(), F.planes(sc.spheres, p), "features between two launches of passes")
        finally:
            t.close()
    a, b = out
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "accumulation"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "estimate state"
    assert a[2:5] == b[2:5] and a[5] == b[5] + 96 * 54
    assert (a[0][..., 3] == 2 * k * 2).all()


def test_canvas_and_textures_do_not_notice():
    sc = scenes.default_scene(96, 54, spp=2, max_depth=8)
    p = sc.params.copy()
    p.render_count, p.should_average, p.last_frame_weight = 1, 1, 1.0
    out = []
    for with_features in (True, False):
        t = context(sc.spheres, p, abi.PT_GEOM_SMALL, features=with_features)
        try:
            t.clear_textures()
            t.render_frame(1)
            if with_features:
                held = (t.read_canvas(), t.read_texture(0), t.read_texture(1))
                t.render_features()
                now = (t.read_canvas(), t.read_texture(0), t.read_texture(1))
                assert all(np.array_equal(x, y) for x, y in zip(held, now))
                assert held[0].any()
            q = p.copy()
            q.render_count, q.first_pass = 2, 1
            t.set_params(q)
            t.render_frame(2)
            out.append((t.read_canvas(), t.read_texture(0), t.read_texture(1)))
        finally:
            t.close()
    assert all(np.array_equal(x, y) for x, y in zip(*out))


def test_overlay_and_roulette_do_not_act():
    c = R.default_case()
    p = resized(c.params, 96, 54)
    t = context(c.spheres, p, abi.PT_GEOM_SMALL)
    try:
        plain, _ = render(t)
        assert_planes_equal(plain, F.planes(c.spheres, p), "plain")
        t.set_debug_overlay(True, *c.overlay)
        got, seg = render(t)
        assert t.last_trace_build() == abi.BUILD_FEATURES and seg == 96 * 54
        assert_planes_equal(got, plain, "with the overlay on")
        t.render_passes(1)
        assert t.last_trace_build() == abi.BUILD_DEBUG_OVERLAY
        t.set_debug_overlay(False)
        t.set_russian_roulette(2)
        got, seg = render(t)
        assert t.last_trace_build() == abi.BUILD_FEATURES and seg == 96 * 54
        assert_planes_equal(got, plain, "with roulette on")
        t.render_passes(1)
        assert t.last_trace_build() == abi.BUILD_ROULETTE
    finally:
        t.close()


def test_an_unsettled_auto_context_uses_its_cold_path_and_measures_nothing():
    sph, p = scene("small9")
    t = context(sph, p)  # PT_GEOM_AUTO, nothing rendered yet
    try:
        st0 = t.stats()
        got, seg = render(t)
        st = t.stats()
        assert (st.geometry_tuned, st.geometry_path) == (st0.geometry_tuned, st0.geometry_path) and st0.geometry_tuned == 0
        assert_planes_equal(got, reference("small9"), "unsettled PT_GEOM_AUTO")
    finally:
        t.close()


def test_torch_views_of_the_device_planes():
    import torch

    sph, p = scene("cover")
    t = PathTracer(W, H, use_torch=True)
    try:
        t.set_spheres(sph)
        t.feature_planes(True)
        t.set_params(p)
        t.render_features()
        views = t.features()
        assert all(v.is_cuda and tuple(v.shape) == (H, W, 4) for v in views.values())
        assert views["ids"].dtype == torch.int32 and views["albedo"].dtype == torch.float32
        assert_planes_equal({k: v.cpu().numpy() for k, v in views.items()}, reference("cover"), "torch views")
        picked = int(views["ids"][H // 2, W // 2, 1])  # a device pick is IDS[y][x]
        assert picked == int(reference("cover")["ids"][H // 2, W // 2, 1])
        torch.cuda.synchronize()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (g) validity and errors
def _rc_read(t, plane=abi.PT_FEAT_IDS):
    buf = np.zeros((max(t.local_rows, 1), t.width, 4), np.int32)
    return t.lib.pt_read_features(t._ctx, plane, buf.ctypes.data_as(C.c_void_p))


def _rc_ptr(t, plane=abi.PT_FEAT_IDS):
    ptr, n = C.c_void_p(), C.c_size_t()
    return t.lib.pt_features_ptr(t._ctx, plane, C.byref(ptr), C.byref(n)), ptr.value, n.value


def test_errors_of_the_three_entry_points():
    sph, p = scene("cover")
    t = PathTracer(W, H)
    lib = t.lib
    try:
        assert lib.pt_render_features(t._ctx) == abi.PT_ERR_NOT_READY and b"pt_set_spheres" in lib.pt_last_error(t._ctx)
        t.set_spheres(sph)
        assert lib.pt_render_features(t._ctx) == abi.PT_ERR_NOT_READY  # no uniforms yet
        t.set_params(p)
        assert lib.pt_render_features(t._ctx) == abi.PT_ERR_NOT_READY and b"PT_OPT_FEATURES" in lib.pt_last_error(t._ctx)
        assert _rc_read(t) == abi.PT_ERR_NOT_READY and _rc_ptr(t)[0] == abi.PT_ERR_NOT_READY
        assert lib.pt_set_option(t._ctx, abi.PT_OPT_FEATURES, 2) == abi.PT_ERR_INVALID
        t.feature_planes(True)
        rc, ptr, n = _rc_ptr(t, abi.PT_FEAT_ALBEDO)
        assert rc == abi.PT_OK and ptr and n == W * H * 16
        assert [_rc_ptr(t, k)[1] - ptr for k in range(4)] == [k * n for k in range(4)]  # one allocation, plane k at k * local pixels
        assert _rc_read(t) == abi.PT_ERR_NOT_READY  # planes, but nothing rendered into them yet
        for plane in (-1, abi.PT_FEAT_PLANES):
            assert _rc_ptr(t, plane)[0] == abi.PT_ERR_INVALID and _rc_read(t, plane) == abi.PT_ERR_INVALID
        assert lib.pt_features_ptr(t._ctx, 0, None, None) == abi.PT_ERR_INVALID and lib.pt_read_features(t._ctx, 0, None) == abi.PT_ERR_INVALID
        t.render_features()
        assert _rc_read(t) == abi.PT_OK
        t.set_count_work(True)
        assert lib.pt_render_features(t._ctx) == abi.PT_ERR_INVALID and b"COUNT_WORK" in lib.pt_last_error(t._ctx)
        assert _rc_read(t) == abi.PT_ERR_INVALID
        t.set_count_work(False)
        assert _rc_read(t) == abi.PT_OK
    finally:
        t.close()


def test_a_call_inside_a_stream_capture_is_refused():
    import torch

    sph, p = scene("cover")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = PathTracer(W, H, use_torch=True)  # binds the side stream as its launch stream
        t.set_spheres(sph)
        t.feature_planes(True)
        t.set_params(p)
        t.render_features()
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        buf = torch.zeros((H, W, 4), dtype=torch.int32, device="cuda")
        with torch.cuda.graph(g, stream=side):
            rc_render = t.lib.pt_render_features(t._ctx)
            rc_read = t.lib.pt_read_features(t._ctx, abi.PT_FEAT_IDS, C.c_void_p(buf.data_ptr()))
            t.render_passes(1)  # (something to capture)
    assert rc_render == abi.PT_ERR_INVALID and rc_read == abi.PT_ERR_INVALID
    torch.cuda.synchronize()
    assert_planes_equal({k: v.cpu().numpy() for k, v in t.features().items()}, reference("cover"), "the planes rendered before the capture")
    t.close()


def test_what_ends_the_planes_validity_and_what_restores_it():
    sph, p = scene("cover")
    ref = reference("cover")
    t = context(sph, p, abi.PT_GEOM_GRID)

    def stale_then_fresh(what, want):
        assert _rc_read(t) == abi.PT_ERR_NOT_READY, what
        assert _rc_ptr(t)[0] == abi.PT_OK and _rc_ptr(t)[2] == t.local_rows * t.width * 16, what  # the pointer keeps answering
        got, seg = render(t)
        assert_planes_equal(got, want, "rendered again after " + what)
        assert _rc_read(t) == abi.PT_OK

    try:
        got, _ = render(t)
        assert_planes_equal(got, ref, "first render")
        t.set_spheres(sph)
        stale_then_fresh("pt_set_spheres", ref)
        t.set_params(p)
        stale_then_fresh("pt_set_params", ref)
        t.feature_planes(False)
        assert _rc_read(t) == abi.PT_ERR_NOT_READY and _rc_ptr(t)[0] == abi.PT_ERR_NOT_READY
        t.feature_planes(True)
        stale_then_fresh("the option off and on", ref)
        for w, h in ((20, 11), (64, 40)):  # a smaller and a larger frame: the planes are reallocated for the new rows
            assert t.lib.pt_resize(t._ctx, w, h) == abi.PT_OK
            t.width, t.height = w, h
            assert _rc_read(t) == abi.PT_ERR_NOT_READY, "pt_resize"
            assert t.lib.pt_render_features(t._ctx) == abi.PT_ERR_NOT_READY  # uniforms of the new size must come first
            q = scenes.config2(w, h, 1, 1, 8).params
            t.set_params(q)
            stale_then_fresh("pt_resize to %dx%d" % (w, h), F.planes(sph, q))
        # a repartition reallocates too
        q = scenes.config2(64, 40, 1, 1, 8).params
        q.band_rows, q.band_index, q.band_count = 8, 1, 2
        t.set_params(q)
        stale_then_fresh("a repartition", F.planes(sph, q))
        # pt_refit_grid when it rebuilds: the camera moves out of the grid's near region
        far = R.look_at(64, 40, 1, 8, (48.0, 8.0, 11.0), (0.0, 0.0, 0.0), 16.0, 40.0)
        t.set_params(far)
        want = F.planes(sph, far)
        stale_then_fresh("pt_set_params (far camera)", want)
        near0 = t.stats().grid_near_factor
        assert t.stats().grid_fit_stale == 1
        t.refit_grid(False)
        assert t.stats().grid_near_factor != near0, "the refit rebuilt the grid"
        stale_then_fresh("pt_refit_grid", want)
        t.refit_grid(False)  # nothing to rebuild: the planes still speak
        assert _rc_read(t) == abi.PT_OK
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (h) full size
@pytest.mark.parametrize("name", ["default", "cover"])
def test_full_size_ids_equal_the_first_hit_map(name):
    """1280x702: more items than resident lanes, so lanes are refilled within the launch"""
    sc = scenes.default_scene(1280, 702, spp=1, max_depth=8) if name == "default" else scenes.config2(960, 540, 1, 1, 8)
    p = sc.params
    want = F.first_hit_map(sc.spheres, p)
    t = context(sc.spheres, p)
    try:
        got, seg = render(t)
        assert seg == p.width * p.height
        ids = got["ids"]
        assert np.array_equal(ids[..., 1], want)
        hit = want >= 0
        assert np.array_equal(sc.spheres["uuid"][ids[..., 0][hit]], want[hit]) and (ids[..., 0][~hit] == -1).all()
        assert np.array_equal(got["albedo"][..., :3][hit], sc.spheres["albedo"][ids[..., 0][hit]])
        assert (got["albedo"][..., 3][hit] > 0).all() and not got["normal"][~hit].view(np.uint32).any()
    finally:
        t.close()


def test_config5_on_the_grid_pt_tune_kept_equals_the_scalar_walk():
    sc = scenes.config5(1920, 1080, 1, 1, 8)
    t = context(sc.spheres, sc.params)
    try:
        t.tune(1)
        st = t.stats()
        assert st.geometry_tuned == 1 and st.geometry_path == abi.PT_GEOM_GRID
        got, seg = render(t)
        assert seg == 1920 * 1080 and kernel_of(t, abi.PT_GEOM_GRID) in ("grid_cells_feat", "grid_gmem_feat")
        t.set_geometry_path(abi.PT_GEOM_SCALAR)
        want, seg = render(t)
        assert seg == 1920 * 1080
        assert_planes_equal(got, want, "config 5 through the tuned grid against the scalar walk")
        idx = want["ids"][..., 0]
        assert (idx >= 0).mean() > 0.5 and len(np.unique(idx)) > 1000
    finally:
        t.close()
