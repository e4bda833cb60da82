"""Russian roulette (PT_OPT_RUSSIAN_ROULETTE), every kernel build, bit for bit.

The reference has no roulette, so for a long time this mode was only checked statistically (tests/test_gpu_roulette.py: the
EXPECTATION is kept).  The step itself is a few lines of plain fp32 (csrc/pt_shade.hpp), restated in the CPU oracle
(oracle/pt_oracle.c roulette_step, pinned by tests/test_oracle_roulette.py) — so each of the twelve roulette kernels of
csrc/pt_kernels_extra.hip is held to the standard of every other kernel here: equal uint32 views of the accumulation buffer
(NaNs by bit pattern) and equal segment counts, tolerance none.

  (a) same walk       k = max_depth and k = 1 000 000: the step is never reached, the build must be its namesake's walk —
                      the oracle WITHOUT roulette;
  (b) same roulette   k in {1, 3, max_depth - 1}: the oracle with that k.  Several passes in one launch and one pass per
                      launch, PT_TIME_STEP_DECORRELATED, lens on, and one row band against the oracle's banded render;
  (c) one-layer grid  pt_trace_kernel_grid_rr walks three axes where the plain kernel walks two;
  (d) scheduling      PT_OPT_CARRY_LANES / PT_OPT_REFILL_MIN at their ends: roulette ends lanes early;
  (e) fuzz            random scenes through the small-list, hierarchy and grid builds, albedo 0, NaN albedo;
  (f) frames          pt_render_frame / pt_render_frames against the oracle's tick-by-tick simulation;
  (g) the LDS row     PT_GEOM_LDS + roulette renders through the scalar row, and returns to the LDS walk without it.
Which kernel a launch got is read from PtStats (geometry_path, list length, the sizes that decide what is staged in the LDS,
grid_kernel_build) and collected in REACHED; the last test fails if one of the twelve was never reached.
"""
import math
import os

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_fuzz import random_scene
from trace_builds import build_of

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(16, os.cpu_count() or 1)
K_MAX = 1000000  # the largest value pt_set_option accepts
KERNELS = ["small_t0_rr", "small_t1_rr", "small_t2_rr", "small_t3_rr", "scalar_rr", "scalar_nolds_rr", "bvh_rr", "bvh_nodes_rr",
           "bvh_gmem_rr", "grid_rr", "grid_cells_rr", "grid_gmem_rr"]
REACHED = {}  # kernel -> what was compared through it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (
            what, len(bad), g.size, tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(ref)[tuple(bad[0])]))


def kernel_of(st, roulette=True):
    """the roulette kernel the last launch of this context was (kTraceKernels of csrc/pt_trace_table.hpp, by row), from PtStats"""
    assert roulette
    if st.geometry_path == abi.PT_GEOM_LDS:
        raise AssertionError("roulette through geometry path %d: the LDS list walk has no roulette build" % st.geometry_path)
    return build_of(st, "_rr")  # (one roulette build serves a grid of one layer and of several)


def oracle(ora, sph, p, n_passes, k):
    return ora.render(sph, p, n_passes, nthreads=ORACLE_THREADS, roulette=k)


def gpu(t, p, k, n_passes, per_launch=None):
    """(accumulation, statistics) of n_passes passes with roulette k on a context that has its scene"""
    per_launch = per_launch or n_passes
    t.set_russian_roulette(k)
    t.set_params(p)
    t.reserve_passes(per_launch)
    t.reset()
    done = 0
    while done < n_passes:
        q = p.copy()
        q.first_pass = p.first_pass + done
        t.set_params(q)
        n = min(per_launch, n_passes - done)
        t.render_passes(n)
        done += n
    return t.accum(), t.stats()


def context(sph, w, h, path, **options):
    t = PathTracer(w, h)
    t.set_geometry_path(path)
    if "carry_lanes" in options:
        t.set_carry_lanes(options["carry_lanes"])
    if "refill_min" in options:
        t.set_refill_min(options["refill_min"])
    t.set_spheres(sph)
    return t


def with_lens_and_step(p):
    p = p.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    if p.lens_radius == 0.0:
        p.lens_radius = 0.03
    return p


def small_list(n, seed):
    return lambda: random_scene(np.random.default_rng(47000 + seed), n, 96, 54, 2, 8, 3)


def field(n, w=64, h=36):
    return lambda: scenes.config5(w, h, 2, 2, 8, n=n)


# (kernel, scene, forced geometry path): the scenes by which tests/test_gpu_parity.py reaches the plain builds
# (test_small_list_twin_and_remainder_builds_agree, test_sphere_list_beyond_lds_capacity, test_hierarchy_in_global_memory,
# test_grid_kernels_for_scenes_beyond_the_lds, test_grid_in_global_memory), at sizes whose WHOLE frame the oracle renders
BUILDS = [
    ("small_t0_rr", small_list(12, 3), abi.PT_GEOM_SMALL),
    ("small_t1_rr", small_list(9, 0), abi.PT_GEOM_SMALL),
    ("small_t2_rr", small_list(10, 1), abi.PT_GEOM_SMALL),
    ("small_t3_rr", small_list(11, 2), abi.PT_GEOM_SMALL),
    ("scalar_rr", lambda: scenes.config2(96, 54, 2, 3, 8), abi.PT_GEOM_SCALAR),
    ("scalar_nolds_rr", field(12000), abi.PT_GEOM_SCALAR),
    ("bvh_rr", lambda: scenes.config2(96, 54, 2, 3, 8), abi.PT_GEOM_BVH),
    ("bvh_nodes_rr", field(3000), abi.PT_GEOM_BVH),
    ("bvh_gmem_rr", field(20000), abi.PT_GEOM_BVH),
    ("grid_rr", lambda: scenes.config2(96, 54, 2, 3, 8), abi.PT_GEOM_GRID),  # one layer of cells
    ("grid_rr", field(1500), abi.PT_GEOM_GRID),                                # several layers
    ("grid_cells_rr", field(10000), abi.PT_GEOM_GRID),
    ("grid_gmem_rr", field(60000), abi.PT_GEOM_GRID),
]


@pytest.mark.parametrize("case", BUILDS, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BUILDS)])
def test_every_roulette_build_equals_the_oracle(ora, case):
    kernel, make, path = case
    sc = make()
    sph, n_passes = sc.spheres, sc.n_passes
    p = with_lens_and_step(sc.params)
    w, h, depth = p.width, p.height, p.max_depth
    assert depth == 8 and n_passes >= 2
    t = context(sph, w, h, path)
    try:
        # (a) the same walk: roulette on, never reached
        plain, seg_plain = oracle(ora, sph, p, n_passes, 0)
        for k in (depth, K_MAX):
            got, st = gpu(t, p, k, n_passes)
            assert kernel_of(st) == kernel, (kernel, kernel_of(st), st.geometry_path, st.n_spheres, st.bvh_nodes, st.bvh_slots, st.grid_kernel_build)
            assert_bit_equal(got, plain, "%s, k = %d (inactive)" % (kernel, k))
            assert st.segments == seg_plain, (kernel, k, st.segments, seg_plain)
        # (b) the same roulette
        for k in (1, 3, depth - 1):
            ref, seg = oracle(ora, sph, p, n_passes, k)
            if k < depth - 1:  # the step is at work in this scene (few paths are still under way one bounce before the end)
                assert seg < seg_plain and not np.array_equal(bits(ref), bits(plain))
            if k == 3:
                full, seg_full = ref, seg
            got, st = gpu(t, p, k, n_passes)
            assert kernel_of(st) == kernel
            assert_bit_equal(got, ref, "%s, k = %d, %d passes in one launch" % (kernel, k, n_passes))
            assert st.segments == seg, (kernel, k, st.segments, seg)
            if k == 3:
                got, st = gpu(t, p, k, n_passes, per_launch=1)
                assert kernel_of(st) == kernel and st.render_launches == n_passes
                assert_bit_equal(got, ref, "%s, k = %d, one pass per launch" % (kernel, k))
                assert st.segments == seg, (kernel, k, st.segments, seg)
        if path == abi.PT_GEOM_GRID:
            assert st.grid_fit_stale != 1 and st.grid_walk_flat == (1 if st.grid_kernel_build == 1 and st.grid_cells[1] == 1 else 0)
    finally:
        t.close()
    # one row band of three, reassembled against the oracle's banded render: the middle band, and the segments of all three
    seg_bands = 0
    for r in range(3):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = 4, r, 3
        tb = context(sph, w, h, path)
        try:
            part, st = gpu(tb, q, 3, n_passes)
            assert kernel_of(st) == kernel
            ys = abi.owned_rows(h, 4, r, 3)
            assert part.shape[0] == len(ys)
            assert_bit_equal(part, full[ys], "%s, k = 3, band %d of 3 against the rows of the whole frame" % (kernel, r))
            if r == 1:
                ref, seg = oracle(ora, sph, q, n_passes, 3)
                assert_bit_equal(part, ref, "%s, k = 3, band 1 of 3 against the oracle's banded render" % kernel)
                assert st.segments == seg
            seg_bands += st.segments
        finally:
            tb.close()
    assert seg_bands == seg_full
    REACHED.setdefault(kernel, []).append("%d spheres, %dx%d" % (len(sph), w, h))


# ------------------------------------------------------------------------------------- (c) the one-layer grid
@pytest.mark.parametrize("factor", [3.0, 8.0])
def test_the_roulette_build_on_a_one_layer_grid_next_to_the_flat_walk(ora, factor):
    """A flat field: nx x 1 x nz cells.  Without roulette the launch is pt_trace_kernel_grid, the two-axis walk; with it
    pt_trace_kernel_grid_rr, which walks three axes on any grid.  Each against its oracle, at the default margin class and at
    a wide one (another d_near, other margins, other entries), on the same context."""
    from test_gpu_grid_classes import camera, need_factor
    from test_gpu_grid_flat import flat_field, unit
    from test_grid import build

    w, h = 96, 54
    sph = flat_field(400, 32, 12.0)
    rc, g = build(sph, near_factor=factor)
    assert rc == 0 and tuple(int(x) for x in g["n"])[1] == 1
    c0, s0 = g["c0"].astype(np.float64), float(g["s0"])
    rho = 0.98 * (factor / 1.01 - 1.0) * 0.9999 * s0
    assert need_factor(rho, s0) == factor
    t = context(sph, w, h, abi.PT_GEOM_GRID)
    try:
        t.set_grid_fit(True)  # the class the camera needs, unmeasured
        p = camera(w, h, 2, 8, c0, s0, rho, unit([0.15, 0.95, 0.27]))
        p.time_step = abi.PT_TIME_STEP_DECORRELATED
        t.set_params(p)
        t.reserve_passes(2)
        t.tune(1)
        for k in (2, 0, 7, 8):
            got, st = gpu(t, p, k, 2)
            assert st.geometry_path == abi.PT_GEOM_GRID and st.grid_near_factor == factor and st.grid_fit_stale == 0
            assert st.grid_cells[1] == 1 and st.grid_kernel_build == 1 and st.grid_walk_flat == 1
            ref, seg = oracle(ora, sph, p, 2, k if k < 8 else 0)
            assert_bit_equal(got, ref, "flat field, class %g, roulette %d" % (factor, k))
            assert st.segments == seg, (factor, k, st.segments, seg)
        REACHED.setdefault("grid_rr", []).append("flat field at class %g" % factor)
    finally:
        t.close()


# ------------------------------------------------------------------------------------- (d) scheduling only
@pytest.mark.parametrize("path", [abi.PT_GEOM_BVH, abi.PT_GEOM_GRID], ids=["hierarchy", "grid"])
def test_carry_lanes_and_refill_min_do_not_change_the_roulette_image(ora, path):
    """Roulette ends lanes early: waves run emptier, stragglers are carried and refills deferred in patterns the roulette-free
    kernels never see.  Scheduling only: lockstep or always carrying, refill at once or only for a whole wave — the same bits."""
    sc = scenes.config2(160, 90, 2, 2, 50)
    p = with_lens_and_step(sc.params)
    ref, seg = oracle(ora, sc.spheres, p, 2, 2)
    for carry, refill in ((0, 1), (64, 64), (0, 64), (64, 1)):
        t = context(sc.spheres, 160, 90, path, carry_lanes=carry, refill_min=refill)
        try:
            got, st = gpu(t, p, 2, 2)
            assert kernel_of(st) == ("bvh_rr" if path == abi.PT_GEOM_BVH else "grid_rr")
            assert_bit_equal(got, ref, "carry_lanes %d refill_min %d" % (carry, refill))
            assert st.segments == seg
        finally:
            t.close()


# ------------------------------------------------------------------------------------- (e) fuzz
def _fuzz_scene(which, seed):
    rng = np.random.default_rng({"small": 61000, "hierarchy": 62000, "grid": 63000}[which] + seed)
    n = int(rng.integers(1, 17)) if which == "small" else int(rng.choice([16, 17, 33, 40, 130, 400]))
    depth = int(rng.choice([3, 8, 50]))
    sc = random_scene(rng, n, int(rng.integers(9, 97)), int(rng.integers(5, 55)), int(rng.integers(1, 5)), depth, int(rng.integers(1, 3)))
    if which == "grid" and seed % 3 != 1:  # mostly small spheres, spread out: what a grid is for
        small = rng.random(n) < 0.9
        sc.spheres["radius"][small] = (np.sign(sc.spheres["radius"][small]) * rng.uniform(0.05, 0.4, small.sum())).astype(np.float32)
        sc.spheres["center"] *= np.float32(rng.choice([2.0, 6.0, 20.0]))
    if which == "grid" and seed % 4 == 0:  # a flat field: one layer of cells
        sc.spheres["center"][:, 1] = np.float32(0.3)
    if which == "hierarchy" and seed % 3 == 0:
        sc.spheres["center"] *= np.float32(rng.choice([4.0, 15.0]))
    k = int(rng.choice([1, 2] if depth == 3 else [1, 2, 3, 7]))
    return sc, k, int(rng.integers(1, sc.n_passes + 1))


@pytest.mark.parametrize("which,path", [("small", abi.PT_GEOM_SMALL), ("hierarchy", abi.PT_GEOM_BVH), ("grid", abi.PT_GEOM_GRID)],
                         ids=["small", "hierarchy", "grid"])
def test_random_scenes_with_roulette_bit_exact(ora, which, path):
    """tests/test_gpu_fuzz.py's scenes — duplicates, concentric and negative-radius spheres, every material, emissive albedo
    up to 8 (q clamps), cameras inside spheres, lens on and off — with roulette on: a dozen seeds through each family."""
    bad, through = [], 0
    for seed in range(12):
        sc, k, per_launch = _fuzz_scene(which, seed)
        t = context(sc.spheres, sc.params.width, sc.params.height, path)
        try:
            got, st = gpu(t, sc.params, k, sc.n_passes, per_launch=per_launch)
            ref, seg = oracle(ora, sc.spheres, sc.params, sc.n_passes, k)
            if which == "grid":  # a scene the grid cannot represent falls back to the hierarchy
                assert st.geometry_path in (abi.PT_GEOM_GRID, abi.PT_GEOM_BVH)
            else:
                assert st.geometry_path == path
            through += int(st.geometry_path == path)
            kernel_of(st)
            if not (np.array_equal(bits(got), bits(ref)) and st.segments == seg):
                bad.append((seed, len(sc.spheres), k, int((bits(got) != bits(ref)).sum()), int(st.segments), seg, int(st.geometry_path)))
        finally:
            t.close()
    assert not bad, bad
    assert through >= 9, through


@pytest.mark.parametrize("what", ["albedo 0", "NaN albedo"])
def test_black_and_nan_albedo_with_roulette(ora, what):
    """Albedo 0: q = 0 at the first decision after such a bounce, the path ends there.  A NaN channel: max ignores it, the
    other two decide q and the NaN is carried on; all three NaN: q = min(NaN, 1) = 1.  The cover scene with every third
    sphere (the ground among them) so changed, through the hierarchy and the grid; the reference's scene through its list."""
    value = 0.0 if what == "albedo 0" else float("nan")
    cover = scenes.config2(96, 54, 2, 2, 8)
    cover.spheres["albedo"][0::3, 0] = value
    cover.spheres["albedo"][0::6, 1:] = value
    nine = scenes.default_scene(96, 54, spp=2, max_depth=8, n_passes=2)
    nine.spheres["albedo"][0::2, 0] = value
    nine.spheres["albedo"][0, 1:] = value
    for sc, path in ((cover, abi.PT_GEOM_BVH), (cover, abi.PT_GEOM_GRID), (nine, abi.PT_GEOM_SMALL), (nine, abi.PT_GEOM_SCALAR)):
        p = with_lens_and_step(sc.params)
        t = context(sc.spheres, 96, 54, path)
        try:
            for k in (1, 3):
                got, st = gpu(t, p, k, 2)
                ref, seg = oracle(ora, sc.spheres, p, 2, k)
                assert st.geometry_path == path
                assert_bit_equal(got, ref, "%s, path %d, k = %d" % (what, path, k))
                assert st.segments == seg
                if what == "NaN albedo":
                    assert np.isnan(ref[..., :3]).any() and np.isfinite(ref[..., :3]).any()
        finally:
            t.close()


# ------------------------------------------------------------------------------------- (f) frames
def test_frames_with_roulette_match_the_oracle_simulation(ora):
    """pt_render_frame tick by tick, and pt_render_frames replaying a group of four frames (one trace launch, four blends)
    plus a single frame from its graphs, with roulette after two bounces: the canvas is the oracle's simulation of the
    reference's loop (one pass, then the shader's render() blend, per tick) with the same roulette."""
    from ray_tracer_webgl_amd.app import FrameLoop

    w, h, n, k = 96, 54, 5, 2
    loops = []
    for _ in range(2):
        loop = FrameLoop(w, h, mode="reference")
        loop.state.set_flags(is_paused=False)
        loop.state.set_quality(2, 8)
        loop.tracer.set_geometry_path(abi.PT_GEOM_SMALL)
        loop.tracer.set_russian_roulette(k)
        loops.append(loop)
    a, b = loops
    try:
        spheres = a.state.spheres()
        tex = [np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)]
        plain_differs = False
        for i in range(n):
            now = 100.0 + 16.5 * i
            assert a.frame(now) is True
            v, p = a.state.view(), a.state.to_params(now)
            acc, _ = oracle(ora, spheres, p, 1, k)
            expect = ora.blend_rgba8(acc, p.samples_per_pixel, p, tex[(v.even_odd_count + 1) % 2])
            acc0, _ = oracle(ora, spheres, p, 1, 0)
            plain_differs = plain_differs or not np.array_equal(expect, ora.blend_rgba8(acc0, p.samples_per_pixel, p, tex[(v.even_odd_count + 1) % 2]))
            tex[v.even_odd_count % 2] = expect
            assert np.array_equal(a.canvas, expect), "tick %d" % i
        assert plain_differs  # (the comparison can tell the two estimators apart after quantisation to RGBA8)
        assert kernel_of(a.tracer.stats()) == "small_t1_rr"
        assert b.frames(n, 100.0, 16.5) == n
        assert np.array_equal(b.canvas, expect), "replayed frames"
        ta, tb = a.textures, b.textures
        assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
        assert b.tracer.stats().segments == a.tracer.stats().segments
        assert kernel_of(b.tracer.stats()) == "small_t1_rr"
        REACHED.setdefault("small_t1_rr", []).append("frames")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------- (g) the LDS row
def test_the_lds_list_walk_with_roulette_renders_through_the_scalar_row(ora):
    """kTraceKernels has no roulette build of the LDS list walk; csrc/pt_geom_plan.hpp steers PT_GEOM_LDS + roulette to the
    scalar row (tests/test_geom_plan.py pins the policy, this the device).  The image is the ROULETTE oracle's, so the request
    was not served by the plain kernel of the LDS row; without roulette the same context walks the LDS list again."""
    for sc in (scenes.default_scene(96, 54, spp=3, max_depth=8, n_passes=2), scenes.config2(96, 54, 2, 2, 8)):
        p = with_lens_and_step(sc.params)
        plain, seg_plain = oracle(ora, sc.spheres, p, 2, 0)
        ref, seg = oracle(ora, sc.spheres, p, 2, 3)
        assert seg < seg_plain and not np.array_equal(bits(ref), bits(plain))
        t = context(sc.spheres, 96, 54, abi.PT_GEOM_LDS)
        try:
            for k, want_path, want, want_seg in ((0, abi.PT_GEOM_LDS, plain, seg_plain), (3, abi.PT_GEOM_SCALAR, ref, seg),
                                                 (0, abi.PT_GEOM_LDS, plain, seg_plain), (8, abi.PT_GEOM_SCALAR, plain, seg_plain)):
                got, st = gpu(t, p, k, 2)
                assert st.geometry_path == want_path, (sc.name, k, st.geometry_path)
                assert_bit_equal(got, want, "%s, PT_GEOM_LDS, roulette %d" % (sc.name, k))
                assert st.segments == want_seg
            REACHED.setdefault("scalar_rr", []).append("%s by way of PT_GEOM_LDS" % sc.name)
        finally:
            t.close()


def test_config4_under_the_autotuner_with_roulette(ora):
    """BASELINE config 4 — the scene the mode exists for, nine spheres — left to PT_GEOM_AUTO with roulette after three
    bounces, one pass per launch: the cold launch and the first trial walk the small list (length 1 modulo 4), the trial of
    the LDS walk is steered to the scalar row, then the scalar walk's own trial; whatever is kept, no launch ever reports the
    LDS walk, and the six passes are the roulette oracle's bits."""
    sc = scenes.config4(48, 48, 4, 6, 50)
    p = with_lens_and_step(sc.params)
    t = PathTracer(48, 48)
    try:
        t.set_russian_roulette(3)
        t.set_spheres(sc.spheres)
        t.reserve_passes(1)
        seen = []
        for i in range(6):
            q = p.copy()
            q.first_pass = i
            t.set_params(q)
            t.render_passes(1)
            st = t.stats()
            seen.append(int(st.geometry_path))
            kernel_of(st)
        print("config 4, PT_GEOM_AUTO, roulette 3: geometry path per launch %s, tuned %d" % (seen, st.geometry_tuned))
        assert seen[:4] == [abi.PT_GEOM_SMALL, abi.PT_GEOM_SMALL, abi.PT_GEOM_SCALAR, abi.PT_GEOM_SCALAR], seen
        assert st.geometry_tuned == 1 and set(seen[4:]) <= {abi.PT_GEOM_SMALL, abi.PT_GEOM_SCALAR}, seen
        ref, seg = oracle(ora, sc.spheres, p, 6, 3)
        assert_bit_equal(t.accum(), ref, "config 4 under PT_GEOM_AUTO, roulette 3")
        assert st.segments == seg
        plain_seg = oracle(ora, sc.spheres, p, 6, 0)[1]
        assert seg < 0.5 * plain_seg  # what the mode is for
        REACHED.setdefault("small_t1_rr", []).append("config 4 under PT_GEOM_AUTO")
    finally:
        t.close()


def test_every_roulette_kernel_was_reached():
    """(runs after the tests above) each of the twelve roulette kernels of csrc/pt_kernels_extra.hip was launched and compared"""
    print("roulette kernels reached\n" + "\n".join("  %-16s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in KERNELS))
    assert sorted(REACHED) == sorted(KERNELS), sorted(set(KERNELS) - set(REACHED))
