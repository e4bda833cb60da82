"""Next-event estimation (PT_OPT_NEXT_EVENT), every kernel build, bit for bit.

The option changes the samples and keeps the expectation, so the oracle cannot check it; tests/nee_ref.py restates the
estimator path by path on the oracle's exported pieces (tests/test_nee_ref.py pins the restatement itself).  Each of the
twelve next-event kernels of csrc/pt_kernels_nee.hip is held to the standard of every other kernel here: equal uint32 views
of the accumulation buffer and equal segment counts, tolerance none.

  (a) same walk       a scene without lights, and a scene with lights at max_depth == 1: the light sample is never reached,
                      the build must be its namesake's walk — the ORACLE's bits;
  (b) same estimator  the two-light room, random scenes with 1 to 3 lights and fields with three: tests/nee_ref.py's bits.
                      Several passes in one launch and one pass per launch, PT_TIME_STEP_DECORRELATED, lens on, one row band;
  (c) identity        pt_last_trace_build and the kernel a launch got (tests/trace_builds.py build_of), collected in REACHED:
                      the last test fails if one of the twelve was never reached;
  (d) scheduling      PT_OPT_CARRY_LANES / PT_OPT_REFILL_MIN at their ends;
  (e) frames          pt_render_frame / pt_render_frames against the restatement's ticks, and the plain frames once the option
                      is off again;
  (f) the context     exclusions, the option before and after pt_set_spheres, two lights -> none, the doors;
  (g) expectation     the two-light room: the next-event frame against the plain frame, block means within 5 standard errors.
The fields' frames are small (32 x 18, 16 x 9 at 60 000 spheres): the restatement walks the whole list per segment in Python.
"""
import os

import numpy as np
import pytest

import hierarchy_edges
import nee_ref
import nee_scenes
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer, PtError
from trace_builds import build_of

pytestmark = pytest.mark.gpu

ORACLE_THREADS = min(16, os.cpu_count() or 1)
KERNELS = ["small_t0_nee", "small_t1_nee", "small_t2_nee", "small_t3_nee", "scalar_nee", "scalar_nolds_nee", "bvh_nee", "bvh_nodes_nee",
           "bvh_gmem_nee", "grid_nee", "grid_cells_nee", "grid_gmem_nee"]
REACHED = {}
W, H, SPP, PASSES, DEPTH = 64, 36, 2, 2, 6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (
            what, len(bad), g.size, tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(ref)[tuple(bad[0])]))


def kernel_of(t):
    """the next-event kernel the last launch of this context was: pt_last_trace_build says that it was one, PtStats which row"""
    assert t.last_trace_build() == abi.BUILD_NEXT_EVENT, t.last_trace_build()
    return build_of(t.stats(), "_nee")


def context(sph, w, h, path, next_event=True, **options):
    t = PathTracer(w, h)
    t.set_geometry_path(path)
    if "carry_lanes" in options:
        t.set_carry_lanes(options["carry_lanes"])
    if "refill_min" in options:
        t.set_refill_min(options["refill_min"])
    t.set_spheres(sph)
    t.next_event(next_event)
    return t


def gpu(t, p, n_passes, per_launch=None):
    per_launch = per_launch or n_passes
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


def with_lens_and_step(p):
    p = p.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    if p.lens_radius == 0.0:
        p.lens_radius = 0.03
    return p


def padded_room(w=W, h=H):
    """the two-light room with eight small diffuse spheres on its floor: 18 spheres, enough for a hierarchy and a grid"""
    sc = nee_scenes.two_light_room(w, h, SPP, PASSES, DEPTH)
    extra = np.zeros(8, abi.SPHERE_DTYPE)
    for k in range(8):
        extra[k]["center"] = (-0.8 + 0.22 * k, -0.92, 0.55 - 0.1 * (k % 3))
        extra[k]["radius"] = 0.08
        extra[k]["type"] = abi.PT_DIFFUSE
        extra[k]["albedo"] = (0.3 + 0.05 * k, 0.5, 0.7 - 0.05 * k)
    sc.spheres = np.concatenate([sc.spheres, extra])
    sc.spheres["uuid"] = np.arange(len(sc.spheres))
    return sc


def lit_field(m, w, h):
    """the ground and the first m spheres of tests/hierarchy_edges.py's field under config 5's camera, three of them lights"""
    sc = hierarchy_edges.scene(m, w, h, SPP, PASSES, DEPTH)
    return nee_scenes.with_lights(sc, [2, 11, min(m, 150)])


def lit_config5(n, w, h):
    return nee_scenes.with_lights(scenes.config5(w, h, SPP, PASSES, DEPTH, n=n), [2, 11, 150])


# (kernel, scene, forced geometry path)
BUILDS = [
    ("small_t0_nee", lambda: nee_scenes.random_lit(3, 12, 1), abi.PT_GEOM_SMALL),
    ("small_t1_nee", lambda: nee_scenes.random_lit(0, 9, 2), abi.PT_GEOM_SMALL),
    ("small_t2_nee", lambda: nee_scenes.two_light_room(W, H, SPP, PASSES, DEPTH), abi.PT_GEOM_SMALL),
    ("small_t3_nee", lambda: nee_scenes.random_lit(2, 11, 3), abi.PT_GEOM_SMALL),
    ("scalar_nee", padded_room, abi.PT_GEOM_SCALAR),
    ("scalar_nolds_nee", lambda: lit_field(10232, 32, 18), abi.PT_GEOM_SCALAR),  # 10 233 spheres: one past the LDS copy
    ("bvh_nee", padded_room, abi.PT_GEOM_BVH),
    ("bvh_nee", lambda: lit_field(hierarchy_edges.M_BVH_FULL, W, H), abi.PT_GEOM_BVH),
    ("bvh_nodes_nee", lambda: lit_field(hierarchy_edges.M_NODES_FIRST, W, H), abi.PT_GEOM_BVH),
    ("bvh_gmem_nee", lambda: lit_field(hierarchy_edges.M_GMEM_FIRST, 32, 18), abi.PT_GEOM_BVH),
    ("grid_nee", padded_room, abi.PT_GEOM_GRID),
    ("grid_nee", lambda: lit_config5(1500, W, H), abi.PT_GEOM_GRID),
    ("grid_cells_nee", lambda: lit_config5(10000, 32, 18), abi.PT_GEOM_GRID),
    ("grid_gmem_nee", lambda: lit_config5(60000, 16, 9), abi.PT_GEOM_GRID),
]


@pytest.mark.parametrize("case", BUILDS, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BUILDS)])
def test_every_next_event_build_equals_the_restatement(ora, case):
    kernel, make, path = case
    sc = make()
    sph, n_passes = sc.spheres, sc.n_passes
    p = with_lens_and_step(sc.params)
    w, h = p.width, p.height
    assert n_passes == 2 and p.max_depth == DEPTH and p.samples_per_pixel == SPP
    assert len(nee_ref.lights_of(sph)) in (1, 2, 3)
    # (a) the same walk: no lights, and lights at a depth of one
    unlit = nee_scenes.without_lights(sc).spheres
    t = context(unlit, w, h, path)
    try:
        ref, seg = ora.render(unlit, p, n_passes, nthreads=ORACLE_THREADS)
        got, st = gpu(t, p, n_passes)
        assert kernel_of(t) == kernel, (kernel, kernel_of(t))
        assert_bit_equal(got, ref, "%s, no lights: the oracle" % kernel)
        assert st.segments == seg, (kernel, st.segments, seg)
    finally:
        t.close()
    t = context(sph, w, h, path)
    try:
        p1 = p.copy()
        p1.max_depth = 1
        ref, seg = ora.render(sph, p1, n_passes, nthreads=ORACLE_THREADS)
        got, st = gpu(t, p1, n_passes)
        assert kernel_of(t) == kernel
        assert_bit_equal(got, ref, "%s, max_depth 1: the oracle" % kernel)
        assert st.segments == seg
        # (b) the same estimator
        full, seg_full, shadow = nee_ref.render(sph, p, n_passes)
        plain, seg_plain = ora.render(sph, p, n_passes, nthreads=ORACLE_THREADS)
        assert shadow > 0 and not np.array_equal(bits(full), bits(plain)), "the light sample is at work in this scene"
        got, st = gpu(t, p, n_passes)
        assert kernel_of(t) == kernel
        assert_bit_equal(got, full, "%s, %d passes in one launch" % (kernel, n_passes))
        assert st.segments == seg_full, (kernel, st.segments, seg_full)
        got, st = gpu(t, p, n_passes, per_launch=1)
        assert kernel_of(t) == kernel and st.render_launches == n_passes
        assert_bit_equal(got, full, "%s, one pass per launch" % kernel)
        assert st.segments == seg_full
        if path == abi.PT_GEOM_GRID:
            assert st.grid_fit_stale != 1
    finally:
        t.close()
    # one row band of three (the seeds are per pixel: the rows of the whole frame)
    q = p.copy()
    q.band_rows, q.band_index, q.band_count = 4, 1, 3
    tb = context(sph, w, h, path)
    try:
        part, st = gpu(tb, q, n_passes)
        assert kernel_of(tb) == kernel
        ys = abi.owned_rows(h, 4, 1, 3)
        assert part.shape[0] == len(ys)
        assert_bit_equal(part, full[ys], "%s, band 1 of 3 against the rows of the whole frame" % kernel)
    finally:
        tb.close()
    REACHED.setdefault(kernel, []).append("%d spheres, %dx%d, %d shadow segments of %d" % (len(sph), w, h, shadow, seg_full))


# ------------------------------------------------------------------------------------- (d) scheduling only
@pytest.mark.parametrize("path", [abi.PT_GEOM_BVH, abi.PT_GEOM_GRID], ids=["hierarchy", "grid"])
def test_carry_lanes_and_refill_min_do_not_change_the_next_event_image(path):
    """Shadow segments are short walks beside long ones: stragglers are carried while a lane is between its light sample and its
    scattered ray.  Scheduling only — lockstep or always carrying, refill at once or only for a whole wave: the same bits."""
    sc = nee_scenes.with_lights(scenes.config2(W, H, SPP, PASSES, DEPTH), [1, 30, 200])
    p = with_lens_and_step(sc.params)
    ref, seg, shadow = nee_ref.render(sc.spheres, p, PASSES)
    assert shadow > 0
    for carry, refill in ((0, 1), (64, 64), (0, 64), (64, 1)):
        t = context(sc.spheres, W, H, path, carry_lanes=carry, refill_min=refill)
        try:
            got, st = gpu(t, p, PASSES)
            assert kernel_of(t) == ("bvh_nee" if path == abi.PT_GEOM_BVH else "grid_nee")
            assert_bit_equal(got, ref, "carry_lanes %d refill_min %d" % (carry, refill))
            assert st.segments == seg
        finally:
            t.close()


# ------------------------------------------------------------------------------------- (e) frames
def test_frames_with_next_event_match_the_restatements_ticks(ora):
    """pt_render_frame tick by tick and pt_render_frames replaying the same ticks from its graphs, the option on: the canvas is
    the reference's loop with the restatement's pass per tick.  Then the option off between two replayed series: the plain
    loop's canvas, so a replayed graph is keyed on the option."""
    from ray_tracer_webgl_amd.app import FrameLoop
    from test_gpu_parity import _host_spheres

    w, h, n = 48, 27, 5
    sph = scenes.default_scene(w, h, spp=2, max_depth=DEPTH).spheres.copy()
    sph[3]["type"], sph[3]["albedo"] = abi.PT_EMISSIVE, (5.0, 4.0, 3.0)
    sph["uuid"] = np.arange(len(sph))
    loops = []
    for _ in range(2):
        loop = FrameLoop(w, h, mode="reference", host_spheres=_host_spheres(sph), next_event=True)
        loop.state.set_flags(is_paused=False)
        loop.state.set_quality(2, DEPTH)
        loop.tracer.set_geometry_path(abi.PT_GEOM_SMALL)
        loops.append(loop)
    a, b = loops
    try:
        spheres = a.state.spheres()
        assert len(nee_ref.lights_of(spheres)) == 1
        tex = [np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)]
        tex0 = [t.copy() for t in tex]
        differs = False
        for i in range(n):
            now = 100.0 + 16.5 * i
            assert a.frame(now) is True
            v, p = a.state.view(), a.state.to_params(now)
            acc, _, _ = nee_ref.render(spheres, p, 1)
            prev = tex[(v.even_odd_count + 1) % 2]
            expect = ora.blend_rgba8(acc, p.samples_per_pixel, p, prev)
            acc0, _ = ora.render(spheres, p, 1, nthreads=ORACLE_THREADS)
            plain = ora.blend_rgba8(acc0, p.samples_per_pixel, p, tex0[(v.even_odd_count + 1) % 2])
            tex0[v.even_odd_count % 2] = plain
            differs = differs or not np.array_equal(expect, ora.blend_rgba8(acc0, p.samples_per_pixel, p, prev))
            tex[v.even_odd_count % 2] = expect
            assert np.array_equal(a.canvas, expect), "tick %d" % i
        assert differs
        assert kernel_of(a.tracer) == "small_t1_nee"
        assert b.frames(n, 100.0, 16.5) == n
        assert np.array_equal(b.canvas, expect), "replayed frames"
        assert b.tracer.stats().segments == a.tracer.stats().segments
        REACHED.setdefault("small_t1_nee", []).append("frames")
        # the option turned off again before the series: the plain loop's canvas
        d = FrameLoop(w, h, mode="reference", host_spheres=_host_spheres(sph), next_event=True)
        try:
            d.state.set_flags(is_paused=False)
            d.state.set_quality(2, DEPTH)
            d.tracer.set_geometry_path(abi.PT_GEOM_SMALL)
            d.tracer.next_event(False)
            assert d.frames(n, 100.0, 16.5) == n
            assert d.tracer.last_trace_build() == abi.BUILD_PLAIN
            assert np.array_equal(d.canvas, plain), "the option off: the plain loop's canvas"
        finally:
            d.close()
    finally:
        a.close()
        b.close()


def test_a_replayed_series_follows_the_option_off_and_on_again(ora):
    """ONE context: a series replayed with the option on, one with it off, one with it on again — the frame graphs are keyed on
    the option (the plan holds the kernel, the table and its length), so the second series is the plain estimator's and the
    third the first one's bits again."""
    w, h = 48, 27
    sc = nee_scenes.two_light_room(w, h, 2, 1, DEPTH)
    p = sc.params.copy()
    p.time_step = 16.5
    t = PathTracer(w, h)
    try:
        t.set_geometry_path(abi.PT_GEOM_SMALL)
        t.set_spheres(sc.spheres)
        t.set_params(p)
        canv = []
        for on in (True, False, True):
            t.next_event(on)
            t.clear_textures()
            t.set_params(p)
            t.render_frames(0, 1, 4)
            canv.append(t.read_canvas().copy())
            assert t.last_trace_build() == (abi.BUILD_NEXT_EVENT if on else abi.BUILD_PLAIN)
        assert np.array_equal(canv[0], canv[2]) and not np.array_equal(canv[0], canv[1])
    finally:
        t.close()


# ------------------------------------------------------------------------------------- (f) the context
def test_exclusions_are_refused_and_leave_the_context_usable(ora):
    sc = nee_scenes.two_light_room(W, H, SPP, PASSES, DEPTH)
    p = with_lens_and_step(sc.params)
    ref, seg, _ = nee_ref.render(sc.spheres, p, PASSES)
    t = context(sc.spheres, W, H, abi.PT_GEOM_SMALL)
    try:
        for refused in (lambda: t.set_russian_roulette(3), lambda: t.set_debug_overlay(True, 1, (0.0, 0.0, 0.0)), lambda: t.set_count_work(True)):
            with pytest.raises(PtError) as e:
                refused()
            assert e.value.code == abi.PT_ERR_INVALID and "exclude each other" in str(e.value), str(e.value)
        with pytest.raises(PtError) as e:
            t._check(t.lib.pt_set_option(t._ctx, abi.PT_OPT_NEXT_EVENT, 2))
        assert e.value.code == abi.PT_ERR_INVALID
        got, st = gpu(t, p, PASSES)
        assert kernel_of(t) == "small_t2_nee"
        assert_bit_equal(got, ref, "after the refusals")
        assert st.segments == seg
        # ... and the other way round: each of the three first, the option second
        t.next_event(False)
        for first, undo in ((lambda: t.set_russian_roulette(3), lambda: t.set_russian_roulette(0)),
                            (lambda: t.set_debug_overlay(True, 1, (0.0, 0.0, 0.0)), lambda: t.set_debug_overlay(False)),
                            (lambda: t.set_count_work(True), lambda: t.set_count_work(False))):
            first()
            with pytest.raises(PtError) as e:
                t.next_event(True)
            assert e.value.code == abi.PT_ERR_INVALID and "exclude each other" in str(e.value), str(e.value)
            undo()
        plain, seg_plain = ora.render(sc.spheres, p, PASSES, nthreads=ORACLE_THREADS)
        got, st = gpu(t, p, PASSES)
        assert t.last_trace_build() == abi.BUILD_PLAIN
        assert_bit_equal(got, plain, "the option off again: the oracle")
        assert st.segments == seg_plain
    finally:
        t.close()


def test_the_option_before_and_after_the_scene_and_a_scene_without_lights(ora):
    sc = nee_scenes.two_light_room(W, H, SPP, PASSES, DEPTH)
    p = with_lens_and_step(sc.params)
    ref, seg, _ = nee_ref.render(sc.spheres, p, PASSES)
    t = PathTracer(W, H)
    try:
        t.set_geometry_path(abi.PT_GEOM_SMALL)
        t.next_event(True)  # before any scene: the table follows pt_set_spheres
        t.set_spheres(sc.spheres)
        got, st = gpu(t, p, PASSES)
        assert kernel_of(t) == "small_t2_nee"
        assert_bit_equal(got, ref, "the option before pt_set_spheres")
        t.next_event(False)
        t.next_event(True)  # over the installed scene
        got, st = gpu(t, p, PASSES)
        assert_bit_equal(got, ref, "the option after pt_set_spheres")
        assert st.segments == seg
        # two lights -> none: the oracle's bits through the same build
        unlit = nee_scenes.without_lights(sc).spheres
        t.set_spheres(unlit)
        plain, seg_plain = ora.render(unlit, p, PASSES, nthreads=ORACLE_THREADS)
        got, st = gpu(t, p, PASSES)
        assert kernel_of(t) == "small_t2_nee"
        assert_bit_equal(got, plain, "a scene without lights")
        assert st.segments == seg_plain
        # ... and back
        t.set_spheres(sc.spheres)
        got, st = gpu(t, p, PASSES)
        assert_bit_equal(got, ref, "the two lights again")
    finally:
        t.close()


def test_the_query_and_radiance_doors_stay_the_plain_estimator():
    sc = padded_room()
    p = with_lens_and_step(sc.params)
    rng = np.random.default_rng(5)
    o = np.tile(np.asarray([[0.0, 0.0, 3.0]], np.float32), (257, 1))
    d = (rng.uniform(-0.4, 0.4, (257, 3)) + np.asarray([0.0, 0.0, -1.0])).astype(np.float32)
    out = []
    for on in (False, True):
        t = context(sc.spheres, W, H, abi.PT_GEOM_BVH, next_event=on)
        try:
            t.set_params(p)
            t.reserve_passes(2)
            t.ray_queries(True)
            t.feature_planes(True)
            hits = t.query_rays(o, d)
            rad = t.query_radiance(o, d, passes=2)
            t.render_features()
            feat = t.features()
            out.append((hits, rad, feat))
        finally:
            t.close()
    for a, b in zip(out[0], out[1]):
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.ascontiguousarray(a[key]).tobytes() == np.ascontiguousarray(b[key]).tobytes(), key


# ------------------------------------------------------------------------------------- (g) expectation on the device
def test_the_next_event_frame_has_the_plain_frames_expectation():
    """The two-light room at 64 x 64, 40 independent passes of 16 samples each way (a pass per launch, decorrelated time step, the
    accumulation cleared between them): per 8 x 8 block and channel, and for the whole frame, the two means differ by at most 5
    standard errors of their difference, the standard errors taken from the passes' own spread."""
    w = h = 64
    n, spp = 40, 16
    sc = nee_scenes.two_light_room(w, h, spp, 1, DEPTH)
    p = sc.params.copy()
    p.time_step = abi.PT_TIME_STEP_DECORRELATED
    means = {}
    for on in (False, True):
        t = context(sc.spheres, w, h, abi.PT_GEOM_SMALL, next_event=on)
        try:
            t.reserve_passes(1)
            per_pass = np.zeros((n, h // 8, w // 8, 3))
            for k in range(n):
                q = p.copy()
                q.first_pass = k
                t.set_params(q)
                t.reset()
                t.render_passes(1)
                acc = t.accum().astype(np.float64)
                per_pass[k] = (acc[..., :3] / spp).reshape(h // 8, 8, w // 8, 8, 3).mean(axis=(1, 3))
            assert t.last_trace_build() == (abi.BUILD_NEXT_EVENT if on else abi.BUILD_PLAIN)
            means[on] = per_pass
        finally:
            t.close()
    worst = 0.0
    for view in (lambda a: a, lambda a: a.mean(axis=(1, 2), keepdims=True)):
        a, b = view(means[False]), view(means[True])
        diff = a.mean(axis=0) - b.mean(axis=0)
        se = np.sqrt(a.var(axis=0, ddof=1) / n + b.var(axis=0, ddof=1) / n)
        z = np.abs(diff) / np.maximum(se, 1e-30)
        worst = max(worst, float(z.max()))
        print("next-event against plain: worst |difference| / standard error %.2f over %d means; frame means %s vs %s" % (
            float(z.max()), z.size, means[False].mean(axis=(0, 1, 2)), means[True].mean(axis=(0, 1, 2))))
        assert (z <= 5.0).all(), (float(z.max()), np.argwhere(z > 5.0)[:5])
    # the estimators differ: the next-event passes scatter far less where the lamp matters
    assert means[True].var(axis=0).mean() < means[False].var(axis=0).mean()


def test_every_next_event_kernel_was_reached():
    """(runs after the tests above) each of the twelve kernels of csrc/pt_kernels_nee.hip was launched and compared"""
    print("next-event kernels reached\n" + "\n".join("  %-18s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in KERNELS))
    assert sorted(REACHED) == sorted(KERNELS), sorted(set(KERNELS) - set(REACHED))
