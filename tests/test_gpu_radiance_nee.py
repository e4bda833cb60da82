"""pt_query_radiance_nee, pt_gather_irradiance_nee and pt_bake_probes_nee (include/ptrace.h has the contract) on the device,
bit for bit.

Every comparison is equal uint32 views of the raw records against tests/radiance_nee_ref.py — tests/radiance_ref.py's records
with tests/nee_ref.py's path in ora_ray_color's place, pinned on the CPU by tests/test_radiance_nee_ref.py.  Tolerance: none.
Each test first asserts that the reference holds no NaN.  PtStats.segments moves by exactly the reference's total (path segments
plus shadow segments); samples, total_spp and render_launches do not move.  Unless stated: the time step
PT_TIME_STEP_DECORRELATED, max_depth 6, 2 samples per pixel, 3 passes.

  (a) every build    each of the twelve kernels of csrc/pt_kernels_radiance_nee.hip on the lit scenes of test_gpu_next_event.py,
                     48x27 down to 16x9 at 60 000 spheres: the context's pinhole rays, 200 bounce-style rays from hit points, 50
                     rays from inside spheres (two batches).  Of the REFERENCE: shadow segments, an occluded shadow ray, a
                     record that differs from the plain restatement's
  (b) batch edges    n = 1, 63, 64, 65, 776, 777, 778, 2*777 + 5 at 37x21 on a small-list and a grid row; what lies behind out[n]
  (c) gather         both calls, 5 items of 64 directions and 9 of 192 at 37x21 (items straddle batches), one item invalid; the
                     plain gather over the same context afterwards
  (d) no lights, and lights that change
  (e) undisturbed    accumulation, estimate, feature planes, history, canvas, first_pass, build, path; the plain call before and
                     after; a next-event render after
  (f) invalid rays   every class at places 0, 63, 64 and the last
  (g) bands          a band answers by its own rows' seeds; a band without rows
  (h) errors         the option off in either order, n_passes, a stream capture; the context stays usable
  (i) device arrays  torch tensors in and out, all four combinations over three batches
"""
import ctypes as C

import numpy as np
import pytest

import gather_ref as G
import hierarchy_edges
import nee_ref
import nee_scenes
import query_ref as Q
import radiance_nee_ref as RN
import radiance_ref as RR
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_gather import FLOATS, items_of
from test_gpu_ray_queries import SplitMix64, pack
from trace_builds import build_of

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0xa5a5a5a5
SPP, PASSES, DEPTH = 2, 3, 6
W, H = 37, 21
PIX = W * H  # 777 places: the batch of the 37x21 contexts
KERNELS = sorted(v + "_rad_nee" for v in ("small_t0", "small_t1", "small_t2", "small_t3", "scalar", "scalar_nolds", "bvh", "bvh_nodes", "bvh_gmem", "grid",
                                          "grid_cells", "grid_gmem"))
REACHED = {}


def settings(p, first_pass=0):
    q = p.copy()
    q.samples_per_pixel, q.max_depth, q.first_pass, q.time_step = SPP, DEPTH, first_pass, abi.PT_TIME_STEP_DECORRELATED
    return q


def context(sph, p, path=None, reserve=PASSES, next_event=True, use_torch=False):
    t = PathTracer(p.width, p.height, use_torch=use_torch) if use_torch else PathTracer(p.width, p.height)
    if path is not None:
        t.set_geometry_path(path)
    t.set_spheres(sph)
    t.ray_queries(True)
    if next_event:
        t.next_event(True)
    t.reserve_passes(reserve)
    t.set_params(p)
    return t


def radiance(t, o, d, n_passes=PASSES, segments=None, fn=None):
    """the raw records, (n, 4) uint32, through the C entry point (pt_query_radiance_nee unless `fn`); three records of guard
    words behind out[n] stay as they are; PtStats.segments moves by `segments` and nothing else of the tallies moves"""
    rays = pack(o, d)
    n = len(rays)
    out = np.full((n + 3, 4), GUARD, np.uint32)
    before = t.stats()
    t._check((fn or t.lib.pt_query_radiance_nee)(t._ctx, rays.ctypes.data_as(C.c_void_p), n, n_passes, out.ctypes.data_as(C.c_void_p)))
    after = t.stats()
    assert (out[n:] == GUARD).all(), "records written behind out[n]"
    if segments is not None:
        assert after.segments - before.segments == segments, (after.segments - before.segments, segments)
    assert (after.samples, after.total_spp, after.render_launches) == (before.samples, before.total_spp, before.render_launches)
    return out[:n]


def assert_records_equal(got, ref, what):
    assert not RN.has_nan(ref), what + ": the restatement holds a NaN"
    want = RN.raw(ref)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=1))[:, 0]
        k = int(bad[0])
        raise AssertionError("%s: %d of %d records differ, first ray %d:\n got  %r\n want %r" % (
            what, len(bad), len(got), k, got[k].view(F), want[k].view(F)))


def kernel_of(t, path):
    """the kernel a _nee call through the forced `path` launched: the row's cell of kRadNeeKernels (pinned on the CPU:
    tests/test_radiance_nee_ref.py), the row read from PtStats as for every other column"""
    return build_of(t.stats(), "_rad_nee", path=abi.PT_GEOM_SCALAR if path == abi.PT_GEOM_LDS else path)


def mixed_rays(sph, p, seed):
    """the context's pinhole rays, 200 bounce-style rays from their hit points and 50 rays from inside spheres"""
    o, d = Q.pinhole_rays(p)
    first = Q.records(sph, p, o, d)
    pts = first["point"][first["index"] >= 0]
    rng = SplitMix64(seed)
    bo, bd = pts[(np.arange(200) * 3) % len(pts)], rng.unit(200)
    io, idir = sph["center"][(np.arange(50) * 7 + 1) % len(sph)].astype(F), rng.unit(50)
    return np.concatenate([o, bo, io]), np.concatenate([d, bd, idir])


# ------------------------------------------------------------------------------------------------ (a) every build
def padded_room(w, h):
    """test_gpu_next_event.py's: the two-light room with eight small diffuse spheres on its floor, enough for a hierarchy and a grid"""
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
    return nee_scenes.with_lights(hierarchy_edges.scene(m, w, h, SPP, PASSES, DEPTH), [2, 11, min(m, 150)])


def lit_config5(n, w, h):
    return nee_scenes.with_lights(scenes.config5(w, h, SPP, PASSES, DEPTH, n=n), [2, 11, 150])


# (kernel, scene, forced geometry path): the scenes of test_gpu_next_event.py's builds, the largest frames at 48x27
BUILDS = [
    ("small_t0_rad_nee", lambda: nee_scenes.random_lit(3, 12, 1, width=48, height=27), abi.PT_GEOM_SMALL),
    ("small_t1_rad_nee", lambda: nee_scenes.random_lit(0, 9, 2, width=48, height=27), abi.PT_GEOM_SMALL),
    ("small_t2_rad_nee", lambda: nee_scenes.two_light_room(48, 27, SPP, PASSES, DEPTH), abi.PT_GEOM_SMALL),
    ("small_t3_rad_nee", lambda: nee_scenes.random_lit(2, 11, 3, width=48, height=27), abi.PT_GEOM_SMALL),
    ("scalar_rad_nee", lambda: padded_room(48, 27), abi.PT_GEOM_SCALAR),
    ("scalar_nolds_rad_nee", lambda: lit_field(10232, 32, 18), abi.PT_GEOM_SCALAR),  # 10 233 spheres: one past the LDS copy
    ("bvh_rad_nee", lambda: lit_field(hierarchy_edges.M_BVH_FULL, 48, 27), abi.PT_GEOM_BVH),
    ("bvh_nodes_rad_nee", lambda: lit_field(hierarchy_edges.M_NODES_FIRST, 48, 27), abi.PT_GEOM_BVH),
    ("bvh_gmem_rad_nee", lambda: lit_field(hierarchy_edges.M_GMEM_FIRST, 32, 18), abi.PT_GEOM_BVH),
    ("grid_rad_nee", lambda: padded_room(48, 27), abi.PT_GEOM_GRID),
    ("grid_rad_nee", lambda: lit_config5(1500, 48, 27), abi.PT_GEOM_GRID),
    ("grid_cells_rad_nee", lambda: lit_config5(10000, 32, 18), abi.PT_GEOM_GRID),
    ("grid_gmem_rad_nee", lambda: lit_config5(60000, 16, 9), abi.PT_GEOM_GRID),
]


def build_reference(case):
    """(spheres, params, origins, directions, lit records, segments, shadow segments, of them occluded, plain records) of a case"""
    kernel, make, path = case
    sc = make()
    p = settings(sc.params)
    o, d = mixed_rays(sc.spheres, p, 0x3200 + len(sc.spheres))
    info = {}
    ref, seg, shadow = RN.records(sc.spheres, p, o, d, PASSES, info=info)
    plain, seg_plain = RR.records(sc.spheres, p, o, d, PASSES)
    return sc.spheres, p, o, d, ref, seg, shadow, info["occluded"], plain, seg_plain


@pytest.mark.parametrize("case", BUILDS, ids=["%s-%d" % (b[0], i) for i, b in enumerate(BUILDS)])
def test_every_build_equals_the_restatement(case):
    kernel, _, path = case
    sph, p, o, d, ref, seg, shadow, occluded, plain, seg_plain = build_reference(case)
    assert not RN.has_nan(ref) and len(o) == RR.batch(p) + 250, "two batches"
    assert len(nee_ref.lights_of(sph)) in (1, 2, 3)
    assert shadow > 0 and occluded > 0, "the light sample is at work in this scene, and some shadow ray is occluded"
    assert (RN.raw(ref) != RR.raw(plain)).any(axis=1).any(), "some record differs from the plain restatement's"
    t = context(sph, p, path)
    try:
        build0, st0 = t.last_trace_build(), t.stats()
        got = radiance(t, o, d, PASSES, seg)
        assert kernel_of(t, path) == kernel, (kernel, kernel_of(t, path))
        st = t.stats()
        assert t.last_trace_build() == build0 and (st.geometry_path, st.geometry_tuned) == (st0.geometry_path, st0.geometry_tuned)
        assert_records_equal(got, ref, "%d spheres through %s" % (len(sph), kernel))
        assert (got[:, 3].view(F) == SPP * PASSES).all()
        if path == abi.PT_GEOM_GRID:
            assert st.grid_fit_stale != 1
        REACHED.setdefault(kernel, []).append("%d spheres, %dx%d, %d shadow segments of %d, %d occluded" % (len(sph), p.width, p.height, shadow, seg, occluded))
    finally:
        t.close()


def test_every_rad_nee_kernel_was_reached():
    """(runs after the test above) each of the twelve kernels of csrc/pt_kernels_radiance_nee.hip was launched and compared"""
    print("_rad_nee kernels reached\n" + "\n".join("  %-22s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in KERNELS))
    assert len(KERNELS) == 12 and sorted(REACHED) == KERNELS, sorted(set(KERNELS) - set(REACHED))


# ------------------------------------------------------------------------------------------------ the 37x21 scenes
def room():
    sc = nee_scenes.two_light_room(W, H, SPP, PASSES, DEPTH)
    return sc.spheres, settings(sc.params)


def padded():
    sc = padded_room(W, H)
    return sc.spheres, settings(sc.params)


SCENES = {"room": room, "padded": padded}
_ROOM_RAYS = {}


def room_rays(name="room", n=160):
    """n of the scene's mixed rays, from all over them: (origins, directions, lit records, segments), made once"""
    if (name, n) not in _ROOM_RAYS:
        sph, p = SCENES[name]()
        o, d = mixed_rays(sph, p, 0x3237)
        pick = (np.arange(n) * 5) % len(o)
        o, d = o[pick], d[pick]
        ref, seg, shadow = RN.records(sph, p, o, d, PASSES)
        assert shadow > 0 and not RN.has_nan(ref)
        ref.setflags(write=False)
        _ROOM_RAYS[(name, n)] = (o, d, ref, seg)
    return _ROOM_RAYS[(name, n)]


# ------------------------------------------------------------------------------------------------ (b) batch edges
COUNTS = [1, 63, 64, 65, PIX - 1, PIX, PIX + 1, 2 * PIX + 5]
_EDGE = {}


def _records_from(sph, p, o, d, a, b):
    """the records of rays a .. b - 1 of a call (their indices count), every ray before them marked invalid: no record, no segment"""
    oo, dd = o[:b].copy(), d[:b].copy()
    dd[:a] = 0.0
    ref, seg, _ = RN.records(sph, p, oo, dd, PASSES)
    return ref[a:b], seg


def edge_rays(name):
    """2 * 777 + 5 different rays (the mixed rays in another order, longer from batch to batch) and, per count, the
    restatement's records and segments — a ray's record depends on its index only, so the records of n rays are the first n"""
    if name not in _EDGE:
        sph, p = SCENES[name]()
        o, d = mixed_rays(sph, p, 0x3238)
        i = np.arange(COUNTS[-1])
        pick = (i * 7) % len(o)
        oo, dd = o[pick], d[pick] * (1 + i // PIX).astype(F)[:, None]
        ref = np.zeros((len(i), 4), F)
        seg_upto, last = {0: 0}, 0
        for n in COUNTS:  # in pieces, so that every count has its segment total
            part, seg = _records_from(sph, p, oo, dd, last, n)
            ref[last:n] = part
            seg_upto[n] = seg_upto[last] + seg
            last = n
        assert not RN.has_nan(ref)
        ref.setflags(write=False)
        _EDGE[name] = (oo, dd, ref, seg_upto)
    return _EDGE[name]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,path", [("room", abi.PT_GEOM_SMALL), ("padded", abi.PT_GEOM_GRID)], ids=["small", "grid"])
def test_batch_edges(name, path, n):
    sph, p = SCENES[name]()
    o, d, ref, seg_upto = edge_rays(name)
    t = context(sph, p, path)
    try:
        got = radiance(t, o[:n], d[:n], PASSES, seg_upto[n])  # (the guard behind out[n], segments exactly)
        assert_records_equal(got, ref[:n], "%s, n = %d" % (name, n))
        assert kernel_of(t, path) == ("small_t2_rad_nee" if name == "room" else "grid_rad_nee")
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (c) gather
KINDS = [(G.IRRADIANCE, "irradiance"), (G.PROBE, "probes")]
G_PASSES = 2


def gather_items(n):
    """n items in the two-light room: on the floor, the walls, in the air, beside the lamp; item 2 is invalid"""
    pos = [(0.0, -0.95, 0.0), (0.9, 0.0, 0.2), (np.inf, 0.0, 0.0), (-0.9, -0.5, -0.5), (0.25, 0.2, -0.2), (0.0, 0.9, 0.3), (-0.5, -0.2, 0.6),
           (0.6, 0.6, 0.4), (0.0, 0.0, 1.5)]
    nrm = [(0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.2, 0.1), (0.0, 1.0, 0.0), (0.0, -2.0, 0.0), (0.3, 0.1, -0.7), (-1e-3, -1.0, 0.0),
           (0.0, 0.0, -1.0)]
    return np.asarray(pos[:n], F), np.asarray(nrm[:n], F)


def fn_of(t, kind, next_event=True):
    if next_event:
        return t.lib.pt_bake_probes_nee if kind == G.PROBE else t.lib.pt_gather_irradiance_nee
    return t.lib.pt_bake_probes if kind == G.PROBE else t.lib.pt_gather_irradiance


def gather(t, kind, pos, nrm, D, segments, next_event=True):
    it = items_of(pos, nrm)
    n = len(it)
    out = np.full((n + 2, FLOATS[kind]), GUARD, np.uint32)
    before = t.stats()
    t._check(fn_of(t, kind, next_event)(t._ctx, it.ctypes.data_as(C.c_void_p), n, D, G_PASSES, out.ctypes.data_as(C.c_void_p)))
    after = t.stats()
    assert (out[n:] == GUARD).all(), "records written behind out[n]"
    assert after.segments - before.segments == segments, (after.segments - before.segments, segments)
    assert (after.samples, after.total_spp, after.render_launches) == (before.samples, before.total_spp, before.render_launches)
    return out[:n]


@pytest.mark.parametrize("kind,kind_name", KINDS, ids=[k[1] for k in KINDS])
@pytest.mark.parametrize("n,D", [(5, 64), (9, 192)], ids=["5x64", "9x192"])
def test_the_gather_calls_are_the_reduce_over_the_lit_records(n, D, kind, kind_name):
    sph, p = room()
    pos, nrm = gather_items(n)
    assert (n * D) % PIX != 0 and PIX % 64 != 0 and n * D < 3 * PIX, "items straddle the batches"
    normals = nrm if kind == G.IRRADIANCE else None
    ref, seg, shadow, rec = RN.gather(sph, p, kind, pos, normals, D, G_PASSES)
    plain, seg_plain, _ = G.gather(sph, p, kind, pos, normals, D, G_PASSES)
    assert not np.isnan(ref).any() and not np.isnan(plain).any() and shadow > 0
    assert not ref[2].view(np.uint32).any() and (np.delete(ref[:, -1], 2) == D * G_PASSES * SPP).all(), "item 2 is invalid: samples == 0 is the mark"
    assert not np.array_equal(G.raw(ref), G.raw(plain))
    t = context(sph, p, abi.PT_GEOM_SMALL, reserve=G_PASSES)
    try:
        build0 = t.last_trace_build()
        got = gather(t, kind, pos, nrm, D, seg)
        assert np.array_equal(got, G.raw(ref)), "%s, %d items of %d directions" % (kind_name, n, D)
        assert kernel_of(t, abi.PT_GEOM_SMALL) == "small_t2_rad_nee" and t.last_trace_build() == build0
        # the plain gather over the same context afterwards: still the plain estimator
        got = gather(t, kind, pos, nrm, D, seg_plain, next_event=False)
        assert np.array_equal(got, G.raw(plain)), "the plain %s afterwards" % kind_name
        # ... and the Python door
        res = t.bake_probes(pos, directions=D, passes=G_PASSES, next_event=True) if kind == G.PROBE else t.gather_irradiance(
            pos, nrm, directions=D, passes=G_PASSES, next_event=True)
        flat = np.concatenate([np.ascontiguousarray(res["sh" if kind == G.PROBE else "e"]).reshape(n, -1), res["samples"].reshape(n, 1)], axis=1)
        assert np.array_equal(G.raw(flat), G.raw(ref))
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (d) no lights; lights that change
def test_no_lights_and_lights_that_change():
    sph, p = padded()
    o, d, ref, seg = room_rays("padded")
    unlit = nee_scenes.without_lights(scenes.Scene("padded", sph, p, PASSES, "")).spheres
    plain, seg_plain = RR.records(unlit, p, o, d, PASSES)
    one = sph.copy()  # two lights -> one: the dome becomes a diffuse shell
    dome = [i for i, s in enumerate(one) if s["type"] == abi.PT_EMISSIVE][0]
    one[dome]["type"], one[dome]["albedo"] = abi.PT_DIFFUSE, (0.4, 0.5, 0.7)
    assert len(nee_ref.lights_of(sph)) == 2 and len(nee_ref.lights_of(one)) == 1 and nee_ref.lights_of(unlit) == []
    ref_one, seg_one, shadow_one = RN.records(one, p, o, d, PASSES)
    assert not RR.has_nan(plain) and not RN.has_nan(ref_one) and shadow_one > 0
    assert not np.array_equal(RN.raw(ref_one), RN.raw(ref))
    t = context(unlit, p, abi.PT_GEOM_BVH)
    try:
        got = radiance(t, o, d, PASSES, seg_plain)
        assert kernel_of(t, abi.PT_GEOM_BVH) == "bvh_rad_nee"
        assert_records_equal(got, plain, "a scene without lights: pt_query_radiance's bits through the _rad_nee build")
        t.set_spheres(sph)
        assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "two lights")
        t.set_spheres(one)
        assert_records_equal(radiance(t, o, d, PASSES, seg_one), ref_one, "two lights swapped for one: the new table")
        t.set_spheres(sph)
        assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "the two lights again")
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (e) undisturbed
def test_nothing_else_of_the_context_moves():
    """two contexts do the same things; one of them asks for the three _nee calls in between.  Every read-out and every later
    result agree; the plain call before and after gives the plain bytes; the next-event render after it gives nee_ref.render's"""
    sc = nee_scenes.two_light_room(W, H, SPP, PASSES, DEPTH)
    p = settings(sc.params, first_pass=3)
    p.render_count, p.should_average, p.last_frame_weight = 1, 1, 1.0
    sph = sc.spheres
    o, d, _, _ = room_rays()
    ref, seg, _ = RN.records(sph, p, o, d, 2)
    plain, seg_plain = RR.records(sph, p, o, d, 2)
    frame, seg_frame, _ = nee_ref.render(sph, p, 2)
    assert not RN.has_nan(ref) and not RR.has_nan(plain) and not np.isnan(frame).any()
    pos, nrm = gather_items(5)
    out = []
    for asks in (True, False):
        t = context(sph, p, abi.PT_GEOM_SMALL, reserve=2)
        try:
            t.feature_planes(True)
            t.error_estimate(True)
            t.reproject_option(True)
            t.reset()
            t.render_passes(2)
            assert t.last_trace_build() == abi.BUILD_NEXT_EVENT
            assert np.array_equal(t.accum().view(np.uint32), frame.view(np.uint32))
            t.render_features()
            t.keep_history()
            t.clear_textures()
            t.render_frame(1)
            if asks:
                def held():
                    st = t.stats()
                    return (t.accum(), t.error_state(), t.features(), t.read_canvas(), t.read_texture(0), t.read_texture(1), t.last_trace_build(),
                            st.geometry_path, st.geometry_tuned, t.lib.pt_last_error(t._ctx))

                assert_records_equal(radiance(t, o, d, 2, seg_plain, fn=t.lib.pt_query_radiance), plain, "the plain call before")
                before = held()
                got = radiance(t, o, d, 2, seg)
                assert_records_equal(got, ref, "between render calls")
                for kind, _ in KINDS:
                    it, rec = items_of(pos, nrm), np.zeros((5, FLOATS[kind]), F)
                    t._check(fn_of(t, kind)(t._ctx, it.ctypes.data_as(C.c_void_p), 5, 64, 2, rec.ctypes.data_as(C.c_void_p)))
                after = held()
                assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)), "accumulation"
                assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32)), "estimate state"
                assert all(np.array_equal(before[2][k].view(np.uint32), after[2][k].view(np.uint32)) for k in before[2]), "feature planes"
                assert all(np.array_equal(before[k], after[k]) for k in (3, 4, 5)), "canvas and textures"
                assert before[6:] == after[6:], "pt_last_trace_build, the path and the error state"
                assert np.array_equal(radiance(t, o, d, 2, seg), got), "first_pass did not move: the same call, the same bits"
                assert_records_equal(radiance(t, o, d, 2, seg_plain, fn=t.lib.pt_query_radiance), plain, "the plain call after")
            t.reproject()  # (the history planes kept before the calls still answer)
            rs = t.reproject_stats()
            t.reset()
            t.render_passes(2)  # (the same first_pass: had a call moved it, these passes would differ)
            assert t.last_trace_build() == abi.BUILD_NEXT_EVENT
            assert np.array_equal(t.accum().view(np.uint32), frame.view(np.uint32)), "a next-event render afterwards: nee_ref.render's bits"
            out.append((t.accum(), t.error_state(), (rs.pixels_hit, rs.pixels_kept, rs.samples_kept), t.last_trace_build(), t.stats().total_spp))
        finally:
            t.close()
    a, b = out
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2] and a[2][1] > 0, "the history planes: reprojection's tallies"
    assert a[3:] == b[3:]


# ------------------------------------------------------------------------------------------------ (f) invalid rays
@pytest.mark.parametrize("name,path", [("room", abi.PT_GEOM_SMALL), ("padded", abi.PT_GEOM_GRID)], ids=["small", "grid"])
def test_invalid_rays_give_zeros_and_no_segment(name, path):
    sph, p = SCENES[name]()
    n = 160
    o, d, ref, seg_n = room_rays(name, n)
    bad_o, bad_d = Q.invalid_rays()
    places = [0, 63, 64, n - 1]
    only = np.arange(n)[:, None]
    per_ray = [RN.records(sph, p, np.where(only == k, o, 0), np.where(only == k, d, 0), PASSES)[1] for k in places]  # the replaced rays' segments
    t = context(sph, p, path)
    try:
        for call in range(5):  # 19 classes over 5 x 4 places
            oo, dd = o.copy(), d.copy()
            for j, at in enumerate(places):
                k = (call * len(places) + j) % len(bad_o)
                oo[at], dd[at] = bad_o[k], bad_d[k]
            assert int(Q.valid(oo, dd).sum()) == n - len(places)
            got = radiance(t, oo, dd, PASSES, seg_n - sum(per_ray))  # (no segment is counted for an invalid ray)
            want = RN.raw(ref).copy()
            want[places] = 0
            assert np.array_equal(got, want), "call %d" % call
        all_bad = radiance(t, bad_o[np.arange(PIX + 3) % 19], bad_d[np.arange(PIX + 3) % 19], PASSES, 0)
        assert not all_bad.any()
        assert np.array_equal(radiance(t, o, d, PASSES, seg_n), RN.raw(ref)), "after the invalid batches"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (g) bands
def test_a_band_answers_by_its_own_rows_seeds():
    sph, p = padded()
    o, d, whole, _ = room_rays("padded", 400)
    for rows, index, count in ((4, 1, 3), (8, 0, 2)):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = rows, index, count
        ref, seg, shadow = RN.records(sph, q, o, d, PASSES)
        assert shadow > 0 and not RN.has_nan(ref)
        assert not np.array_equal(RN.raw(ref), RN.raw(whole)), "a band's places have other pixel centres and batches"
        t = context(sph, q, abi.PT_GEOM_GRID)
        try:
            assert 0 < t.local_rows < H and t.query_batch() == t.local_rows * W == RR.batch(q)  # (296 and 481 places: the 400 rays in batches of the band's size)
            assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "band %d of %d" % (index, count))
        finally:
            t.close()


def test_a_band_without_rows_cannot_answer():
    sph, p = padded()
    q = p.copy()
    q.band_rows, q.band_index, q.band_count = 4, 7, 8  # 21 rows are six chunks of four: ranks 6 and 7 own none
    t = context(sph, q, abi.PT_GEOM_GRID)
    try:
        assert t.local_rows == 0
        rays, out = pack([[0, 0, 0]], [[0, 0, -1]]), np.full((1, 4), GUARD, np.uint32)
        rp, op = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        for fn in (t.lib.pt_query_radiance_nee, t.lib.pt_query_radiance):  # refused as the namesake is
            assert fn(t._ctx, rp, 1, 1, op) == abi.PT_ERR_NOT_READY
            assert b"owns no rows" in t.lib.pt_last_error(t._ctx) and (out == GUARD).all()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (h) errors
def test_errors_of_the_entry_points():
    sph, p = room()
    o, d, ref, seg = room_rays()
    rays, out = pack(o[:1], d[:1]), np.full((2, 28), GUARD, np.uint32)
    it = items_of(*gather_items(2))
    rp, ip, op = rays.ctypes.data_as(C.c_void_p), it.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for order in ("queries first", "next event first"):
        t = PathTracer(W, H)
        lib = t.lib
        calls = (("pt_query_radiance_nee", lambda n_passes=1, r=rp, o_=op, n=1: lib.pt_query_radiance_nee(t._ctx, r, n, n_passes, o_)),
                 ("pt_gather_irradiance_nee", lambda n_passes=1, r=ip, o_=op, n=2: lib.pt_gather_irradiance_nee(t._ctx, r, n, 64, n_passes, o_)),
                 ("pt_bake_probes_nee", lambda n_passes=1, r=ip, o_=op, n=2: lib.pt_bake_probes_nee(t._ctx, r, n, 64, n_passes, o_)))
        try:
            t.set_spheres(sph)
            t.set_params(p)
            # the option off, in either order of turning the two on
            if order == "queries first":
                t.ray_queries(True)
                for name, call in calls:
                    assert call() == abi.PT_ERR_NOT_READY, name
                    err = lib.pt_last_error(t._ctx)
                    assert err.startswith(name.encode() + b": ") and b"is off (pt_set_option PT_OPT_NEXT_EVENT)" in err, err
                t.next_event(True)
            else:
                t.next_event(True)
                for name, call in calls:
                    assert call() == abi.PT_ERR_NOT_READY, name
                    err = lib.pt_last_error(t._ctx)
                    assert err.startswith(name.encode() + b": ") and b"are off (pt_set_option PT_OPT_RAY_QUERIES)" in err, err
                t.ray_queries(True)
            seg0 = t.stats().segments
            for name, call in calls:
                assert call(r=None) == abi.PT_ERR_INVALID and b"NULL" in lib.pt_last_error(t._ctx)
                assert call(o_=None) == abi.PT_ERR_INVALID
                assert call(n=0, r=None, o_=None) == abi.PT_OK, "n == 0: nothing done"
                assert call(n_passes=0) == abi.PT_ERR_INVALID and lib.pt_last_error(t._ctx) == name.encode() + b": n_passes == 0"
                assert call(n_passes=2) == abi.PT_ERR_CAPACITY and b"reserved" in lib.pt_last_error(t._ctx)  # one pass is reserved
            assert lib.pt_gather_irradiance_nee(t._ctx, ip, 2, 63, 1, op) == abi.PT_ERR_INVALID and b"directions" in lib.pt_last_error(t._ctx)
            assert (out == GUARD).all() and t.stats().segments == seg0, "refused before anything was launched"
            # the namesake's checks come first: with the option off again, n_passes == 0 is still what is said
            t.next_event(False)
            assert calls[0][1](n_passes=0) == abi.PT_ERR_INVALID and b"n_passes == 0" in lib.pt_last_error(t._ctx)
            assert calls[1][1](n_passes=0) == abi.PT_ERR_INVALID and lib.pt_gather_irradiance_nee(t._ctx, ip, 2, 63, 1, op) == abi.PT_ERR_INVALID
            assert b"directions" in lib.pt_last_error(t._ctx)
            assert calls[0][1]() == abi.PT_ERR_NOT_READY and b"PT_OPT_NEXT_EVENT" in lib.pt_last_error(t._ctx)
            assert lib.pt_query_radiance(t._ctx, rp, 1, 1, op) == abi.PT_OK, "the plain call does not ask for the option"
            out[:] = GUARD
            t.next_event(True)
            # ... and the context is usable
            t.reserve_passes(PASSES)
            assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "after the refusals (%s)" % order)
        finally:
            t.close()


def test_a_call_inside_a_stream_capture_is_refused():
    import torch

    sph, p = room()
    o, d, ref, seg = room_rays()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = context(sph, p, use_torch=True)  # binds the side stream as its launch stream
        rays = torch.from_numpy(pack(o[:64], d[:64])).cuda()
        out = torch.full((64, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        seg0 = t.stats().segments
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = t.lib.pt_query_radiance_nee(t._ctx, C.c_void_p(rays.data_ptr()), 64, 1, C.c_void_p(out.data_ptr()))
            err = t.lib.pt_last_error(t._ctx)
            t.render_passes(1)  # (something to capture)
    torch.cuda.synchronize()
    assert rc == abi.PT_ERR_INVALID and b"capture" in err
    assert (out.cpu().numpy() == 0x5a5a5a5a).all() and t.stats().segments == seg0, "refused before anything was launched"
    assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "the context is still usable")
    t.close()


# ------------------------------------------------------------------------------------------------ (i) device arrays
def test_torch_device_tensors_in_and_out_give_the_host_paths_bytes():
    import torch

    sph, p = room()
    o, d, ref, seg_upto = edge_rays("room")
    n = len(o)
    assert n == 2 * PIX + 5, "three batches, the last of five rays"
    t = context(sph, p, abi.PT_GEOM_SMALL, use_torch=True)
    try:
        host = radiance(t, o, d, PASSES, seg_upto[n])
        assert_records_equal(host, ref, "host rays, host records")
        host_rays = pack(o, d)
        rays = torch.from_numpy(host_rays).cuda()
        out = torch.full((n + 3, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        fn = t.lib.pt_query_radiance_nee
        t._check(fn(t._ctx, C.c_void_p(rays.data_ptr()), n, PASSES, C.c_void_p(out.data_ptr())))
        dev = out.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host), "device rays, device records"
        mixed = np.full((n, 4), GUARD, np.uint32)
        t._check(fn(t._ctx, C.c_void_p(rays.data_ptr()), n, PASSES, mixed.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(mixed, host), "device rays, host records"
        out.fill_(0x5a5a5a5a)
        t._check(fn(t._ctx, host_rays.ctypes.data_as(C.c_void_p), n, PASSES, C.c_void_p(out.data_ptr())))
        dev = out.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host), "host rays, device records"
        # the Python door: tensors in, tensors out; arrays in, arrays out; the default is the plain call
        got = t.query_radiance(torch.from_numpy(o[:100]).cuda(), torch.from_numpy(d[:100]).cuda(), passes=PASSES, next_event=True)
        arr = t.query_radiance(o[:100], d[:100], passes=PASSES, next_event=True)
        assert all(v.is_cuda and v.dtype == torch.float32 for v in got.values()) and all(isinstance(v, np.ndarray) for v in arr.values())
        for res in ({k: v.cpu().numpy() for k, v in got.items()}, arr):
            assert np.array_equal(np.ascontiguousarray(res["sum"]).view(np.uint32), host[:100, :3])
            assert np.array_equal(np.ascontiguousarray(res["samples"]).view(np.uint32), host[:100, 3])
        default = t.query_radiance(o[:100], d[:100], passes=PASSES)
        plain, _ = RR.records(sph, p, o[:100], d[:100], PASSES)
        assert np.array_equal(np.ascontiguousarray(default["sum"]).view(np.uint32), RR.raw(plain)[:, :3])
        torch.cuda.synchronize()
    finally:
        t.close()
