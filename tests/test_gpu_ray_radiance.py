"""Radiance queries (pt_query_radiance; include/ptrace.h has the contract) on the device, bit for bit.

Every comparison is equal uint32 views of the raw 16-byte records against tests/radiance_ref.py — the contract restated from
the oracle's exported pieces, pinned on the CPU by tests/test_radiance_ref.py.  Tolerance: none.  The restatement's records of
every tested ray hold no NaN, which each test asserts of the reference before it compares.  PtStats.segments moves by exactly
the restatement's segment total; samples, total_spp and render_launches do not move.  Unless stated: the time step
PT_TIME_STEP_DECORRELATED, max_depth 6, 2 samples per pixel, 3 passes, at 37x21 (777 places).

  (a) every row      each of the twelve kernels of csrc/pt_kernels_radiance.hip, with the scenes of test_gpu_features.py: the
                     context's own 777 pinhole rays, 200 bounce-style rays from hit points, 50 rays from inside spheres
  (b) batch edges    n = 1, 63, 64, 65, 776, 777, 778, 2*777 + 5 on the small-list and the grid row; what lies behind out[n]
  (c) passes, params n_passes 1 and the whole reservation, 1 and 5 samples, first_pass, time_step 0, depth 1 and 50, a black
                     background, a negative radius, an emissive sphere, the same call twice
  (d) far rays, the literal loop
  (e) invalid rays   every class at places 0, 31, 63, 64 and the last, and a whole wave of them
  (f) undisturbed    accumulation, estimate, feature planes, history, canvas, textures, first_pass, build, path; roulette, overlay
  (g) bands          a band answers by its own rows' seeds; a band without rows
  (h) errors         every PT_ERR_* of the header that can be raised, a stream capture
  (i) device arrays  torch tensors in and out
  (j) full size      config 5 at 1920x1080 on the grid pt_tune kept
"""
import ctypes as C

import numpy as np
import pytest

import overlay_ref as R
import query_ref as Q
import radiance_ref as RR
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_features import H, ROW_IDS, ROWS, W, scene
from test_gpu_ray_queries import SplitMix64, pack, pinhole
from trace_builds import build_of

pytestmark = pytest.mark.gpu

PIX = W * H  # 777 local pixels: the batch
KERNELS = sorted({k.replace("_feat", "_rad") for k, _, _ in ROWS})
REACHED = {}
GUARD = 0xa5a5a5a5
PASSES = 3
D, M, G, E = abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS, abi.PT_EMISSIVE


def settings(p, spp=2, depth=6, first_pass=0, step=abi.PT_TIME_STEP_DECORRELATED, bg=None):
    q = p.copy()
    q.samples_per_pixel, q.max_depth, q.first_pass, q.time_step = spp, depth, first_pass, step
    if bg is not None:
        q.background_mode = bg
    return q


def context(sph, p, path=None, reserve=PASSES, features=False, use_torch=False):
    t = PathTracer(p.width, p.height, use_torch=use_torch) if use_torch else PathTracer(p.width, p.height)
    if path is not None:
        t.set_geometry_path(path)
    t.set_spheres(sph)
    if features:
        t.feature_planes(True)
    t.ray_queries(True)
    t.reserve_passes(reserve)
    t.set_params(p)
    return t


def radiance(t, o, d, n_passes=PASSES, segments=None):
    """the raw records, (n, 4) uint32, through the C entry point; three records of guard bytes behind out[n] stay as they are;
    PtStats.segments moves by `segments` (the restatement's total) and nothing else of the tallies moves"""
    rays = pack(o, d)
    n = len(rays)
    out = np.full((n + 3, 4), GUARD, np.uint32)
    before = t.stats()
    t._check(t.lib.pt_query_radiance(t._ctx, rays.ctypes.data_as(C.c_void_p), n, n_passes, out.ctypes.data_as(C.c_void_p)))
    after = t.stats()
    assert (out[n:] == GUARD).all(), "records written behind out[n]"
    if segments is not None:
        assert after.segments - before.segments == segments, (after.segments - before.segments, segments)
    assert (after.samples, after.total_spp, after.render_launches) == (before.samples, before.total_spp, before.render_launches)
    return out[:n]


def assert_records_equal(got, ref, what):
    assert not RR.has_nan(ref), what + ": the restatement holds a NaN"
    want = RR.raw(ref)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=1))[:, 0]
        k = int(bad[0])
        raise AssertionError("%s: %d of %d records differ, first ray %d:\n got  %r\n want %r" % (
            what, len(bad), len(got), k, got[k].view(np.float32), want[k].view(np.float32)))


def check(t, sph, p, o, d, what, n_passes=PASSES):
    ref, seg = RR.records(sph, p, o, d, n_passes)
    got = radiance(t, o, d, n_passes, seg)
    assert_records_equal(got, ref, what)
    return got, ref


def kernel_of(t, path):
    """the radiance kernel a launch through the forced `path` is: the row's cell of the table's radiance column (pinned on the CPU: test_trace_builds.py)"""
    return build_of(t.stats(), "_rad", path=abi.PT_GEOM_SCALAR if path == abi.PT_GEOM_LDS else path)


# ------------------------------------------------------------------------------------------------ (a) every row
_ROW_RAYS = {}


def row_rays(name):
    """(origins, directions, first-hit records, radiance records, segments) of the 777 pinhole rays of scene(name), 200
    bounce-style rays from their hit points and 50 rays from inside spheres, under the common settings: made once"""
    if name not in _ROW_RAYS:
        sph, p = scene(name)
        o, d, first = pinhole(name)
        hit = first["index"] >= 0
        rng = SplitMix64(0x2400 + len(sph))
        pts = first["point"][hit]
        bo, bd = pts[(np.arange(200) * 3) % len(pts)], rng.unit(200)
        io, idir = sph["center"][(np.arange(50) * 7 + 1) % len(sph)].astype(np.float32), rng.unit(50)
        oo, dd = np.concatenate([o, bo, io]), np.concatenate([d, bd, idir])
        ref, seg = RR.records(sph, settings(p), oo, dd, PASSES)
        _ROW_RAYS[name] = (oo, dd, Q.records(sph, p, oo, dd), ref, seg)
    return _ROW_RAYS[name]


@pytest.mark.parametrize("row", ROWS, ids=[i.replace("_feat", "_rad") for i in ROW_IDS])
def test_every_row_of_the_variant_table(row):
    kernel, name, path = row[0].replace("_feat", "_rad"), row[1], row[2]
    sph, p = scene(name)
    o, d, first, ref, seg = row_rays(name)
    assert len(o) == PIX + 250 and (first["index"] < 0).any(), "the case shows a miss"
    for ty in (D, M, G):  # ... and a first hit of every material its scene has
        assert ty not in set(sph["type"].tolist()) or (first["type"] == ty).any(), (name, ty)
    assert seg > 2 * PASSES * len(o), "paths of more than one segment"
    t = context(sph, settings(p), path)
    try:
        build0, st0 = t.last_trace_build(), t.stats()
        got = radiance(t, o, d, PASSES, seg)  # (two batches: the bounce-style and inside rays take the second one's passes)
        assert kernel_of(t, path) == kernel, (kernel, kernel_of(t, path))
        st = t.stats()
        assert t.last_trace_build() == build0 and (st.geometry_path, st.geometry_tuned) == (st0.geometry_path, st0.geometry_tuned)
        assert_records_equal(got, ref, "%s through %s" % (name, kernel))
        assert (got[:, 3].view(np.float32) == 2 * PASSES).all()
        REACHED.setdefault(kernel, []).append("%s/%s" % (name, abi.GEOM_NAMES[path]))
    finally:
        t.close()


def test_every_radiance_kernel_was_reached():
    """(runs after the test above) each of the twelve kernels of csrc/pt_kernels_radiance.hip was launched and compared"""
    print("radiance kernels reached\n" + "\n".join("  %-18s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in KERNELS))
    assert len(KERNELS) == 12 and sorted(REACHED) == KERNELS, sorted(set(KERNELS) - set(REACHED))


# ------------------------------------------------------------------------------------------------ (b) batch edges
COUNTS = [1, 63, 64, 65, PIX - 1, PIX, PIX + 1, 2 * PIX + 5]
_EDGE = {}


def edge_rays(name):
    """2 * 777 + 5 different rays (pinhole directions in another order, longer from batch to batch) and, per count, the
    restatement's records and segments — a ray's record depends on its index only, so the records of n rays are the first n"""
    if name not in _EDGE:
        sph, p = scene(name)
        o, d, _ = pinhole(name)
        i = np.arange(COUNTS[-1])
        pick = (i * 7) % PIX
        dd = d[pick] * (1 + i // PIX).astype(np.float32)[:, None]
        oo = o[pick]
        ref = np.zeros((len(i), 4), np.float32)
        seg_upto = {0: 0}
        last = 0
        for n in COUNTS:  # in pieces, so that every count has its segment total
            part, seg = _records_from(sph, settings(p), oo, dd, last, n)
            ref[last:n] = part
            seg_upto[n] = seg_upto[last] + seg
            last = n
        _EDGE[name] = (oo, dd, ref, seg_upto)
    return _EDGE[name]


def _records_from(sph, p, o, d, a, b, n_passes=PASSES):
    """the records of rays a .. b - 1 of a call (their indices count): the whole call's restatement is made of valid rays only
    where it is asked, by marking every other ray invalid"""
    oo, dd = o[:b].copy(), d[:b].copy()
    dd[:a] = 0.0  # a direction of three zeros: no record, no segment
    ref, seg = RR.records(sph, p, oo, dd, n_passes)
    return ref[a:b], seg


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,path", [("small9", abi.PT_GEOM_SMALL), ("cover", abi.PT_GEOM_GRID)], ids=["small", "grid"])
def test_batch_edges(name, path, n):
    sph, p = scene(name)
    o, d, ref, seg_upto = edge_rays(name)
    t = context(sph, settings(p), path)
    try:
        got = radiance(t, o[:n], d[:n], PASSES, seg_upto[n])  # (the guard behind out[n], segments exactly)
        assert_records_equal(got, ref[:n], "%s, n = %d" % (name, n))
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (c) passes and params
def some_rays(name, n=160):
    o, d, first, _, _ = row_rays(name)
    pick = (np.arange(n) * 5) % len(o)
    return o[pick], d[pick]


@pytest.mark.parametrize("name,path", [("small9", abi.PT_GEOM_SMALL), ("cover", abi.PT_GEOM_BVH), ("field1500", abi.PT_GEOM_GRID)],
                         ids=["small", "bvh", "grid"])
def test_passes_and_params(name, path):
    sph, p = scene(name)
    o, d = some_rays(name)
    t = context(sph, settings(p), path, reserve=4)
    try:
        check(t, sph, settings(p), o, d, "n_passes 1", 1)
        got, _ = check(t, sph, settings(p), o, d, "the whole reservation", 4)
        again = radiance(t, o, d, 4)
        assert np.array_equal(got, again), "the same call twice"
        for what, q in (("1 spp", settings(p, spp=1)), ("5 spp", settings(p, spp=5)), ("first_pass 11", settings(p, first_pass=11)),
                        ("time_step 0", settings(p, step=0.0, first_pass=2)), ("max_depth 1", settings(p, depth=1)),
                        ("max_depth 50", settings(p, depth=50)), ("a black background", settings(p, bg=abi.PT_BG_BLACK))):
            t.set_params(q)
            check(t, sph, q, o, d, what)
        # a negative radius (a hollow shell: the normal flips) and an emissive sphere, on the spheres these rays meet first
        first = Q.records(sph, p, o, d)
        seen = [int(i) for i in np.unique(first["index"]) if i >= 0]
        assert len(seen) >= 2
        other = sph.copy()
        other["radius"][seen[0]] = -other["radius"][seen[0]]
        other["type"][seen[1]], other["albedo"][seen[1]] = E, (3.0, 2.0, 1.5)
        t.set_spheres(other)
        t.set_params(settings(p))
        got, ref = check(t, other, settings(p), o, d, "a negative radius and an emissive sphere")
        assert (ref[:, :3].max(axis=1) > 2.0 * 2 * PASSES).any(), "the emissive sphere is seen"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (d) far and literal-loop rays
@pytest.mark.parametrize("name", ["field1500", "field10000"])
def test_far_rays_through_the_gathering_grid_build(name):
    sph, _ = scene(name)
    c = sph["center"].astype(np.float64)
    mid, ext = c[1:].mean(axis=0), float(np.abs(c[1:] - c[1:].mean(axis=0)).max())
    # (the uniforms of test_gpu_features' far view: the grid's fit is stale, so the build that gathers its entries runs)
    p = settings(R.look_at(W, H, 1, 8, mid + np.array([60.0, 15.0, 60.0]) * ext / 4.0, mid, 8.0, 100.0))
    rng = SplitMix64(0x24c0 + len(sph))
    out = rng.unit(100).astype(np.float64)
    out[:, 1] = np.abs(out[:, 1])  # from above the ground
    out /= np.linalg.norm(out, axis=1)[:, None]
    o = (mid + 5.0 * ext * out).astype(np.float32)
    d = ((mid + 0.5 * ext * rng.unit(100)) - o).astype(np.float32)
    t = context(sph, p, abi.PT_GEOM_GRID)
    try:
        far0 = t.stats().far_rays
        got, ref = check(t, sph, p, o, d, "%s from five radii out" % name)
        st = t.stats()
        assert st.grid_fit_stale == 1 and st.far_rays - far0 > 0, (st.grid_fit_stale, st.far_rays - far0)
        assert kernel_of(t, abi.PT_GEOM_GRID) == "grid_cells_rad"
        t.set_geometry_path(abi.PT_GEOM_SCALAR)
        far1 = t.stats().far_rays
        scalar = radiance(t, o, d)
        assert t.stats().far_rays == far1 and np.array_equal(got, scalar), "the grid's far path against the scalar walk"
    finally:
        t.close()


@pytest.mark.parametrize("path", [abi.PT_GEOM_SMALL, abi.PT_GEOM_SCALAR, abi.PT_GEOM_BVH, abi.PT_GEOM_GRID], ids=lambda v: abi.GEOM_NAMES[v])
def test_irregular_but_valid_rays_take_the_literal_loop(path):
    name = "small9" if path == abi.PT_GEOM_SMALL else "cover"
    sph, p = scene(name)
    o, d, pin = pinhole(name)
    pick = np.arange(0, PIX, 6)
    o, d, pin = o[pick], d[pick], pin[pick]
    len2 = (d.astype(np.float64) ** 2).sum(axis=1)
    short = (d * np.sqrt(1e-13 / len2)[:, None]).astype(np.float32)
    long_ = (d * np.sqrt(1e7 / len2)[:, None]).astype(np.float32)
    a_short, a_long = (short.astype(np.float64) ** 2).sum(axis=1), (long_.astype(np.float64) ** 2).sum(axis=1)
    assert (a_short < 1e-12).all() and (a_long > 1e6).all()   # outside regular_ray's (1e-12, 1e6)
    near = (pin["point"].astype(np.float64) - 0.01 * d / np.sqrt(len2)[:, None]).astype(np.float32)
    o_short = np.where((pin["index"] >= 0)[:, None], near, o)
    far_o = np.float32([[2e15, 0.5, 0.25], [0.5, 2e15, 0.25], [0.5, 0.25, -2e15]] * 4)
    far_d = np.concatenate([-far_o[:3] / np.float32(2e15), SplitMix64(0x24d0).unit(9)]).astype(np.float32)
    oo, dd = np.concatenate([o_short, o, far_o]), np.concatenate([short, long_, far_d])
    t = context(sph, settings(p), path)
    try:
        check(t, sph, settings(p), oo, dd, "irregular rays through %s" % abi.GEOM_NAMES[path])
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (e) invalid rays
@pytest.mark.parametrize("name,path", [("small9", abi.PT_GEOM_SMALL), ("cover", abi.PT_GEOM_GRID)], ids=["small", "grid"])
def test_invalid_rays_give_zeros_and_their_neighbours_do_not_notice(name, path):
    sph, p = scene(name)
    p = settings(p)
    o, d, _ = pinhole(name)
    bad_o, bad_d = Q.invalid_rays()
    n = 200
    places = [0, 31, 63, 64, n - 1]
    ref, _ = RR.records(sph, p, o, d, PASSES)
    assert not RR.has_nan(ref)
    per_ray = [RR.records(sph, p, np.where(np.arange(n)[:, None] == k, o[:n], 0), np.where(np.arange(n)[:, None] == k, d[:n], 0), PASSES)[1]
               for k in places]  # the segments of the rays that are replaced
    seg_n = RR.records(sph, p, o[:n], d[:n], PASSES)[1]
    t = context(sph, p, path)
    try:
        for call in range(4):  # 19 classes over 4 x 5 places
            oo, dd = o[:n].copy(), d[:n].copy()
            for j, at in enumerate(places):
                k = (call * len(places) + j) % len(bad_o)
                oo[at], dd[at] = bad_o[k], bad_d[k]
            assert int(Q.valid(oo, dd).sum()) == n - len(places)
            got = radiance(t, oo, dd, PASSES, seg_n - sum(per_ray))  # (no segment is counted for an invalid ray)
            want = RR.raw(ref[:n]).copy()
            want[places] = 0
            assert np.array_equal(got, want), "call %d" % call
        # a whole wave of invalid rays, and a batch of nothing else: the waves go on to the items behind them
        oo, dd = o.copy(), d.copy()
        oo[64:128], dd[64:128] = bad_o[np.arange(64) % 19], bad_d[np.arange(64) % 19]
        got = radiance(t, oo, dd)
        want = RR.raw(ref).copy()
        want[64:128] = 0
        assert np.array_equal(got, want)
        all_bad = radiance(t, bad_o[np.arange(PIX + 3) % 19], bad_d[np.arange(PIX + 3) % 19], PASSES, 0)
        assert not all_bad.any()
        got = radiance(t, o, d)
        assert np.array_equal(got, RR.raw(ref)), "after the invalid batches"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (f) nothing else moves
def test_nothing_else_of_the_context_moves():
    """two contexts do the same things; one of them asks for radiance in between.  Every read-out and every later result agree:
    k passes, a query, k more passes give the bits of 2 k uninterrupted passes."""
    sc = scenes.default_scene(96, 54, spp=2, max_depth=6)
    p = sc.params.copy()
    p.time_step, p.first_pass = abi.PT_TIME_STEP_DECORRELATED, 3
    p.render_count, p.should_average, p.last_frame_weight = 1, 1, 1.0
    o, d = Q.pinhole_rays(scenes.default_scene(37, 21, spp=1, max_depth=8).params)
    ref, seg = RR.records(sc.spheres, p, o, d, 2)
    hits_ref = Q.records(sc.spheres, p, o[:64], d[:64])
    out = []
    for asks in (True, False):
        t = context(sc.spheres, p, abi.PT_GEOM_SMALL, reserve=2, features=True)
        try:
            t.error_estimate(True)
            t.reproject_option(True)
            t.reset()
            t.render_passes(2)
            t.render_features()
            t.keep_history()
            t.clear_textures()
            t.render_frame(1)
            rays64 = pack(o[:64], d[:64])
            hits = np.zeros((64, 16), np.uint32)
            t._check(t.lib.pt_query_rays(t._ctx, rays64.ctypes.data_as(C.c_void_p), 64, hits.ctypes.data_as(C.c_void_p)))
            if asks:
                held = (t.accum(), t.error_state(), t.features(), t.read_canvas(), t.read_texture(0), t.read_texture(1), t.last_trace_build(),
                        hits.copy(), t.stats())
                got = radiance(t, o, d, 2, seg)
                assert_records_equal(got, ref, "between render calls")
                now = (t.accum(), t.error_state(), t.features(), t.read_canvas(), t.read_texture(0), t.read_texture(1), t.last_trace_build(),
                       hits, t.stats())
                assert np.array_equal(held[0].view(np.uint32), now[0].view(np.uint32)), "accumulation"
                assert np.array_equal(held[1].view(np.uint32), now[1].view(np.uint32)), "estimate state"
                assert all(np.array_equal(held[2][k].view(np.uint32), now[2][k].view(np.uint32)) for k in held[2]), "feature planes (still valid)"
                assert all(np.array_equal(held[k], now[k]) for k in (3, 4, 5)), "canvas and textures"
                assert held[6] == now[6], "pt_last_trace_build"
                assert np.array_equal(held[7], now[7]) and np.array_equal(hits, Q.raw(hits_ref)), "the records of an earlier pt_query_rays"
                assert (held[8].geometry_path, held[8].geometry_tuned) == (now[8].geometry_path, now[8].geometry_tuned), "the path"
                # first_pass did not move: the same query again gives the same bits
                assert np.array_equal(radiance(t, o, d, 2, seg), got)
            t.reproject()   # (the history planes kept before the query still answer)
            rs = t.reproject_stats()
            t.render_passes(2)  # (the same first_pass: had the query moved it, these passes would differ)
            out.append((t.accum(), t.error_state(), (rs.pixels_hit, rs.pixels_kept, rs.samples_kept), t.last_trace_build(), t.stats().total_spp))
        finally:
            t.close()
    a, b = out
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "accumulation: k passes, a query, k passes against 2 k passes"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "estimate state"
    assert a[2] == b[2] and a[2][1] > 0, "the history planes: reprojection's tallies"
    assert a[3:] == b[3:]


def test_overlay_and_roulette_do_not_act():
    c = R.default_case()
    p = settings(c.params)
    p.width, p.height = W, H
    o, d = some_rays("small9")
    ref, seg = RR.records(c.spheres, p, o, d, PASSES)
    t = context(c.spheres, p, abi.PT_GEOM_SMALL)
    try:
        assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "plain")
        t.set_debug_overlay(True, *c.overlay)
        assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "with the overlay on")
        t.render_passes(1)
        assert t.last_trace_build() == abi.BUILD_DEBUG_OVERLAY
        assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "after an overlay launch")
        assert t.last_trace_build() == abi.BUILD_DEBUG_OVERLAY
        t.set_debug_overlay(False)
        t.set_russian_roulette(2)
        assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "with roulette on")
        t.render_passes(1)
        assert t.last_trace_build() == abi.BUILD_ROULETTE
    finally:
        t.close()


def test_an_unsettled_auto_context_answers_and_settles_nothing():
    sph, p = scene("small9")
    o, d = some_rays("small9")
    t = context(sph, settings(p))  # PT_GEOM_AUTO, nothing rendered yet
    try:
        st0 = t.stats()
        check(t, sph, settings(p), o, d, "unsettled PT_GEOM_AUTO")
        st = t.stats()
        assert (st.geometry_tuned, st.geometry_path) == (st0.geometry_tuned, st0.geometry_path) and st0.geometry_tuned == 0
    finally:
        t.close()


def test_the_camera_the_lens_and_render_count_do_not_enter():
    sph, p = scene("cover")
    o, d = some_rays("cover")
    q = settings(R.look_at(W, H, 2, 6, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 5.0))  # another camera
    q.lens_radius, q.render_count = 0.3, 9
    q.time = p.time
    ref, seg = RR.records(sph, settings(p), o, d, PASSES)
    t = context(sph, q, abi.PT_GEOM_GRID)
    try:
        assert_records_equal(radiance(t, o, d, PASSES, seg), ref, "under another camera's uniforms")
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (g) bands
def test_a_band_answers_by_its_own_rows_seeds():
    sph, p = scene("cover")
    o, d = some_rays("cover", 400)
    whole, _ = RR.records(sph, settings(p), o, d, PASSES)
    for rows, index, count in ((4, 1, 3), (8, 0, 2)):
        q = settings(p)
        q.band_rows, q.band_index, q.band_count = rows, index, count
        t = context(sph, q, abi.PT_GEOM_GRID)
        try:
            assert 0 < t.local_rows < H and t.query_batch() == t.local_rows * W == RR.batch(q)
            got, ref = check(t, sph, q, o, d, "band %d of %d" % (index, count))  # several batches of the band's size
            assert not np.array_equal(RR.raw(ref), RR.raw(whole)), "a band's places have other pixel centres and batches"
        finally:
            t.close()


def test_a_band_without_rows_cannot_answer():
    sph, p = scene("cover")
    q = settings(p)
    q.band_rows, q.band_index, q.band_count = 4, 7, 8  # 21 rows are six chunks of four: ranks 6 and 7 own none
    t = context(sph, q, abi.PT_GEOM_GRID)
    try:
        assert t.local_rows == 0
        rays, out = pack([[0, 0, 0]], [[0, 0, -1]]), np.full((1, 4), GUARD, np.uint32)
        assert t.lib.pt_query_radiance(t._ctx, rays.ctypes.data_as(C.c_void_p), 1, 1, out.ctypes.data_as(C.c_void_p)) == abi.PT_ERR_NOT_READY
        assert b"owns no rows" in t.lib.pt_last_error(t._ctx) and (out == GUARD).all()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (h) errors
def test_errors_of_the_entry_point():
    sph, p = scene("cover")
    p = settings(p)
    t = PathTracer(W, H)
    lib = t.lib
    rays, out = pack([[0, 0, 5]], [[0, 0, -1]]), np.full((2, 4), GUARD, np.uint32)
    rp, op = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    try:
        assert lib.pt_query_radiance(t._ctx, rp, 1, 1, op) == abi.PT_ERR_NOT_READY and b"PT_OPT_RAY_QUERIES" in lib.pt_last_error(t._ctx)
        t.ray_queries(True)
        assert lib.pt_query_radiance(t._ctx, rp, 1, 1, op) == abi.PT_ERR_NOT_READY and b"pt_set_spheres" in lib.pt_last_error(t._ctx)
        t.set_spheres(sph)
        assert lib.pt_query_radiance(t._ctx, rp, 1, 1, op) == abi.PT_ERR_NOT_READY  # no uniforms yet
        t.set_params(p)
        assert lib.pt_query_radiance(t._ctx, None, 1, 1, op) == abi.PT_ERR_INVALID and lib.pt_query_radiance(t._ctx, rp, 1, 1, None) == abi.PT_ERR_INVALID
        seg = t.stats().segments
        assert lib.pt_query_radiance(t._ctx, None, 0, 0, None) == abi.PT_OK and t.stats().segments == seg  # n == 0: nothing done
        t.set_count_work(True)
        assert lib.pt_query_radiance(t._ctx, rp, 1, 1, op) == abi.PT_ERR_INVALID and b"COUNT_WORK" in lib.pt_last_error(t._ctx)
        t.set_count_work(False)
        assert lib.pt_query_radiance(t._ctx, rp, 1, 0, op) == abi.PT_ERR_INVALID and b"n_passes == 0" in lib.pt_last_error(t._ctx)
        assert lib.pt_query_radiance(t._ctx, rp, 1, 2, op) == abi.PT_ERR_CAPACITY and b"reserved" in lib.pt_last_error(t._ctx)  # one pass is reserved
        assert (out == GUARD).all() and t.stats().segments == seg
        assert lib.pt_query_radiance(t._ctx, rp, 1, 1, op) == abi.PT_OK and (out[1] == GUARD).all() and out[0, 3] == np.float32(2.0).view(np.uint32)
        t.reserve_passes(2)
        assert lib.pt_query_radiance(t._ctx, rp, 1, 2, op) == abi.PT_OK and out[0, 3] == np.float32(4.0).view(np.uint32)
        t.ray_queries(False)
        assert lib.pt_query_radiance(t._ctx, rp, 1, 1, op) == abi.PT_ERR_NOT_READY
    finally:
        t.close()


def test_a_call_inside_a_stream_capture_is_refused():
    import torch

    sph, p = scene("cover")
    p = settings(p)
    o, d = some_rays("cover", 64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = context(sph, p, use_torch=True)  # binds the side stream as its launch stream
        rays = torch.from_numpy(pack(o, d)).cuda()
        out = torch.full((64, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        seg = t.stats().segments
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = t.lib.pt_query_radiance(t._ctx, C.c_void_p(rays.data_ptr()), 64, 1, C.c_void_p(out.data_ptr()))
            t.render_passes(1)  # (something to capture)
    torch.cuda.synchronize()
    assert rc == abi.PT_ERR_INVALID and b"capture" in t.lib.pt_last_error(t._ctx)
    assert (out.cpu().numpy() == 0x5a5a5a5a).all() and t.stats().segments == seg, "refused before anything was launched"
    t.close()


# ------------------------------------------------------------------------------------------------ (i) device arrays
def test_torch_device_tensors_in_and_out_give_the_same_bytes():
    import torch

    sph, p = scene("cover")
    p = settings(p)
    o, d, ref, _ = edge_rays("cover")
    n = len(o)
    assert n == 2 * PIX + 5
    t = context(sph, p, use_torch=True)
    try:
        host = radiance(t, o, d)
        assert_records_equal(host, ref, "host arrays")
        rays = torch.from_numpy(pack(o, d)).cuda()
        out = torch.full((n + 3, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        t._check(t.lib.pt_query_radiance(t._ctx, C.c_void_p(rays.data_ptr()), n, PASSES, C.c_void_p(out.data_ptr())))
        dev = out.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host)
        # ... mixed: device rays, host records
        mixed = np.full((n, 4), GUARD, np.uint32)
        t._check(t.lib.pt_query_radiance(t._ctx, C.c_void_p(rays.data_ptr()), n, PASSES, mixed.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(mixed, host)
        # ... and the other way round: host rays (three batches, the last of five rays), device records
        out.fill_(0x5a5a5a5a)
        host_rays = pack(o, d)
        t._check(t.lib.pt_query_radiance(t._ctx, host_rays.ctypes.data_as(C.c_void_p), n, PASSES, C.c_void_p(out.data_ptr())))
        dev = out.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host)
        # the Python door: tensors in, tensors out; arrays in, arrays out; the mean is sum / samples, 0 for an invalid ray
        oo, dd = o[:100].copy(), d[:100].copy()
        dd[7] = 0.0
        got = t.query_radiance(torch.from_numpy(oo).cuda(), torch.from_numpy(dd).cuda(), passes=PASSES)
        arr = t.query_radiance(oo, dd, passes=PASSES)
        assert all(v.is_cuda and v.dtype == torch.float32 for v in got.values()) and all(isinstance(v, np.ndarray) for v in arr.values())
        want = RR.raw(ref[:100]).copy()
        want[7] = 0
        for res in ({k: v.cpu().numpy() for k, v in got.items()}, arr):
            assert res["sum"].shape == res["mean"].shape == (100, 3) and res["samples"].shape == (100,)
            assert np.array_equal(np.ascontiguousarray(res["sum"]).view(np.uint32), want[:, :3])
            assert np.array_equal(np.ascontiguousarray(res["samples"]).view(np.uint32), want[:, 3])
            assert not res["mean"][7].view(np.uint32).any() and res["samples"][7] == 0
            ok = np.arange(100) != 7
            assert np.array_equal(res["mean"][ok], res["sum"][ok] / np.float32(2 * PASSES))
        torch.cuda.synchronize()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (j) full size
def test_config5_full_size_on_the_grid_pt_tune_kept():
    sc = scenes.config5(1920, 1080, 1, 1, 8)
    p = settings(sc.params, spp=1, depth=8)
    t = context(sc.spheres, p, reserve=1)
    try:
        t.tune(1)
        st = t.stats()
        assert st.geometry_tuned == 1 and st.geometry_path == abi.PT_GEOM_GRID
        o, d = Q.pinhole_rays(sc.params)
        pick = (np.arange(512) * 4051) % len(o)  # 512 of the frame's own rays, from all over it
        o, d = o[pick], d[pick]
        first = Q.records(sc.spheres, p, o, d)
        assert (first["index"] >= 0).mean() > 0.5 and len(np.unique(first["index"])) > 100
        check(t, sc.spheres, p, o, d, "config 5 at 1920x1080", 1)
        assert kernel_of(t, abi.PT_GEOM_GRID) in ("grid_cells_rad", "grid_gmem_rad")
    finally:
        t.close()
