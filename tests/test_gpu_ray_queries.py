"""Ray queries (PT_OPT_RAY_QUERIES, pt_query_rays; include/ptrace.h has the contract) on the device, bit for bit.

Every comparison is equal uint32 views of the raw 64-byte records against tests/query_ref.py — the contract restated from the
oracle's exported pieces, pinned on the CPU by tests/test_query_ref.py — or against the feature planes / the scalar walk of the
same context.  Tolerance: none.  The restatement's records of every tested ray hold no NaN, which each test asserts of the
reference before it compares (NaN payloads are no part of the contract).

  (a) every row      each of the twelve kernels of csrc/pt_kernels_query.hip, reached with the scenes of
                     test_gpu_features.py at 37x21: the context's own 777 pinhole rays (which also equal the feature planes
                     of the same context), 200 bounce-style rays from hit points, 50 rays from inside spheres
  (b) batch edges    n = 1, 63, 64, 65, 776, 777, 778, 2*777 + 5 on the small-list and the grid row; what lies behind hits[n]
  (c) far rays       origins five scene radii out, through the gathering grid build, against the scalar walk and the oracle
  (d) literal loop   |d|^2 of 1e-13 and 1e7, an origin component of 2e15
  (e) invalid rays   every class at lanes 0, 31, 63, 64 and the last index, and a whole wave of them
  (f) undisturbed    accumulation, estimate, feature planes, history, canvas, textures, first_pass, tile order, build, path
  (g) bands          a band answers like the whole image; a band without rows
  (h) errors         every PT_ERR_* of the header that can be raised, a stream capture
  (i) device arrays  torch tensors in and out
  (j) full size      config 5 at 1920x1080 on the grid pt_tune kept against pt_render_features
"""
import ctypes as C

import numpy as np
import pytest

import overlay_ref as R
import query_ref as Q
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gpu_features import H, ROW_IDS, ROWS, W, scene
from trace_builds import build_of

pytestmark = pytest.mark.gpu

PIX = W * H  # 777 local pixels: the batch
KERNELS = sorted({k.replace("_feat", "_qry") for k, _, _ in ROWS})
REACHED = {}
GUARD = 0xa5a5a5a5


def context(sph, p, path=None, features=True, queries=True):
    t = PathTracer(p.width, p.height)
    if path is not None:
        t.set_geometry_path(path)
    t.set_spheres(sph)
    if features:
        t.feature_planes(True)
    if queries:
        t.ray_queries(True)
    t.set_params(p)
    return t


def pack(o, d):
    """(n, 8) float32 PtRay records; the pads hold NaN, which the library must not read"""
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    rays = np.full((len(o), 8), np.nan, np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    return rays


def query(t, o, d):
    """the raw records, (n, 16) uint32, through the C entry point; three records of guard bytes behind hits[n] stay as they are;
    PtStats.segments moves by the valid rays and nothing else of the tallies moves"""
    rays = pack(o, d)
    n = len(rays)
    hits = np.full((n + 3, 16), GUARD, np.uint32)
    before = t.stats()
    t._check(t.lib.pt_query_rays(t._ctx, rays.ctypes.data_as(C.c_void_p), n, hits.ctypes.data_as(C.c_void_p)))
    after = t.stats()
    assert (hits[n:] == GUARD).all(), "records written behind hits[n]"
    assert after.segments - before.segments == int(Q.valid(o, d).sum()), (after.segments - before.segments, n)
    assert (after.samples, after.total_spp, after.render_launches) == (before.samples, before.total_spp, before.render_launches)
    return hits[:n]


def assert_records_equal(got, ref, what):
    assert not Q.has_nan(ref), what + ": the restatement holds a NaN"
    want = Q.raw(ref)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=1))[:, 0]
        k = int(bad[0])
        raise AssertionError("%s: %d of %d records differ, first ray %d:\n got  %r\n want %r" % (
            what, len(bad), len(got), k, got[k].view(Q.HIT_DTYPE)[0], want[k].view(Q.HIT_DTYPE)[0]))


def kernel_of(t, path):
    """the query kernel a launch through the forced `path` is: the row's cell of the table's query column (pinned on the CPU: test_trace_builds.py)"""
    st = t.stats()
    return build_of(st, "_qry", path=abi.PT_GEOM_SCALAR if path == abi.PT_GEOM_LDS else path)


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & 0xffffffffffffffff

    def next(self):
        self.s = (self.s + 0x9e3779b97f4a7c15) & 0xffffffffffffffff
        z = self.s
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & 0xffffffffffffffff
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & 0xffffffffffffffff
        return z ^ (z >> 31)

    def unit(self, n):
        """(n, 3) float32 in [-1, 1): 24 bits each"""
        return np.float32([[(self.next() >> 40) / float(1 << 23) - 1.0 for _ in range(3)] for _ in range(n)])


# ------------------------------------------------------------------------------------------------ (a) every row
_PINHOLE = {}


def pinhole(name):
    """(origins, directions, records) of the 777 pinhole rays of scene(name): the reference is made once"""
    if name not in _PINHOLE:
        sph, p = scene(name)
        o, d = Q.pinhole_rays(p)
        _PINHOLE[name] = (o, d, Q.records(sph, p, o, d))
    return _PINHOLE[name]


@pytest.mark.parametrize("row", ROWS, ids=[i.replace("_feat", "_qry") for i in ROW_IDS])
def test_every_row_of_the_variant_table(row):
    kernel, name, path = row[0].replace("_feat", "_qry"), row[1], row[2]
    sph, p = scene(name)
    o, d, ref = pinhole(name)
    t = context(sph, p, path)
    try:
        assert t.query_batch() == PIX
        build0 = t.last_trace_build()
        got = query(t, o, d)
        assert kernel_of(t, path) == kernel, (kernel, kernel_of(t, path))
        assert t.last_trace_build() == build0, "a query is no render launch"
        assert_records_equal(got, ref, "%s: pinhole rays through %s" % (name, kernel))
        hit = ref["index"] >= 0
        assert hit.any() and (~hit).any() and len(np.unique(ref["index"])) >= 5, "the case shows hits on several spheres and misses"
        # ... and the same rays through the feature build of the same context
        t.render_features()
        planes = Q.planes_as_records(t.features())
        assert np.array_equal(got, Q.raw(planes)), "%s: the query records differ from the feature planes" % kernel
        # bounce-style rays from hit points of the first batch, and rays from inside spheres
        rng = SplitMix64(0x2300 + len(sph))
        pts = ref["point"][hit]
        bo = pts[(np.arange(200) * 3) % len(pts)]
        bd = rng.unit(200)
        centres = sph["center"][(np.arange(50) * 7 + 1) % len(sph)].astype(np.float32)
        io, idir = centres, rng.unit(50)
        o2, d2 = np.concatenate([bo, io]), np.concatenate([bd, idir])
        ref2 = Q.records(sph, p, o2, d2)
        got2 = query(t, o2, d2)
        assert_records_equal(got2, ref2, "%s: bounce-style and inside rays through %s" % (name, kernel))
        assert (ref2["index"][200:] >= 0).all() and (ref2["front_face"][200:][sph["radius"][ref2["index"][200:]] > 0] == 0).any()
        REACHED.setdefault(kernel, []).append("%s/%s" % (name, abi.GEOM_NAMES[path]))
    finally:
        t.close()


def test_every_query_kernel_was_reached():
    """(runs after the test above) each of the twelve kernels of csrc/pt_kernels_query.hip was launched and compared"""
    print("query kernels reached\n" + "\n".join("  %-18s %s" % (k, "; ".join(REACHED.get(k, [])) or "-") for k in KERNELS))
    assert len(KERNELS) == 12 and sorted(REACHED) == KERNELS, sorted(set(KERNELS) - set(REACHED))


# ------------------------------------------------------------------------------------------------ (b) batch edges
COUNTS = [1, 63, 64, 65, PIX - 1, PIX, PIX + 1, 2 * PIX + 5]
_EDGE = {}


def edge_rays(name):
    """2 * 777 + 5 different rays (pinhole directions in another order, longer from batch to batch) and their records, once"""
    if name not in _EDGE:
        sph, p = scene(name)
        o, d, _ = pinhole(name)
        i = np.arange(COUNTS[-1])
        pick = (i * 7) % PIX
        dd = d[pick] * (1 + i // PIX).astype(np.float32)[:, None]
        _EDGE[name] = (o[pick], dd, Q.records(sph, p, o[pick], dd))
    return _EDGE[name]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,path", [("small9", abi.PT_GEOM_SMALL), ("cover", abi.PT_GEOM_GRID)], ids=["small", "grid"])
def test_batch_edges(name, path, n):
    sph, p = scene(name)
    o, d, ref = edge_rays(name)
    t = context(sph, p, path)
    try:
        got = query(t, o[:n], d[:n])  # (query: the guard behind hits[n], segments by exactly n)
        assert_records_equal(got, ref[:n], "%s, n = %d" % (name, n))
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (c) far rays
@pytest.mark.parametrize("name", ["field1500", "field10000"])
def test_far_rays_through_the_gathering_grid_build(name):
    sph, _ = scene(name)
    c = sph["center"].astype(np.float64)
    mid, ext = c[1:].mean(axis=0), float(np.abs(c[1:] - c[1:].mean(axis=0)).max())
    # (the uniforms of test_gpu_features' far view: the grid's fit is stale, so the build that gathers its entries runs)
    p = R.look_at(W, H, 1, 8, mid + np.array([60.0, 15.0, 60.0]) * ext / 4.0, mid, 8.0, 100.0)
    rng = SplitMix64(0x23c0 + len(sph))
    out = rng.unit(200).astype(np.float64)
    out[:, 1] = np.abs(out[:, 1])  # from above the ground
    out /= np.linalg.norm(out, axis=1)[:, None]
    o = (mid + 5.0 * ext * out).astype(np.float32)
    d = ((mid + 0.5 * ext * rng.unit(200)) - o).astype(np.float32)
    ref = Q.records(sph, p, o, d)
    assert (ref["index"] >= 0).mean() > 0.5
    t = context(sph, p, abi.PT_GEOM_GRID)
    try:
        far0 = t.stats().far_rays
        got = query(t, o, d)
        st = t.stats()
        assert st.grid_fit_stale == 1 and st.far_rays - far0 > 0, (st.grid_fit_stale, st.far_rays - far0)
        assert kernel_of(t, abi.PT_GEOM_GRID) == "grid_cells_qry"
        assert_records_equal(got, ref, "%s from five radii out" % name)
        t.set_geometry_path(abi.PT_GEOM_SCALAR)
        far1 = t.stats().far_rays
        scalar = query(t, o, d)
        assert t.stats().far_rays == far1 and np.array_equal(got, scalar), "the grid's far path against the scalar walk"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (d) literal-loop rays
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
    # t is in units of the direction and ends at 1e5: a ray 3.2e-7 long reaches 0.03 units, so the short rays start 0.01 before
    # the surface their pixel shows (and where it shows none, at the camera)
    near = (pin["point"].astype(np.float64) - 0.01 * d / np.sqrt(len2)[:, None]).astype(np.float32)
    o_short = np.where((pin["index"] >= 0)[:, None], near, o)
    far_o = np.float32([[2e15, 0.5, 0.25], [0.5, 2e15, 0.25], [0.5, 0.25, -2e15]] * 4)
    far_d = np.concatenate([-far_o[:3] / np.float32(2e15), SplitMix64(0x23d0).unit(9)]).astype(np.float32)
    oo, dd = np.concatenate([o_short, o, far_o]), np.concatenate([short, long_, far_d])
    ref = Q.records(sph, p, oo, dd)
    n = len(o)
    # mostly the surfaces the pinhole rays of those pixels meet, at another t (a long ray's t may fall below 0.001)
    assert ((ref["index"][:n] == pin["index"]) & (pin["index"] >= 0)).sum() >= 20, ref["index"][:n]
    assert ((ref["index"][n:2 * n] == pin["index"]) & (pin["index"] >= 0)).sum() >= 20, ref["index"][n:2 * n]
    t = context(sph, p, path)
    try:
        got = query(t, oo, dd)
        assert_records_equal(got, ref, "irregular rays through %s" % abi.GEOM_NAMES[path])
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (e) invalid rays
@pytest.mark.parametrize("name,path", [("small9", abi.PT_GEOM_SMALL), ("cover", abi.PT_GEOM_GRID)], ids=["small", "grid"])
def test_invalid_rays_get_the_sentinel_and_their_neighbours_do_not_notice(name, path):
    sph, p = scene(name)
    o, d, ref = pinhole(name)
    bad_o, bad_d = Q.invalid_rays()
    n = 200
    places = [0, 31, 63, 64, n - 1]
    sentinel = np.zeros(16, np.uint32)
    sentinel[12:15] = 0xfffffffe
    t = context(sph, p, path)
    try:
        for call in range(4):  # 19 classes over 4 x 5 places
            oo, dd = o[:n].copy(), d[:n].copy()
            for j, at in enumerate(places):
                k = (call * len(places) + j) % len(bad_o)
                oo[at], dd[at] = bad_o[k], bad_d[k]
            assert int(Q.valid(oo, dd).sum()) == n - len(places)
            got = query(t, oo, dd)  # (segments move by the valid rays only)
            want = Q.raw(ref[:n]).copy()
            want[places] = sentinel
            assert not Q.has_nan(ref[:n]) and np.array_equal(got, want), "call %d" % call
        # a whole wave of invalid rays, and a batch of nothing else: the waves go on to the items behind them
        oo, dd = o.copy(), d.copy()
        oo[64:128], dd[64:128] = bad_o[np.arange(64) % 19], bad_d[np.arange(64) % 19]
        got = query(t, oo, dd)
        want = Q.raw(ref).copy()
        want[64:128] = sentinel
        assert np.array_equal(got, want)
        all_bad = query(t, bad_o[np.arange(PIX + 3) % 19], bad_d[np.arange(PIX + 3) % 19])
        assert (all_bad == sentinel).all()
        got = query(t, o, d)
        assert np.array_equal(got, Q.raw(ref)), "after the invalid batches"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (f) nothing else moves
def test_nothing_else_of_the_context_moves():
    """two contexts do the same things; one of them asks about rays in between.  Every read-out and every later result agree."""
    sc = scenes.default_scene(96, 54, spp=2, max_depth=8)
    p = sc.params.copy()
    p.time_step, p.first_pass = abi.PT_TIME_STEP_DECORRELATED, 3
    p.render_count, p.should_average, p.last_frame_weight = 1, 1, 1.0
    nxt = p.copy()
    nxt.camera_origin[0] += 0.05
    nxt.lower_left_corner[0] += 0.05
    o, d = Q.pinhole_rays(scenes.default_scene(37, 21, spp=1, max_depth=8).params)
    ref = Q.records(sc.spheres, p, o, d)
    out = []
    for asks in (True, False):
        t = context(sc.spheres, p, abi.PT_GEOM_SMALL)
        try:
            t.error_estimate(True)
            t.reproject_option(True)
            t.reserve_passes(2)
            t.reset()
            t.render_passes(2)
            t.render_features()
            t.keep_history()
            t.clear_textures()
            t.render_frame(1)

            def ask(n):
                held = (t.accum(), t.error_state(), t.features(), t.read_canvas(), t.read_texture(0), t.read_texture(1), t.last_trace_build())
                got = query(t, o[:n], d[:n])
                assert_records_equal(got, ref[:n], "between render calls")
                now = (t.accum(), t.error_state(), t.features(), t.read_canvas(), t.read_texture(0), t.read_texture(1), t.last_trace_build())
                assert np.array_equal(held[0].view(np.uint32), now[0].view(np.uint32)), "accumulation"
                assert np.array_equal(held[1].view(np.uint32), now[1].view(np.uint32)), "estimate state"
                assert all(np.array_equal(held[2][k].view(np.uint32), now[2][k].view(np.uint32)) for k in held[2]), "feature planes (still valid)"
                assert all(np.array_equal(held[k], now[k]) for k in (3, 4, 5)), "canvas and textures"
                assert held[6] == now[6], "pt_last_trace_build"

            if asks:
                ask(PIX)
            t.set_params(nxt)
            t.render_features()
            if asks:
                ask(5)  # (the history planes are in use here: kept, not yet reprojected)
            t.reproject()
            rs = t.reproject_stats()
            t.render_passes(2)  # (the same first_pass: had a query moved it, these passes would differ)
            if asks:
                ask(64)
            out.append((t.accum(), t.error_state(), (rs.pixels_hit, rs.pixels_kept, rs.samples_kept), t.last_trace_build(), t.stats().total_spp))
        finally:
            t.close()
    a, b = out
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "accumulation after reprojection and more passes"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "estimate state"
    assert a[2] == b[2] and a[2][1] > 0, "the history planes: reprojection's tallies"
    assert a[3:] == b[3:]


def test_the_tile_order_stays_what_it_is():
    """The order is a buffer nobody can read but a partial round of pt_render_adaptive, which reports the cost order it
    partitioned (`base`).  tests/test_gpu_adaptive.py's recipe: one uniform launch reports costs; a state loaded by hand makes
    the next two rounds partial; the first brings the order up to date, the second runs no order kernel (a partial launch
    reports no cost) and must find the first one's `base` entry for entry — with queries of one, two and many tile rows in
    between, which neither run the order kernel (it would write the identity: their launches report no cost) nor write the table
    (theirs is another)."""
    import adaptive_ref as A
    import error_ref as E

    w, h, target = 61, 37, 0.025
    sph, p = E.estimate_scene(w, h, spp=4)
    o, d = Q.pinhole_rays(p)
    ref = Q.records(sph, p, o, d)
    t = context(sph, p, features=False)
    try:
        t.reserve_passes(2)
        t.error_estimate(True)
        t.render_passes(2)
        even = np.arange(40) % 2 == 0
        state = E.empty_state(h, w)
        state[..., 0, :3] = 1.0
        state[..., 0, 3] = 2.0
        state[..., 1, 3] = 8.0
        state[A.pixel_mask(even, h, w), 1, :3] = 100.0
        t.load_error_state(state)
        st, ad = t.render_adaptive(target, 2, 2)
        assert (ad.rounds, ad.partial_rounds) == (1, 1)
        base_a, order_a, n_a = t.adaptive_tiles()
        assert sorted(base_a.tolist()) == list(range(40)) and base_a.tolist() != list(range(40)), "a cost-sorted order is in place"
        for n in (1, 100, len(o)):
            assert_records_equal(query(t, o[:n], d[:n]), ref[:n], "%d rays between two partial rounds" % n)
        assert t.adaptive_tiles()[0].tolist() == base_a.tolist() and t.adaptive_tiles()[2] == n_a  # the round's tables still answer
        flags = A.select(t.error_state(), target)
        assert flags.any() and not flags.all()
        st, ad = t.render_adaptive(target, 2, 2)
        assert (ad.rounds, ad.partial_rounds) == (1, 1)
        base_b, order_b, n_b = t.adaptive_tiles()
        assert base_b.tolist() == base_a.tolist(), "a query moved the context's tile order"
        assert order_b.tolist() == A.partition(base_a, flags).tolist() and n_b == int(flags.sum())
    finally:
        t.close()


def test_an_unsettled_auto_context_answers_and_settles_nothing():
    sph, p = scene("small9")
    o, d, ref = pinhole("small9")
    t = context(sph, p)  # PT_GEOM_AUTO, nothing rendered yet
    try:
        st0 = t.stats()
        got = query(t, o, d)
        st = t.stats()
        assert (st.geometry_tuned, st.geometry_path) == (st0.geometry_tuned, st0.geometry_path) and st0.geometry_tuned == 0
        assert_records_equal(got, ref, "unsettled PT_GEOM_AUTO")
    finally:
        t.close()


def test_the_camera_and_the_sample_counts_do_not_enter():
    sph, p = scene("cover")
    o, d, ref = pinhole("cover")
    q = R.look_at(W, H, 7, 3, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 5.0)  # another camera, 7 spp, depth 3
    q.lens_radius, q.time, q.time_step, q.first_pass = 0.3, 117.0, 0.5, 9
    t = context(sph, q, abi.PT_GEOM_GRID)
    try:
        assert_records_equal(query(t, o, d), ref, "under another camera's uniforms")
        black = q.copy()
        black.background_mode = abi.PT_BG_BLACK
        t.set_params(black)
        got = query(t, o, d).copy()
        want = Q.raw(ref).copy()
        want[ref["index"] < 0, 0:3] = 0  # a miss: the background of the context's mode
        assert np.array_equal(got, want) and (ref["index"] < 0).any()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (g) bands
def test_a_band_answers_like_the_whole_image():
    sph, p = scene("cover")
    o, d, ref = pinhole("cover")
    for rows, index, count in ((4, 1, 3), (8, 0, 2)):
        q = p.copy()
        q.band_rows, q.band_index, q.band_count = rows, index, count
        t = context(sph, q, abi.PT_GEOM_GRID)
        try:
            assert 0 < t.local_rows < H and t.query_batch() == t.local_rows * W
            assert_records_equal(query(t, o, d), ref, "band %d of %d" % (index, count))  # several batches of the band's size
        finally:
            t.close()


def test_a_band_without_rows_cannot_answer():
    sph, p = scene("cover")
    q = p.copy()
    q.band_rows, q.band_index, q.band_count = 4, 7, 8  # 21 rows are six chunks of four: ranks 6 and 7 own none
    t = context(sph, q, abi.PT_GEOM_GRID)
    try:
        assert t.local_rows == 0 and t.query_batch() == 0
        rays, hits = pack([[0, 0, 0]], [[0, 0, -1]]), np.full((1, 16), GUARD, np.uint32)
        assert t.lib.pt_query_rays(t._ctx, rays.ctypes.data_as(C.c_void_p), 1, hits.ctypes.data_as(C.c_void_p)) == abi.PT_ERR_NOT_READY
        assert b"owns no rows" in t.lib.pt_last_error(t._ctx) and (hits == GUARD).all()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (h) errors
def test_errors_of_the_entry_point():
    sph, p = scene("cover")
    t = PathTracer(W, H)
    lib = t.lib
    rays, hits = pack([[0, 0, 5]], [[0, 0, -1]]), np.full((2, 16), GUARD, np.uint32)
    rp, hp = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    try:
        assert lib.pt_query_rays(t._ctx, rp, 1, hp) == abi.PT_ERR_NOT_READY and b"PT_OPT_RAY_QUERIES" in lib.pt_last_error(t._ctx)
        assert lib.pt_set_option(t._ctx, abi.PT_OPT_RAY_QUERIES, 2) == abi.PT_ERR_INVALID
        t.ray_queries(True)
        assert lib.pt_query_rays(t._ctx, rp, 1, hp) == abi.PT_ERR_NOT_READY and b"pt_set_spheres" in lib.pt_last_error(t._ctx)
        assert t.query_batch() == 0
        t.set_spheres(sph)
        assert lib.pt_query_rays(t._ctx, rp, 1, hp) == abi.PT_ERR_NOT_READY  # no uniforms yet
        t.set_params(p)
        assert t.query_batch() == PIX
        assert lib.pt_query_rays(t._ctx, None, 1, hp) == abi.PT_ERR_INVALID and lib.pt_query_rays(t._ctx, rp, 1, None) == abi.PT_ERR_INVALID
        seg = t.stats().segments
        assert lib.pt_query_rays(t._ctx, None, 0, None) == abi.PT_OK and t.stats().segments == seg  # n == 0: nothing done
        t.set_count_work(True)
        assert lib.pt_query_rays(t._ctx, rp, 1, hp) == abi.PT_ERR_INVALID and b"COUNT_WORK" in lib.pt_last_error(t._ctx)
        t.set_count_work(False)
        assert (hits == GUARD).all()
        assert lib.pt_query_rays(t._ctx, rp, 1, hp) == abi.PT_OK and (hits[1] == GUARD).all() and hits[0, 12] != GUARD
        # the option off releases the planes; on again, after a resize, they fit the new rows
        t.ray_queries(False)
        assert lib.pt_query_rays(t._ctx, rp, 1, hp) == abi.PT_ERR_NOT_READY and t.query_batch() == 0
        t.ray_queries(True)
        assert lib.pt_resize(t._ctx, 20, 11) == abi.PT_OK
        t.width, t.height = 20, 11
        assert lib.pt_query_rays(t._ctx, rp, 1, hp) == abi.PT_ERR_NOT_READY  # uniforms of the new size must come first
        t.set_params(scenes.config2(20, 11, 1, 1, 8).params)
        assert t.query_batch() == 220
        o, d, ref = pinhole("cover")
        assert_records_equal(query(t, o, d), ref, "after a resize to 20x11: four batches")
    finally:
        t.close()


def test_a_call_inside_a_stream_capture_is_refused():
    import torch

    sph, p = scene("cover")
    o, d, ref = pinhole("cover")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = PathTracer(W, H, use_torch=True)  # binds the side stream as its launch stream
        t.set_spheres(sph)
        t.ray_queries(True)
        t.set_params(p)
        rays = torch.from_numpy(pack(o[:64], d[:64])).cuda()
        hits = torch.full((64, 16), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        seg = t.stats().segments
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = t.lib.pt_query_rays(t._ctx, C.c_void_p(rays.data_ptr()), 64, C.c_void_p(hits.data_ptr()))
            t.render_passes(1)  # (something to capture)
    torch.cuda.synchronize()
    assert rc == abi.PT_ERR_INVALID and b"capture" in t.lib.pt_last_error(t._ctx)
    assert (hits.cpu().numpy() == 0x5a5a5a5a).all() and t.stats().segments == seg, "refused before anything was launched"
    got = t.query_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    assert np.array_equal(got["uuid"].cpu().numpy(), ref["uuid"])
    t.close()


# ------------------------------------------------------------------------------------------------ (i) device arrays
def test_torch_device_tensors_in_and_out_give_the_same_bytes():
    import torch

    sph, p = scene("cover")
    o, d, ref = pinhole("cover")
    n = 2 * PIX + 5
    oo, dd = np.tile(o, (3, 1))[:n], np.tile(d, (3, 1))[:n] * np.float32(1.5)
    t = PathTracer(W, H, use_torch=True)
    try:
        t.set_spheres(sph)
        t.ray_queries(True)
        t.set_params(p)
        host = query(t, oo, dd)
        rays = torch.from_numpy(pack(oo, dd)).cuda()
        hits = torch.full((n + 3, 16), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        t._check(t.lib.pt_query_rays(t._ctx, C.c_void_p(rays.data_ptr()), n, C.c_void_p(hits.data_ptr())))
        dev = hits.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host)
        # ... mixed: device rays, host records
        mixed = np.full((n, 16), GUARD, np.uint32)
        t._check(t.lib.pt_query_rays(t._ctx, C.c_void_p(rays.data_ptr()), n, mixed.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(mixed, host)
        # ... and the other way round: host rays (three batches, the last of five rays), device records
        hits.fill_(0x5a5a5a5a)
        host_rays = pack(oo, dd)
        t._check(t.lib.pt_query_rays(t._ctx, host_rays.ctypes.data_as(C.c_void_p), n, C.c_void_p(hits.data_ptr())))
        dev = hits.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host)
        # the Python door: tensors in, tensors out; arrays in, arrays out
        got = t.query_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
        assert all(v.is_cuda for v in got.values()) and got["index"].dtype == torch.int32 and got["t"].dtype == torch.float32
        arr = t.query_rays(o, d)
        assert not Q.has_nan(ref)
        for k in ("albedo", "t", "normal", "point", "index", "uuid", "type", "front_face"):
            assert tuple(got[k].shape) == arr[k].shape == ref[k].shape, k
            assert np.array_equal(got[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)), k
            assert np.array_equal(np.ascontiguousarray(arr[k]).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)), k
        torch.cuda.synchronize()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ (j) full size
def test_config5_full_size_one_batch_equals_the_feature_planes():
    sc = scenes.config5(1920, 1080, 1, 1, 8)
    t = context(sc.spheres, sc.params)
    try:
        t.tune(1)
        st = t.stats()
        assert st.geometry_tuned == 1 and st.geometry_path == abi.PT_GEOM_GRID
        o, d = Q.pinhole_rays(sc.params)
        assert t.query_batch() == 1920 * 1080 == len(o)
        got = query(t, o, d)
        assert kernel_of(t, abi.PT_GEOM_GRID) in ("grid_cells_qry", "grid_gmem_qry")
        t.render_features()
        planes = Q.planes_as_records(t.features())
        assert not Q.has_nan(planes) and np.array_equal(got, Q.raw(planes)), "one full batch against pt_render_features"
        assert (planes["index"] >= 0).mean() > 0.5 and len(np.unique(planes["index"])) > 1000
    finally:
        t.close()
