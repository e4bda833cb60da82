"""Gather queries (pt_gather_irradiance, pt_bake_probes; include/ptrace.h has the contract) on the device.

Bit for bit: every comparison of records is equal uint32 views against tests/gather_ref.py — the defining sentence restated: the
rays in numpy float32, tests/radiance_ref.py for their records, the reduction in its stated order (pinned on the CPU by
tests/test_gather_ref.py).  Tolerance: none.  PtStats moves exactly as the one pt_query_radiance call of the defining sentence
moves it.  2 passes of 2 samples at depth 6, the time step PT_TIME_STEP_DECORRELATED.

  A   the default nine spheres at 24x10: a batch is 240 rays, no multiple of 64; D = 64 and n = 9 make 576 rays in three
      batches, and items 3 and 7 straddle the two boundaries (their lanes' sums are carried); through the small-list and the
      scalar door
  C   the same items, size and counts over the cover scene's 484 spheres, whose hierarchy and grid the forced paths walk
  B   tests/nee_scenes.py's two-light room at 32x16: a batch is 512 rays; D = 128 and n = 5 make two batches of whole items

THE CLOSED FORMS (the last section) are fp32 on the device against the float64 quadrature of the same set.  THE MARGIN: a record
is a sum of D terms, each at most T = w max |L Y| in magnitude (w = 4 pi / D or pi / D, the maximum over the record's terms).
(a) A term is made by at most 24 fp32 roundings — the direction (the division, the subtraction, the fma, the square root, the
products; sincos2pi's polynomials are good to two units), the sky (normalize, t, the mix), the mean (the pass sums, the
division), the basis (three) and the product — so it is off by at most 24 * 2^-24 T.  (b) A lane adds D / 64 terms and the tree
adds 6 levels: D / 64 + 6 roundings, each relative to a partial sum of at most D T.  Together
    margin = (D / 64 + 30) * D * 2^-24 * T,
the multiple D / 64 + 30 of D 2^-24 relative to the largest term: 31 at D = 64, 32 at D = 128."""
import ctypes as C

import numpy as np
import pytest

import gather_ref as G
import nee_scenes
import radiance_ref as RR
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer
from test_gather_ref import cosine_bound, probe_bounds
from test_gpu_ray_queries import pack
from trace_builds import build_of

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0xa5a5a5a5
PASSES, SPP, DEPTH = 2, 2, 6
KINDS = [(G.IRRADIANCE, "irradiance"), (G.PROBE, "probes")]
FLOATS = {G.IRRADIANCE: 4, G.PROBE: 28}


def settings(p, first_pass=0):
    q = p.copy()
    q.samples_per_pixel, q.max_depth, q.first_pass, q.time_step = SPP, DEPTH, first_pass, abi.PT_TIME_STEP_DECORRELATED
    return q


def context(sph, p, path=None, reserve=PASSES, use_torch=False):
    t = PathTracer(p.width, p.height, use_torch=use_torch) if use_torch else PathTracer(p.width, p.height)
    if path is not None:
        t.set_geometry_path(path)
    t.set_spheres(sph)
    t.ray_queries(True)
    t.reserve_passes(reserve)
    t.set_params(p)
    return t


def items_of(positions, normals=None):
    """(n, 8) float32 PtGatherPoint records; the pads hold NaN, which the library must not read"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    it = np.full((len(pos), 8), np.nan, F)
    it[:, 0:3] = pos
    it[:, 4:7] = 0.0 if normals is None else np.asarray(normals, F).reshape(-1, 3)
    return it


def fn_of(t, kind):
    return t.lib.pt_bake_probes if kind == G.PROBE else t.lib.pt_gather_irradiance


def stats_dict(st):
    """every number of PtStats by name, an array's elements as name[i]"""
    out = {}
    for f in st._fields_:
        v = getattr(st, f[0])
        if isinstance(v, (int, float)):
            out[f[0]] = v
        else:
            out.update({"%s[%d]" % (f[0], i): x for i, x in enumerate(v)})
    return out


def gather(t, kind, positions, normals, D, n_passes=PASSES, segments=None):
    """the raw records, (n, 4 or 28) uint32, through the C entry point with host arrays; two records of guard words behind
    out[n] stay as they are; PtStats.segments moves by `segments` and samples, total_spp and render_launches do not move"""
    it = items_of(positions, normals)
    n = len(it)
    out = np.full((n + 2, FLOATS[kind]), GUARD, np.uint32)
    before = t.stats()
    t._check(fn_of(t, kind)(t._ctx, it.ctypes.data_as(C.c_void_p), n, D, n_passes, out.ctypes.data_as(C.c_void_p)))
    after = t.stats()
    assert (out[n:] == GUARD).all(), "records written behind out[n]"
    if segments is not None:
        assert after.segments - before.segments == segments, (after.segments - before.segments, segments)
    assert (after.samples, after.total_spp, after.render_launches) == (before.samples, before.total_spp, before.render_launches)
    return out[:n]


def assert_equal(got, ref, what):
    assert not np.isnan(ref).any(), what + ": the restatement holds a NaN"
    want = G.raw(ref)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=1))[:, 0]
        k = int(bad[0])
        raise AssertionError("%s: %d of %d records differ, first item %d:\n got  %r\n want %r" % (
            what, len(bad), len(got), k, got[k].view(F), want[k].view(F)))


# ---- the two cases, their items and their references: made once -------------------------------------------------------------
def case_a():
    sc = scenes.default_scene(24, 10, spp=SPP, max_depth=DEPTH)
    return sc.spheres, settings(sc.params)


def case_b():
    sc = nee_scenes.two_light_room(32, 16, SPP, PASSES, DEPTH)
    return sc.spheres, settings(sc.params)


def items_a():
    """nine items about the default scene: on the ground, on and above the spheres, normals of any length, the frame's pole"""
    pos = [(0.0, -0.49, -1.0), (0.6, -0.2, -1.2), (-1.0, 0.0, -1.0), (0.0, 0.55, -1.0), (1.0, 0.1, -0.6), (-0.4, -0.3, -0.5), (0.0, 0.0, 0.2),
           (2.0, 1.0, -3.0), (-0.2, -0.45, -1.6)]
    nrm = [(0.0, 1.0, 0.0), (0.3, 2.0, 0.1), (-1.0, 0.0, 0.0), (0.0, 1e-20, 0.0), (0.5, 0.5, 0.7), (0.0, 0.0, -1.0), (0.0, 0.0, 3.0),
           (-0.2, -0.9, 0.4), (0.0, 1.0, -1e-3)]
    return np.asarray(pos, F), np.asarray(nrm, F)


def items_b():
    pos = [(0.0, -0.95, 0.0), (0.9, 0.0, 0.2), (0.0, 0.0, 1.5), (-0.9, -0.5, -0.5), (0.25, 0.2, -0.2)]
    nrm = [(0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (1.0, 0.2, 0.1), (0.0, 1.0, 0.0)]
    return np.asarray(pos, F), np.asarray(nrm, F)


def case_c():
    sc = scenes.config2(24, 10, SPP, PASSES, DEPTH)
    return sc.spheres, settings(sc.params)


def items_c():
    """nine items over the cover scene's ground and among its spheres, the normals of case A"""
    pos = [(0.0, 0.01, 0.0), (4.0, 1.0, 0.0), (-4.0, 1.0, 2.5), (0.0, 2.1, 0.0), (3.0, 0.3, 3.0), (-6.0, 0.25, -5.0), (8.0, 3.0, 2.0), (1.5, 0.21, -2.5),
           (-2.0, 0.5, 6.0)]
    return np.asarray(pos, F), items_a()[1]


CASES = {"A": (case_a, items_a, 64), "B": (case_b, items_b, 128), "C": (case_c, items_c, 64)}
_REF = {}


def reference(case, kind, first_pass=0, band=None):
    """(spheres, params, positions, normals, D, records, segments) of a case: the restatement, made once and left unchanged"""
    key = (case, kind, first_pass, band)
    if key not in _REF:
        make, items, D = CASES[case]
        sph, p = make()
        p.first_pass = first_pass
        if band is not None:
            p.band_rows, p.band_index, p.band_count = band
        pos, nrm = items()
        rec, seg, rays = G.gather(sph, p, kind, pos, nrm if kind == G.IRRADIANCE else None, D, PASSES)
        assert not np.isnan(rec).any() and seg > 2 * PASSES * SPP * len(pos) * D / 2, "paths of more than one segment"
        assert (rec[:, -1] == D * PASSES * SPP).all()
        rec.setflags(write=False)
        _REF[key] = (sph, p, pos, nrm, D, rec, seg)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ bit equality
DOORS = [("A", abi.PT_GEOM_SMALL), ("A", abi.PT_GEOM_SCALAR), ("C", abi.PT_GEOM_BVH), ("C", abi.PT_GEOM_GRID)]


@pytest.mark.parametrize("kind,kind_name", KINDS, ids=[k[1] for k in KINDS])
@pytest.mark.parametrize("case,path", DOORS, ids=[abi.GEOM_NAMES[d[1]] for d in DOORS])
def test_straddling_items_through_each_door_path(case, path, kind, kind_name):
    sph, p, pos, nrm, D, rec, seg = reference(case, kind)
    assert RR.batch(p) == 240 and D == 64 and len(pos) * D == 576, "three batches, items 3 and 7 straddle the boundaries"
    t = context(sph, p, path)
    try:
        build0, st0 = t.last_trace_build(), t.stats()
        got = gather(t, kind, pos, nrm, D, PASSES, seg)
        assert_equal(got, rec, "case %s, %s through %s" % (case, kind_name, abi.GEOM_NAMES[path]))
        st = t.stats()
        assert t.last_trace_build() == build0 and (st.geometry_path, st.geometry_tuned) == (st0.geometry_path, st0.geometry_tuned)
        # the radiance build the forced path launches (the table's radiance column, pinned on the CPU by test_trace_builds.py)
        kernel = build_of(st, "_rad", path=abi.PT_GEOM_SCALAR if path == abi.PT_GEOM_LDS else path)
        assert kernel.startswith({abi.PT_GEOM_SMALL: "small_t", abi.PT_GEOM_SCALAR: "scalar", abi.PT_GEOM_BVH: "bvh", abi.PT_GEOM_GRID: "grid"}[path]), kernel
    finally:
        t.close()


@pytest.mark.parametrize("kind,kind_name", KINDS, ids=[k[1] for k in KINDS])
@pytest.mark.parametrize("path", [None, abi.PT_GEOM_GRID], ids=["auto", "grid"])
def test_case_b_whole_items_per_batch(path, kind, kind_name):
    sph, p, pos, nrm, D, rec, seg = reference("B", kind)
    assert RR.batch(p) == 512 and 512 % D == 0 and len(pos) * D == 640
    t = context(sph, p, path)
    try:
        got = gather(t, kind, pos, nrm, D, PASSES, seg)
        assert_equal(got, rec, "case B, %s" % kind_name)
        assert (rec[:, :-1] != 0).any(axis=1).all(), "the lights are seen"
    finally:
        t.close()


@pytest.mark.parametrize("kind,kind_name", KINDS, ids=[k[1] for k in KINDS])
def test_device_arrays_and_the_python_doors(kind, kind_name):
    import torch

    sph, p, pos, nrm, D, rec, seg = reference("A", kind)
    n, floats = len(pos), FLOATS[kind]
    t = context(sph, p, abi.PT_GEOM_SMALL, use_torch=True)
    try:
        host = gather(t, kind, pos, nrm, D, PASSES, seg)
        assert_equal(host, rec, "host arrays")
        it = torch.from_numpy(items_of(pos, nrm)).cuda()
        out = torch.full((n + 2, floats), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        t._check(fn_of(t, kind)(t._ctx, C.c_void_p(it.data_ptr()), n, D, PASSES, C.c_void_p(out.data_ptr())))
        dev = out.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host), "device items, device records"
        mixed = np.full((n, floats), GUARD, np.uint32)
        t._check(fn_of(t, kind)(t._ctx, C.c_void_p(it.data_ptr()), n, D, PASSES, mixed.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(mixed, host), "device items, host records"
        out.fill_(0x5a5a5a5a)
        t._check(fn_of(t, kind)(t._ctx, items_of(pos, nrm).ctypes.data_as(C.c_void_p), n, D, PASSES, C.c_void_p(out.data_ptr())))
        dev = out.cpu().numpy().view(np.uint32)
        assert (dev[n:] == 0x5a5a5a5a).all() and np.array_equal(dev[:n], host), "host items, device records"
        # the Python doors: arrays in, arrays out; tensors in, tensors out
        if kind == G.PROBE:
            a, b = t.bake_probes(pos, directions=D, passes=PASSES), t.bake_probes(torch.from_numpy(pos).cuda(), directions=D, passes=PASSES)
            names = (("sh", (n, 9, 3)), ("samples", (n,)))
        else:
            a = t.gather_irradiance(pos, nrm, directions=D, passes=PASSES)
            b = t.gather_irradiance(torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda(), directions=D, passes=PASSES)
            names = (("e", (n, 3)), ("samples", (n,)))
        assert all(isinstance(v, np.ndarray) for v in a.values()) and all(v.is_cuda and v.dtype == torch.float32 for v in b.values())
        for res in (a, {k: v.cpu().numpy() for k, v in b.items()}):
            flat = np.concatenate([np.ascontiguousarray(res[k]).reshape(n, -1) for k, _ in names], axis=1)
            assert all(res[k].shape == shape for k, shape in names) and np.array_equal(G.raw(flat), host)
        torch.cuda.synchronize()
    finally:
        t.close()


@pytest.mark.parametrize("kind,kind_name", KINDS, ids=[k[1] for k in KINDS])
def test_a_band_of_a_two_band_context(kind, kind_name):
    band = (2, 1, 2)  # rows in chunks of two, the second of two ranks
    sph, p, pos, nrm, D, rec, seg = reference("A", kind, band=band)
    whole = reference("A", kind)[5]
    t = context(sph, p, abi.PT_GEOM_SMALL)
    try:
        assert 0 < t.local_rows < 10 and t.query_batch() == t.local_rows * 24 == RR.batch(p)
        got = gather(t, kind, pos, nrm, D, PASSES, seg)
        assert_equal(got, rec, "a band")
        assert not np.array_equal(G.raw(rec), G.raw(whole)), "a band's places have other pixel centres and batches"
    finally:
        t.close()


def test_the_same_call_twice_and_another_first_pass():
    kind = G.IRRADIANCE
    sph, p, pos, nrm, D, rec, seg = reference("A", kind)
    _, p7, _, _, _, rec7, seg7 = reference("A", kind, first_pass=7)
    t = context(sph, p, abi.PT_GEOM_SMALL)
    try:
        first = gather(t, kind, pos, nrm, D, PASSES, seg)
        again = gather(t, kind, pos, nrm, D, PASSES, seg)
        assert np.array_equal(first, again), "first_pass is not advanced"
        assert_equal(first, rec, "first_pass 0")
        t.set_params(p7)
        other = gather(t, kind, pos, nrm, D, PASSES, seg7)
        assert_equal(other, rec7, "first_pass 7")
        assert not np.array_equal(other[:, :3], first[:, :3]), "other passes, other samples"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ edge items
@pytest.mark.parametrize("kind,kind_name", KINDS, ids=[k[1] for k in KINDS])
def test_an_invalid_item_between_valid_ones(kind, kind_name):
    sph, p, pos, nrm, D, rec, seg = reference("A", kind)
    bad_pos, bad_nrm = pos.copy(), nrm.copy()
    bad_pos[3, 1] = np.inf  # item 3 straddles the first batch boundary: its lanes' sums would be carried
    want, seg_bad, rays = G.gather(sph, p, kind, bad_pos, bad_nrm if kind == G.IRRADIANCE else None, D, PASSES)
    assert not want[3].view(np.uint32).any() and not rays[3 * D:4 * D].view(np.uint32).any() and 0 < seg_bad < seg
    keep = np.arange(len(pos)) != 3
    assert np.array_equal(G.raw(want[keep]), G.raw(rec[keep])), "the neighbours' records depend on their indices only"
    t = context(sph, p, abi.PT_GEOM_SMALL)
    try:
        got = gather(t, kind, bad_pos, bad_nrm, D, PASSES, seg_bad)  # (segments: the valid items' only)
        assert_equal(got, want, "an invalid item")
        assert not got[3].any(), "all +0; samples == 0 is the mark"
        if kind == G.IRRADIANCE:  # a normal of three zeros, and a NaN in the normal: invalid here, and only here
            for nb in ((0.0, -0.0, 0.0), (0.0, np.nan, 1.0)):
                nn = nrm.copy()
                nn[3] = nb
                got = gather(t, kind, pos, nn, D, PASSES, seg_bad)
                assert_equal(got, want, "a normal %r" % (nb,))
        every = gather(t, kind, np.full((4, 3), np.nan, F), np.ones((4, 3), F), D, PASSES, 0)
        assert not every.any(), "a call of invalid items only traces nothing"
    finally:
        t.close()


def test_no_items_and_one_item_of_4096_directions():
    sph, p = case_a()
    pos, nrm = np.asarray([(0.2, -0.3, -0.4)], F), np.asarray([(0.1, 1.0, -0.2)], F)
    t = context(sph, p, abi.PT_GEOM_SMALL)
    try:
        st = stats_dict(t.stats())
        out = np.full((1, 28), GUARD, np.uint32)
        for kind, _ in KINDS:
            assert fn_of(t, kind)(t._ctx, None, 0, 64, PASSES, None) == abi.PT_OK
            assert fn_of(t, kind)(t._ctx, items_of(pos, nrm).ctypes.data_as(C.c_void_p), 0, 0, 0, out.ctypes.data_as(C.c_void_p)) == abi.PT_OK
        assert (out == GUARD).all() and stats_dict(t.stats()) == st, "n == 0: nothing done"
        # 4096 rays in eighteen batches of 240: one item carried over seventeen boundaries
        for kind, name in KINDS:
            want, seg, _ = G.gather(sph, p, kind, pos, nrm if kind == G.IRRADIANCE else None, 4096, PASSES)
            got = gather(t, kind, pos, nrm, 4096, PASSES, seg)
            assert_equal(got, want, "D = 4096, %s" % name)
            assert got[0, -1].view(F) == 4096 * PASSES * SPP
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ leaves alone
def test_nothing_else_moves_and_the_stats_move_as_the_one_radiance_call():
    sc = scenes.default_scene(24, 10, spp=SPP, max_depth=DEPTH)
    p = settings(sc.params, first_pass=3)
    p.render_count, p.should_average, p.last_frame_weight = 1, 1, 1.0
    pos, nrm = items_a()
    D = 64
    t = context(sc.spheres, p, abi.PT_GEOM_SMALL)
    try:
        t.feature_planes(True)
        t.error_estimate(True)
        t.reset()
        t.render_passes(2)
        t.render_features()
        t.clear_textures()
        t.render_frame(1)

        def held():
            return (t.accum(), t.error_state(), t.features(), t.read_canvas(), t.read_texture(0), t.read_texture(1), t.last_trace_build(),
                    t.stats().geometry_path, t.stats().geometry_tuned)

        for kind, name in KINDS:
            normals = nrm if kind == G.IRRADIANCE else None
            o, d = G.rays(kind, pos, normals, D)
            rays, rec = pack(o, d), np.zeros((len(o), 4), F)
            s0 = stats_dict(t.stats())
            t._check(t.lib.pt_query_radiance(t._ctx, rays.ctypes.data_as(C.c_void_p), len(rays), PASSES, rec.ctypes.data_as(C.c_void_p)))
            s1 = stats_dict(t.stats())
            before = held()
            got = gather(t, kind, pos, nrm, D)
            s2 = stats_dict(t.stats())
            after = held()
            assert {k: s2[k] - s1[k] for k in s0} == {k: s1[k] - s0[k] for k in s0}, "%s: PtStats moves as the one pt_query_radiance call" % name
            assert s1["segments"] > s0["segments"]
            # ... and the records are that call's, reduced
            want = np.stack([G.reduce_item(kind, rec[i * D:(i + 1) * D], D) for i in range(len(pos))])
            assert_equal(got, want, "%s from the radiance call's own records" % name)
            assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)), "accumulation"
            assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32)), "estimate state"
            assert all(np.array_equal(before[2][k].view(np.uint32), after[2][k].view(np.uint32)) for k in before[2]), "feature planes"
            assert all(np.array_equal(before[k], after[k]) for k in (3, 4, 5)), "canvas and textures"
            assert before[6:] == after[6:], "pt_last_trace_build and the geometry path"
        # first_pass did not move: two more passes are the passes of an undisturbed context
        t.render_passes(2)
        u = context(sc.spheres, p, abi.PT_GEOM_SMALL)
        try:
            u.reset()
            u.render_passes(2)
            u.render_passes(2)
            assert np.array_equal(t.accum().view(np.uint32), u.accum().view(np.uint32)), "k passes, the gathers, k passes against 2 k passes"
        finally:
            u.close()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ error codes
def test_errors_of_the_entry_points():
    sph, p = case_a()
    pos, nrm = items_a()
    it = items_of(pos[:2], nrm[:2])
    for kind, _ in KINDS:
        t = PathTracer(24, 10)
        fn, lib = fn_of(t, kind), t.lib
        out = np.full((3, FLOATS[kind]), GUARD, np.uint32)
        ip, op = it.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        try:
            assert fn(t._ctx, ip, 2, 64, 1, op) == abi.PT_ERR_NOT_READY and b"PT_OPT_RAY_QUERIES" in lib.pt_last_error(t._ctx)
            t.ray_queries(True)
            assert fn(t._ctx, ip, 2, 64, 1, op) == abi.PT_ERR_NOT_READY and b"pt_set_spheres" in lib.pt_last_error(t._ctx)
            t.set_spheres(sph)
            assert fn(t._ctx, ip, 2, 64, 1, op) == abi.PT_ERR_NOT_READY  # no uniforms yet
            t.set_params(p)
            seg = t.stats().segments
            assert fn(t._ctx, None, 2, 64, 1, op) == abi.PT_ERR_INVALID and fn(t._ctx, ip, 2, 64, 1, None) == abi.PT_ERR_INVALID
            assert b"NULL" in lib.pt_last_error(t._ctx)
            assert fn(t._ctx, ip, 2, 64, 0, op) == abi.PT_ERR_INVALID and b"n_passes == 0" in lib.pt_last_error(t._ctx)
            assert fn(t._ctx, ip, 2, 64, 2, op) == abi.PT_ERR_CAPACITY and b"reserved" in lib.pt_last_error(t._ctx)  # one pass is reserved
            for bad in (0, 63, 4160, 96, 8192):
                assert fn(t._ctx, ip, 2, bad, 1, op) == abi.PT_ERR_INVALID and b"directions" in lib.pt_last_error(t._ctx), bad
            # n_passes is asked before directions, and n * D beyond 2^32 - 1 after them
            assert fn(t._ctx, ip, 2, 63, 0, op) == abi.PT_ERR_INVALID and b"n_passes == 0" in lib.pt_last_error(t._ctx)
            assert fn(t._ctx, ip, 2, 63, 9, op) == abi.PT_ERR_CAPACITY
            assert fn(t._ctx, ip, 1 << 26, 64, 1, op) == abi.PT_ERR_INVALID and b"2^32 - 1" in lib.pt_last_error(t._ctx)
            assert (out == GUARD).all() and t.stats().segments == seg, "refused before anything was launched"
            assert lib.pt_set_option(t._ctx, 14, 1) == abi.PT_ERR_INVALID and b"unknown key" in lib.pt_last_error(t._ctx)
            # ... and the context is still usable
            assert fn(t._ctx, ip, 2, 64, 1, op) == abi.PT_OK and (out[2] == GUARD).all() and out[0, -1].view(F) == 64 * SPP
            t.ray_queries(False)
            assert fn(t._ctx, ip, 2, 64, 1, op) == abi.PT_ERR_NOT_READY
            t.ray_queries(True)
            assert fn(t._ctx, ip, 2, 64, 1, op) == abi.PT_OK, "the workspace comes back with the option"
        finally:
            t.close()


def test_a_call_inside_a_stream_capture_is_refused():
    import torch

    sph, p = case_a()
    pos, nrm = items_a()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = context(sph, p, use_torch=True)  # binds the side stream as its launch stream
        it = torch.from_numpy(items_of(pos, nrm)).cuda()
        out = torch.full((len(pos), 28), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        torch.cuda.current_stream().synchronize()
        seg = t.stats().segments
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rcs = [fn_of(t, kind)(t._ctx, C.c_void_p(it.data_ptr()), len(pos), 64, 1, C.c_void_p(out.data_ptr())) for kind, _ in KINDS]
            err = t.lib.pt_last_error(t._ctx)
            t.render_passes(1)  # (something to capture)
    torch.cuda.synchronize()
    assert rcs == [abi.PT_ERR_INVALID] * 2 and b"capture" in err
    assert (out.cpu().numpy() == 0x5a5a5a5a).all() and t.stats().segments == seg, "refused before anything was launched"
    got = gather(t, G.PROBE, pos, None, 64, 1)  # ... and the context is still usable
    assert (got[:, -1].view(F) == 64 * SPP).all()
    t.close()


# ------------------------------------------------------------------------------------------------ closed forms
def margin(D, T):
    """module docstring: (D / 64 + 30) * D * 2^-24 * T"""
    return (D / 64 + 30) * D * 2.0 ** -24 * T


def one_far_sphere():
    """one small sphere behind t_max = 1e5: the scene is not empty and no ray of any probe can reach it"""
    s = np.zeros(1, abi.SPHERE_DTYPE)
    s["center"], s["radius"], s["type"], s["albedo"], s["uuid"] = (0.0, 0.0, 3e5), 1.0, abi.PT_DIFFUSE, (0.5, 0.5, 0.5), 0
    return s


@pytest.mark.parametrize("D", [64, 128])
def test_the_sky_in_closed_form(D):
    p = settings(scenes.default_scene(24, 10, spp=SPP, max_depth=DEPTH).params)
    assert p.background_mode == abi.PT_BG_SKY
    pos = np.asarray([(0.0, 0.0, 0.0), (3.0, -2.0, 1.0)], F)
    normals = np.asarray([(0.0, 1.0, 0.0), (0.6, 0.48, -0.64)], F)
    t = context(one_far_sphere(), p)
    try:
        sh = gather(t, G.PROBE, pos, None, D, PASSES, 2 * D * PASSES * SPP).view(F)   # every ray is one segment: a miss
        want = G.probe64(G.sky, D)
        T = 4.0 * np.pi / D * np.abs(G.basis64(G.sphere64(D))[:, :, None] * G.sky(G.sphere64(D))[:, None, :]).max()
        for i in range(2):
            err = np.abs(sh[i, :27].reshape(9, 3) - want)
            print("D = %d, probe %d: largest error %.3g, margin %.3g" % (D, i, err.max(), margin(D, T)))
            assert (err <= margin(D, T)).all(), (err.max(), margin(D, T))
            assert sh[i, 27] == D * PASSES * SPP
        # ... and so the closed forms, up to the quadrature (tests/test_gather_ref.py derives the bounds)
        closed = np.zeros((9, 3))
        closed[0] = 4.0 * np.pi * 0.282095 * np.array([0.75, 0.85, 1.0])
        closed[1] = 4.0 * np.pi / 3.0 * 0.488603 * 0.5 * np.array([-0.5, -0.3, 0.0])
        assert (np.abs(sh[0, :27].reshape(9, 3) - closed) <= probe_bounds(D) + margin(D, T)).all()
        e = gather(t, G.IRRADIANCE, pos, normals, D, PASSES, 2 * D * PASSES * SPP).view(F)
        for i in range(2):
            want_e = G.irradiance64(G.sky, normals[i].astype(np.float64), D)
            Te = np.pi / D * np.abs(G.sky(G.hemisphere64(normals[i].astype(np.float64), D))).max()
            err = np.abs(e[i, :3] - want_e)
            print("D = %d, point %d: largest error %.3g, margin %.3g" % (D, i, err.max(), margin(D, Te)))
            assert (err <= margin(D, Te)).all(), (err, margin(D, Te))
        assert (np.abs(e[0, :3] - np.pi * (1.0 / 6.0 + 5.0 / 6.0 * np.array([0.5, 0.7, 1.0]))) <= cosine_bound((0, 1, 0), D) + margin(D, np.pi / D)).all()
    finally:
        t.close()


@pytest.mark.parametrize("D", [64, 128])
def test_the_furnace_in_closed_form(D):
    """A probe inside one PT_EMISSIVE sphere of albedo e: every ray returns e after one segment."""
    e = np.array([1.5, 0.75, 2.0])
    s = np.zeros(1, abi.SPHERE_DTYPE)
    s["center"], s["radius"], s["type"], s["albedo"], s["uuid"] = (0.0, 0.0, 0.0), 2.0, abi.PT_EMISSIVE, e, 0
    p = settings(scenes.default_scene(24, 10, spp=SPP, max_depth=DEPTH).params)
    pos = np.asarray([(0.3, -0.2, 0.1)], F)
    nrm = np.asarray([(0.2, -0.5, 0.8)], F)
    t = context(s, p)
    try:
        sh = gather(t, G.PROBE, pos, None, D, PASSES, D * PASSES * SPP).view(F)[0]
        const = lambda w: np.ones((len(w), 1)) * e
        want = G.probe64(const, D)
        T = 4.0 * np.pi / D * 1.1 * e.max()  # (|Y_k| <= 1.1)
        got = sh[:27].reshape(9, 3).astype(np.float64)
        assert (np.abs(got - want) <= margin(D, T)).all(), (np.abs(got - want).max(), margin(D, T))
        closed = np.zeros((9, 3))
        closed[0] = 4.0 * np.pi * 0.282095 * e   # 2 sqrt(pi) e with the header's six-decimal constant
        bound = probe_bounds(D, A=e, B=np.zeros(3)) + margin(D, T)
        assert (np.abs(got - closed) <= bound).all(), "sh[0] = 2 sqrt(pi) e, the rest is 0 up to the quadrature"
        assert np.allclose(closed[0], 2.0 * np.sqrt(np.pi) * e, rtol=1.8e-6)
        irr = gather(t, G.IRRADIANCE, pos, nrm, D, PASSES, D * PASSES * SPP).view(F)[0]
        assert (np.abs(irr[:3] - np.pi * e) <= margin(D, np.pi / D * e.max())).all(), "pi e: the cosine set's weights add up to pi exactly"
        n = nrm[0].astype(np.float64) / np.linalg.norm(nrm[0].astype(np.float64))
        band = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
        through_sh = abi.sh_irradiance(got, n)
        slack = (band[:, None] * np.abs(G.basis64(n))[:, None] * bound).sum(axis=0) + 3.6e-6 * np.pi * e.max()  # (the constants, twice)
        assert (np.abs(through_sh - np.pi * e) <= slack).all() and (np.abs(through_sh - irr[:3]) <= slack + margin(D, np.pi / D * e.max())).all()
    finally:
        t.close()
