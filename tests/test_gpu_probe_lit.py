"""Probe lattices (pt_bake_lattice, pt_shade_probes; include/ptrace.h has the contract) on the device.

Bit for bit wherever two things are said to be equal: records against pt_bake_probes / pt_bake_probes_nee on host-made points
(the defining sentence), texels against tests/probe_ref.py (the header's statement list in numpy float32, pinned to
csrc/pt_probe.hpp on the CPU by tests/test_probe_ref.py).  Frames of 40 x 24 and 67 x 19 — the odd size leaves partial 8 x 8
blocks at the right and top edges — lattices of 2 x 2 x 2 and 3 x 2 x 5, D = 64, one pass of 2 samples at depth 6.

  1  the bake equals the explicit call, whole and as two slices; PT_LATTICE_SKIP_BURIED
  2  the shading equals the restatement: baked and synthetic records, the half-space test, the bias, both clamps, g == 0 and the
     last node on a hit point, host and device pointers, a row band
  3  partition of unity: identical records, records linear in the node position
  4  a closed form, end to end: a small sphere under the sky
  5  nothing else moves
  6  errors, with the context usable afterwards
  7  the pipeline: the frame goes into pt_meter and pt_resolve_toned as a device source

TOLERANCES.  (3a) eight identical records: the texel is albedo * max(E, 0) / pi with E the single record's value; the blend is
S / W with S = sum w_k E (fmas) and W = sum w_k in fp32, a weighted MEAN of equal values.  The tolerance is the feature's stated
one, 4 ulp of the texel: the partial sums S_k and E W_k take their roundings at the same steps, so S / W stays within a few
roundings of E, and the two multiplications behind it (v * 0.318309886f, albedo * that) are the same statements on both sides and
carry the quotient's error through.  The worst distance met is printed.
(3b) records linear in the node position, no corner dropped: trilinear weights reproduce a linear function exactly in real
arithmetic; in fp32 the weights (three subtractions, two products: 5 roundings), the eight fmas and adds, the nine-term E_k and
the division leave a few 2^-24 of the largest corner value, and the values are all positive and within a factor of three of
each other: the feature's 1e-5 is asked relative to the linear function's own value at q.
(4) see the test's docstring."""
import ctypes as C

import numpy as np
import pytest

import gather_ref as G
import probe_ref as P
from ray_tracer_webgl_amd import abi, scenes
from ray_tracer_webgl_amd.tracer import PathTracer, PtError
from test_gather_ref import probe_bounds
from test_gpu_gather import stats_dict

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0xa5a5a5a5
SPP, DEPTH, D = 2, 6, 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def settings(p):
    q = p.copy()
    q.samples_per_pixel, q.max_depth, q.first_pass, q.time_step = SPP, DEPTH, 0, abi.PT_TIME_STEP_DECORRELATED
    return q


def random_scene(w, h):
    """twelve spheres of every type — an unknown one among them — over a ground sphere, under the sky"""
    rng = np.random.default_rng(0x5EED33)
    items = [scenes._sphere((0.0, -100.5, -1.0), 100.0, abi.PT_DIFFUSE, (0.6, 0.6, 0.5))]
    types = [abi.PT_DIFFUSE, abi.PT_METAL, abi.PT_GLASS, abi.PT_EMISSIVE, 7, abi.PT_DIFFUSE]
    for k in range(12):
        c = (rng.uniform(-1.6, 1.6), rng.uniform(-0.35, 0.5), rng.uniform(-2.2, -0.4))
        items.append(scenes._sphere(c, rng.uniform(0.12, 0.3), types[k % 6], tuple(rng.uniform(0.2, 0.95, 3)), fuzz=0.2, ri=1.5))
    p = scenes._base_params(SPP, DEPTH)
    scenes._state_camera(scenes._lib(), p, w, h)
    return scenes.Scene("random", scenes._pack(items), p, 1)


def scene_of(name, w, h):
    if name == "default":
        sc = scenes.default_scene(w, h, spp=SPP, max_depth=DEPTH)
    elif name == "room":
        sc = scenes.config4(w, h, SPP, 1, DEPTH)
    else:
        sc = random_scene(w, h)
    return sc.spheres, settings(sc.params)


# the scenes at their sizes, and where their lattices stand: {name: (w, h, origin, extent)}
CASES = {"default": (40, 24, (-1.4, -0.45, -1.9), (2.8, 1.2, 2.4)), "room": (67, 19, (-0.9, -0.9, -0.9), (1.8, 1.8, 1.8)),
         "random": (40, 24, (-1.5, -0.4, -2.3), (3.0, 1.1, 2.2))}
LATTICES = {"2x2x2": (2, 2, 2), "3x2x5": (3, 2, 5)}


def lattice_of(name, dims, flags=0):
    _, _, origin, extent = CASES[name]
    n = LATTICES[dims]
    return abi.PtProbeLattice(origin=origin, step=tuple(F(extent[c]) / F(n[c] - 1) for c in range(3)), n=n, flags=flags)


def context(name, nee=False, use_torch=False, band=None):
    w, h = CASES[name][:2]
    sph, p = scene_of(name, w, h)
    if band is not None:
        p.band_rows, p.band_index, p.band_count = band
    t = PathTracer(w, h, use_torch=True) if use_torch else PathTracer(w, h)
    t.set_spheres(sph)
    t.ray_queries(True)
    t.feature_planes(True)
    if nee:
        t.next_event(True)
    t.reserve_passes(1)
    t.set_params(p)
    return t, sph, p


def bake_lattice(t, lat, first, count, estimator=0, directions=D):
    """the raw records of pt_bake_lattice into a host array with two records of guard words behind it, and PtStats' segments"""
    out = np.full((count + 2, 28), GUARD, np.uint32)
    before = t.stats().segments
    t._check(t.lib.pt_bake_lattice(t._ctx, C.byref(lat), first, count, directions, 1, estimator, out.ctypes.data_as(C.c_void_p)))
    assert (out[count:] == GUARD).all(), "records written behind out[count]"
    return out[:count], t.stats().segments - before


def bake_points(t, points, estimator=0, directions=D):
    it = np.full((len(points), 8), np.nan, F)  # (the pads hold NaN, which the library must not read)
    it[:, 0:3], it[:, 4:7] = points, 0.0
    out = np.full((len(points), 28), GUARD, np.uint32)
    fn = t.lib.pt_bake_probes_nee if estimator else t.lib.pt_bake_probes
    before = t.stats().segments
    t._check(fn(t._ctx, it.ctypes.data_as(C.c_void_p), len(points), directions, 1, out.ctypes.data_as(C.c_void_p)))
    return out, t.stats().segments - before


def shade(t, lat, probes, options=None):
    """pt_shade_probes through the C entry point with host arrays; two texels of guard words behind the frame stay"""
    n = t.local_rows * t.width
    out = np.full((n + 2, 4), GUARD, np.uint32)
    rec = np.ascontiguousarray(probes, dtype=F)
    assert rec.shape == (lat.nodes, 28)
    t._check(t.lib.pt_shade_probes(t._ctx, C.byref(lat), rec.ctypes.data_as(C.c_void_p), C.byref(options) if options is not None else None,
                                   out.ctypes.data_as(C.c_void_p)))
    assert (out[n:] == GUARD).all(), "texels written behind the frame"
    return out[:n].view(F).reshape(t.local_rows, t.width, 4)


def restated(t, feats, lat, probes, options=None, stats=None):
    flags = abi.PT_PROBE_HALFSPACE if options is None else options.flags
    bias = 0.0 if options is None else options.normal_bias
    return P.shade(feats["albedo"], feats["normal"], feats["point"], feats["ids"], lat, probes, flags, bias, tuple(t.params.camera_origin), stats)


def assert_texels(got, want, what):
    assert not np.isnan(want).any(), what + ": the restatement holds a NaN"
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere((bits(got) != bits(want)).any(axis=2))
        y, x = bad[0]
        raise AssertionError("%s: %d of %d texels differ, first (%d, %d):\n got  %r\n want %r" % (what, len(bad), got.shape[0] * got.shape[1], x, y, got[y, x], want[y, x]))


def synthetic(nodes, seed=7, empty_every=5):
    """records with coefficients of both signs, band 0 mostly positive; samples == 0 at every fifth node"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(-0.6, 0.9, (nodes, 28)).astype(F)
    r[:, 0:3] += F(1.5)
    r[:, 27] = 128.0
    if empty_every:
        r[::empty_every, 27] = 0.0
    return r


# ------------------------------------------------------------------------------------------- 1. the bake
@pytest.mark.parametrize("dims", sorted(LATTICES))
@pytest.mark.parametrize("name,estimator", [("default", 0), ("random", 0), ("room", 0), ("room", 1)])
def test_the_bake_equals_the_explicit_call(name, estimator, dims):
    t, sph, p = context(name, nee=bool(estimator))
    try:
        lat = lattice_of(name, dims)
        pts = P.lattice_points(lat, sph)
        assert np.array_equal(bits(pts), bits(abi.probe_lattice_positions(lat)))
        n = lat.nodes
        whole, seg = bake_lattice(t, lat, 0, n, estimator)
        want, seg_want = bake_points(t, pts, estimator)
        assert np.array_equal(whole, want) and seg == seg_want and seg > 0
        assert (whole.view(F)[:, 27] == D * SPP).all()
        cut = n // 2 + 1
        for first, count in ((0, cut), (cut, n - cut)):
            part, seg = bake_lattice(t, lat, first, count, estimator)
            want_part, seg_want = bake_points(t, pts[first:first + count], estimator)
            assert np.array_equal(part, want_part) and seg == seg_want, (first, count)
            if first:
                assert not np.array_equal(part, whole[first:]), "an item's seeds follow its index in the call: a slice draws other samples"
        zero, seg = bake_lattice(t, lat, n, 0, estimator)
        assert len(zero) == 0 and seg == 0
        # the wrapper, and the device as `out`
        d = t.bake_lattice(lat, directions=D, passes=1, next_event=bool(estimator))
        assert np.array_equal(bits(d["sh"]).reshape(n, 27), whole[:, :27]) and np.array_equal(bits(d["samples"]), whole[:, 27])
    finally:
        t.close()


@pytest.mark.parametrize("name", ["default", "random"])
def test_skip_buried(name):
    t, sph, p = context(name)
    try:
        lat = lattice_of(name, "3x2x5", flags=abi.PT_LATTICE_SKIP_BURIED)
        lat.origin[1] = -0.7  # (the lower layer lies in the ground sphere)
        pts = P.lattice_points(lat, sph)
        buried = np.isnan(pts).all(axis=1)
        assert buried.any() and not buried.all() and np.isnan(pts).any(axis=1).sum() == buried.sum()
        got, seg = bake_lattice(t, lat, 0, lat.nodes)
        want, seg_want = bake_points(t, pts)
        assert np.array_equal(got, want) and seg == seg_want
        assert not got[buried].any(), "a buried node: all +0, samples == 0"
        assert (got.view(F)[~buried, 27] == D * SPP).all()
        lat.flags = 0
        plain, seg_plain = bake_lattice(t, lat, 0, lat.nodes)
        assert (plain.view(F)[:, 27] == D * SPP).all() and seg_plain > seg, "the flag off: every node is traced"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------- 2. the shading
@pytest.fixture(scope="module")
def lit():
    """per scene: the context with its feature planes rendered, the planes on the host, the baked records per lattice"""
    made = {}

    def get(name):
        if name not in made:
            t, sph, p = context(name, nee=name == "room")
            t.render_features()
            feats = t.features()
            baked = {dims: records_of(t, lattice_of(name, dims), next_event=name == "room") for dims in LATTICES}
            made[name] = (t, sph, p, feats, baked)
        return made[name]

    yield get
    for v in made.values():
        v[0].close()


def records_of(t, lat, **kw):
    d = t.bake_lattice(lat, directions=D, passes=1, **kw)
    return np.concatenate([d["sh"].reshape(-1, 27), d["samples"].reshape(-1, 1)], axis=1)


@pytest.mark.parametrize("dims", sorted(LATTICES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_shading_equals_the_restatement(lit, name, dims):
    t, sph, p, feats, all_baked = lit(name)
    lat = lattice_of(name, dims)
    typ, hit = feats["ids"][..., 2], feats["ids"][..., 0] >= 0
    assert hit.any() and ((~hit).any() or name == "room"), "the room is closed: every pixel hits"
    baked = all_baked[dims]  # (baked AFTER the feature launch: the bake goes through the query planes and leaves these alone)
    assert (baked[:, 27] == D * SPP).all()
    kept_any = 0
    for probes, what in ((baked, "baked"), (synthetic(lat.nodes), "synthetic")):
        for flags in (abi.PT_PROBE_HALFSPACE, 0):
            for bias in (0.0, 0.05):
                opt = abi.PtProbeShadeOptions(flags, bias)
                stats = {}
                want = restated(t, feats, lat, probes, opt, stats)
                got = shade(t, lat, probes, opt)
                assert_texels(got, want, "%s %s records, flags %d, bias %g" % (name, what, flags, bias))
                kept_any += int(stats["kept"].sum())
                lit_px = hit & np.isin(typ, (0, 1, 2))
                assert (got[~hit][:, 3] == 1).all() and np.array_equal(bits(got[~hit][:, :3]), bits(feats["albedo"][~hit][:, :3])), "a miss is the background"
                assert set(np.unique(got[..., 3]).tolist()) <= {0.0, 1.0} and (got[..., :3] >= 0).all()
                if what == "synthetic" and flags:
                    assert (stats["kept"][lit_px] < 8).any(), "the half-space test and the empty records drop corners"
    assert kept_any > 0
    assert_texels(shade(t, lat, baked, None), restated(t, feats, lat, baked, abi.PtProbeShadeOptions()), "options NULL: the half-space test on, no bias")
    if name == "random":
        assert (typ[hit] == 7).any() and not shade(t, lat, baked)[hit & (typ == 7)][:, :3].any(), "a type outside the four absorbs"
    if name != "default":
        e = hit & (typ == abi.PT_EMISSIVE)
        assert e.any() and np.array_equal(bits(shade(t, lat, baked)[e][:, :3]), bits(feats["albedo"][e][:, :3]))


def test_both_clamps_and_lattices_pinned_on_a_hit_point(lit):
    t, sph, p, feats, _ = lit("default")
    hit = np.argwhere((feats["ids"][..., 0] >= 0) & (feats["ids"][..., 2] == abi.PT_DIFFUSE))
    hp_all = feats["point"][..., :3]
    # a lattice smaller than the scene: hit points below its first and beyond its last node on every axis
    small = abi.PtProbeLattice(origin=(-0.3, -0.2, -1.2), step=(0.3, 0.2, 0.2), n=(3, 2, 5))
    g = (hp_all[hit[:, 0], hit[:, 1]].astype(np.float64) - np.array(list(small.origin))) / np.array(list(small.step))
    assert (g < 0).any(axis=0).all() and (g > np.array([2, 1, 4])).any(axis=0).all(), "both clamps act on every axis"
    probes = synthetic(small.nodes, empty_every=0)
    for opt in (abi.PtProbeShadeOptions(0, 0.0), abi.PtProbeShadeOptions(1, 0.05)):
        assert_texels(shade(t, small, probes, opt), restated(t, feats, small, probes, opt), "a lattice smaller than the scene")
    # origin = a read-back hit point's own bits: g == 0 there; and a lattice whose LAST node is that point (a dyadic step, and a
    # hit point for which fma(n - 1, step, origin) gives its bits back)
    step, n = F(0.5), (3, 2, 5)
    done = 0
    for y, x in hit[:: max(1, len(hit) // 40)]:
        hp = hp_all[y, x]
        first = abi.PtProbeLattice(origin=tuple(hp), step=(step,) * 3, n=n)
        origin = np.array([hp[c] - F(n[c] - 1) * step for c in range(3)], F)
        last = abi.PtProbeLattice(origin=tuple(origin), step=(step,) * 3, n=n)
        if not np.array_equal(bits(P.node_positions(last)[-1]), bits(hp)):
            continue
        probes = synthetic(first.nodes, seed=11, empty_every=0)
        for lat, what in ((first, "g == 0"), (last, "the last node")):
            opt = abi.PtProbeShadeOptions(0, 0.0)
            stats = {}
            want = restated(t, feats, lat, probes, opt, stats)
            got = shade(t, lat, probes, opt)
            assert_texels(got, want, what)
            assert stats["kept"][y, x] == 1, "on a node every fraction is 0 or 1: one corner, weight 1"
            node = 0 if lat is first else lat.nodes - 1
            E = P.shade(feats["albedo"][y, x][None], feats["normal"][y, x][None], feats["point"][y, x][None], feats["ids"][y, x][None], lat,
                        np.repeat(probes[node][None], lat.nodes, axis=0), 0, 0.0, tuple(t.params.camera_origin))
            assert np.array_equal(bits(got[y, x]), bits(E[0])), "that node's record alone"
        done += 1
        if done == 2:
            break
    assert done, "no hit point gives its bits back as a last node"


def test_host_and_device_pointers():
    import torch

    name = "random"
    t, sph, p = context(name, use_torch=True)
    try:
        t.render_features()
        lat = lattice_of(name, "3x2x5")
        probes = synthetic(lat.nodes)
        feats = {k: v.cpu().numpy() for k, v in t.features().items()}
        opt = abi.PtProbeShadeOptions(1, 0.05)
        want = restated(t, feats, lat, probes, opt)
        n = t.local_rows * t.width
        for probes_dev in (False, True):
            for out_dev in (False, True):
                pr = torch.from_numpy(probes).cuda() if probes_dev else probes
                out = torch.full((n + 2, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda") if out_dev else np.full((n + 2, 4), 0x5a5a5a5a, np.int32)
                ptr = lambda a: C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a.ctypes.data_as(C.c_void_p)
                t._check(t.lib.pt_shade_probes(t._ctx, C.byref(lat), ptr(pr), C.byref(opt), ptr(out)))
                torch.cuda.synchronize()
                got = out.cpu().numpy() if out_dev else out
                assert (got[n:] == 0x5a5a5a5a).all()
                assert_texels(got[:n].view(F).reshape(t.local_rows, t.width, 4), want, "probes on the %s, frame on the %s" % ("device" if probes_dev else "host", "device" if out_dev else "host"))
        # the wrapper: numpy in gives numpy out, a device tensor in gives a tensor out
        a = t.probe_lit_image(lat, probes, opt)
        b = t.probe_lit_image(lat, torch.from_numpy(probes).cuda(), opt)
        assert isinstance(a, np.ndarray) and torch.is_tensor(b) and b.is_cuda
        assert_texels(a, want, "probe_lit_image, numpy")
        assert_texels(b.cpu().numpy(), want, "probe_lit_image, torch")
        baked = t.bake_lattice(lat, directions=D)
        assert torch.is_tensor(baked["sh"]) and baked["sh"].is_cuda, "under use_torch the records stay on the device"
        c = t.probe_lit_image(lat, baked, opt)
        rec = np.concatenate([baked["sh"].cpu().numpy().reshape(-1, 27), baked["samples"].cpu().numpy().reshape(-1, 1)], axis=1)
        assert_texels(c.cpu().numpy(), restated(t, feats, lat, rec, opt), "baked and shaded without leaving the device")
    finally:
        t.close()


def test_a_row_band_against_the_whole_frame(lit):
    name = "room"
    t, sph, p, feats, _ = lit(name)
    lat = lattice_of(name, "3x2x5")
    probes = synthetic(lat.nodes)
    whole = shade(t, lat, probes)
    for index in (0, 1):
        b, _, pb = context(name, band=(8, index, 2))
        try:
            rows = [int(b.lib.pt_band_row(8, index, 2, l)) for l in range(b.local_rows)]
            assert b.local_rows == len(rows) and 0 < len(rows) < 19
            b.render_features()
            assert_texels(shade(b, lat, probes), whole[rows], "band %d of 2" % index)
        finally:
            b.close()
    # a band that owns no rows: PT_OK, nothing written
    e, _, _ = context(name, band=(32, 1, 2))
    try:
        assert e.local_rows == 0
        e.render_features()
        out = np.full((2, 4), GUARD, np.uint32)
        e._check(e.lib.pt_shade_probes(e._ctx, C.byref(lat), probes.ctypes.data_as(C.c_void_p), None, out.ctypes.data_as(C.c_void_p)))
        assert (out == GUARD).all()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------- 3. partition of unity
def ulps(a, b):
    """the distance of two arrays of non-negative floats in units in the last place"""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.mark.parametrize("name", sorted(CASES))
def test_identical_records_give_the_single_record_value(lit, name):
    t, sph, p, feats, _ = lit(name)
    lat = lattice_of(name, "3x2x5")
    one = synthetic(1, seed=3, empty_every=0)[0]
    probes = np.repeat(one[None], lat.nodes, axis=0)
    d = (feats["ids"][..., 0] >= 0) & (feats["ids"][..., 2] == abi.PT_DIFFUSE)
    for opt in (abi.PtProbeShadeOptions(0, 0.0), abi.PtProbeShadeOptions(1, 0.0)):
        got = shade(t, lat, probes, opt)
        shaded = d & (got[..., 3] == 1)
        assert shaded.sum() > 20
        n = feats["normal"][..., :3][shaded]
        E = (P.B_DIFFUSE[None, :, None] * G.sh_basis(n)[:, :, None] * one[:27].reshape(9, 3)[None]).astype(np.float64).sum(axis=1)
        # the single-record value by the statements: E_k's fma chain, max, * 1 / pi, * albedo — the blend of one corner of weight 1
        Ef = np.zeros((len(n), 3), F)
        B = (P.B_DIFFUSE[None, :] * G.sh_basis(n)).astype(F)
        for j in range(9):
            Ef = G.fma(B[:, j:j + 1], one[3 * j:3 * j + 3][None, :], Ef)
        assert np.allclose(Ef, E, rtol=1e-5, atol=1e-6)
        v = np.where(Ef > 0, Ef, F(0.0)).astype(F)
        want = feats["albedo"][..., :3][shaded] * (v * P.INV_PI)
        worst = int(ulps(got[shaded][:, :3], want).max())
        print("%s, flags %d: %d shaded DIFFUSE pixels, worst distance %d ulp" % (name, opt.flags, shaded.sum(), worst))
        assert worst <= 4


def test_records_linear_in_the_node_position_give_the_linear_function(lit):
    t, sph, p, feats, _ = lit("default")
    lat = lattice_of("default", "3x2x5")
    pos = P.node_positions(lat).astype(np.float64)
    a, k = np.array([1.3, 1.1, 0.9]), np.array([[0.21, -0.13, 0.08], [0.05, 0.17, -0.11], [-0.09, 0.04, 0.15]])  # value_c = a_c + k_c . x > 0 here
    value = a[None] + pos @ k.T
    assert (value > 0.2).all()
    probes = np.zeros((lat.nodes, 28), F)
    probes[:, 0:3] = value / (np.pi * 0.282095)  # band 0 alone: E = pi * Y0 * sh[0]
    probes[:, 27] = 64.0
    opt = abi.PtProbeShadeOptions(0, 0.0)
    got = shade(t, lat, probes, opt)
    d = (feats["ids"][..., 0] >= 0) & (feats["ids"][..., 2] == abi.PT_DIFFUSE)
    q = feats["point"][..., :3][d].astype(np.float64)
    g = (q - np.array(list(lat.origin), np.float64)) / np.array(list(lat.step), np.float64)
    inside = ((g >= 0) & (g <= np.array([2, 1, 4]))).all(axis=1)  # (outside, the border cell's clamped fractions answer: not the linear function)
    assert inside.sum() > 20
    want = (a[None] + q[inside] @ k.T) / np.pi * feats["albedo"][..., :3][d][inside].astype(np.float64)
    err = np.abs(got[d][inside][:, :3].astype(np.float64) - want) / np.abs(want)
    print("linear records: %d pixels inside, worst relative error %.3g" % (inside.sum(), err.max()))
    assert err.max() <= 1e-5


# ------------------------------------------------------------------------------------------- 4. a closed form
def test_a_small_sphere_under_the_sky_end_to_end():
    """One DIFFUSE sphere of radius r = 0.05 under PT_BG_SKY, centred in a 2 x 2 x 2 lattice of step 4, D = 4096.  The sky is
    L_c = A_c + B_c y (A = (1 + col) / 2, B = (col - 1) / 2, col = (0.5, 0.7, 1)): bands 0 and 1 hold it exactly, and the convex
    sphere lights itself by nothing, so every shaded pixel is albedo_c * (A_c + (2 / 3) B_c n_y).

    THE BOUND, per channel, of |texel - that|, derived and not fitted — two terms per coefficient of a probe:
      (a) the quadrature: coefficient j is off by at most probe_bounds(4096)[j] (tests/test_gather_ref.py, derived there from the
          set: the midpoint rule and Abel summation);
      (b) the sphere's share of a probe's sky: the sphere fills (r / d)^2 / 4 of a probe's sphere of directions, d = 2 sqrt 3 its
          distance: 5.2e-5, below 6e-5.  Over that share the radiance is anything in [0, 1] instead of the sky's (at most 1):
          |dL| <= 1, so coefficient j moves by at most 4 pi * 6e-5 * max|Y_j|, max|Y_j| <= 1.1.
      E(n) = sum_j b_j Y_j(n) sh_j: the two terms per coefficient times b_j |Y_j(n)|, summed over j; the blend is a convex
      combination of the probes' E (weights >= 0, / W), so one probe's bound holds for it; then / pi and * albedo.  Nothing is
      added for fp32 or for the basis' six-decimal constants.
    (The set is discrete: counted in float64 below, ONE of the 4 096 directions hits the sphere from three of the eight probes and
    none from the other five — a share of 1 / 4096 there, 0 elsewhere, about (b)'s figure on average.  That count is asserted
    apart; the bound is (a) + (b) as stated.)
    The noise of the path tracer does not enter: a ray that misses the sphere returns the sky exactly at any sample count."""
    D4 = 4096
    r, step = 0.05, 4.0
    albedo = (0.8, 0.6, 0.4)
    items = [scenes._sphere((0.0, 0.0, 0.0), r, abi.PT_DIFFUSE, albedo)]
    w, h = 40, 24
    p = scenes._base_params(1, DEPTH)
    scenes._look_at(scenes._lib(), p, w, h, (0.0, 0.05, 0.4), (0.0, 0.0, 0.0), 20.0, 0.0, 0.4)
    p = settings(p)
    p.samples_per_pixel = 1
    t = PathTracer(w, h)
    try:
        t.set_spheres(scenes._pack(items))
        t.ray_queries(True)
        t.feature_planes(True)
        t.reserve_passes(1)
        t.set_params(p)
        lat = abi.PtProbeLattice(origin=(-2.0, -2.0, -2.0), step=(step,) * 3, n=(2, 2, 2))
        rec = np.concatenate([t.bake_lattice(lat, directions=D4)[k].reshape(8, -1) for k in ("sh", "samples")], axis=1)
        t.render_features()
        feats = t.features()
        got = shade(t, lat, rec)
        on = feats["ids"][..., 0] >= 0
        assert on.sum() > 30 and (got[on][:, 3] == 1).all(), "every pixel of the sphere finds a probe in front of its tangent plane"
        n = feats["normal"][..., :3][on].astype(np.float64)
        col = np.array([0.5, 0.7, 1.0])
        A, B = (1.0 + col) / 2.0, (col - 1.0) / 2.0
        want = np.array(albedo)[None] * (A[None] + 2.0 / 3.0 * B[None] * n[:, 1:2])
        # the directions of the set that hit the sphere, probe by probe, in float64: at most one, and the solid angle's share
        dirs = G.sphere64(D4)
        pos = P.node_positions(lat).astype(np.float64)
        to_centre = -pos / np.linalg.norm(pos, axis=1)[:, None]
        k = ((dirs @ to_centre.T) > np.sqrt(1.0 - (r / np.linalg.norm(pos[0])) ** 2)).sum(axis=0)
        assert k.max() <= 1 and (r / np.linalg.norm(pos[0])) ** 2 / 4.0 < 6e-5
        band = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
        per_coeff = probe_bounds(D4) + 4.0 * np.pi * 6e-5 * 1.1  # (9, 3): (a) + (b)
        Y = np.abs(G.basis64(n))  # (pixels, 9)
        bound = ((band[None, :] * Y)[:, :, None] * per_coeff[None]).sum(axis=1) / np.pi * np.array(albedo)[None]
        err = np.abs(got[on][:, :3].astype(np.float64) - want)
        print("a small sphere under the sky: %d pixels, hits per probe %s, worst error %.3g, its bound %.3g, worst error / bound %.3g"
              % (on.sum(), k.tolist(), err.max(), bound.flat[np.argmax(err)], (err / bound).max()))
        assert (err <= bound).all()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------- 5. nothing else moves
def test_nothing_else_moves():
    name = "room"
    t, sph, p = context(name, nee=True)
    u, _, _ = context(name, nee=True)
    try:
        lat = lattice_of(name, "2x2x2")
        probes = synthetic(lat.nodes, empty_every=0)
        k = 1
        t.render_features()
        t.render_passes(k)
        t.synchronize()
        accum = t.accum().copy()
        planes = {n: v.copy() for n, v in t.features().items()}
        stats, build = stats_dict(t.stats()), t.last_trace_build()
        img = shade(t, lat, probes)
        assert img[..., 3].any()
        assert np.array_equal(bits(t.accum()), bits(accum)), "the accumulation"
        for n, v in t.features().items():
            assert np.array_equal(v.view(np.uint32), planes[n].view(np.uint32)), n
        assert stats_dict(t.stats()) == stats and t.last_trace_build() == build
        t.render_passes(k)
        t.synchronize()
        u.render_features()
        u.render_passes(k)
        u.render_passes(k)
        u.synchronize()
        assert np.array_equal(bits(t.accum()), bits(u.accum())), "k passes, a shade, k passes equals 2 k passes"
        assert stats_dict(t.stats())["segments"] == stats_dict(u.stats())["segments"]
    finally:
        t.close()
        u.close()


# ------------------------------------------------------------------------------------------- 6. errors
def code_of(fn):
    with pytest.raises(PtError) as e:
        fn()
    return e.value.code, str(e.value)


def test_errors_leave_the_context_usable():
    name = "default"
    t, sph, p = context(name)
    try:
        lat = lattice_of(name, "2x2x2")
        probes = synthetic(8, empty_every=0)
        out = np.zeros((8, 28), F)

        def bake(L, first=0, count=8, directions=D, passes=1, estimator=0):
            t._check(t.lib.pt_bake_lattice(t._ctx, C.byref(L), first, count, directions, passes, estimator, out.ctypes.data_as(C.c_void_p)))

        # no feature launch yet, then stale planes, then the option off
        code, msg = code_of(lambda: shade(t, lat, probes))
        assert code == abi.PT_ERR_NOT_READY and "no pt_render_features" in msg
        t.render_features()
        good = shade(t, lat, probes)
        for change in (lambda: t.set_params(p), lambda: t.set_spheres(sph), lambda: (t.lib.pt_resize(t._ctx, p.width + 8, p.height), t.lib.pt_resize(t._ctx, p.width, p.height))):
            change()
            assert code_of(lambda: shade(t, lat, probes))[0] == abi.PT_ERR_NOT_READY
            t.set_params(p)
            t.render_features()
            assert_texels(shade(t, lat, probes), good, "after the change and a new pt_render_features")
        t.feature_planes(False)
        code, msg = code_of(lambda: shade(t, lat, probes))
        assert code == abi.PT_ERR_NOT_READY and "PT_OPT_FEATURES" in msg
        t.feature_planes(True)
        t.render_features()
        # every lattice limit, in both calls
        def lattice(**kw):
            L = lat.copy()
            for k, v in kw.items():
                if k in ("origin", "step"):
                    getattr(L, k)[:] = v
                else:
                    setattr(L, k, v)
            return L
        bad = [lattice(nx=1), lattice(ny=257), lattice(nz=0), lattice(nx=256, ny=256, nz=17), lattice(step=(0.0, 1.0, 1.0)), lattice(step=(1.0, -2.0, 1.0)),
               lattice(step=(1.0, 1.0, np.inf)), lattice(step=(np.nan, 1.0, 1.0)), lattice(origin=(np.inf, 0.0, 0.0)), lattice(origin=(0.0, np.nan, 0.0)), lattice(flags=2)]
        for L in bad:
            words = P.lattice_error(L)
            assert words
            for call in (lambda: bake(L), lambda: t._check(t.lib.pt_shade_probes(t._ctx, C.byref(L), probes.ctypes.data_as(C.c_void_p), None, out.ctypes.data_as(C.c_void_p)))):
                code, msg = code_of(call)
                assert code == abi.PT_ERR_INVALID and words in msg, (msg, words)
        assert not out.any(), "a refused call writes nothing"
        for kw in (dict(first=1, count=8), dict(first=9, count=0), dict(first=2 ** 32 - 1, count=2), dict(estimator=2), dict(estimator=-1), dict(directions=100),
                   dict(passes=0)):
            assert code_of(lambda: bake(lat, **kw))[0] == abi.PT_ERR_INVALID, kw
        assert code_of(lambda: bake(lat, passes=2))[0] == abi.PT_ERR_CAPACITY
        code, msg = code_of(lambda: bake(lat, estimator=1))
        assert code == abi.PT_ERR_NOT_READY and "PT_OPT_NEXT_EVENT" in msg
        for opt in (abi.PtProbeShadeOptions(2, 0.0), abi.PtProbeShadeOptions(1, float("nan")), abi.PtProbeShadeOptions(0, float("inf"))):
            assert code_of(lambda: shade(t, lat, probes, opt))[0] == abi.PT_ERR_INVALID
        t.ray_queries(False)
        assert code_of(lambda: bake(lat))[0] == abi.PT_ERR_NOT_READY
        t.ray_queries(True)
        t.set_count_work(True)
        code, msg = code_of(lambda: shade(t, lat, probes))
        assert code == abi.PT_ERR_INVALID and "PT_OPT_COUNT_WORK" in msg
        assert code_of(lambda: bake(lat))[0] == abi.PT_ERR_INVALID
        t.set_count_work(False)
        # ... and the context still answers, with the bits of a fresh one
        t.render_features()
        assert_texels(shade(t, lat, probes), good, "after the errors")
        bake(lat)
        fresh, _, _ = context(name)
        try:
            want, _ = bake_lattice(fresh, lat, 0, 8)
        finally:
            fresh.close()
        assert np.array_equal(bits(out), want)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------- 7. the pipeline
def test_the_frame_goes_straight_into_the_read_outs():
    import torch

    name = "room"
    t, sph, p = context(name, use_torch=True)
    try:
        t.tone_mapping(True)
        t.render_features()
        lat = lattice_of(name, "3x2x5")
        probes = torch.from_numpy(synthetic(lat.nodes, empty_every=0) * F(4.0)).cuda()
        frame = t.probe_lit_image(lat, probes)
        assert torch.is_tensor(frame) and frame.is_cuda
        tone = abi.PtToneOptions()
        t.meter(src=frame)
        rec_dev, hist_dev = t.exposure()
        toned_dev = t.toned_image(tone, src=frame).cpu().numpy()
        host = frame.cpu().numpy()
        t.tone_mapping(False)
        t.tone_mapping(True)  # (the exposure forgotten: the same first metering again)
        t.meter(src=host)
        rec_host, hist_host = t.exposure()
        toned_host = t.toned_image(tone, src=host)
        assert np.array_equal(hist_dev, hist_host) and bytes(rec_dev) == bytes(rec_host)
        assert np.array_equal(bits(toned_dev), bits(toned_host)) and toned_host[..., :3].any()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------- the shared-cell form
def test_the_shared_cell_form_gives_the_same_bits_and_both_ways_are_reached():
    """include/ptrace_dev.h pt_debug_probe_form: form 1 stages a coherent wave's cell in LDS.  A frame in which every wave is
    coherent (one huge cell), a frame in which the waves are not (a step of about a pixel's footprint), the same bits as form 0
    on both, and the per-tile path words say that both ways ran."""
    import torch

    name = "default"
    t, sph, p = context(name, use_torch=True)
    try:
        t.render_features()
        feats = {k: v.cpu().numpy() for k, v in t.features().items()}
        lit_px = (feats["ids"][..., 0] >= 0) & np.isin(feats["ids"][..., 2], (0, 1, 2))
        tiles_x, tiles_y = (t.width + 7) // 8, (t.local_rows + 7) // 8
        tile_of = lambda y, x: (y // 8) * tiles_x + x // 8

        def expected_ways(lat, bias):
            """per tile: 0 no lit lane, 2 its lit pixels share one cell (the restatement's cells), 1 they do not"""
            cells = {}
            dims = (int(lat.nx), int(lat.ny), int(lat.nz))
            n, hp = feats["normal"][..., :3], feats["point"][..., :3]
            idx = []
            for c in range(3):
                q = P.fma(F(bias), n[..., c], hp[..., c])
                idx.append(P.cells((q - F(lat.origin[c])) / F(lat.step[c]), dims[c])[0])
            node = (idx[2] * dims[1] + idx[1]) * dims[0] + idx[0]
            for y, x in np.argwhere(lit_px):
                cells.setdefault(tile_of(y, x), set()).add(int(node[y, x]))
            want = np.zeros(tiles_x * tiles_y, np.int32)
            for tile, found in cells.items():
                want[tile] = 2 if len(found) == 1 else 1
            return want

        lit_tiles = expected_ways(abi.PtProbeLattice(), 0.0) > 0
        huge = abi.PtProbeLattice(origin=(-200.0, -200.0, -200.0), step=(400.0, 400.0, 400.0), n=(2, 2, 2))
        fine = abi.PtProbeLattice(origin=(-1.3, -0.5, -2.0), step=(0.04, 0.04, 0.04), n=(64, 32, 64))
        seen = set()
        for lat, what in ((huge, "one huge cell"), (fine, "cells of a pixel's footprint")):
            probes = synthetic(lat.nodes)
            if lat is huge:
                probes[:, 27] = 128.0
            dev = torch.from_numpy(probes).cuda()
            for opt in (abi.PtProbeShadeOptions(1, 0.0), abi.PtProbeShadeOptions(0, 0.05)):
                want = restated(t, feats, lat, probes, opt)
                frames = {}
                paths = torch.zeros(tiles_x * tiles_y, dtype=torch.int32, device="cuda")
                for form in (0, 1):
                    t._check(t.lib.pt_debug_probe_form(t._ctx, form, C.c_void_p(paths.data_ptr()) if form else None))
                    out = torch.full((t.local_rows * t.width + 2, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
                    t._check(t.lib.pt_shade_probes(t._ctx, C.byref(lat), C.c_void_p(dev.data_ptr()), C.byref(opt), C.c_void_p(out.data_ptr())))
                    torch.cuda.synchronize()
                    got = out.cpu().numpy()
                    assert (got[-2:] == 0x5a5a5a5a).all()
                    frames[form] = got[:-2].view(F).reshape(t.local_rows, t.width, 4)
                    assert_texels(frames[form], want, "%s, form %d" % (what, form))
                way = paths.cpu().numpy()
                expect = expected_ways(lat, opt.normal_bias)
                assert np.array_equal(way, expect), "a wave stages its cell exactly where its lit pixels share one, and reports only where a lane is lit"
                if lat is huge:
                    assert (way[lit_tiles] == 2).all(), "one cell: every wave stages it"
                else:
                    # NO coherent wave at all is out of reach on a real frame: a wave with ONE lit lane (a sphere's rim in a block of
                    # sky) shares its cell with itself.  Every wave with lit pixels in two cells or more loads for itself — the equality
                    # above — and those are most waves of this frame:
                    lit_count = np.bincount([tile_of(y, x) for y, x in np.argwhere(lit_px)], minlength=len(way))
                    print("%s, bias %g: %d waves load for themselves, %d stage a cell (their lit lanes: %s)" % (
                        what, opt.normal_bias, (way == 1).sum(), (way == 2).sum(), lit_count[way == 2].tolist()))
                    assert (way == 1).sum() > (way == 2).sum()
                seen |= set(way[lit_tiles].tolist())
        assert seen == {1, 2}, "both ways of the kernel were reached"
        assert t.lib.pt_debug_probe_form(t._ctx, 2, None) == abi.PT_ERR_INVALID and t.lib.pt_debug_probe_form(t._ctx, 0, C.c_void_p(8)) == abi.PT_ERR_INVALID
        t._check(t.lib.pt_debug_probe_form(t._ctx, -1, None))
    finally:
        t.close()
